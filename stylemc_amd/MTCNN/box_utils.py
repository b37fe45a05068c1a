"""Host-side box arithmetic of the MTCNN detector (numpy / PIL), restating MTCNN/box_utils.py of the reference.

Boxes are float rows (x1, y1, x2, y2, score) with INCLUSIVE corners: a box's width is x2 - x1 + 1.  The uint8
conversion and the PIL bilinear resize of the cut-outs stay on the host exactly where the reference has them: they decide
which boxes survive the next stage's threshold.
"""
import numpy as np
from PIL import Image


def nms(boxes, overlap_threshold=0.5, mode="union"):
    """Greedy non-maximum suppression (box_utils.py:5-68): take the best-scoring box, drop every remaining box whose
    overlap with it exceeds the threshold, repeat.  Overlap is intersection over union, or over the smaller area for
    mode 'min'.  Returns the picked indices, best first."""
    if len(boxes) == 0:
        return []
    if mode not in ("union", "min"):
        raise ValueError(f"nms mode {mode!r}: 'union' or 'min'")
    x1, y1, x2, y2, score = (boxes[:, i] for i in range(5))
    area = (x2 - x1 + 1.0) * (y2 - y1 + 1.0)
    order = np.argsort(score)  # ascending: the best is last
    pick = []
    while order.size > 0:
        best, rest = order[-1], order[:-1]
        pick.append(best)
        w = np.maximum(0.0, np.minimum(x2[best], x2[rest]) - np.maximum(x1[best], x1[rest]) + 1.0)
        h = np.maximum(0.0, np.minimum(y2[best], y2[rest]) - np.maximum(y1[best], y1[rest]) + 1.0)
        inter = w * h
        if mode == "min":
            overlap = inter / np.minimum(area[best], area[rest])
        else:
            overlap = inter / (area[best] + area[rest] - inter)
        order = rest[~(overlap > overlap_threshold)]
    return pick


def convert_to_square(bboxes):
    """Grow each box about its centre to a square of its longer side (box_utils.py:71-91).  Column 4 comes back 0, as
    in the reference (np.zeros_like, only the corners filled); detect_faces overwrites it before reading it."""
    out = np.zeros_like(bboxes)
    x1, y1, x2, y2 = (bboxes[:, i] for i in range(4))
    h = y2 - y1 + 1.0
    w = x2 - x1 + 1.0
    side = np.maximum(h, w)
    out[:, 0] = x1 + w * 0.5 - side * 0.5
    out[:, 1] = y1 + h * 0.5 - side * 0.5
    out[:, 2] = out[:, 0] + side - 1.0
    out[:, 3] = out[:, 1] + side - 1.0
    return out


def calibrate_box(bboxes, offsets):
    """Move the corners by the nets' regression outputs, which are fractions of the box's width (x) and height (y)
    (box_utils.py:94-124).  Updates ``bboxes`` in place and returns it, as the reference does."""
    w = (bboxes[:, 2] - bboxes[:, 0] + 1.0)[:, None]
    h = (bboxes[:, 3] - bboxes[:, 1] + 1.0)[:, None]
    bboxes[:, 0:4] = bboxes[:, 0:4] + np.hstack([w, h, w, h]) * offsets
    return bboxes


def correct_bboxes(bboxes, width, height):
    """Clip boxes to a width x height image and say where the kept part sits in the w x h cut-out
    (box_utils.py:162-223).  Returns int32 arrays [dy, edy, dx, edx, y, ey, x, ex, w, h]: cut-out rows dy..edy and
    columns dx..edx receive image rows y..ey and columns x..ex (all inclusive).  The clipping writes through to the
    corner columns of ``bboxes`` -- the reference's arrays are views of it -- which detect_faces relies on."""
    x, y, ex, ey = (bboxes[:, i] for i in range(4))  # views
    w, h = ex - x + 1.0, ey - y + 1.0
    n = bboxes.shape[0]
    dx, dy = np.zeros((n,)), np.zeros((n,))
    edx, edy = w.copy() - 1.0, h.copy() - 1.0

    over = np.where(ex > width - 1.0)[0]
    edx[over] = w[over] + width - 2.0 - ex[over]
    ex[over] = width - 1.0
    over = np.where(ey > height - 1.0)[0]
    edy[over] = h[over] + height - 2.0 - ey[over]
    ey[over] = height - 1.0
    under = np.where(x < 0.0)[0]
    dx[under] = 0.0 - x[under]
    x[under] = 0.0
    under = np.where(y < 0.0)[0]
    dy[under] = 0.0 - y[under]
    y[under] = 0.0
    return [a.astype("int32") for a in (dy, edy, dx, edx, y, ey, x, ex, w, h)]


def _preprocess(img):
    """[h, w, c] pixel values -> [1, c, h, w] in about [-1, 1]: (v - 127.5) / 128 (box_utils.py:226-238)."""
    return (np.expand_dims(img.transpose((2, 0, 1)), 0) - 127.5) * 0.0078125


def get_image_boxes(bounding_boxes, img, size=24):
    """The boxes' cut-outs from a PIL image, zero where a box leaves it, each resized to size x size with PIL's bilinear
    filter on uint8 and preprocessed: float32 [n, 3, size, size] (box_utils.py:127-159)."""
    n = len(bounding_boxes)
    width, height = img.size
    dy, edy, dx, edx, y, ey, x, ex, w, h = correct_bboxes(bounding_boxes, width, height)
    pixels = np.asarray(img, "uint8")
    out = np.zeros((n, 3, size, size), "float32")
    for i in range(n):
        cut = np.zeros((h[i], w[i], 3), "uint8")
        cut[dy[i]:edy[i] + 1, dx[i]:edx[i] + 1, :] = pixels[y[i]:ey[i] + 1, x[i]:ex[i] + 1, :]
        cut = np.asarray(Image.fromarray(cut).resize((size, size), Image.BILINEAR), "float32")
        out[i] = _preprocess(cut)
    return out
