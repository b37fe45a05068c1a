"""Stage 1 of the detector: P-Net on one level of the image pyramid (restating MTCNN/first_stage.py of the reference)."""
import math

import numpy as np
from PIL import Image

from .box_utils import _preprocess, nms

PNET_STRIDE = 2   # P-Net is fully convolutional: its output cell (i, j) sees the 12 x 12 window at (2 i, 2 j)
PNET_CELL = 12


def scaled_input(image, scale):
    """The pyramid level as P-Net's input: PIL bilinear resize to ceil(size * scale) on uint8, then the preprocess
    (first_stage.py:27-33): float32 [1, 3, sh, sw]."""
    width, height = image.size
    sw, sh = math.ceil(width * scale), math.ceil(height * scale)
    img = np.asarray(image.resize((sw, sh), Image.BILINEAR), "float32")
    return _preprocess(img).astype("float32")


def _generate_bboxes(probs, offsets, scale, threshold):
    """Cells whose face probability exceeds the threshold, as boxes in the unscaled image (first_stage.py:49-99).
    probs [n, m], offsets [1, 4, n, m] -> [n_boxes, 9] rows (x1, y1, x2, y2, score, tx1, ty1, tx2, ty2); an empty array
    when no cell passes.  The window's corner is taken at 2 * index + 1, as the reference takes it."""
    rows, cols = np.where(probs > threshold)
    if rows.size == 0:
        return np.array([])
    regress = np.array([offsets[0, i, rows, cols] for i in range(4)])
    return np.vstack([
        np.round((PNET_STRIDE * cols + 1.0) / scale),
        np.round((PNET_STRIDE * rows + 1.0) / scale),
        np.round((PNET_STRIDE * cols + 1.0 + PNET_CELL) / scale),
        np.round((PNET_STRIDE * rows + 1.0 + PNET_CELL) / scale),
        probs[rows, cols], regress,
    ]).T


def run_first_stage(image, net, scale, threshold):
    """P-Net on the image scaled by ``scale``, boxes above ``threshold``, NMS at 0.5 within the level
    (first_stage.py:9-46).  ``net``: float32 [1, 3, h, w] -> (offsets [1, 4, h', w'], probs [1, 2, h', w']) as numpy
    arrays.  Returns [n_boxes, 9] or None."""
    offsets, probs = net(scaled_input(image, scale))
    boxes = _generate_bboxes(probs[0, 1, :, :], offsets, scale, threshold)
    if len(boxes) == 0:
        return None
    return boxes[nms(boxes[:, 0:5], overlap_threshold=0.5)]
