"""MTCNN face detector: image pyramid -> P-Net -> R-Net -> O-Net (restating MTCNN/detector.py:10-129 of the reference).

The three nets are passed in (or built once and cached per weights / device: the reference rebuilds and reloads them on
every call, detector.py:28-31).  A net is any callable on a float32 numpy batch [n, 3, h, w] that returns numpy arrays:
P-Net and R-Net (offsets, probs), O-Net (landmarks, offsets, probs) -- mtcnn_hip.HipMTCNN on the GPU, get_nets.TorchMTCNN
on the CPU, or recorded outputs in the tests.

Deviation: where no pyramid level yields a box the reference fails inside np.vstack([]) (a ValueError its callers
swallow with a bare except); here that case, and an empty survivor list after any stage, returns ([], []).
"""
import numpy as np
import torch
from PIL import Image

from .box_utils import calibrate_box, convert_to_square, get_image_boxes, nms
from .first_stage import run_first_stage

MIN_DETECTION_SIZE = 12
PYRAMID_FACTOR = 0.707  # about sqrt(0.5): each level halves the area

_cached = {}


def pyramid_scales(width, height, min_face_size=20.0):
    """Scales at which a min_face_size face becomes P-Net's 12-px window, shrinking by 0.707 until the image's short side
    would fall to 12 px (detector.py:34-53)."""
    m = MIN_DETECTION_SIZE / min_face_size
    length = min(height, width) * m
    scales, k = [], 0
    while length > MIN_DETECTION_SIZE:
        scales.append(m * PYRAMID_FACTOR ** k)
        length *= PYRAMID_FACTOR
        k += 1
    return scales


def default_nets(weights="MTCNN/weights", device="cuda"):
    """The executor for a weights directory (or 'synthetic'), built once per (weights, device)."""
    key = (str(weights), str(device))
    if key not in _cached:
        from .. import mtcnn_hip
        _cached[key] = mtcnn_hip.build_mtcnn(weights, device=device)
    return _cached[key]


def detect_faces(image, min_face_size=20.0, thresholds=(0.6, 0.7, 0.8), nms_thresholds=(0.7, 0.7, 0.7), device="cuda",
                 nets=None, weights="MTCNN/weights"):
    """image: a PIL image, or an [H, W, 3] tensor of 0..255 values (truncated to uint8, detector.py:24-25).
    Returns (boxes [n, 5] as (x1, y1, x2, y2, score), landmarks [n, 10] as five x then five y), or ([], [])."""
    if isinstance(image, torch.Tensor):
        image = Image.fromarray(image.detach().cpu().numpy().astype(np.uint8))
    if nets is None:
        nets = default_nets(weights, device)
    width, height = image.size

    # stage 1: P-Net over the pyramid, NMS per level and then across levels
    levels = [run_first_stage(image, nets.pnet, scale=s, threshold=thresholds[0])
              for s in pyramid_scales(width, height, min_face_size)]
    levels = [b for b in levels if b is not None]
    if not levels:
        return [], []
    boxes = np.vstack(levels)
    boxes = boxes[nms(boxes[:, 0:5], nms_thresholds[0])]
    boxes = calibrate_box(boxes[:, 0:5], boxes[:, 5:])
    boxes = convert_to_square(boxes)
    boxes[:, 0:4] = np.round(boxes[:, 0:4])

    # stage 2: R-Net on 24-px cut-outs
    offsets, probs = nets.rnet(get_image_boxes(boxes, image, size=24))
    keep = np.where(probs[:, 1] > thresholds[1])[0]
    boxes = boxes[keep]
    boxes[:, 4] = probs[keep, 1].reshape((-1,))
    offsets = offsets[keep]
    keep = nms(boxes, nms_thresholds[1])
    if len(keep) == 0:
        return [], []
    boxes = calibrate_box(boxes[keep], offsets[keep])
    boxes = convert_to_square(boxes)
    boxes[:, 0:4] = np.round(boxes[:, 0:4])

    # stage 3: O-Net on 48-px cut-outs; its landmarks are fractions of the (square, clipped) box
    landmarks, offsets, probs = nets.onet(get_image_boxes(boxes, image, size=48))
    keep = np.where(probs[:, 1] > thresholds[2])[0]
    if len(keep) == 0:
        return [], []
    boxes = boxes[keep]
    boxes[:, 4] = probs[keep, 1].reshape((-1,))
    offsets = offsets[keep]
    landmarks = landmarks[keep]
    w = boxes[:, 2] - boxes[:, 0] + 1.0
    h = boxes[:, 3] - boxes[:, 1] + 1.0
    landmarks[:, 0:5] = boxes[:, 0:1] + w[:, None] * landmarks[:, 0:5]
    landmarks[:, 5:10] = boxes[:, 1:2] + h[:, None] * landmarks[:, 5:10]
    boxes = calibrate_box(boxes, offsets)
    keep = nms(boxes, nms_thresholds[2], mode="min")
    return boxes[keep], landmarks[keep]
