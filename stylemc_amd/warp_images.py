"""``crop_face`` of the reference's warp_images.py (:71-110): the square crop around a detected face that the landmark
regressor reads.  The triangle-warp helpers of that module are not part of this project.

The crop is a square of 1.2 x the box's shorter side about the box's centre, clipped to the image.  On the tensor path
the clipped window is resized with bilinear interpolation (align_corners False, no antialias) by
smc_crop_bilinear_norm_f32, on the GPU; on the PIL path the part that left the image is zero-padded first
(cv2.copyMakeBorder in the reference) and the resize is cv2.resize's default bilinear.  cv2 is not installed where this
project is built: the PIL path uses PIL's bilinear filter with ``reducing_gap=None`` on the same array, and ITS PARITY
WITH cv2.resize IS UNPINNED (the two agree on upscaling to rounding; on downscaling PIL widens its filter support, cv2
does not).
"""
import numpy as np
import torch
from PIL import Image

from . import mobilenet_hip


def crop_box(width, height, face):
    """The crop window of one face row (left, top, right, bottom, ...; inclusive corners) in a width x height image
    (warp_images.py:78-98): a square of 1.2 x the box's shorter side (truncated), placed so that the box's centre pixel
    sits at its centre pixel.  Returns ([x1, y1, x2, y2] clipped to the image, exclusive ends; (dx, dy, edx, edy), how
    many columns / rows of the square fell outside on the left, top, right and bottom)."""
    left, top, right, bottom = face[:4]
    box_w, box_h = right - left + 1, bottom - top + 1
    side = int(1.2 * min(box_w, box_h))
    x0 = left + box_w // 2 - side // 2
    y0 = top + box_h // 2 - side // 2
    outside = tuple(int(max(0, v)) for v in (-x0, -y0, x0 + side - width, y0 + side - height))
    return [int(max(0, x0)), int(max(0, y0)), int(min(width, x0 + side)), int(min(height, y0 + side))], outside


def crop_face(img, faces, out_size):
    """img: an [H, W, 3] tensor of 0..255 values on the GPU, or a PIL image; faces: detect_faces' boxes -- the FIRST row
    is used, whatever its score (warp_images.py:78).  Returns (crop [out_size, out_size, 3], the clipped window's
    height, [x1, y1, x2, y2])."""
    if isinstance(img, torch.Tensor):
        height, width = img.size(0), img.size(1)
        box, _ = crop_box(width, height, faces[0])
        planes = img.permute(2, 0, 1).unsqueeze(0).to(torch.float32)
        boxes = torch.tensor([box], dtype=torch.int32, device=img.device)
        face = mobilenet_hip.crop_bilinear_norm(planes, boxes, out_size, denorm=False)[0].permute(1, 2, 0)
        return face, box[3] - box[1], box
    if not isinstance(img, Image.Image):
        raise TypeError(f"crop_face: a tensor or a PIL image, not {type(img).__name__}")
    width, height = img.size
    box, (dx, dy, edx, edy) = crop_box(width, height, faces[0])
    cropped = np.array(img)[box[1]:box[3], box[0]:box[2]]
    if dx > 0 or dy > 0 or edx > 0 or edy > 0:
        pad = ((dy, edy), (dx, edx)) + ((0, 0),) * (cropped.ndim - 2)
        cropped = np.pad(cropped, pad, mode="constant", constant_values=0)
    face = np.asarray(Image.fromarray(cropped).resize((out_size, out_size), Image.BILINEAR))
    return face, cropped.shape[0], box
