"""Inputs of the landmarks fixture (tests/golden/landmarks.npz), shared by make_golden_landmarks.py and the tests: seeded,
regenerated, never stored."""
import numpy as np
import torch

THRESHOLDS = (0.6, 0.6, 0.6)         # detect_faces thresholds of the end-to-end case
NMS_THRESHOLDS = (0.7, 0.7, 0.7)
IMAGE_HW = (96, 128)
PNET_SHAPES = {"13x12": (13, 12), "37x50": (37, 50)}   # (h, w): one output cell with a 12-px edge; several cells, odd
MARGIN = 1e-3


def detect_image(seed):
    """96 x 128 RGB uint8: sinusoids plus noise (textured enough that the seeded nets pass some windows)."""
    h, w = IMAGE_HW
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        fx, fy, ph = rng.uniform(0.05, 0.4), rng.uniform(0.05, 0.4), rng.uniform(0, 6.28)
        img[..., c] = 127.5 + 70.0 * np.sin(fx * xx + fy * yy + ph) + 25.0 * np.cos(0.9 * fy * xx - 0.7 * fx * yy)
    img += rng.normal(0, 20.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def net_input(name, n=5, hw=None):
    """Seeded float32 batches in the preprocessed range: P-Net [1, 3, h, w], R-Net [n, 3, 24, 24], O-Net [n, 3, 48, 48]."""
    size = {"rnet": (24, 24), "onet": (48, 48)}.get(name, hw)
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 1000 + size[0] * 64 + size[1])
    return (torch.rand(1 if name == "pnet" else n, 3, size[0], size[1], generator=g) * 2 - 1).numpy()


def host_boxes(n=40, seed=3):
    """Random boxes (x1, y1, x2, y2, score) with integer corners around a 128 x 96 image, some leaving it."""
    rng = np.random.RandomState(seed)
    x1 = rng.randint(-10, 110, n).astype(np.float64)
    y1 = rng.randint(-10, 80, n).astype(np.float64)
    w = rng.randint(8, 50, n)
    h = rng.randint(8, 50, n)
    return np.stack([x1, y1, x1 + w - 1, y1 + h - 1, rng.permutation(n) / n + 0.003], axis=1)


def host_offsets(n=40, seed=4):
    return np.random.RandomState(seed).normal(0, 0.1, (n, 4)).astype(np.float32)


def pnet_maps(seed=6, hw=(9, 13)):
    rng = np.random.RandomState(seed)
    probs = rng.uniform(0, 1, hw).astype(np.float32)
    offsets = rng.normal(0, 0.1, (1, 4) + hw).astype(np.float32)
    return probs, offsets


def crop_case():
    """A [H, W, 3] float image in 0..255 (after denorm_img) and two face rows: one inside, one leaving the image."""
    g = torch.Generator().manual_seed(21)
    img = torch.rand(72, 88, 3, generator=g) * 255
    faces = {"inside": np.array([[20.0, 15.0, 60.0, 58.0, 0.9]]), "clipped": np.array([[55.0, 30.0, 95.0, 80.0, 0.8]])}
    return img, faces


ALIGN_KW = dict(output_size=64, transform_size=256)


def align_case(key):
    """A seeded [H, W, 3] uint8 photograph and 68 integer landmarks of a plausible face.  'nopad': a small face in the
    middle (the crop square lies inside the image); 'pad': a large face near the corner (the square leaves the image, so
    the reflect-pad runs, and it is large enough that the pre-shrink runs too)."""
    h, w, eye, cx, cy = {"nopad": (200, 240, 24.0, 120.0, 90.0), "pad": (300, 320, 90.0, 95.0, 80.0)}[key]
    rng = np.random.RandomState({"nopad": 31, "pad": 32}[key])
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    img = np.stack([127.5 + 90 * np.sin(xx / (7.0 + 3 * c) + c) * np.cos(yy / (9.0 + 2 * c)) for c in range(3)], axis=-1)
    img = np.clip(np.rint(img + rng.normal(0, 12.0, img.shape)), 0, 255).astype(np.uint8)
    lm = np.zeros((68, 2))
    lm[:] = (cx, cy) + rng.normal(0, eye * 0.8, (68, 2))                       # the points align_face does not read
    tilt = np.array([[np.cos(0.2), -np.sin(0.2)], [np.sin(0.2), np.cos(0.2)]])  # a head turned by 0.2 rad
    ring = np.array([[np.cos(a), 0.5 * np.sin(a)] for a in np.arange(6) * np.pi / 3]) * eye * 0.18
    lm[36:42] = (cx, cy) + (ring + [-eye / 2, 0]) @ tilt.T
    lm[42:48] = (cx, cy) + (ring + [eye / 2, 0]) @ tilt.T
    mouth = np.array([[np.cos(a), 0.4 * np.sin(a)] for a in np.pi - np.arange(12) * np.pi / 6]) * eye * 0.4
    lm[48:60] = (cx, cy) + (mouth + [0, eye * 1.1]) @ tilt.T
    return img, np.rint(lm).astype(int)
