"""FFHQ-style face alignment from a photograph (drop-in for the reference's align_faces.py).

    python -m stylemc_amd.align_faces --input_image photo.jpg --out aligned.png [--output_size 1024]

``detect_landmarks`` (align_faces.py:26-58) finds the faces with MTCNN, takes the BEST-SCORING one (find_direction's
variant takes the first), crops it on crop_face's PIL path, runs the MobileNet-GDConv regressor and returns the 68 points
as integer pixel coordinates.  ``align_face`` (:61-160) is the FFHQ recipe: an oriented square around the eyes and the
mouth, an optional pre-shrink, a crop, a reflect-pad with a blurred and median-faded border where the square leaves the
image, a QUAD warp to transform_size and a LANCZOS reduction to output_size (the reference's ``Image.ANTIALIAS`` is
``Image.LANCZOS`` on current Pillow).  The detector and the regressor run on the gfx950 kernels (mtcnn_hip,
mobilenet_hip); align_face is host code (numpy / PIL / scipy.ndimage), pinned to the reference by
tests/golden/landmarks.npz in one case that pads and one that does not.
"""
import math
import os

import numpy as np
import torch
from PIL import Image

from . import utils
from .MTCNN import detect_faces
from .warp_images import crop_face

DEFAULT_CHECKPOINT = "mobilenet_224_model_best_gdconv_external.pth.tar"
DEFAULT_MTCNN = "MTCNN/weights"


def load_model(device, checkpoint=DEFAULT_CHECKPOINT, input_size=224):
    """(regressor, mean, std): the MobileNet-GDConv executor with a checkpoint's weights ('synthetic': the seeded net)
    and the normalisation constants (align_faces.py:17-23)."""
    from . import mobilenet_facial, mobilenet_hip
    sd = None if checkpoint == "synthetic" else mobilenet_facial.load_checkpoint(checkpoint)
    mean, std = utils.get_mean_std(device)
    return mobilenet_hip.build_mobilenet(sd, device=device, input_size=input_size), mean, std


def detect_landmarks(img, model, device, mean, std, mtcnn=None, out_size=224, **detect_kwargs):
    """68 integer landmarks [68, 2] of the best-scoring face of one [H, W, 3] uint8 numpy image, or None without a face.
    mtcnn: the detector's nets (MTCNN.detector.default_nets when None); detect_kwargs go to detect_faces."""
    faces, _ = detect_faces(torch.from_numpy(img.copy()), device=device, nets=mtcnn, **detect_kwargs)
    if not len(faces):
        return None
    best = faces[np.argmax(faces[:, 4])]
    cropped, side, box = crop_face(Image.fromarray(img), [best], out_size)
    pixels = torch.from_numpy(np.array(cropped)).to(device, torch.float32).permute(2, 0, 1)[None]
    batch = (pixels / 255 - mean[None]) / std[None]
    with torch.no_grad():
        points = model(batch.contiguous()).reshape(-1, 2)          # fractions of the crop's side
    origin = torch.tensor(box[:2], device=points.device, dtype=points.dtype)
    return (points * side + origin).cpu().numpy().astype(int)


def _quarter_turn(v):
    """v turned by 90 degrees: (a, b) -> (-b, a)."""
    return np.array([-v[1], v[0]])


def _length(v):
    return np.hypot(v[0], v[1])


def _square(centre, x, y):
    """Corners of the oriented square with half-axes x and y, in the order PIL's QUAD transform reads them
    (upper left, lower left, lower right, upper right)."""
    return np.stack([centre + sx * x + sy * y for sx, sy in ((-1, -1), (-1, 1), (1, 1), (1, -1))])


def _face_frame(landmarks, rotate_level):
    """(centre, half-axis x, half-axis y) of the FFHQ crop square (align_faces.py:64-95).  The square is sized by the
    larger of twice the eye distance and 1.8 x the eye-to-mouth distance, centred a tenth of the way from the eyes to
    the mouth; with rotate_level its x axis follows the eye line, corrected by the eye-to-mouth normal, otherwise it
    is the image's."""
    pts = landmarks.copy()
    left_eye, right_eye = pts[36:42].mean(axis=0), pts[42:48].mean(axis=0)   # six points around each eye
    eyes = (left_eye + right_eye) * 0.5
    across = right_eye - left_eye
    down = (pts[48] + pts[54]) * 0.5 - eyes                                  # to the middle of the mouth's corners
    half = max(_length(across) * 2.0, _length(down) * 1.8)
    if rotate_level:
        x = across - _quarter_turn(down)
        x = x / _length(x) * half
    else:
        x = np.array([1.0, 0.0]) * half
    return eyes + down * 0.1, x, _quarter_turn(x)


def _bounds(quad):
    """(left, top, right, bottom) of the quadrilateral in whole pixels, rounded outwards."""
    lo, hi = quad.min(axis=0), quad.max(axis=0)
    return math.floor(lo[0]), math.floor(lo[1]), math.ceil(hi[0]), math.ceil(hi[1])


def _shifted_square(centre, x, y, random_shift, retry_crops, width, height):
    """The square moved by a normal draw of std random_shift x its side (align_faces.py:103-118); with retry_crops up to
    1000 draws until it lies inside the image, None if none does."""
    side = _length(x) * 2
    for _ in range(1000):
        quad = _square(centre + side * random_shift * np.random.normal(0, 1, centre.shape), x, y)
        left, top, right, bottom = _bounds(quad)
        if not retry_crops or (left >= 0 and top >= 0 and right < width and bottom < height):
            return quad
    return None


def _reflect_pad_and_fade(img, margins, side):
    """The image grown by `margins` (left, top, right, bottom) with its mirror image, the new border blurred and faded
    into the picture's median colour (align_faces.py:143-153): the further into the padding, the more blur and the more
    median.  Returns the padded uint8 RGB image."""
    import scipy.ndimage
    left, top, right, bottom = margins
    arr = np.pad(np.float32(img), ((top, bottom), (left, right), (0, 0)), "reflect")
    h, w = arr.shape[:2]
    cols, rows = np.arange(w), np.arange(h)
    # 0 at the padded image's edge, 1 where the padding ends, per axis; depth = 1 at the edge, <= 0 inside the picture
    near_x = np.minimum(np.float32(cols) / left, np.float32(w - 1 - cols) / right)
    near_y = np.minimum(np.float32(rows) / top, np.float32(h - 1 - rows) / bottom)
    depth = np.maximum(1.0 - near_x[None, :, None], 1.0 - near_y[:, None, None])
    sigma = side * 0.02
    for target, weight in ((lambda a: scipy.ndimage.gaussian_filter(a, [sigma, sigma, 0]), depth * 3.0 + 1.0),
                           (lambda a: np.median(a, axis=(0, 1)), depth)):
        arr += (target(arr) - arr) * np.clip(weight, 0.0, 1.0)
    return Image.fromarray(np.clip(np.rint(arr), 0, 255).astype(np.uint8), "RGB")


def align_face(image, landmarks, output_size=1024, transform_size=4096, enable_padding=True, rotate_level=True,
               random_shift=0.0, retry_crops=False):
    """image [H, W, 3] uint8, landmarks [68, 2] -> the aligned PIL image (output_size square), or None when
    retry_crops rejected 1000 shifted crops.  Signature of the reference's align_face (align_faces.py:61-62)."""
    centre, x, y = _face_frame(landmarks, rotate_level)
    img = Image.fromarray(image)
    quad, side = _square(centre, x, y), _length(x) * 2
    if random_shift != 0:
        quad = _shifted_square(centre, x, y, random_shift, retry_crops, img.width, img.height)
        if quad is None:
            print("rejected image")
            return None

    # a face much larger than the output: reduce the photograph by a whole factor first (LANCZOS), so that the warp
    # below samples it near its own scale
    factor = int(side / output_size // 2)
    if factor > 1:
        img = img.resize((round(img.width / factor), round(img.height / factor)), Image.LANCZOS)
        quad, side = quad / factor, side / factor

    # keep the square and a border of a tenth of its side (3 px at least); drop the rest of the photograph
    border = max(round(side * 0.1), 3)
    left, top, right, bottom = _bounds(quad)
    window = (max(left - border, 0), max(top - border, 0), min(right + border, img.width), min(bottom + border, img.height))
    if window[2] - window[0] < img.width or window[3] - window[1] < img.height:
        img = img.crop(window)
        quad = quad - window[:2]

    # where square + border leave the picture, grow it (by 0.3 of the side at least)
    left, top, right, bottom = _bounds(quad)
    missing = (max(border - left, 0), max(border - top, 0), max(right - img.width + border, 0),
               max(bottom - img.height + border, 0))
    if enable_padding and max(missing) > border - 4:
        margins = np.maximum(missing, round(side * 0.3))
        img = _reflect_pad_and_fade(img, margins, side)
        quad = quad + margins[:2]

    img = img.transform((transform_size, transform_size), Image.QUAD, (quad + 0.5).ravel(), Image.BILINEAR)
    return img.resize((output_size, output_size), Image.LANCZOS) if output_size < transform_size else img


def align_image(image, device="cuda", checkpoint=DEFAULT_CHECKPOINT, mtcnn_weights=DEFAULT_MTCNN, output_size=1024,
                transform_size=4096, **detect_kwargs):
    """PIL photograph -> aligned PIL image: detector, regressor, align_face.  Raises when no face is found."""
    from . import mtcnn_hip
    for what, path, ok in (("regressor checkpoint", checkpoint, os.path.isfile(checkpoint)),
                           ("MTCNN weights", mtcnn_weights, os.path.isdir(mtcnn_weights))):
        if path != "synthetic" and not ok:
            raise SystemExit(f"{what} not found: {path} (or pass 'synthetic' for the seeded net)")
    model, mean, std = load_model(device, checkpoint)
    nets = mtcnn_hip.build_mtcnn(mtcnn_weights, device=device)
    pixels = np.asarray(image.convert("RGB"), dtype=np.uint8)
    landmarks = detect_landmarks(pixels, model, device, mean, std, mtcnn=nets, **detect_kwargs)
    if landmarks is None:
        raise SystemExit("no face found in the image")
    return align_face(pixels, landmarks, output_size=output_size, transform_size=transform_size)


def _cli():
    import click

    @click.command(help="Detect the face of a photograph (MTCNN), its 68 landmarks (MobileNet-GDConv) and write the "
                        "FFHQ-aligned crop that encoder4editing.infer expects.")
    @click.option("--input_image", type=str, required=True)
    @click.option("--out", type=str, required=True, help="aligned image to write (any format PIL writes)")
    @click.option("--output_size", type=int, default=1024, show_default=True)
    @click.option("--transform_size", type=int, default=4096, show_default=True)
    @click.option("--mobilenet_checkpoint", type=str, default=DEFAULT_CHECKPOINT, show_default=True,
                  help="landmark regressor checkpoint, or 'synthetic'")
    @click.option("--mtcnn_weights", type=str, default=DEFAULT_MTCNN, show_default=True,
                  help="directory with pnet.npy / rnet.npy / onet.npy, or 'synthetic'")
    def main(input_image, out, output_size, transform_size, mobilenet_checkpoint, mtcnn_weights):
        if not os.path.exists(input_image):
            raise SystemExit(f"input image not found: {input_image}")
        aligned = align_image(Image.open(input_image), checkpoint=mobilenet_checkpoint, mtcnn_weights=mtcnn_weights,
                              output_size=output_size, transform_size=transform_size)
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        aligned.save(out)
        print(f"wrote {out}: {aligned.size[0]} x {aligned.size[1]}")

    return main


if __name__ == "__main__":
    _cli()()
