"""Face-landmark kernels on the GPU (csrc/landmarks.hip) and the MobileNet-GDConv executor built on them.

  smc_dwconv_f32              against fp64 F.conv2d(groups=C) + affine + ReLU6, bound per output
                              (k*k + 4) * 2^-24 * (|scale| * sum|w||x| + |shift|): k*k products and k*k - 1 additions of
                              one chain in any order, plus the fma of the affine (ReLU6 is 1-Lipschitz); two runs bit-equal
  smc_maxpool2d_f32           bit-equal to F.max_pool2d(ceil_mode=True)
  smc_crop_bilinear_norm_f32  against fp32 CPU F.interpolate of the denormed crop, then the normalise; bound in 0..255
                              units 4 * 2^-24 * Smax * D + 8 * 2^-24 * 255 (Smax: largest source coordinate, D: largest
                              neighbour difference in the crop -- the rounding of the interpolation weight times what it
                              multiplies -- plus a few roundings of values up to 255), divided by 255 * std_c
  HipMobileNetGDConv          against the fp64 run of the mobilenet_facial module; allowed 4 x e_ref, e_ref the error of
                              the same module run in fp32 on the CPU against fp64 (summation order and the MFMA's
                              accumulation differ).  Measured on an MI355X (profiles/landmarks/README.md):
                                _56 net, n = 2:  e_ref 2.94e-06, HIP 2.30e-06 (max|y| 2.3)
                                224 net, n = 1:  e_ref 6.60e-06, HIP 3.89e-06 (max|y| 3.6)
"""
import pytest
import torch
import torch.nn.functional as F

from stylemc_amd import _hip, mobilenet_facial, mobilenet_hip, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ depthwise

def _dw_case(n, C, h, w, k, stride, pad, act, affine, seed):
    """Returns (worst err / bound, runs bit-equal)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, h, w, generator=g)
    wt = torch.randn(C, k, k, generator=g) / k
    scale = torch.randn(C, generator=g) + 1.5 if affine else None
    shift = torch.randn(C, generator=g) * 2 if affine else None
    xd, wd = x.to(DEV), wt.to(DEV)
    sd, hd = (scale.to(DEV), shift.to(DEV)) if affine else (None, None)
    ys = [mobilenet_hip.dwconv(xd, wd, stride, pad, sd, hd, act) for _ in range(2)]
    torch.cuda.synchronize()
    s64 = scale.double().view(1, C, 1, 1) if affine else torch.ones(1, C, 1, 1, dtype=torch.float64)
    h64 = shift.double().view(1, C, 1, 1) if affine else torch.zeros(1, C, 1, 1, dtype=torch.float64)
    conv = F.conv2d(x.double(), wt.double().unsqueeze(1), stride=stride, padding=pad, groups=C)
    ref = conv * s64 + h64
    if act == _hip.DW_ACT_RELU6:
        ref = ref.clamp(0.0, 6.0)
    mag = F.conv2d(x.double().abs(), wt.double().abs().unsqueeze(1), stride=stride, padding=pad, groups=C)
    bound = (k * k + 4) * EPS * (s64.abs() * mag + h64.abs())
    y = ys[0].double().cpu()
    assert y.shape == ref.shape, (y.shape, ref.shape)
    assert torch.isfinite(y).all()
    ratio = ((y - ref).abs() / bound.clamp_min(1e-300)).max().item()
    return ratio, torch.equal(ys[0], ys[1])


# 9x11: odd, stride 2 drops a column; 17x5: one strip and a quarter; 8x12 and 16x8: the 16-byte paths at stride 1
# (w % 4 == 0) and stride 2 (w % 8 == 0); 14x14 at C = 960, n = 3 walks two output rows per thread
DW_PLANES = [(1, 1), (7, 7), (9, 11), (14, 14), (17, 5), (8, 12), (16, 8)]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("plane", DW_PLANES, ids=lambda p: f"{p[0]}x{p[1]}")
def test_dwconv_3x3_against_fp64(plane, stride):
    h, w = plane
    worst, seed = 0.0, 0
    for C in (1, 3, 33, 960):
        for n in (1, 3):
            for act in (_hip.DW_ACT_LINEAR, _hip.DW_ACT_RELU6):
                for affine in (False, True):
                    seed += 1
                    ratio, same = _dw_case(n, C, h, w, 3, stride, 1, act, affine, seed)
                    assert same, (n, C, h, w, stride, act, affine)
                    assert ratio <= 1.0, (ratio, n, C, h, w, stride, act, affine)
                    worst = max(worst, ratio)
    print(f"dwconv 3x3 {h}x{w} stride {stride}: worst err / bound = {worst:.3f}")


@pytest.mark.parametrize("stride", [1, 2])
def test_dwconv_3x3_long_row_walk(stride):
    """960 channels x 3 images of 28 x 28: enough work items that a thread walks 8 output rows (stride 1: 28 = 3 * 8 + 4,
    a short last segment) with its rolling three-row window."""
    ratio, same = _dw_case(3, 960, 28, 28, 3, stride, 1, _hip.DW_ACT_RELU6, True, 77 + stride)
    print(f"dwconv 3x3 28x28 C 960 n 3 stride {stride}: err / bound = {ratio:.3f}")
    assert same and ratio <= 1.0, ratio


@pytest.mark.parametrize("k", [2, 7])
def test_dwconv_global_against_fp64(k):
    worst, seed = 0.0, 100
    for C in (1, 3, 33, 960):
        for n in (1, 3):
            for act in (_hip.DW_ACT_LINEAR, _hip.DW_ACT_RELU6):
                for affine in (False, True):
                    seed += 1
                    ratio, same = _dw_case(n, C, k, k, k, 1, 0, act, affine, seed)
                    assert same, (n, C, k, act, affine)
                    assert ratio <= 1.0, (ratio, n, C, k, act, affine)
                    worst = max(worst, ratio)
    print(f"dwconv global k {k}: worst err / bound = {worst:.3f}")


def test_dwconv_unaligned_views_take_the_scalar_path():
    """An x that is 4 bytes off 16-byte alignment (a view into a larger buffer) gives the same bits as the aligned copy."""
    g = torch.Generator().manual_seed(5)
    buf = torch.randn(2 * 8 * 8 * 8 + 1, generator=g).to(DEV)
    x_off = buf[1:].view(2, 8, 8, 8)
    assert x_off.data_ptr() % 16 == 4
    wt = torch.randn(8, 3, 3, generator=g).to(DEV)
    for stride in (1, 2):
        a = mobilenet_hip.dwconv(x_off, wt, stride, 1)
        b = mobilenet_hip.dwconv(x_off.clone(), wt, stride, 1)
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ max-pool

@pytest.mark.parametrize("k,h,w", [(2, 5, 5), (2, 4, 7), (3, 10, 11), (3, 4, 4), (3, 3, 3)])
def test_maxpool_bit_equal_to_torch(k, h, w):
    g = torch.Generator().manual_seed(k * 100 + h * 10 + w)
    x = torch.randn(2, 3, h, w, generator=g)
    ref = F.max_pool2d(x, k, 2, ceil_mode=True)
    y = mobilenet_hip.maxpool2d(x.to(DEV), k).cpu()
    assert y.shape == ref.shape, (y.shape, ref.shape)
    assert torch.equal(y, ref)
    neg = -x.abs() - 1.0   # all negative: a clipped window must not see an implicit 0
    assert torch.equal(mobilenet_hip.maxpool2d(neg.to(DEV), k).cpu(), F.max_pool2d(neg, k, 2, ceil_mode=True))


def test_maxpool_propagates_nan_as_torch_does():
    x = torch.randn(1, 2, 7, 7, generator=torch.Generator().manual_seed(3))
    x[0, 0, 2, 3] = float("nan")      # inside windows
    x[0, 1, 6, 6] = float("nan")      # the clipped corner window's last element
    x[0, 1, 0, 0] = float("nan")      # a window's first element
    for k in (2, 3):
        ref = F.max_pool2d(x, k, 2, ceil_mode=True)
        y = mobilenet_hip.maxpool2d(x.to(DEV), k).cpu()
        assert torch.isnan(ref).any() and torch.equal(torch.isnan(y), torch.isnan(ref))
        assert torch.equal(torch.nan_to_num(y, nan=0.0), torch.nan_to_num(ref, nan=0.0))


# ------------------------------------------------------------------------------------------------ crop + resize

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
IMG_H, IMG_W = 40, 52
# (x1, y1, x2, y2), exclusive ends, inside the 52 x 40 image
CROP_BOXES = {
    "interior": (10, 8, 34, 32), "left_top": (0, 0, 20, 20), "right": (30, 5, 52, 27), "bottom": (12, 18, 34, 40),
    "whole": (0, 0, 52, 40), "one_px_wide": (17, 3, 18, 30), "one_px_high": (5, 21, 45, 22), "one_px": (51, 39, 52, 40),
    "small": (20, 20, 25, 24),
}


@pytest.fixture(scope="module")
def crop_image():
    g = torch.Generator().manual_seed(11)
    return torch.randn(len(CROP_BOXES), 3, IMG_H, IMG_W, generator=g) * 0.7   # beyond [-1, 1] in places: the clamp acts


@pytest.mark.parametrize("S", [8, 224])
def test_crop_bilinear_norm_against_torch(crop_image, S):
    names = sorted(CROP_BOXES)
    boxes = torch.tensor([CROP_BOXES[k] for k in names], dtype=torch.int32)
    got = mobilenet_hip.crop_bilinear_norm(crop_image.to(DEV), boxes.to(DEV), S, MEAN, STD).cpu()
    assert got.shape == (len(names), 3, S, S) and torch.isfinite(got).all()
    mean, std = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    for i, name in enumerate(names):
        x1, y1, x2, y2 = CROP_BOXES[name]
        den = (crop_image[i:i + 1] * 127.5 + 128).clamp(0, 255)
        crop = den[:, :, y1:y2, x1:x2]
        ref = (F.interpolate(crop, size=(S, S), mode="bilinear", align_corners=False) / 255 - mean) / std
        smax = float(max(x2 - x1, y2 - y1))
        dx = (crop[..., :, 1:] - crop[..., :, :-1]).abs().max().item() if x2 - x1 > 1 else 0.0
        dy = (crop[..., 1:, :] - crop[..., :-1, :]).abs().max().item() if y2 - y1 > 1 else 0.0
        bound = (4 * EPS * smax * max(dx, dy) + 8 * EPS * 255) / (255 * std)
        ratio = ((got[i:i + 1] - ref).abs() / bound).max().item()
        print(f"crop {name} -> {S}: err / bound = {ratio:.3f}")
        assert ratio <= 1.0, (name, S, ratio)


def test_crop_clips_boxes_to_the_image(crop_image):
    """A box that leaves the image (the host clips them, warp_images.py:89-97) is clipped by the kernel too."""
    img = crop_image[:2].to(DEV)
    out = torch.tensor([[-7, -3, 60, 30], [40, 30, 90, 90]], dtype=torch.int32).to(DEV)
    clipped = torch.tensor([[0, 0, IMG_W, 30], [40, 30, IMG_W, IMG_H]], dtype=torch.int32).to(DEV)
    a = mobilenet_hip.crop_bilinear_norm(img, out, 8, MEAN, STD)
    b = mobilenet_hip.crop_bilinear_norm(img, clipped, 8, MEAN, STD)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ whole regressor

@pytest.mark.parametrize("size,n", [(56, 2), (224, 1)])
def test_mobilenet_gdconv_against_fp64(size, n):
    cls = mobilenet_facial.MobileNet_GDConv if size == 224 else mobilenet_facial.MobileNet_GDConv_56
    ref_net = cls(136).eval().requires_grad_(False)
    sd = synthetic.mobilenet_state_dict(ref_net, seed=7)
    ref_net.load_state_dict(sd)
    g = torch.Generator().manual_seed(size + n)
    x = torch.randn(n, 3, size, size, generator=g)
    with torch.no_grad():
        y32 = ref_net(x).double()
        y64 = ref_net.double()(x.double())
    e_ref = (y32 - y64).abs().max().item()
    net = mobilenet_hip.build_mobilenet(sd, device=DEV, input_size=size)
    ys = [net(x.to(DEV)) for _ in range(2)]
    assert ys[0].shape == (n, 136) and torch.equal(ys[0], ys[1])
    err = (ys[0].double().cpu() - y64).abs().max().item()
    print(f"MobileNet-GDConv {size} px n {n}: max|y| {y64.abs().max().item():.3f}, e_ref {e_ref:.2e}, HIP err {err:.2e}")
    assert e_ref > 0 and err <= 4 * e_ref, (err, e_ref)
