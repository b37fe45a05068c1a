"""Face landmarks, host side (CPU): the new C-ABI entry points reject bad arguments on the host before any launch (fake
non-null pointers: a call that reached a launch would fault; the pattern of test_e4e_cpu.py), and the restated
MobileNet-GDConv modules have the checkpoint layout the executor loads."""
import ctypes

import pytest
import torch

from stylemc_amd import _hip, mobilenet_facial, synthetic

FAKE = ctypes.c_void_p(256)


def test_new_entry_points_are_exported():
    lib = _hip.load()
    for name in ("smc_dwconv_f32", "smc_dwconv_supported", "smc_maxpool2d_f32", "smc_crop_bilinear_norm_f32"):
        assert hasattr(lib, name) and name in _hip.exported_symbols()
    assert lib.smc_abi_version() == 6


def _dw(lib, n=1, c=8, h=7, w=7, k=3, stride=1, pad=1, act=0, x=FAKE, wt=FAKE, y=FAKE):
    return lib.smc_dwconv_f32(x, n, c, h, w, wt, k, stride, pad, None, None, act, y, None)


@pytest.mark.parametrize("kwargs,word", [
    ({"k": 5}, b"k = 3"), ({"stride": 3}, b"stride"), ({"stride": 0}, b"stride"), ({"pad": 2}, b"pad"),
    ({"k": 7, "pad": 0, "h": 7, "w": 8}, b"k == in_h == in_w"), ({"k": 3, "pad": 0, "h": 7, "w": 7}, b"k == in_h == in_w"),
    ({"k": 9, "pad": 0, "h": 9, "w": 9}, b"2 <= k <= 8"), ({"k": 1, "pad": 0, "h": 1, "w": 1}, b"2 <= k <= 8"),
    ({"k": 7, "pad": 0, "stride": 2}, b"stride 1"), ({"n": 0}, b">= 1"), ({"c": 0}, b">= 1"), ({"h": 0}, b">= 1"),
    ({"n": 1 << 16, "c": 1 << 16}, b"planes"), ({"act": 2}, b"act"),
    ({"x": None}, b"null"), ({"wt": None}, b"null"), ({"y": None}, b"null"),
])
def test_dwconv_rejects_bad_arguments_on_the_host(kwargs, word):
    lib = _hip.load()
    assert _dw(lib, **kwargs) == 1, kwargs
    assert word in lib.smc_last_error(), (kwargs, lib.smc_last_error())


def test_dwconv_supported():
    lib = _hip.load()
    for args in ((1, 1, 1, 1, 3, 1, 1), (8, 960, 7, 7, 3, 1, 1), (3, 33, 9, 11, 3, 2, 1), (8, 1280, 7, 7, 7, 1, 0),
                 (2, 1280, 2, 2, 2, 1, 0)):
        assert lib.smc_dwconv_supported(*args) == 1, args
    for args in ((1, 8, 7, 7, 5, 1, 1), (1, 8, 7, 7, 3, 3, 1), (1, 8, 7, 8, 7, 1, 0), (1, 8, 9, 9, 9, 1, 0),
                 (1, 8, 7, 7, 3, 1, 2), (0, 8, 7, 7, 3, 1, 1)):
        assert lib.smc_dwconv_supported(*args) == 0, args


@pytest.mark.parametrize("args,word", [
    ((FAKE, 4, 8, 8, 4, 2, FAKE), b"(k, stride)"), ((FAKE, 4, 8, 8, 3, 1, FAKE), b"(k, stride)"),
    ((FAKE, 4, 8, 8, 2, 1, FAKE), b"(k, stride)"), ((FAKE, 0, 8, 8, 2, 2, FAKE), b"shape"),
    ((FAKE, 4, 2, 8, 3, 2, FAKE), b"shape"), ((FAKE, 1 << 32, 8, 8, 2, 2, FAKE), b"planes"),
    ((None, 4, 8, 8, 2, 2, FAKE), b"null"), ((FAKE, 4, 8, 8, 3, 2, None), b"null"),
])
def test_maxpool_rejects_bad_arguments_on_the_host(args, word):
    lib = _hip.load()
    assert lib.smc_maxpool2d_f32(*args, None) == 1, args
    assert word in lib.smc_last_error(), (args, lib.smc_last_error())


def test_crop_bilinear_norm_rejects_bad_arguments_on_the_host():
    lib = _hip.load()
    m3, s3, z3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.2, 0.2, 0.2), (ctypes.c_float * 3)(0.2, 0, 1)

    def crop(img=FAKE, n=1, h=16, w=16, boxes=FAKE, s=8, mean=m3, std=s3, out=FAKE):
        return lib.smc_crop_bilinear_norm_f32(img, n, h, w, boxes, s, 1, mean, std, out, None)

    for kwargs, word in (({"n": 0}, b"shape"), ({"s": 0}, b"shape"), ({"h": 0}, b"shape"), ({"w": 1 << 20}, b"32768"),
                         ({"img": None}, b"null"), ({"boxes": None}, b"null"), ({"out": None}, b"null"),
                         ({"mean": None}, b"null"), ({"std": None}, b"null"), ({"std": z3}, b"std[1]")):
        assert crop(**kwargs) == 1, kwargs
        assert word in lib.smc_last_error(), (kwargs, lib.smc_last_error())


def test_mobilenet_modules_have_the_checkpoint_layout():
    """mobilenet_facial.py:55-68 of the reference: base_net = Sequential(features), linear7 a depthwise conv over the whole
    plane, linear1 1280 -> 136; torchvision's nesting of the trunk (key-name parity with torchvision itself is unpinned)."""
    net = mobilenet_facial.MobileNet_GDConv(136)
    keys = list(net.state_dict().keys())
    for k in ("base_net.0.0.0.weight", "base_net.0.0.1.running_var", "base_net.0.1.conv.0.0.weight",
              "base_net.0.1.conv.1.weight", "base_net.0.1.conv.2.running_mean", "base_net.0.2.conv.0.0.weight",
              "base_net.0.2.conv.1.0.weight", "base_net.0.2.conv.2.weight", "base_net.0.2.conv.3.bias",
              "base_net.0.17.conv.3.weight", "base_net.0.18.0.weight", "base_net.0.18.1.num_batches_tracked",
              "linear7.conv.weight", "linear7.bn.running_mean", "linear1.conv.weight", "linear1.bn.bias"):
        assert k in keys, k
    sd = net.state_dict()
    assert tuple(sd["linear7.conv.weight"].shape) == (1280, 1, 7, 7)
    assert tuple(sd["linear1.conv.weight"].shape) == (136, 1280, 1, 1)
    assert tuple(sd["base_net.0.14.conv.1.0.weight"].shape) == (576, 1, 3, 3)      # a stride-2 depthwise layer
    assert net.base_net[0][14].conv[1][0].stride == (2, 2) and not net.base_net[0][14].use_res_connect
    assert net.base_net[0][3].use_res_connect and not net.base_net[0][2].use_res_connect
    assert len(net.base_net[0]) == 19
    assert tuple(mobilenet_facial.MobileNet_GDConv_56(136).state_dict()["linear7.conv.weight"].shape) == (1280, 1, 2, 2)
    n_params = sum(p.numel() for p in net.parameters())
    assert n_params == 2223872 + (1280 * 49 + 2 * 1280) + (136 * 1280 + 2 * 136), n_params  # MobileNetV2 features + heads


def test_mobilenet_output_shape_and_input_dependence():
    net = mobilenet_facial.MobileNet_GDConv_56(136).eval()
    net.load_state_dict(synthetic.mobilenet_state_dict(net, seed=7))
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        y = net(torch.randn(2, 3, 56, 56, generator=g))
    assert y.shape == (2, 136) and torch.isfinite(y).all()
    spread = (y[0] - y[1]).abs().max().item() / y.abs().max().item()
    print(f"max |y0 - y1| / max|y| = {spread:.3f}")
    assert spread > 0.05, spread   # the seeded net's output is driven by the image, not by its BatchNorm biases


def test_checkpoint_loader_reads_the_reference_layout(tmp_path):
    """find_direction.py:275-278: torch.load(...)['state_dict'] of a DataParallel(MobileNet_GDConv(136)): 'module.'
    prefixes, the trunk twice (pretrain_net.features.* and base_net.0.*) and pretrain_net's unused classifier."""
    net = mobilenet_facial.MobileNet_GDConv_56(136)
    sd = synthetic.mobilenet_state_dict(net, seed=3)
    saved = {"module." + k: v for k, v in sd.items()}
    saved.update({"module.pretrain_net.features." + k[len("base_net.0."):]: v for k, v in sd.items()
                  if k.startswith("base_net.0.")})
    saved["module.pretrain_net.classifier.1.weight"] = torch.zeros(1000, 1280)
    path = str(tmp_path / "ckpt.pth.tar")
    torch.save({"epoch": 3, "state_dict": saved}, path)
    got = mobilenet_facial.load_checkpoint(path)
    assert sorted(got) == sorted(sd)
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    net.load_state_dict(got, strict=True)
