"""Host logic of the weight-gradient entry points and the two op modules built on them (no GPU)."""
import ctypes

import pytest
import torch

from stylemc_amd import _hip

FAKE = ctypes.c_void_p(256)


def wgrad(lib, n, cin, cout, in_h, in_w, out_h, out_w, k, stride, pad, ws=None, ws_bytes=0):
    return lib.smc_conv_wgrad_f32(FAKE, n, cin, in_h, in_w, FAKE, cout, out_h, out_w, k, k, stride, pad, pad, FAKE,
                                  ws, ws_bytes, None)


def test_symbols_load():
    lib = _hip.load()
    for name in ("smc_conv_wgrad_workspace_size", "smc_conv_wgrad_f32", "smc_conv_wgrad_last_nsplit"):
        assert hasattr(lib, name), name
        assert name in _hip.exported_symbols()
    assert lib.smc_conv_wgrad_last_nsplit() >= 0


@pytest.mark.parametrize("what,args,word", [
    ("5x5 kernel", (1, 4, 4, 8, 8, 4, 4, 5, 1, 0), b"kernel"),
    ("stride 3", (1, 4, 4, 9, 9, 3, 3, 3, 3, 0), b"stride"),
    ("out_h inconsistent", (1, 4, 4, 8, 8, 7, 8, 3, 1, 1), b"inconsistent"),
    ("input of exactly 2^31 bytes", (1, 512, 4, 1024, 1024, 1024, 1024, 3, 1, 1), b"2 GiB"),
    ("pad 3", (1, 4, 4, 8, 8, 12, 12, 3, 1, 3), b"padding"),
])
def test_validation_fails_before_any_launch(what, args, word):
    """Fake non-null pointers: a call that reached a launch would fault, host-side validation returns 1."""
    lib = _hip.load()
    before = lib.smc_conv_wgrad_last_nsplit()
    assert wgrad(lib, *args) == 1, what
    assert word in lib.smc_last_error(), (what, lib.smc_last_error())
    assert lib.smc_conv_wgrad_last_nsplit() == before


def test_workspace_query_and_check():
    lib = _hip.load()
    # one 32 x 32 tile over K = 4096: the planner splits, so the query is a whole number of partial dw blocks
    nb = lib.smc_conv_wgrad_workspace_size(4, 32, 32, 32, 32, 32, 32, 3, 3, 1)
    assert nb > 0 and nb % (32 * 32 * 9 * 4) == 0
    assert wgrad(lib, 4, 32, 32, 32, 32, 32, 32, 3, 1, 1, FAKE, nb - 4) == 1
    assert b"workspace" in lib.smc_last_error()
    assert wgrad(lib, 4, 32, 32, 32, 32, 32, 32, 3, 1, 1, None, 0) == 1
    assert b"workspace" in lib.smc_last_error()
    # degenerate and unsupported sizes: no workspace
    assert lib.smc_conv_wgrad_workspace_size(0, 32, 32, 32, 32, 32, 32, 3, 3, 1) == 0
    assert lib.smc_conv_wgrad_workspace_size(4, 32, 32, 32, 32, 32, 32, 5, 5, 1) == 0
    # K too short to split: none either
    assert lib.smc_conv_wgrad_workspace_size(2, 4, 5, 7, 7, 7, 7, 3, 3, 1) == 0


def test_ops_reject_cpu_tensors_and_dilation():
    from stylemc_amd.torch_utils.ops import conv2d_gradfix, conv2d_resample
    x, w = torch.zeros(1, 4, 8, 8), torch.zeros(4, 4, 3, 3)
    with pytest.raises(RuntimeError):
        conv2d_gradfix.conv2d(x, w, padding=1)
    with pytest.raises(RuntimeError):
        conv2d_gradfix.conv_transpose2d(x, w, stride=2)
    with pytest.raises(RuntimeError):
        conv2d_resample.conv2d_resample(x, w, padding=1)
    # the checks that need no tensor data come first: dilation is refused whatever the device
    for dev in ("cpu", "meta"):
        with pytest.raises(NotImplementedError, match="dilation"):
            conv2d_gradfix.conv2d(x.to(dev), w.to(dev), padding=1, dilation=2)
        with pytest.raises(NotImplementedError, match="dilation"):
            conv2d_gradfix.conv_transpose2d(x.to(dev), w.to(dev), stride=2, dilation=2)
    with pytest.raises(NotImplementedError):
        conv2d_resample.conv2d_resample(x, w, up=4)


def test_no_weight_gradients_flag_restores():
    from stylemc_amd.torch_utils.ops import conv2d_gradfix
    assert conv2d_gradfix.enabled and not conv2d_gradfix.weight_gradients_disabled
    with conv2d_gradfix.no_weight_gradients():
        assert conv2d_gradfix.weight_gradients_disabled
        with conv2d_gradfix.no_weight_gradients():
            assert conv2d_gradfix.weight_gradients_disabled
        assert conv2d_gradfix.weight_gradients_disabled
    assert not conv2d_gradfix.weight_gradients_disabled


def test_enabled_false_raises(monkeypatch):
    """The reference's `enabled = False` selects the stock torch ops; there is no such path here, so it raises."""
    from stylemc_amd.torch_utils.ops import conv2d_gradfix
    monkeypatch.setattr(conv2d_gradfix, "enabled", False)
    x, w = torch.zeros(1, 4, 8, 8, device="meta"), torch.zeros(4, 4, 3, 3, device="meta")
    with pytest.raises(RuntimeError, match="enabled"):
        conv2d_gradfix.conv2d(x, w, padding=1)
    with pytest.raises(RuntimeError, match="enabled"):
        conv2d_gradfix.conv_transpose2d(x, w, stride=2)
