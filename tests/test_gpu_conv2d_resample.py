"""The HIP conv2d_resample / conv2d_gradfix ops against the reference's golden vectors and the fp64 oracle.

Tolerances, relative to the reference tensor's max magnitude: 2e-5 for a forward that is one exact-fp32 direct conv
(the project's bound for that GEMM), 3e-5 where an FIR precedes or follows it (that bound plus the FIR's own 1e-5),
1e-4 for gradients (the project's backward bound).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN_CASES = ["up2_grouped_noflip", "same3x3_grouped", "conv1x1", "up2_plain", "down2", "up2_1x1"]
TOL_CONV, TOL_RESAMPLED, TOL_GRAD = 2e-5, 3e-5, 1e-4


def t(a, dev="cpu"):
    return torch.from_numpy(np.asarray(a)).to(dev)


def close(a, b, tol, what=""):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu() if torch.is_tensor(b) else torch.from_numpy(np.asarray(b)).double()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} != {tuple(b.shape)}"
    scale = max(b.abs().max().item(), 1e-12)
    err = (a - b).abs().max().item()
    assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol:.1e} * {scale:.3e}"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stylemc_amd import build
    build.build(verbose=False)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False


def _golden_case(g, case):
    up, down, pad, groups, flip = [int(v) for v in g[f"{case}/meta"]]
    kw = dict(up=up, down=down, padding=pad, groups=groups, flip_weight=bool(flip))
    return kw, TOL_CONV if up == 1 and down == 1 else TOL_RESAMPLED


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_golden(golden, case):
    from stylemc_amd.torch_utils.ops import conv2d_resample
    g = golden("ops_conv2d_resample.npz")
    kw, tol = _golden_case(g, case)
    x = t(g[f"{case}/x"], DEV).requires_grad_(True)
    y = conv2d_resample.conv2d_resample(x, t(g[f"{case}/w"], DEV), f=t(g["f4"], DEV), **kw)
    close(y, g[f"{case}/y"], tol, f"{case} y")
    (dx,) = torch.autograd.grad(y, x, t(g[f"{case}/dy"], DEV))
    close(dx, g[f"{case}/dx"], tol, f"{case} dx")


def _oracle64(x, w, f, dy, **kw):
    """y, dx, dw of oracle.ops.conv2d_resample on the CPU in float64."""
    from oracle import ops as O
    x = x.detach().double().cpu().requires_grad_(True)
    w = w.detach().double().cpu().requires_grad_(True)
    y = O.conv2d_resample(x, w, f=None if f is None else f.double().cpu(), **kw)
    dx, dw = torch.autograd.grad(y, [x, w], dy.double().cpu())
    return y.detach(), dx, dw


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_weight_gradient(golden, case, monkeypatch):
    from stylemc_amd import _hip
    from stylemc_amd.torch_utils.ops import conv2d_gradfix, conv2d_resample
    g = golden("ops_conv2d_resample.npz")
    kw, _ = _golden_case(g, case)
    x, f, dy = t(g[f"{case}/x"], DEV), t(g["f4"], DEV), t(g[f"{case}/dy"], DEV)
    w = t(g[f"{case}/w"], DEV).requires_grad_(True)
    y = conv2d_resample.conv2d_resample(x, w, f=f, **kw)
    (dw,) = torch.autograd.grad(y, w, dy)
    _, _, dw_ref = _oracle64(x, w, f, dy, **kw)
    close(dw, dw_ref, TOL_GRAD, f"{case} dw")
    # no_weight_gradients(): the weight gets no gradient and the weight-gradient kernel is not called.  The launches
    # are counted at the module's one call site (one per group): that is the check that can fail.  The split record is
    # per thread and a GPU backward runs on autograd's device thread, so the `== before` assertion at the end, read
    # from this thread, cannot fail; it is kept as a statement of the contract only.
    lib = _hip.load()
    calls = []
    monkeypatch.setattr(conv2d_gradfix, "_wgrad", lambda *a, _f=conv2d_gradfix._wgrad: calls.append(1) or _f(*a))
    (dw2,) = torch.autograd.grad(conv2d_resample.conv2d_resample(x, w, f=f, **kw), w, dy)
    assert len(calls) == kw["groups"] and torch.equal(dw2, dw)
    before = lib.smc_conv_wgrad_last_nsplit()
    xg = x.clone().requires_grad_(True)
    with conv2d_gradfix.no_weight_gradients():
        y = conv2d_resample.conv2d_resample(xg, w, f=f, **kw)
        dx, dw_none = torch.autograd.grad(y, [xg, w], dy, allow_unused=True)
    assert dw_none is None and dx is not None
    assert len(calls) == kw["groups"], "the weight-gradient kernel ran under no_weight_gradients()"
    assert lib.smc_conv_wgrad_last_nsplit() == before


@pytest.mark.parametrize("shape", ["conv1_64to64_32px", "conv0_up2_64to32_16px"])
def test_synthesis_widths(shape):
    """Synthesis-layer widths: no channel padding on any launch, forward and both gradients against fp64."""
    from stylemc_amd.torch_utils.ops import conv2d_gradfix, conv2d_resample, upfirdn2d
    gen = torch.Generator().manual_seed(11)
    if shape == "conv1_64to64_32px":
        x = torch.randn(2, 64, 32, 32, generator=gen)
        w = torch.randn(64, 64, 3, 3, generator=gen) / 24
        f, kw, tol = None, dict(up=1, padding=1), TOL_CONV
    else:
        x = torch.randn(2, 64, 16, 16, generator=gen)
        w = torch.randn(32, 64, 3, 3, generator=gen) / 24
        f, kw, tol = upfirdn2d.setup_filter([1, 3, 3, 1]), dict(up=2, padding=1, flip_weight=False), TOL_RESAMPLED
    xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    pads = conv2d_gradfix.channel_pad_count
    y = conv2d_resample.conv2d_resample(xg, wg, f=None if f is None else f.to(DEV), **kw)
    dy = torch.randn(y.shape, generator=gen)
    dx, dw = torch.autograd.grad(y, [xg, wg], dy.to(DEV))
    assert conv2d_gradfix.channel_pad_count == pads, "a synthesis width was channel-padded"
    y_ref, dx_ref, dw_ref = _oracle64(x, w, f, dy, **kw)
    close(y, y_ref, tol, f"{shape} y")
    close(dx, dx_ref, TOL_GRAD, f"{shape} dx")
    close(dw, dw_ref, TOL_GRAD, f"{shape} dw")


def test_gradfix_direct():
    from stylemc_amd.torch_utils.ops import conv2d_gradfix
    gen = torch.Generator().manual_seed(5)
    # conv2d, stride 2, padding 1, bias
    x = torch.randn(2, 16, 8, 8, generator=gen)
    w = torch.randn(32, 16, 3, 3, generator=gen) / 12
    b = torch.randn(32, generator=gen)
    leaves = [v.to(DEV).requires_grad_(True) for v in (x, w, b)]
    y = conv2d_gradfix.conv2d(*leaves, stride=2, padding=1)
    ref = [v.double().requires_grad_(True) for v in (x, w, b)]
    y_ref = F.conv2d(*ref, stride=2, padding=1)
    dy = torch.randn(y_ref.shape, generator=gen)
    close(y, y_ref, TOL_CONV, "conv2d y")
    for name, a, r in zip(("dx", "dw", "db"), torch.autograd.grad(y, leaves, dy.to(DEV)),
                          torch.autograd.grad(y_ref, ref, dy.double())):
        close(a, r, TOL_GRAD, f"conv2d {name}")
    # conv_transpose2d, stride 2, padding 0
    x = torch.randn(2, 16, 5, 4, generator=gen)
    w = torch.randn(16, 32, 3, 3, generator=gen) / 12
    leaves = [v.to(DEV).requires_grad_(True) for v in (x, w)]
    y = conv2d_gradfix.conv_transpose2d(*leaves, stride=2)
    ref = [v.double().requires_grad_(True) for v in (x, w)]
    y_ref = F.conv_transpose2d(*ref, stride=2)
    dy = torch.randn(y_ref.shape, generator=gen)
    close(y, y_ref, TOL_CONV, "conv_transpose2d y")
    for name, a, r in zip(("dx", "dw"), torch.autograd.grad(y, leaves, dy.to(DEV)),
                          torch.autograd.grad(y_ref, ref, dy.double())):
        close(a, r, TOL_GRAD, f"conv_transpose2d {name}")
    # no kernel: refused, not approximated
    with pytest.raises(NotImplementedError):
        conv2d_gradfix.conv_transpose2d(*leaves, stride=1)


def test_fused_modconv_pattern():
    """The upstream fused modulated conv -- per-sample weights W * s * d, batch folded into groups -- through the new
    op equals modconv.modulated_conv2d: the operator-level and the module-level drop-in agree."""
    from stylemc_amd import modconv
    from stylemc_amd.torch_utils.ops import conv2d_resample
    gen = torch.Generator().manual_seed(9)
    n, cin, cout, r = 2, 32, 32, 16
    x = torch.randn(n, cin, r, r, generator=gen).to(DEV)
    W = (torch.randn(cout, cin, 3, 3, generator=gen) / 17).to(DEV)
    s = (torch.randn(n, cin, generator=gen) + 1).to(DEV)
    ws = W[None] * s[:, None, :, None, None]                                  # [n, O, I, 3, 3]
    d = (ws.square().sum(dim=[2, 3, 4]) + 1e-8).rsqrt()                       # [n, O]
    ws = ws * d[:, :, None, None, None]
    y = conv2d_resample.conv2d_resample(x.reshape(1, n * cin, r, r), ws.reshape(n * cout, cin, 3, 3), padding=1,
                                        groups=n, flip_weight=True).reshape(n, cout, r, r)
    y_mod = modconv.modulated_conv2d(x, W, s, padding=1, demodulate=True)
    close(y, y_mod, TOL_CONV, "fused-form op vs modulated_conv2d")
