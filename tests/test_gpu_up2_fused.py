"""The fused up=2 launch (smc_modconv_up2_f32: transposed conv + 4x4 FIR + modconv epilogue, T kept in LDS) against
the two-launch path it replaces (bit for bit), against an fp64 CPU reference, and its routing in modconv.

Shapes: the smallest at which the kernel can go wrong -- a plane smaller than one 7 x 18 super-pixel tile, planes that
are no tile multiple (tile restart per image), a non-square plane (row / column swap), 64 output channels (the
two-pass epilogue), several tiles both ways (seams on all four sides), and both store forms (y_w % 4 == 0 or not).
"""
import ctypes
import math

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda"

# n, cin, cout, h, w, epilogue variant
CASES = [
    (1, 16, 32, 5, 5, dict(noise="const", u=True, d=True, bias=True, act="lrelu", gain=math.sqrt(2), clamp=256.0)),
    (2, 64, 32, 33, 33, dict(noise="sample", u=False, d=False, bias=False, act="lrelu", gain=math.sqrt(2), clamp=1.0)),
    (3, 32, 64, 20, 37, dict(noise=None, u=True, d=True, bias=True, act="linear", gain=1.0, clamp=-1.0)),
    (1, 64, 64, 40, 40, dict(noise="const", u=False, d=True, bias=False, act="lrelu", gain=math.sqrt(2), clamp=256.0)),
    # 32 output channels with 16-B row stores (y_w % 4 == 0), saved u, per-sample noise (a plane of more than 9 cout
    # super-pixels: on smaller ones with h w % 4 == 0 the two-launch path scales x, not the weights)
    (2, 32, 32, 16, 18, dict(noise="sample", u=True, d=True, bias=True, act="lrelu", gain=math.sqrt(2), clamp=1.0)),
]
LINEAR = dict(noise="const", u=False, d=True, bias=True, act="linear", gain=1.0, clamp=-1.0)
IDS = [f"{n}x{ci}-{co}x{h}x{w}" for n, ci, co, h, w, _ in CASES]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stylemc_amd import _hip, build
    build.build(verbose=False)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return _hip.load()


_inputs = {}


def inputs(n, cin, cout, h, w):
    """The case's operands, made once (CPU tensors; shared by every test of the case and left unchanged)."""
    key = (n, cin, cout, h, w)
    if key not in _inputs:
        gen = torch.Generator().manual_seed(100 + cin + cout + h + w)
        _inputs[key] = dict(
            W=torch.randn(cout, cin, 3, 3, generator=gen), x=torch.randn(n, cin, h, w, generator=gen),
            s=torch.randn(n, cin, generator=gen) * 0.5 + 1, d=torch.rand(n, cout, generator=gen) * 0.1 + 0.02,
            bias=torch.randn(cout, generator=gen) * 0.3, strength=torch.tensor(0.7),
            noise_const=torch.randn(2 * h, 2 * w, generator=gen),
            noise_sample=torch.randn(n, 1, 2 * h, 2 * w, generator=gen))
    return _inputs[key]


def _epi(modconv, _hip, I, v, n, cout, h, w):
    """(MODACT epilogue, u tensor or None, tensors to keep alive) of variant v on the GPU."""
    nz = None if v["noise"] is None else I["noise_" + v["noise"]].to(DEV)
    nstride = 4 * h * w if v["noise"] == "sample" else 0
    u = torch.full((n, cout, 2 * h, 2 * w), float("nan"), device=DEV) if v["u"] else None
    d = I["d"].to(DEV) if v["d"] else None
    b = I["bias"].to(DEV) if v["bias"] else None
    st = I["strength"].to(DEV) if nz is not None else None
    epi = modconv._epilogue(_hip.EPI_MODACT, d, nz, nstride, st, b, v["act"], 0.2, v["gain"], v["clamp"], u)
    return epi, u, (nz, d, b, st)


def run_fused(I, v, n, cin, cout, h, w):
    from stylemc_amd import _hip, modconv
    P = modconv.PackedConv(I["W"].to(DEV), 2)
    ph, nph, _, _ = P.fwd_phases(h, w)
    x, s = I["x"].to(DEV), I["s"].to(DEV)
    y = torch.full((n, cout, 2 * h, 2 * w), float("nan"), device=DEV)
    epi, u, keep = _epi(modconv, _hip, I, v, n, cout, h, w)
    modconv.fused_up(x, y, ph, nph, cin, cout, s, epi)
    lib = _hip.load()
    name = lib.smc_modconv_up2_route_name(lib.smc_modconv_up2_last_route()).decode()
    # 32 output channels: 256-position tiles (TO 1, TM 2); 64: 128-position tiles, two channel blocks (TO 2, TM 1)
    assert name == f"convt_x3_fir_kernel<{'1,2' if cout == 32 else '2,1'},{'true' if w % 2 == 0 else 'false'}>", name
    torch.cuda.synchronize()
    return y, u


def run_pair(I, v, n, cin, cout, h, w):
    """The two launches (smc_conv_gemm_f32 STORE + smc_modconv_blur_act_f32), unsplit: the planning batch raised until
    the transposed conv's grid fills the chip, and the reported route flags checked."""
    from stylemc_amd import _hip, modconv
    lib = _hip.load()
    P = modconv.PackedConv(I["W"].to(DEV), 2)
    ph, nph, th, tw = P.fwd_phases(h, w)
    x, s = I["x"].to(DEV), I["s"].to(DEV)
    y = torch.full((n, cout, 2 * h, 2 * w), float("nan"), device=DEV)
    t = torch.empty(n, cout, th, tw, device=DEV)
    epi, u, keep = _epi(modconv, _hip, I, v, n, cout, h, w)
    with _hip.plan_batch(4096 * n, n):
        modconv.gemm(x, t, ph, nph, cin, cout, s=s, epi=modconv._epilogue(_hip.EPI_STORE))
        flags = lib.smc_conv_gemm_last_route_flags()
        route = lib.smc_conv_gemm_route_name(lib.smc_conv_gemm_last_route()).decode()
    assert not flags & _hip.ROUTE_SPLIT_K, "the reference conv ran split-K"
    assert not flags & _hip.ROUTE_PRESCALE, "the reference conv scaled x, not the weights"
    assert route.startswith("convt_x3_kernel" if P.use_x3 else "convt_lds_kernel"), route
    _hip.call("smc_modconv_blur_act_f32", t.data_ptr(), 1, 0, y.data_ptr(), n, cout, th, tw, 0, 2 * h, 2 * w, None, 4,
              4, 1, 1, 4.0, 0, ctypes.byref(epi), _hip.stream())
    torch.cuda.synchronize()
    return y, u


@gpu
@pytest.mark.parametrize("n,cin,cout,h,w,v", CASES, ids=IDS)
def test_fused_bit_equal_to_two_launches(lib, n, cin, cout, h, w, v):
    I = inputs(n, cin, cout, h, w)
    # (cin = 16 cannot split -- the cap is cin / 16 / 2 whole chunks; run_pair checks the reported flags of every case)
    yf, uf = run_fused(I, v, n, cin, cout, h, w)
    yp, up = run_pair(I, v, n, cin, cout, h, w)
    assert not torch.isnan(yf).any() and not torch.isnan(yp).any()
    assert torch.equal(yf, yp), f"y differs: max |diff| {(yf - yp).abs().max().item():.3e}"
    if v["u"]:
        assert not torch.isnan(uf).any()
        assert torch.equal(uf, up), f"u differs: max |diff| {(uf - up).abs().max().item():.3e}"


def ref_fp64(I, v, n, cin, cout, h, w):
    """conv_transpose2d of x * s, zero pad 1, 4x4 FIR k k^T / 16, the epilogue -- all in fp64 on the CPU."""
    import torch.nn.functional as F
    xs = (I["x"] * I["s"][:, :, None, None]).double()
    T = F.conv_transpose2d(xs, I["W"].double().transpose(0, 1), stride=2)
    k = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float64)
    f = torch.outer(k, k) / 16
    u = F.conv2d(F.pad(T, [1, 1, 1, 1]).reshape(n * cout, 1, 2 * h + 3, 2 * w + 3), f[None, None])
    z = u.reshape(n, cout, 2 * h, 2 * w)
    if v["d"]:
        z = z * I["d"].double()[:, :, None, None]
    if v["noise"] is not None:
        z = z + I["noise_" + v["noise"]].double() * I["strength"].double()
    if v["bias"]:
        z = z + I["bias"].double()[None, :, None, None]
    assert v["act"] == "linear" and v["clamp"] < 0
    return z * v["gain"]


@gpu
@pytest.mark.parametrize("n,cin,cout,h,w,_v", CASES, ids=IDS)
def test_fused_vs_fp64(lib, monkeypatch, n, cin, cout, h, w, _v):
    """The bounds of tests/test_gpu_ops.py::_both_forms, linear activation (no kinks).  The fused kernel has the
    split-bf16 form only, so the exact-fp32 figure is the two-launch path's with exact-fp32 products on the same
    inputs: that within 2e-5 of the max, the fused launch within 2x that error in max and in relative norm."""
    from stylemc_amd import modconv
    I = inputs(n, cin, cout, h, w)
    ref = ref_fp64(I, LINEAR, n, cin, cout, h, w)
    scale = max(ref.abs().max().item(), 1e-12)

    def errs(y):
        e = y.double().cpu() - ref
        return e.abs().max().item() / scale, (e.norm() / ref.norm()).item()

    monkeypatch.setattr(modconv, "X3", False)
    f_max, f_norm = errs(run_pair(I, LINEAR, n, cin, cout, h, w)[0])
    monkeypatch.setattr(modconv, "X3", True)
    x_max, x_norm = errs(run_fused(I, LINEAR, n, cin, cout, h, w)[0])
    print(f"fp32 pair max {f_max:.3e} norm {f_norm:.3e}; fused x3 max {x_max:.3e} norm {x_norm:.3e}")
    assert f_max <= 2e-5, f"exact fp32: max err {f_max:.3e}"
    assert x_max <= 2 * f_max, f"fused x3 max err {x_max:.3e} > 2 x fp32 {f_max:.3e}"
    assert x_norm <= 2 * f_norm, f"fused x3 norm err {x_norm:.3e} > 2 x fp32 {f_norm:.3e}"


@gpu
def test_rejects_other_filters_and_shapes(lib):
    from stylemc_amd import _hip, modconv
    n, cin, cout, h, w, v = CASES[0]
    I = inputs(n, cin, cout, h, w)
    P = modconv.PackedConv(I["W"].to(DEV), 2)
    ph, nph, _, _ = P.fwd_phases(h, w)
    x, s = I["x"].to(DEV), I["s"].to(DEV)
    y = torch.empty(n, cout, 2 * h, 2 * w, device=DEV)
    epi, _, keep = _epi(modconv, _hip, I, LINEAR, n, cout, h, w)
    ws = torch.empty(1 << 20, device=DEV)
    f = torch.ones(4, 4, device=DEV)
    args = lambda fp, fh, fw, g: (x.data_ptr(), n, cin, h, w, y.data_ptr(), cout, ph, nph, s.data_ptr(), fp, fh, fw, g,
                                  ctypes.byref(epi), ws.data_ptr(), 4 * ws.numel(), _hip.stream())
    assert lib.smc_modconv_up2_f32(*args(f.data_ptr(), 4, 4, 4.0)) == 2      # a filter of the caller's
    assert lib.smc_modconv_up2_f32(*args(None, 3, 3, 4.0)) == 2
    assert lib.smc_modconv_up2_f32(*args(None, 4, 4, 1.0)) == 2              # not the conv0 gain
    assert lib.smc_modconv_up2_last_route() == 0
    assert lib.smc_modconv_up2_f32(*args(None, 4, 4, 4.0)) == 0
    torch.cuda.synchronize()


def _calls(monkeypatch):
    """Record the names of the C-ABI calls modconv makes."""
    from stylemc_amd import _hip
    names = []
    real = _hip.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)

    monkeypatch.setattr(_hip, "call", call)
    return names


@gpu
def test_modconv_routing_and_oracle(lib, monkeypatch):
    """modulated_conv2d at (64 -> 32, 33 x 33): the fused launch with the switch on and an unsplit plan; the two
    launches with the switch off, with another filter, and where the plan splits K.  All four agree with the oracle
    (test_synthesis_layer_vs_oracle's tolerances: y 2e-5, gradients 1e-4 of the max)."""
    from oracle import networks as ON
    from oracle import ops as O
    from stylemc_amd import _hip, modconv
    n, cin, cout, h, w = 2, 64, 32, 33, 33

    def close(a, b, tol, what):
        a, b = a.detach().double().cpu(), b.detach().double()
        scale = max(b.abs().max().item(), 1e-12)
        err = (a - b).abs().max().item()
        assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol:.1e} * {scale:.3e}"

    I = inputs(n, cin, cout, h, w)
    gen = torch.Generator().manual_seed(5)
    cot = torch.randn(n, cout, 2 * h, 2 * w, generator=gen)
    names = _calls(monkeypatch)

    def run(taps, plan, expect_fused):
        f = O.setup_filter(taps)
        xr, sr = I["x"].clone().requires_grad_(True), I["s"].clone().requires_grad_(True)
        yr = ON.modulated_conv2d(xr, I["W"], sr, noise=I["noise_const"], up=2, padding=1, resample_filter=f,
                                 flip_weight=False)
        dxr, dsr = torch.autograd.grad((yr * cot).sum(), [xr, sr])
        xg, sg = I["x"].to(DEV).requires_grad_(True), I["s"].to(DEV).requires_grad_(True)
        del names[:]
        with _hip.plan_batch(plan, n):
            yg = modconv.modulated_conv2d(xg, I["W"].to(DEV), sg, noise=I["noise_const"].to(DEV), up=2, padding=1,
                                          resample_filter=f.to(DEV), flip_weight=False)
            fwd = list(names)
            flags = lib.smc_conv_gemm_last_route_flags()
            dxg, dsg = torch.autograd.grad((yg * cot.to(DEV)).sum(), [xg, sg])
        if expect_fused:
            assert "smc_modconv_up2_f32" in fwd and "smc_modconv_blur_act_f32" not in fwd, fwd
            name = lib.smc_modconv_up2_route_name(lib.smc_modconv_up2_last_route()).decode()
            assert name == "convt_x3_fir_kernel<1,2,false>", name
        else:
            assert "smc_modconv_up2_f32" not in fwd and "smc_modconv_blur_act_f32" in fwd, fwd
        close(yg, yr, 2e-5, "y")
        close(dxg, dxr, 1e-4, "dx")
        close(dsg, dsr, 1e-4, "ds")
        return yg, flags

    y_fused, _ = run([1, 3, 3, 1], 4096 * n, True)
    monkeypatch.setattr(modconv, "FUSED_UP", False)
    y_pair, flags = run([1, 3, 3, 1], 4096 * n, False)
    assert not flags & _hip.ROUTE_SPLIT_K
    assert torch.equal(y_fused, y_pair)
    monkeypatch.setattr(modconv, "FUSED_UP", True)
    # a 4-tap filter other than [1,3,3,1] (a 3-tap one changes the layer's padding, which modconv does not model)
    run([1, 2, 2, 1], 4096 * n, False)
    # the call's own batch: 2 x 10 tiles of 128 super-pixels on a chip of hundreds of CUs -> split-K, two launches
    assert lib.smc_modconv_up2_plan_ok(n, cin, cout, h, w) == 0
    with _hip.plan_batch(4096 * n, n):
        assert lib.smc_modconv_up2_plan_ok(n, cin, cout, h, w) == 1
        assert lib.smc_modconv_up2_plan_ok(n, cin, cout, 15, 15) == 0   # 256 super-pixels <= 9 cout: x may be prescaled
    _, flags = run([1, 3, 3, 1], 0, False)
    assert flags & _hip.ROUTE_SPLIT_K


def test_up2_supported_without_gpu():
    """smc_modconv_up2_supported is host logic (no device call): the 512- and 1024-px conv0 of FFHQ-1024 have the
    fused kernel; 128 output channels, cin % 16 != 0 and inputs of 2 GiB or more do not."""
    from stylemc_amd import _hip, build
    build.build(verbose=False)
    lib = _hip.load()
    assert lib.smc_modconv_up2_supported(4, 64, 32, 512, 512) == 1
    assert lib.smc_modconv_up2_supported(4, 128, 64, 256, 256) == 1
    assert lib.smc_modconv_up2_supported(4, 256, 128, 128, 128) == 0     # cout = 128: the per-phase kernel's layers
    assert lib.smc_modconv_up2_supported(4, 24, 32, 64, 64) == 0         # cin % 16
    assert lib.smc_modconv_up2_supported(8, 64, 32, 1024, 1024) == 0     # 2 GiB input (32-bit buffer offsets)
    assert lib.smc_modconv_up2_supported(4, 64, 32, 1024, 1024) == 1     # 1 GiB
    assert lib.smc_modconv_up2_route_name(0) == b"none" and lib.smc_modconv_up2_route_name(99) is None
