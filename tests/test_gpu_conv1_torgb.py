"""smc_modconv_conv1_torgb_f32 (csrc/wino.hip, wino_rgb_kernel): a 32-channel block's conv1 and its ToRGB in one
Winograd launch, at the kernel level and end to end.

Kernel level, per case:
  y     torch.equal to smc_conv3x3_wino_ws_f32's y on the same operands.  Every case reaches the same style form
        unsplit through that entry point (smc_conv3x3_wino_last_nsplit() == 1 and the same SMC_ROUTE_WINO_FOLD flag:
        with the workspace the folded form, SM 2; without it the style in the kernel, SM 1), so no case needs the fp64
        bound of tests/wino_cases.py instead.
  rgb   against the fp64 ToRGB of the stored y within the bound tests/aux_cases.py holds smc_torgb_fwd_f32 to,
        (cin + 3) EPS (sum |w s| |y| + |b|) with cin = 32: the forward bound of a 32-term dot product in any order
        (+ the product w s, the bias add, and one spare).  With the clamp the comparison is after clamping, leaving out
        the elements whose fp64 value lies within the bound of +-clamp (either side of the kink is then right); at most
        1 % may be left out.
  the NULL-y form writes the same rgb bit for bit; the route report names wino_rgb_kernel<TC,SM>.
The fused kernel has no persistent form (wino_rgb_kernel instantiates the shared loop with PERSIST = 0, the form
wino_kernel is launched in: one work item per workgroup), so "several items" below means several workgroups -- the
work-item decode, the tile-group offsets and the per-image operands (s_rgb, folded taps, noise planes) of items other
than the first.
One case above 4096 positions also holds rgb bit-equal to smc_torgb_fwd_f32 of the stored y: the fused dot runs in the
order of torgb_fwd_kernel's per-position loop (tests/test_gpu_ops.py::test_conv1_torgb_fused_backward compares the two
paths with torch.equal at 1024 px).

End to end: a seeded 64-px generator whose last block has 32 channels, FUSED_TORGB on and off, against oracle/ at the
tolerances of tests/test_gpu_ops.py::test_synthesis_1024_vs_oracle (image 1e-4, direction-row gradients 2e-3 of the
maximum)."""
import collections
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 2.0 ** -24
COUT = 32

Case = collections.namedtuple("Case", "id n cin h w krgb noise bias fold")
CASES = [
    # one work item, 2 x 32 tile block
    Case("item1_tc32_fold", 1, 8, 4, 64, 3, True, True, True),
    Case("item1_tc32_plain_rgb1", 1, 8, 4, 64, 1, False, False, False),
    # 4 x 16 tile block
    Case("tc16_rgb4", 1, 8, 8, 32, 4, True, True, False),
    Case("tc16_fold_nonoise", 1, 8, 8, 32, 3, False, True, True),
    # several items, two images: the per-image s_rgb, folded taps and noise planes
    Case("items_n2_k64_fold", 2, 64, 8, 128, 3, True, True, True),
    Case("items_n2_k64_rgb4_nobias", 2, 64, 8, 128, 4, True, False, False),
    # both style forms on one shape
    Case("n2_k32_fold", 2, 32, 16, 64, 3, True, True, True),
    Case("n2_k32_style_in_kernel", 2, 32, 16, 64, 3, True, True, False),
    # above smc_torgb_fwd_f32's small-plane threshold: also bit-equal to torgb_fwd_kernel
    Case("hw8192_vs_torgb_kernel", 1, 8, 64, 128, 3, True, True, True),
]
CLAMP, CLAMP_RGB = 1.5, 0.6     # both bite (asserted)


def _inputs(c):
    g = torch.Generator().manual_seed(100 + CASES.index(c))
    d = dict(
        x=torch.randn(c.n, c.cin, c.h, c.w, generator=g),
        wt=torch.randn(COUT, c.cin, 3, 3, generator=g) / (9 * c.cin) ** 0.5,
        s=torch.rand(c.n, c.cin, generator=g) + 0.5,
        d=torch.rand(c.n, COUT, generator=g) + 0.5,
        noise=torch.randn(c.n, 1, c.h, c.w, generator=g),
        strength=torch.tensor([0.3]),
        bias=torch.randn(COUT, generator=g) * 0.1,
        w_rgb=torch.randn(c.krgb, COUT, generator=g) / COUT ** 0.5,
        s_rgb=torch.rand(c.n, COUT, generator=g) + 0.5,
        b_rgb=torch.randn(c.krgb, generator=g) * 0.1,
    )
    return d


def _epilogue(c, d):
    from stylemc_amd import _hip
    e = _hip.ConvEpilogue()
    e.mode = _hip.EPI_MODACT
    e.d = d["d"].data_ptr()
    if c.noise:
        e.noise = d["noise"].data_ptr()
        e.noise_nstride = c.h * c.w
        e.noise_strength = d["strength"].data_ptr()
    if c.bias:
        e.bias = d["bias"].data_ptr()
    e.act = _hip.ACT_CODES["lrelu"]
    e.alpha, e.gain, e.clamp = 0.2, 2 ** 0.5, CLAMP
    return e


def _run(c):
    from stylemc_amd import _hip
    lib = _hip.load()
    d = {k: v.to(DEV) for k, v in _inputs(c).items()}
    st = _hip.stream()
    uw = torch.empty(16 * c.cin * COUT, device=DEV)
    _hip.call("smc_wino_weights_f32", d["wt"].data_ptr(), COUT, c.cin, 0, uw.data_ptr(), st)
    e = _epilogue(c, d)
    assert lib.smc_modconv_conv1_torgb_supported(c.n, c.cin, COUT, c.h, c.w, c.krgb, ctypes.byref(e)) == 1
    nb = lib.smc_modconv_conv1_torgb_workspace_size(c.n, c.cin, COUT, c.h, c.w) if c.fold else 0
    assert nb > 0 or not c.fold
    b_rgb = d["b_rgb"] if c.bias else None

    def fused(with_y):
        y = torch.full((c.n, COUT, c.h, c.w), float("nan"), device=DEV) if with_y else None
        rgb = torch.full((c.n, c.krgb, c.h, c.w), float("nan"), device=DEV)
        ws = torch.empty(max(nb // 4, 1), device=DEV)
        _hip.call("smc_modconv_conv1_torgb_f32", d["x"].data_ptr(), c.n, c.cin, c.h, c.w, _hip.ptr(y), COUT,
                  uw.data_ptr(), d["s"].data_ptr(), ctypes.byref(e), d["w_rgb"].data_ptr(), d["s_rgb"].data_ptr(),
                  _hip.ptr(b_rgb), CLAMP_RGB, c.krgb, rgb.data_ptr(), ws.data_ptr() if nb else None, nb, st)
        name = lib.smc_modconv_conv1_torgb_route_name(lib.smc_modconv_conv1_torgb_last_route()).decode()
        return y, rgb, name

    y, rgb, name = fused(True)
    _, rgb_only, name2 = fused(False)
    # the two-launch path's conv on the same operands, the same style form
    y_old = torch.full_like(y, float("nan"))
    nb_old = lib.smc_conv3x3_wino_workspace_size(c.n, c.cin, COUT, c.h, c.w) if c.fold else 0
    ws_old = torch.empty(max(nb_old // 4, 1), device=DEV)
    _hip.call("smc_conv3x3_wino_ws_f32", d["x"].data_ptr(), c.n, c.cin, c.h, c.w, y_old.data_ptr(), COUT, uw.data_ptr(),
              d["s"].data_ptr(), ctypes.byref(e), ws_old.data_ptr() if nb_old else None, nb_old, st)
    old = (lib.smc_conv3x3_wino_last_nsplit(), lib.smc_conv3x3_wino_last_route_flags(),
           lib.smc_conv3x3_wino_route_name(lib.smc_conv3x3_wino_last_route()).decode())
    rgb_kernel = None
    if c.h * c.w > 4096:
        rgb_kernel = torch.full_like(rgb, float("nan"))
        _hip.call("smc_torgb_fwd_f32", y.data_ptr(), d["w_rgb"].data_ptr(), d["s_rgb"].data_ptr(), _hip.ptr(b_rgb),
                  rgb_kernel.data_ptr(), c.n, COUT, c.krgb, c.h, c.w, CLAMP_RGB, st)
    torch.cuda.synchronize()
    return d, y, rgb, rgb_only, (name, name2), y_old, old, rgb_kernel


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_fused_launch(c):
    d, y, rgb, rgb_only, names, y_old, old, rgb_kernel = _run(c)
    tc = 32 if c.w % 64 == 0 and c.h % 4 == 0 else 16
    want = f"wino_rgb_kernel<{tc},{2 if c.fold else 1}>"
    assert names == (want, want), names
    # ---- y: the unsplit launch of the same form through the existing entry point
    nsplit, flags, old_name = old
    assert nsplit == 1 and bool(flags & 16) == c.fold, old
    assert old_name == f"wino_kernel<{tc},{2 if c.fold else 1},1>", old_name
    assert not torch.isnan(y).any() and not torch.isnan(rgb).any()
    assert torch.equal(y, y_old)
    assert (y.abs() == CLAMP).any(), "the conv clamp does not bite"
    # ---- rgb against fp64 of the stored y
    ws = d["w_rgb"].double()[None] * d["s_rgb"].double()[:, None, :]                    # [n, k, 32]
    b = d["b_rgb"].double()[None, :, None, None] if c.bias else torch.zeros(1, 1, 1, 1, dtype=torch.float64, device=DEV)
    y64 = y.double()
    ref = torch.einsum("nkc,nchw->nkhw", ws, y64) + b
    bound = (COUT + 3) * EPS * (torch.einsum("nkc,nchw->nkhw", ws.abs(), y64.abs()) + b.abs())
    near = ((ref.abs() - CLAMP_RGB).abs() <= bound)
    assert (ref.abs() > CLAMP_RGB).any(), "the rgb clamp does not bite"
    assert near.float().mean().item() <= 0.01, near.float().mean().item()
    err = (rgb.double() - ref.clamp(-CLAMP_RGB, CLAMP_RGB)).abs()
    ratio = (err / bound)[~near].max().item()
    print(f"{c.id}: rgb max err / bound = {ratio:.3f}, left out {int(near.sum())} of {near.numel()}")
    assert ratio <= 1.0, ratio
    # ---- the form that stores no y
    assert torch.equal(rgb_only, rgb)
    if rgb_kernel is not None:
        assert torch.equal(rgb, rgb_kernel), "not the summation order of torgb_fwd_kernel"


# ---------------------------------------------------------------------------------------------- end to end
RES, CBASE, UNTIL_K, N = 64, 2048, 4, 2       # channels 512, 256, 128, 64, 32 at 4 .. 64 px
# 8 direction rows that leave the last block's conv1 (row 12) and ToRGB (13) out, as FFHQ-1024's rows 24 and 25 are:
# conv1's styles then need no gradient and the edited branch takes the fused launch, as the 1024-px step does
ROWS = [2, 3, 5, 6, 8, 9, 10, 11]


def _close(a, b, tol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = max(b.abs().max().item(), 1e-12)
    err = (a - b).abs().max().item()
    assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol:.1e} * {scale:.3e}"


@pytest.fixture(scope="module")
def tiny():
    from oracle import synthesis as OS
    from stylemc_amd import networks, synthetic, utils
    from tests.fd_helpers import oracle_generator, per_image_synth
    cfg = synthetic.generator_config(resolution=RES, channel_base=CBASE, conv_clamp=256.0)
    G = networks.build_generator(cfg, synthetic.generator_state_dict(cfg, seed=0), device=DEV)
    assert G.synthesis.b64.conv1.weight.shape[:2] == (32, 32)
    Go = oracle_generator(RES, CBASE, 256.0, seed=0)
    shapes, shapes_o = utils.get_temp_shapes(G), OS.get_temp_shapes(Go)
    assert shapes == shapes_o
    styles = synthetic.synthetic_styles(N, seed=3)
    delta = torch.randn(1, len(ROWS), 512, generator=torch.Generator().manual_seed(4)) * 0.05
    do = delta.clone().requires_grad_(True)
    img_o = per_image_synth(Go, UNTIL_K, styles, shapes_o, "const", delta=do, trainable=ROWS)
    (gd_o,) = torch.autograd.grad(img_o.square().sum(), do)
    with torch.no_grad():
        orig_o = per_image_synth(Go, UNTIL_K, styles, shapes_o, "const")
    return G, shapes, styles.to(DEV), delta.to(DEV), img_o.detach(), gd_o, orig_o


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two_launches"])
def test_tiny_generator_vs_oracle(tiny, fused, monkeypatch):
    from stylemc_amd import _hip, modconv, utils
    G, shapes, styles, delta, img_o, gd_o, orig_o = tiny
    monkeypatch.setattr(modconv, "FUSED_TORGB", fused)
    calls = []
    inner = modconv.fused_torgb

    def counted(x, y, *a, **k):
        inner(x, y, *a, **k)
        lib = _hip.load()
        calls.append((y is not None, lib.smc_modconv_conv1_torgb_route_name(lib.smc_modconv_conv1_torgb_last_route())))

    monkeypatch.setattr(modconv, "fused_torgb", counted)
    d = delta.clone().requires_grad_(True)
    img = utils.generate_image_rows(G, UNTIL_K, styles, shapes, "const", delta=d, trainable=ROWS)
    (gd,) = torch.autograd.grad(img.square().sum(), d)
    with torch.no_grad():
        orig = utils.generate_image_rows(G, UNTIL_K, styles, shapes, "const")
    _close(img, img_o, 1e-4, "edited image")
    _close(orig, orig_o, 1e-4, "original image")
    _close(gd, gd_o, 2e-3, "delta gradient")
    if fused:
        # the last conv1 of both branches: y stored for the backward, not stored without a gradient
        assert calls == [(True, b"wino_rgb_kernel<32,2>"), (False, b"wino_rgb_kernel<32,2>")], calls
    else:
        assert calls == []


def test_no_grad_last_block_allocates_no_y(tiny, monkeypatch):
    """The last block's conv1 + ToRGB with need_y=False and no gradient: the peak of allocated memory over the call
    stays below one [n, 32, H, W] tensor with the fused launch, and holds one with the two launches."""
    from stylemc_amd import modconv
    G = tiny[0]
    blk = G.synthesis.b64
    g = torch.Generator().manual_seed(6)
    x = torch.randn(N, 32, RES, RES, generator=g).to(DEV)
    w1 = (torch.randn(N, 32, generator=g) * 0.5 + 1).to(DEV)     # the block's affines are Identity (get_temp_shapes)
    wr = (torch.randn(N, 32, generator=g) * 0.5 + 1).to(DEV)
    y_bytes = N * 32 * RES * RES * 4
    peaks, outs = {}, {}
    for fused in (True, False):
        monkeypatch.setattr(modconv, "FUSED_TORGB", fused)
        with torch.no_grad():
            blk.conv1_torgb(x, w1, wr, noise_mode="const", need_y=False)    # builds the layer's cached operands
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_stats()["allocated_bytes.all.current"]
            y, rgb = blk.conv1_torgb(x, w1, wr, noise_mode="const", need_y=False)
            torch.cuda.synchronize()
            peaks[fused] = torch.cuda.memory_stats()["allocated_bytes.all.peak"] - base
            outs[fused] = (y, rgb)
            del y, rgb
    assert outs[True][0] is None and outs[False][0] is not None
    assert peaks[True] < y_bytes <= peaks[False], (peaks, y_bytes)
    _close(outs[True][1], outs[False][1], 1e-5, "rgb")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two_launches"])
def test_only_torgb_style_needs_grad(tiny, fused, monkeypatch):
    """The last block with need_y=False where the ToRGB style is the only input that requires a gradient (a direction
    on the last ToRGB row alone): y must be kept, because the ToRGB style gradient reads it.  Forward and gradient
    against the separate conv1 and ToRGB layers.  y is bit-equal.  rgb: 64 px is below the plane size at which the two
    kernels share one order, so each is within (32 + 3) EPS (sum |w s| |y| + |b|) of the exact dot and they differ by
    at most twice that.  The gradient runs the same kernels on bit-equal operands (the cotangent, y; rgb enters only
    through the clamp mask, and no |rgb| reaches the clamp -- asserted), so it is bit-equal too."""
    from stylemc_amd import modconv
    G = tiny[0]
    blk = G.synthesis.b64
    g = torch.Generator().manual_seed(8)
    x = torch.randn(N, 32, RES, RES, generator=g).to(DEV)
    w1 = (torch.randn(N, 32, generator=g) * 0.5 + 1).to(DEV)
    wr0 = torch.randn(N, 32, generator=g) * 0.5 + 1
    cot = torch.randn(N, 3, RES, RES, generator=g).to(DEV)
    monkeypatch.setattr(modconv, "FUSED_TORGB", fused)
    wr = wr0.to(DEV).requires_grad_(True)
    y, rgb = blk.conv1_torgb(x, w1, wr, noise_mode="const", need_y=False)
    assert y is not None
    (ga,) = torch.autograd.grad((rgb * cot).sum(), wr)
    wr2 = wr0.to(DEV).requires_grad_(True)
    y2 = blk.conv1(x, w1, noise_mode="const")
    rgb2 = blk.torgb(y2, wr2)
    (gb,) = torch.autograd.grad((rgb2 * cot).sum(), wr2)
    assert torch.equal(y, y2)
    t = blk.torgb
    ws = t.weight.detach()[:, :, 0, 0].double()[None].abs() * (wr0.to(DEV).double() * t.weight_gain)[:, None, :].abs()
    B = torch.einsum("nkc,nchw->nkhw", ws, y.detach().double().abs()) + t.bias.detach().double().abs()[None, :, None, None]
    assert ((rgb.detach().double() - rgb2.detach().double()).abs() <= 2 * (32 + 3) * EPS * B).all()
    assert (rgb.abs() < t.conv_clamp).all() and (rgb2.abs() < t.conv_clamp).all()
    assert torch.equal(ga, gb), "ToRGB style gradient"
