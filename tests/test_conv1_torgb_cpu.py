"""Host side of smc_modconv_conv1_torgb_f32 (conv1 + ToRGB of a 32-channel block in one Winograd launch): the support
predicate, the workspace query, the route names and the argument checks.  No device call: the library loads without a
GPU."""
import ctypes
import itertools

from stylemc_amd import _hip
from tests import wino_cases as wc

# the shapes tests/test_gpu_conv1_torgb.py launches, and the FFHQ-1024 layer
SHAPES = [(1, 8, 4, 64), (1, 8, 8, 32), (2, 64, 8, 128), (2, 32, 16, 64), (4, 32, 1024, 1024)]


def _epi(**kw):
    e = _hip.ConvEpilogue()
    e.mode = _hip.EPI_MODACT
    e.act = _hip.ACT_CODES["lrelu"]
    e.alpha, e.gain, e.clamp = 0.2, 2 ** 0.5, 256.0
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def test_supported_accepts_the_32_channel_winograd_shapes():
    lib = _hip.load()
    for (n, cin, h, w), krgb in itertools.product(SHAPES, (1, 2, 3, 4)):
        assert lib.smc_conv3x3_wino_supported(n, cin, 32, h, w) == 1
        assert lib.smc_modconv_conv1_torgb_supported(n, cin, 32, h, w, krgb, None) == 1, (n, cin, h, w, krgb)
        assert lib.smc_modconv_conv1_torgb_supported(n, cin, 32, h, w, krgb, ctypes.byref(_epi())) == 1


def test_supported_refuses_what_the_kernel_does_not_compute():
    lib = _hip.load()
    ok = lib.smc_modconv_conv1_torgb_supported
    assert ok(1, 64, 64, 8, 128, 3, None) == 0                      # cout 64: four waves hold the channels
    assert ok(1, 8, 32, 4, 64, 5, None) == 0 and ok(1, 8, 32, 4, 64, 0, None) == 0   # cout_rgb outside 1..4
    assert ok(1, 8, 32, 4, 64, 3, ctypes.byref(_epi(u_save=64))) == 0                # u_save set
    # shapes smc_conv3x3_wino_supported refuses
    for n, cin, h, w in ((1, 8, 6, 64), (1, 12, 4, 64), (1, 8, 4, 34), (1, 8, 16, 16)):
        assert lib.smc_conv3x3_wino_supported(n, cin, 32, h, w) == 0
        assert ok(n, cin, 32, h, w, 3, None) == 0, (n, cin, h, w)
    # the epilogue must be the MODACT lrelu + clamp form
    assert ok(1, 8, 32, 4, 64, 3, ctypes.byref(_epi(act=_hip.ACT_CODES["linear"]))) == 0
    assert ok(1, 8, 32, 4, 64, 3, ctypes.byref(_epi(clamp=-1.0))) == 0
    assert ok(1, 8, 32, 4, 64, 3, ctypes.byref(_epi(mode=_hip.EPI_STORE))) == 0
    # where the two-launch path plans split-K the pair keeps the call
    assert wc.wino_nsplit(1, 512, 32, 32, 32) > 1
    assert ok(1, 512, 32, 32, 32, 3, None) == 0


def test_workspace_is_the_folded_taps():
    lib = _hip.load()
    for n, cin, h, w in SHAPES:
        assert lib.smc_modconv_conv1_torgb_workspace_size(n, cin, 32, h, w) == n * cin * 16 * 32 * 4
        # the same bytes the two-launch path asks for (no split planes at these shapes)
        assert lib.smc_conv3x3_wino_workspace_size(n, cin, 32, h, w) == n * cin * 16 * 32 * 4
    assert lib.smc_modconv_conv1_torgb_workspace_size(1, 64, 64, 8, 128) == 0        # unsupported: nothing to hold
    assert lib.smc_modconv_conv1_torgb_workspace_size(1, 8, 32, 6, 64) == 0


def test_route_names():
    lib = _hip.load()
    count = lib.smc_modconv_conv1_torgb_route_count()
    names = [lib.smc_modconv_conv1_torgb_route_name(i) for i in range(count)]
    assert names[0] == b"none"
    assert sorted(names[1:]) == sorted(f"wino_rgb_kernel<{tc},{sm}>".encode() for tc in (32, 16) for sm in (1, 2))
    assert lib.smc_modconv_conv1_torgb_route_name(-1) is None
    assert lib.smc_modconv_conv1_torgb_route_name(count) is None


def test_null_rgb_fails_on_the_host():
    lib = _hip.load()
    e = _epi()
    # (non-null placeholders are never dereferenced: the argument check fails first)
    rc = lib.smc_modconv_conv1_torgb_f32(16, 1, 8, 4, 64, None, 32, 16, None, ctypes.byref(e), 16, 16, None, 256.0, 3,
                                         None, None, 0, None)
    assert rc == 1
    assert b"smc_modconv_conv1_torgb_f32" in lib.smc_last_error() and b"rgb" in lib.smc_last_error()
    assert lib.smc_modconv_conv1_torgb_last_route() == 0
    # an unsupported shape is SMC_ERR_UNSUPPORTED (2), also before any launch
    rc = lib.smc_modconv_conv1_torgb_f32(16, 1, 64, 8, 128, None, 64, 16, None, ctypes.byref(e), 16, 16, None, 256.0, 3,
                                         16, None, 0, None)
    assert rc == 2 and b"no fused kernel" in lib.smc_last_error()
    assert lib.smc_modconv_conv1_torgb_last_route() == 0
    # so is a NULL epilogue (the STORE default has no fused form), though the predicate takes NULL for the shape alone
    assert lib.smc_modconv_conv1_torgb_supported(1, 8, 32, 4, 64, 3, None) == 1
    rc = lib.smc_modconv_conv1_torgb_f32(16, 1, 8, 4, 64, None, 32, 16, None, None, 16, 16, None, 256.0, 3, 16, None, 0,
                                         None)
    assert rc == 2 and b"no fused kernel" in lib.smc_last_error()


def test_rgb_clamp_cap_holds_for_the_reference_alone():
    """tests/test_gpu_conv1_torgb.py leaves out of its rgb comparison the elements whose fp64 value lies within the
    bound of +-clamp_rgb, at most 1 %.  The cap holds for the fp64 reference alone: with a CPU fp64 conv in place of the
    stored y, the elements within the bound of +-CLAMP_RGB are far below 1 % in every case (a bound of ~2e-6 around two
    values of a continuous distribution)."""
    import torch
    import torch.nn.functional as F
    from tests import test_gpu_conv1_torgb as G
    COUT, EPS, CLAMP, CLAMP_RGB = G.COUT, G.EPS, G.CLAMP, G.CLAMP_RGB
    for c in G.CASES:
        d = {k: v.double() for k, v in G._inputs(c).items()}
        n = c.n
        u = torch.cat([F.conv2d(d["x"][i:i + 1] * d["s"][i][None, :, None, None], d["wt"], padding=1) for i in range(n)])
        z = u * d["d"][:, :, None, None]
        if c.noise:
            z = z + d["noise"] * 0.3
        if c.bias:
            z = z + d["bias"][None, :, None, None]
        y = (F.leaky_relu(z, 0.2) * 2 ** 0.5).clamp(-CLAMP, CLAMP)
        ws = d["w_rgb"][None] * d["s_rgb"][:, None, :]
        b = d["b_rgb"][None, :, None, None] if c.bias else 0.0
        ref = torch.einsum("nkc,nchw->nkhw", ws, y) + b
        bound = (COUT + 3) * EPS * (torch.einsum("nkc,nchw->nkhw", ws.abs(), y.abs()) + abs(b))
        near = (ref.abs() - CLAMP_RGB).abs() <= bound
        assert near.float().mean().item() <= 0.01, (c.id, near.float().mean().item())
        assert (ref.abs() > CLAMP_RGB).any() and (y.abs() == CLAMP).any(), c.id
