"""CPU checks of tests/aux_cases.py (no GPU): the fp64 reference pieces agree with oracle/ops.py run in fp64, every
backward case meets its kink margins, the restated guards give the route each case is built to reach, and the
companion entry points' host-side rejections (which also leave the launch report at "none")."""
import ctypes

import pytest
import torch

from oracle import ops as O
from tests import aux_cases as ac


@pytest.fixture(scope="module")
def lib():
    from stylemc_amd import _hip, build
    build.build(verbose=False)
    return _hip.load()


@pytest.mark.parametrize("filt,pad,flip,gain", [("asym", (1, 1), 0, 1.0), ("asym", (2, 1), 1, 2.0), ("std_rt", (1, 1), 0, 4.0),
                                                ("k3x3", (0, 2), 0, 1.0), ("k6x6", (3, 3), 1, 1.5), ("k1x4", (1, 0), 0, 1.0),
                                                ("k4x1", (2, 2), 1, 1.0), ("k8x8", (4, 4), 0, 1.0)])
def test_fir64_is_upfirdn2d(filt, pad, flip, gain):
    f, fh, fw = ac.taps_of(filt)
    assert tuple(f.shape) == (fh, fw)
    x = torch.randn(2, 3, 11, 13, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    px, py = pad
    want = O.upfirdn2d(x, f.double(), padding=[px, px, py, py], flip_filter=bool(flip), gain=gain)
    got = ac.fir64(x, f.double(), pad, flip, gain)
    assert got.shape == want.shape and torch.equal(got, want)


@pytest.mark.parametrize("pad,flip", [((2, 2), 1), ((1, 1), 0), ((3, 3), 1), ((0, 1), 0)])
def test_adjoint_fir_is_autograd_of_the_forward(pad, flip):
    """What the FIR backward cases assume: the gradient of upfirdn2d (pad p, flip F) is upfirdn2d with pad 3 - p and
    the other flip (upfirdn2d.py:245-264 at up = down = 1, 4x4 taps)."""
    f = ac.taps_of("asym")[0].double()
    gen = torch.Generator().manual_seed(2)
    th, tw = 9 + 2 * pad[1] - 3, 12 + 2 * pad[0] - 3
    T = torch.randn(1, 2, th, tw, dtype=torch.float64, generator=gen).requires_grad_()
    du = torch.randn(1, 2, 9, 12, dtype=torch.float64, generator=gen)
    fwd = O.upfirdn2d(T, f, padding=[3 - pad[0]] * 2 + [3 - pad[1]] * 2, flip_filter=not flip, gain=2.0)
    assert fwd.shape == du.shape
    (dT,) = torch.autograd.grad((fwd * du).sum(), T)
    assert torch.allclose(dT, ac.fir64(du, f, pad, flip, 2.0), rtol=1e-13, atol=1e-13)
    assert O.upfirdn2d_adjoint_padding(th, tw, 9, 12, 4, 4, 1, 1, [3 - pad[0]] * 2 + [3 - pad[1]] * 2) == \
        [pad[0], pad[0], pad[1], pad[1]]


@pytest.mark.parametrize("form", [k for k, f in ac.FORMS.items() if f["mode"] == "MODACT"])
def test_epilogue_formula_is_bias_act(form):
    f = ac.FORMS[form]
    gen = torch.Generator().manual_seed(3)
    n, c, h, w = 2, 3, 5, 6
    ops = ac.epi_ops(gen, form, n, c, h * w)
    u = torch.randn(n, c, h, w, generator=gen)
    ac.push_margins(u, ops, form, h, w)
    dten = ac.dten64(form, ops, n, c)
    u64 = u.double().requires_grad_()
    y, z, pre, _ = ac.epi64(u64, dten, ops, form, h, w)
    assert ac.margins_ok(z, pre, f["clamp"])
    # the same z through the oracle's bias_act (bias folded into z already)
    want = O.bias_act(z.detach(), act=f["act"], alpha=f["alpha"], gain=f["gain"], clamp=f["clamp"])
    assert torch.equal(y.detach(), want)
    g = torch.randn(n, c, h, w, dtype=torch.float64, generator=gen)
    (du,) = torch.autograd.grad((y * g).sum(), u64)
    dz = O.bias_act_grad(g, want, act=f["act"], alpha=f["alpha"], gain=f["gain"], clamp=f["clamp"])
    assert torch.allclose(du, dz * dten[:, :, None, None], rtol=1e-14, atol=0)
    # and the y-referenced formula of the grad_from_y references
    assert torch.equal(ac.act_grad64(form, g, want), dz)


def test_torgb_mask_is_bias_act_grad():
    gen = torch.Generator().manual_seed(4)
    g, y = torch.randn(50, dtype=torch.float64, generator=gen), torch.randn(50, dtype=torch.float64, generator=gen)
    for clamp in (-1.0, 0.3):
        assert torch.equal(ac.act_grad64_linear(g, y, clamp), O.bias_act_grad(g, y, act="linear", gain=1.0, clamp=clamp))


@pytest.mark.parametrize("cid", [c.id for c in ac.CASES if c.ep in ("blur_bwd", "act_bwd", "torgb_bwd", "torgb_act_bwd")])
def test_backward_case_meets_its_margins(cid):
    c = ac.BY_ID[cid]
    d = ac.make_inputs(c)
    assert ac.backward_margins(c, d), cid
    if c.p.get("nocancel"):
        du, dd, B = ac.bwd_grads(c, d)
        assert torch.allclose(dd, B, rtol=1e-12) and (B > 0).all()


def test_restated_guards_give_every_expected_route(lib):
    names = ac.route_names()
    for c in ac.CASES:
        name, flags, _ = ac.planned(c)
        assert (name, flags) == (c.route, c.flags), (c.id, name, flags)
        assert c.route in names, c.id
    assert {c.route for c in ac.CASES} == set(names[1:]), "a case for every route of the table, none waived"
    # the channel split of smc_torgb_act_bwd_f32 at the MI355X's 256 CUs, and one planned for a large batch
    nz = {c.id: ac.planned(c, 256)[2] for c in ac.cases_of("torgb_act_bwd")}
    assert [nz[f"torgb_act_bwd_vec_cin{k}"] for k in (64, 48, 24, 20)] == [8, 2, 1, 1]
    assert nz["torgb_act_bwd_vec_cin64_planned_large"] == 1 and nz["torgb_act_bwd_vec_cin512_66x64"] == 64


def test_workspace_queries_agree_with_the_restated_rules(lib):
    for c in ac.cases_of("act_bwd"):
        p = c.p
        hw = p["h"] * p["w"]
        bpp = max(ac.act_bwd_blocks(hw, hw % 4 == 0), ac.act_bwd_blocks(hw, False))
        assert lib.smc_modconv_act_bwd_workspace_size(p["n"], p["c"], p["h"], p["w"]) == \
            (4 * p["n"] * p["c"] * bpp if bpp > 2 else 0), c.id
    for c in ac.cases_of("blur_bwd"):
        p = c.p
        th, tw = ac.bwd_geometry(p)
        many = ac.cdiv(p["uh"], 32) * ac.cdiv(p["uw"], 64) > 2
        assert lib.smc_modconv_blur_act_bwd_workspace_size(p["n"], p["c"], p["uh"], p["uw"], th, tw) == \
            (4 * p["n"] * p["c"] * ac.cdiv(th, 32) * ac.cdiv(tw, 64) if many else 0), c.id


def _dd_owners(u_len, pad, tile):
    """The dd ownership rule of blur_act_bwd_* along one axis, restated: tile k of the t grid (t = u + 2 pad - 3 long)
    owns u positions [k tile, (k + 1) tile), the last tile everything from k tile on; it can only add what its haloed
    window [k tile - pad, k tile - pad + tile + 3) holds.  Returns how often each u position is added."""
    t_len = u_len + 2 * pad - 3
    tiles = ac.cdiv(t_len, tile)
    count = [0] * u_len
    for k in range(tiles):
        lo, hi = k * tile, (u_len if k == tiles - 1 else (k + 1) * tile)
        for i in range(max(lo, k * tile - pad, 0), min(hi, k * tile - pad + tile + 3, u_len)):
            count[i] += 1
    return count


def test_dd_ownership_covers_u_once_up_to_pad_3_and_not_beyond():
    """Why dd is supported at adjoint pads 0 .. 3 only: there every u row (32-row tiles) and column (64) is owned by
    exactly one tile that has loaded it; from pad 4 on a tile's window ends before its own last rows."""
    for tile in (32, 64):
        for pad in range(4):
            for u_len in list(range(4, 3 * tile + 8)) + [5 * tile + 1]:
                if u_len + 2 * pad - 3 >= 1:
                    assert set(_dd_owners(u_len, pad, tile)) == {1}, (tile, pad, u_len)
        assert 0 in _dd_owners(tile + 8, 4, tile) and 0 in _dd_owners(2 * tile + 6, 5, tile)
    for c in ac.cases_of("blur_bwd"):
        assert not c.p["dd"] or max(c.p["pad"]) <= 3, c.id


def _report(lib):
    return lib.smc_modconv_aux_last_route(), lib.smc_modconv_aux_last_route_flags(), lib.smc_modconv_aux_last_nsplit()


def test_host_side_rejections(lib):
    """Calls that must fail on the host before any launch (fake non-NULL pointers are never dereferenced there), each
    leaving the launch report at "none"."""
    from stylemc_amd import _hip
    fake = ctypes.c_void_p(256)
    epi = _hip.ConvEpilogue()
    epi.mode = _hip.EPI_MODACT
    # a_scaled without scale
    assert lib.smc_channel_dot_f32(fake, fake, None, fake, fake, 1, 400, 0, None) == 1
    assert b"a_scaled needs scale" in lib.smc_last_error() and _report(lib) == (0, 0, 1)
    # ToRGB: cout 5 and cin 1025 are unsupported, in all three entry points
    for cin, cout in ((12, 5), (1025, 3)):
        assert lib.smc_torgb_fwd_f32(fake, fake, fake, None, fake, 1, cin, cout, 4, 4, -1.0, None) == 2
        assert lib.smc_torgb_bwd_f32(fake, fake, fake, fake, fake, 1, cin, cout, 4, 4, -1.0, 1, 0, None) == 2
        epi.grad_from_y = 1
        assert lib.smc_torgb_act_bwd_f32(fake, fake, fake, fake, -1.0, None, fake, fake, 1, cin, cout, 4, 4,
                                         ctypes.byref(epi), None) == 2
        assert _report(lib) == (0, 0, 1)
    assert lib.smc_torgb_bwd_f32(fake, fake, fake, None, fake, 1, 12, 3, 4, 4, -1.0, 1, 0, None) == 1    # scale needs s
    # the FIR forward needs an epilogue (STORE for the bare FIR); filters beyond 8x8 are unsupported
    assert lib.smc_modconv_blur_act_f32(fake, 1, 0, fake, 1, 1, 9, 9, 0, 8, 8, None, 4, 4, 1, 1, 4.0, 0, None, None) == 1
    assert b"needs an epilogue" in lib.smc_last_error() and _report(lib) == (0, 0, 1)
    assert lib.smc_modconv_blur_act_f32(fake, 1, 0, fake, 1, 1, 9, 9, 0, 8, 8, fake, 9, 9, 1, 1, 1.0, 0,
                                        ctypes.byref(epi), None) == 2
    # the FIR backward: dd with grad_from_y, a t shape that is not the adjoint's, a negative adjoint pad, a 3x3 filter
    epi.grad_from_y = 1
    bwd = lambda dd, th, tw, fh, px, py: lib.smc_modconv_blur_act_bwd_f32(
        fake, fake, fake, dd, 1, 1, 8, 8, th, tw, 0, fake, fh, fh, px, py, 1.0, 1, ctypes.byref(epi), None, 0, None)
    assert bwd(fake, 9, 9, 4, 2, 2) == 1 and b"dd needs u" in lib.smc_last_error()
    epi.grad_from_y = 0
    assert bwd(None, 10, 9, 4, 2, 2) == 1 and b"t shape" in lib.smc_last_error()
    assert bwd(None, 3, 3, 4, -1, -1) == 1 and b"negative adjoint pad" in lib.smc_last_error()
    assert bwd(None, 10, 10, 3, 2, 2) == 2
    # dd beyond adjoint pad 3 in either axis (a tile's haloed window would lack part of the 32 x 64 it owns): unsupported
    for px, py in ((4, 4), (4, 2), (2, 4), (6, 3)):
        assert bwd(fake, 8 + 2 * py - 3, 8 + 2 * px - 3, 4, px, py) == 2, (px, py)
        assert b"adjoint pad of at most 3" in lib.smc_last_error() and _report(lib) == (0, 0, 1)
    assert _report(lib) == (0, 0, 1)
    epi.grad_from_y = 1
    assert lib.smc_modconv_act_bwd_f32(fake, fake, fake, fake, 1, 1, 8, 8, ctypes.byref(epi), None, 0, None) == 1
    assert _report(lib) == (0, 0, 1)
    assert lib.smc_modconv_aux_route_name(0) == b"none" and lib.smc_modconv_aux_route_name(-1) is None
    assert lib.smc_modconv_aux_route_name(lib.smc_modconv_aux_route_count()) is None
