"""What tests/irse_cases.py claims, checked without a GPU: its fp64 references are the reference modules' autograd, its
shapes pass the host validators (restated; every rejection asserted by message), its tables hold every form they are
meant to, and every case can tell each mistake of irse_cases.MUTATIONS from rounding."""
import ctypes
import functools

import pytest
import torch

from tests import irse_cases as IC


def _ratio(a, ref, bound):
    d = (a - ref).abs()
    return torch.where(d > 0, d / bound.clamp_min(1e-300), torch.zeros_like(d)).max().item()


@functools.lru_cache(maxsize=None)
def _stage_base(cid):
    c = IC.STAGE_BY_ID[cid]
    I = IC.stage_inputs(c)
    fwd = IC.stage_fwd_ref(c, I)
    dev = {k: v[0].float() for k, v in fwd.items()}
    bwd = IC.stage_bwd_ref(c, I, dev)
    dev.update({k: v[0].float() for k, v in bwd.items()})
    return c, I, fwd, bwd, dev


# ------------------------------------------------------------------------------------------- references

@pytest.mark.parametrize("cid", ["c96_h16_3x5", "c160_h17_5x3", "c32_h3_7x7", "nc_c96_h17_5x3"])
def test_stage_reference_is_semodule_autograd(cid):
    """out = SEModule(r) + shortcut and dr = d sum(dout out) / d r of model_irse.SEModule in fp64."""
    from stylemc_amd.id_loss.model_irse import SEModule, Subsample
    c = IC.STAGE_BY_ID[cid]
    I = IC.stage_inputs(c)
    se = SEModule(c.C, 1)
    se.fc1 = torch.nn.Conv2d(c.C, c.hid, 1, bias=False)
    se.fc2 = torch.nn.Conv2d(c.hid, c.C, 1, bias=False)
    se = se.double()
    with torch.no_grad():
        se.fc1.weight.copy_(I["w1"].double()[:, :, None, None])
        se.fc2.weight.copy_(I["w2"].double()[:, :, None, None])
    r = I["r"].double().requires_grad_(True)
    s = IC.stage_geometry(c)[0]
    short = I["sc"].double() if c.short == "conv" else Subsample(s)(I["x"].double())
    out = se(r) + short
    (dr,) = torch.autograd.grad(out, r, I["dout"].double())
    # the links of the chain taken in fp64 all the way: dev = the fp64 values themselves
    f = IC.stage_fwd_ref(c, I)
    for _ in range(5):                                   # feed the fp64 links back in: one more link exact per pass
        f = IC.stage_fwd_ref(c, I, dev={k: v[0] for k, v in f.items()})
    assert torch.allclose(f["out"][0], out.detach(), rtol=1e-13, atol=1e-13)
    b = IC.stage_bwd_ref(c, I, {k: v[0] for k, v in f.items()})
    b = IC.stage_bwd_ref(c, I, {k: v[0] for k, v in f.items()}, dev={k: v[0] for k, v in b.items()})
    assert torch.allclose(b["dr"][0], dr, rtol=1e-12, atol=1e-13)
    if c.xbn:
        a, bb = I["a"].double()[None, :, None, None], I["b"].double()[None, :, None, None]
        assert torch.allclose(f["xbn"][0], out.detach() * a + bb, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("nid", ["u1_16_32_s2_12", "u1_32_32_s2_34_h3", "u2_16_96_160_8", "u4_24"])
def test_net_restatement_is_module_autograd(nid):
    """net_forward == the fp64 module (BottleneckIRSE units) and net_backward on that module's own activations ==
    torch.autograd.grad."""
    c = IC.NET_BY_ID[nid]
    mod = IC.build_net(c).double()
    x, dfeat = IC.net_inputs(c)
    P = IC.net_params(mod, torch.float64)
    xr = x.double().requires_grad_(True)
    y = mod(xr)
    (dx,) = torch.autograd.grad(y, xr, dfeat.double())
    feat, z, S = IC.net_forward(P, x)
    assert torch.allclose(feat, y.detach(), rtol=1e-11, atol=1e-12)
    dimg = IC.net_backward(P, z, S, dfeat)
    assert torch.allclose(dimg, dx, rtol=1e-10, atol=1e-12 * dx.abs().max().item())
    # the leading-n prefix form: the gradient of the first face alone
    d1 = IC.net_backward(P, z, S, dfeat[:1])
    assert torch.allclose(d1, dx[:1], rtol=1e-10, atol=1e-12 * dx.abs().max().item())


# ------------------------------------------------------------------------------------------- validators

def test_every_stage_case_passes_the_validator():
    for c in IC.STAGE_CASES:
        s, in_h, in_w = IC.stage_geometry(c)
        assert IC.stage_validate(c.n, c.C, c.hid, s, in_h, in_w) is None, c.id
        assert c.oh * c.ow * c.n * c.C <= 16 * 128 * 128 * 3, c.id


BAD_STAGES = [  # (n, C, hid, stride, in_h, in_w)
    (0, 16, 1, 1, 4, 4), (1, 8, 1, 1, 4, 4), (1, 24, 1, 1, 4, 4), (1, 528, 1, 1, 4, 4), (1, 16, 0, 1, 4, 4),
    (1, 16, 257, 1, 4, 4), (1, 16, 1, 3, 6, 6), (1, 16, 1, 0, 4, 4), (1, 16, 1, 2, 5, 4), (1, 16, 1, 2, 4, 5),
    (1, 16, 1, 1, 0, 4), (8, 512, 1, 1, 1024, 512),
]


@pytest.mark.parametrize("bad", BAD_STAGES)
def test_stage_entry_points_reject_on_the_host(bad):
    """Each rejection of se_validate, by message, from both entry points; the restatement agrees."""
    from stylemc_amd import _hip
    lib = _hip.load()
    n, C, hid, s, in_h, in_w = bad
    frag = IC.stage_validate(*bad)
    assert frag is not None
    fake = ctypes.c_void_p(256)
    rc = lib.smc_irse_se_fwd_f32(fake, fake, None, s, in_h, in_w, n, C, fake, fake, hid, None, None, fake, None, fake,
                                 fake, fake, None)
    assert rc == 1 and frag.encode() in lib.smc_last_error(), (bad, lib.smc_last_error())
    if s == 1:
        rc = lib.smc_irse_se_bwd_f32(fake, fake, fake, fake, fake, fake, n, C, hid, in_h, in_w, fake, fake, None)
        assert rc == 1, bad
        err = lib.smc_last_error()
        assert frag.encode() in err or (min(in_h, in_w) < 1 and b"plane" in err), (bad, err)


def test_stage_entry_points_reject_pointers():
    from stylemc_amd import _hip
    lib = _hip.load()
    fake = ctypes.c_void_p(256)
    good = [fake, fake, None, 1, 4, 4, 1, 16, fake, fake, 1, None, None, fake, None, fake, fake, fake, None]
    for i in (0, 8, 9, 13, 15, 16, 17):
        a = list(good)
        a[i] = None
        assert lib.smc_irse_se_fwd_f32(*a) == 1 and b"null pointer" in lib.smc_last_error(), i
    a = list(good)
    a[2] = fake                                           # sc and x
    assert lib.smc_irse_se_fwd_f32(*a) == 1 and b"exactly one of sc and x" in lib.smc_last_error()
    a = list(good)
    a[1] = None                                           # neither
    assert lib.smc_irse_se_fwd_f32(*a) == 1 and b"exactly one of sc and x" in lib.smc_last_error()
    for miss in ((11,), (12,), (14,), (11, 12)):
        a = list(good)
        a[11] = a[12] = a[14] = fake
        for i in miss:
            a[i] = None
        assert lib.smc_irse_se_fwd_f32(*a) == 1 and b"go together" in lib.smc_last_error(), miss
    goodb = [fake] * 6 + [1, 16, 1, 4, 4, fake, fake, None]
    for i in (0, 1, 2, 3, 4, 5, 11, 12):
        a = list(goodb)
        a[i] = None
        assert lib.smc_irse_se_bwd_f32(*a) == 1 and b"null pointer" in lib.smc_last_error(), i


@pytest.mark.parametrize("c", IC.NETS, ids=lambda c: c.id)
def test_saved_layout_is_the_executors(c):
    """saved_layout() against smc_irse_saved_floats (host logic) on a host-side descriptor; the net passes the
    executor's validators at every n the GPU test uses."""
    from stylemc_amd import _hip, irse_hip
    lib = _hip.load()
    pk = irse_hip._Packed(IC.build_net(c), "cpu", c.hw)
    for n in range(1, c.n + 1):
        assert lib.smc_irse_saved_floats(ctypes.byref(pk.net), n) == IC.saved_layout(c, n)[2], n
        assert lib.smc_irse_workspace_bytes(ctypes.byref(pk.net), n) > 0
    for cin, depth, s, hid in c.units:
        assert (depth == 16 or depth % 32 == 0) and (cin == 16 or cin % 32 == 0), c.id
    assert pk.net.flat % 32 == 0 and pk.net.feat % 32 == 0


# ------------------------------------------------------------------------------------------- coverage

def test_stage_table_holds_every_form():
    cs = IC.STAGE_CASES
    assert {16, 32, 96, 160, 512} <= {c.C for c in cs}
    assert {1, 3, 16, 17, 33, 256} <= {c.hid for c in cs}
    assert {(1, 1), (7, 7), (3, 5), (5, 3), (15, 17), (16, 16), (257, 1), (17, 17), (16, 32), (19, 27), (56, 56),
            (128, 128)} <= {(c.oh, c.ow) for c in cs}
    assert any(c.oh == c.ow == 128 and c.C == 16 for c in cs)
    assert {1, 3} <= {c.n for c in cs}
    assert {"conv", "id1", "id2"} <= {c.short for c in cs}
    assert any(c.short == "id2" and c.oh != c.ow for c in cs)
    assert {True, False} == {c.xbn for c in cs} == {c.nocancel for c in cs}
    assert all(c.forms for c in cs)
    # every mutation of the list has stage or executor cases to which it applies
    for mut in IC.MUTATIONS:
        assert any(IC.stage_applies(c, mut) for c in cs) or any(IC.net_applies(c, mut) for c in IC.NETS), mut
    # the kernels' forms, read off the table: pixel splits 1, 2, 3, 13, 64; a ragged and a full last chunk; 1..8 lane
    # terms of the C-dots with and without a ragged one; 1, 2, 3 and 16 passes of the hidden-row loop
    assert {1, 2, 3, 13, 64} <= {IC.zsplit(c.oh * c.ow)[0] for c in cs}
    assert {True, False} == {(c.oh * c.ow) % IC.zsplit(c.oh * c.ow)[1] == 0 for c in cs}
    assert {1, 2, 3, 8} <= {IC.cdiv(c.C, 64) for c in cs} and {True, False} == {c.C % 64 == 0 for c in cs}
    assert {1, 2, 3, 16} <= {IC.cdiv(c.hid, 16) for c in cs}


def test_net_table_holds_every_net():
    want = {((16, 32, 2),): {12, 2, 112}, ((32, 32, 1),): {7}, ((32, 32, 2),): {34}, ((16, 96, 2), (96, 160, 1)): {8},
            ((16, 512, 2),): {4}, ((16, 32, 2), (32, 32, 1), (32, 64, 2), (64, 64, 1)): {24}}
    got = {}
    for c in IC.NETS:
        got.setdefault(tuple(u[:3] for u in c.units), set()).add(c.hw)
    assert got == want
    by = IC.NET_BY_ID
    assert [u[3] for u in by["u1_32_32_s1_7_h5"].units] == [5] and [u[3] for u in by["u1_32_32_s2_34_h3"].units] == [3]
    assert [u[3] for u in by["u2_16_96_160_8"].units] == [17, 33] and by["u1_16_512_s2_4"].units[0][3] == 32
    assert by["u1_16_32_s2_112"].n == 1 and by["u4_24"].n == 3 and IC.U4_TAPS == ((0, 1, 3), (1,), (3,))


# ------------------------------------------------------------------------------------------- power

@pytest.mark.parametrize("c", IC.STAGE_CASES, ids=lambda c: c.id)
def test_stage_case_tells_every_mutation_from_rounding(c):
    c, I, fwd, bwd, dev = _stage_base(c.id)
    weak = []
    for mut in IC.MUTATIONS:
        if not IC.stage_applies(c, mut):
            continue
        mf = IC.stage_fwd_ref(c, I, dev=dev, mut=mut)
        mb = IC.stage_bwd_ref(c, I, dev, dev=dev, mut=mut)
        moved = max([_ratio(mf[k][0], fwd[k][0], fwd[k][1]) for k in fwd] +
                    [_ratio(mb[k][0], bwd[k][0], bwd[k][1]) for k in bwd])
        if mut in ("dm_dropped", "mask_ignored"):                      # backward only: dr must show it
            moved = _ratio(mb["dr"][0], bwd["dr"][0], bwd["dr"][1])
        if moved < IC.POWER:
            weak.append((mut, moved))
    assert not weak, weak


@functools.lru_cache(maxsize=None)
def _net_base(nid):
    c = IC.NET_BY_ID[nid]
    mod = IC.build_net(c)
    x, dfeat = IC.net_inputs(c)
    P64, P32 = IC.net_params(mod, torch.float64), IC.net_params(mod, torch.float32)
    return c, x, dfeat, P64, P32


def _segments(feat, z, S):
    d = {"feat": feat, "z": z}
    for k, sv in enumerate(S):
        for key in ("u1", "r", "h", "g"):
            d[f"{key}{k}"] = sv[key]
    return d


@pytest.mark.parametrize("c", IC.NETS, ids=lambda c: c.id)
def test_net_case_tells_every_mutation_from_rounding(c):
    """e_ref32 on the CPU; a mutation must move a checked output by POWER x MARGIN x e_ref32 of max |ref|."""
    c, x, dfeat, P64, P32 = _net_base(c.id)
    f64 = IC.net_forward(P64, x)
    seg64, seg32 = _segments(*f64), _segments(*IC.net_forward(P32, x))
    e32 = {k: IC.rel_err(seg32[k], seg64[k]) for k in seg64}
    z32 = f64[1].float()
    S32 = [{k: v.float() for k, v in sv.items()} for sv in f64[2]]
    d64 = IC.net_backward(P64, z32, S32, dfeat)
    e32b = IC.rel_err(IC.net_backward(P32, z32, S32, dfeat), d64)
    assert 0 < e32b < 1e-5 and all(0 <= e < 1e-5 for e in e32.values()), (e32b, e32)
    weak = []
    for mut in IC.MUTATIONS:
        if not IC.net_applies(c, mut):
            continue
        moved = []
        if mut in IC.FWD_MUTS:
            segm = _segments(*IC.net_forward(P64, x, mut=mut))
            moved.append(max(IC.rel_err(segm[k], seg64[k]) / max(e32[k], IC.EPS) for k in seg64))
        if mut in IC.BWD_MUTS and (c.id, mut) not in IC.NET_WAIVED:
            moved.append(IC.rel_err(IC.net_backward(P64, z32, S32, dfeat, mut=mut), d64) / e32b)
        if min(moved) < IC.POWER * IC.MARGIN:
            weak.append((mut, moved))
    assert not weak, weak


def test_waived_pairs_have_a_stage_case():
    """A (net, mutation) pair without power in the backward names the stage case that tests the mistake at the same
    plane; that case's own power test holds it to the full condition."""
    for (nid, mut), (reason, cid) in IC.NET_WAIVED.items():
        net, st = IC.NET_BY_ID[nid], IC.STAGE_BY_ID[cid]
        assert reason and IC.net_applies(net, mut) and IC.stage_applies(st, mut)
        assert st.oh == st.ow == net.hw // net.units[0][2]
