"""The IR-SE50 executor's own kernels (csrc/irse.hip) against fp64, case by case (tests/irse_cases.py holds the tables,
the references and the bounds; tests/test_irse_cases_cpu.py holds the cases to their power).

Stage cases: the two SE launch pairs through smc_irse_se_fwd_f32 / smc_irse_se_bwd_f32 into NaN-filled outputs, every
element within its bound of fp64 computed from the device's own operands, and bit-identical on a second run (no atomics).
Executor cases: small networks through smc_irse_forward_f32 / _backward_f32 / _trunk_f32 with the small-plane Winograd
switch on and off, every saved segment, feat, the trunk taps and dimg within MARGIN x the reference's own fp32 error.
The product net: the same backward-from-saved check on the seeded IR-SE50 at n = 2.
Each test prints its figures (fraction of the bound, e_hip / e_ref32) before it asserts; DESIGN.md "IR-SE50 executor
stages" records them.
"""
import pytest
import torch

from tests import irse_cases as IC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stylemc_amd import build
    build.build(verbose=False)


def _frac(a, ref, bound):
    """Largest |a - ref| / bound; an unwritten (NaN) element is infinite, an exact one 0 whatever its bound."""
    d = (a.double() - ref).abs()
    f = torch.where(d > 0, d / bound.clamp_min(1e-300), torch.zeros_like(d))
    f = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), f)
    return f.max().item()


@pytest.mark.parametrize("c", IC.STAGE_CASES, ids=lambda c: c.id)
def test_stage_case(c):
    I = IC.stage_inputs(c)
    fwd = IC.run_stage_fwd(c, I)
    bwd = IC.run_stage_bwd(c, I, fwd)
    fr = {}
    for name, (ref, bound) in IC.stage_fwd_ref(c, I, dev=fwd).items():
        fr[name] = _frac(fwd[name], ref, bound)
    for name, (ref, bound) in IC.stage_bwd_ref(c, I, fwd, dev=bwd).items():
        fr[name] = _frac(bwd[name], ref, bound)
    print(f"\nirse stage {c.id}: fraction of bound " + " ".join(f"{k} {v:.3f}" for k, v in fr.items()))
    assert set(fr) == {"m", "h", "g", "out", "dg", "dr"} | ({"xbn"} if c.xbn else set())
    fwd2 = IC.run_stage_fwd(c, I)
    bwd2 = IC.run_stage_bwd(c, I, fwd2)
    for k in fwd:
        assert torch.equal(fwd[k], fwd2[k]), f"{k} differs between two runs"
    for k in bwd:
        assert torch.equal(bwd[k], bwd2[k]), f"{k} differs between two runs"
    assert all(v <= 1.0 for v in fr.values()), fr


def test_expf_error_is_within_the_recorded_figure():
    """expf's relative error over exact arguments (irse_cases.expf_probe) stays within the recorded EXPF_REL, which is
    2 x the measured figure: at most EXPF_REL, and no less than a quarter of it (the record is then stale)."""
    c, I, t = IC.expf_probe()
    worst = 0.0
    for row in t:
        I["w2"] = row.reshape(16, 1).clone()
        o = IC.run_stage_fwd(c, I)
        assert torch.equal(o["m"], torch.ones(1, 16)) and torch.equal(o["h"], torch.ones(1, 1))
        ref = torch.sigmoid(row.double())
        worst = max(worst, ((o["g"][0].double() - ref).abs() / ref).max().item())
    print(f"\nirse expf: largest relative error {worst:.4e} ({worst / IC.EPS:.3f} x 2^-24) over {t.numel()} arguments")
    assert IC.EXPF_REL / 4 <= worst <= IC.EXPF_REL, worst


def _segments(feat, z, S):
    d = {"feat": feat, "z": z}
    for k, sv in enumerate(S):
        for key in ("u1", "r", "h", "g"):
            d[f"{key}{k}"] = sv[key]
    return d


_REF = {}


def _net_ref(c):
    """fp64 and fp32 CPU forward of a net case, once for both Winograd settings."""
    if c.id not in _REF:
        mod = IC.build_net(c)
        x, dfeat = IC.net_inputs(c)
        P64, P32 = IC.net_params(mod, torch.float64), IC.net_params(mod, torch.float32)
        f64, f32 = IC.net_forward(P64, x), IC.net_forward(P32, x)
        _REF[c.id] = (mod, x, dfeat, P64, P32, f64, f32)
    return _REF[c.id]


def _check_backward(tag, P64, P32, z, S, dfeat, dimg):
    ref = IC.net_backward(P64, z, S, dfeat)
    e32 = IC.rel_err(IC.net_backward(P32, z, S, dfeat), ref)
    e = IC.rel_err(dimg, ref)
    print(f"irse net {tag}: dimg e_hip {e:.3e} e_ref32 {e32:.3e} ratio {e / e32:.2f}")
    return e / e32


@pytest.mark.parametrize("wino_sp", [True, False], ids=["wino", "direct"])
@pytest.mark.parametrize("c", IC.NETS, ids=lambda c: c.id)
def test_net_case(c, wino_sp):
    mod, x, dfeat, P64, P32, f64, f32 = _net_ref(c)
    u4 = c.id == "u4_24"
    res = IC.run_net(c, mod, x, dfeat, wino_sp, n_grads=range(1, c.n + 1) if u4 else None,
                     taps=IC.U4_TAPS if u4 else ())
    tag = f"{c.id} {'wino' if wino_sp else 'direct'}"
    ratios = {}
    # forward: feat and every saved segment
    z, S = IC.split_saved(c, c.n, res["saved"])
    got = _segments(res["feat"], z, S)
    seg64, seg32 = _segments(*f64), _segments(*f32)
    print()
    for k in seg64:
        e, e32 = IC.rel_err(got[k], seg64[k]), IC.rel_err(seg32[k], seg64[k])
        ratios[k] = e / e32 if e32 > 0 else (0.0 if e == 0 else float("inf"))
        print(f"irse net {tag}: {k} e_hip {e:.3e} e_ref32 {e32:.3e} ratio {ratios[k]:.2f}")
    # trunk taps against the same units' outputs
    for tp, outs in res["taps"].items():
        for k, o in zip(tp, outs):
            ref = f64[2][k]["out"]
            e, e32 = IC.rel_err(o, ref), IC.rel_err(f32[2][k]["out"], ref)
            ratios[f"tap{tp}:{k}"] = e / e32
            print(f"irse net {tag}: taps {tp} unit {k} e_hip {e:.3e} e_ref32 {e32:.3e} ratio {e / e32:.2f}")
    # backward from the device's own saved buffer, for every leading-n prefix
    for ng, dimg in res["dimg"].items():
        ratios[f"dimg{ng}"] = _check_backward(f"{tag} n {ng} of {c.n}", P64, P32, z, S, dfeat[:ng], dimg)
    assert all(v <= IC.MARGIN for v in ratios.values()), {k: v for k, v in ratios.items() if v > IC.MARGIN}


def test_irse50_backward_from_saved_vs_fp64():
    """The product net's shapes under the same rule: the seeded IR-SE50 at n = 2, dimg against the fp64 restatement of
    the backward evaluated on the device's own saved buffer, within MARGIN x the fp32 restatement's error."""
    from stylemc_amd import synthetic
    from stylemc_amd.id_loss.model_irse import STAGES, Backbone
    mod = Backbone(112, 50, "ir_se", 0.6).eval()
    mod.load_state_dict(synthetic.seeded_state_dict(mod, seed=3))
    mod.requires_grad_(False)
    units = []
    for cin, depth, k in STAGES[50]:
        units += [(cin, depth, 2, depth // 16)] + [(depth, depth, 1, depth // 16)] * (k - 1)
    c = IC.Net("irse50", tuple(units), 112, 2, 3, 1.0, "the product")
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 112, 112, generator=gen)
    dfeat = torch.randn(2, 512, generator=gen)
    res = IC.run_net(c, mod, x, dfeat, True)
    z, S = IC.split_saved(c, 2, res["saved"])
    P64, P32 = IC.net_params(mod, torch.float64), IC.net_params(mod, torch.float32)
    print()
    ratio = _check_backward("irse50 n 2", P64, P32, z, S, dfeat, res["dimg"][2])
    assert ratio <= IC.MARGIN, ratio
