"""Every kernel instantiation the two Winograd dispatchers can launch (smc_conv3x3_wino_ws_f32: wino_kernel<TC,SM,EK>,
csrc/wino.hip; smc_conv3x3_wino4_f32: wino4_kernel<SM,EK>, csrc/wino4.hip), each through a small case that provably
runs it (smc_conv3x3_wino_last_route / smc_conv3x3_wino4_last_route), and every epilogue form on every block shape,
against an fp64 CPU reference of the same fp32 operands.

The case table, the reference and the derivation of the bounds are in tests/wino_cases.py: raw conv outputs within
TOL B elementwise (F(2x2) 2e-6, F(4x4) 8e-6; B the conv of the operands' magnitudes) and REL in relative norm
(1e-6 / 1e-5), epilogue outputs within gain (|d scale_c| TOL B + 4 2^-24 S) + 2^-24 |residual| at every element.

Short K.  The TOL factors were measured from cin = 16 (F(2x2)) and 12 (F(4x4)) up.  A cin = 4 / 8 case that exceeds
them is listed in wino_cases.SHORT_K with the max err / B of the CPU fp32 model of the same arithmetic
(wino_cases.model_conv: the algorithm, not the kernel, produces the error) and the kernel's figure; it is then held to
the same bounds with twice the model's error, recomputed on the same inputs, in TOL's place.  One case needs it:
f4_prelu_n3_interior (cin = 4), model 1.458e-5 B, kernel 1.42e-5 B.  tests/test_wino_predicates.py checks on the CPU
that every entry has cin 4 or 8 and that the model itself exceeds TOL there.
"""
import pytest
import torch

from tests import wino_cases as wc

pytestmark = pytest.mark.gpu

# Routes no table case has to reach.  One reason is admissible:
#  (a) the route is off by default and asserted by an existing test that enables it.
_X3 = ("(a) `wino_x3_bytes() > 0` needs `g_wino_x3` != 0 (smc_set_wino_x3, 0 by default): asserted by "
       "test_gpu_wino.test_wino_x3_vs_fp64 and test_wino_x3_modact_vs_fp32_kernel, which enable it")
WAIVED = {"wino_x3r_kernel<1>": _X3, "wino_x3r_kernel<2>": _X3}

FLAG_NAMES = {wc.SPLIT: "split-K", wc.FOLD: "style folded into U"}

# errors recorded by test_wino_route_vs_fp64 for the table test_every_wino_route_covered prints:
# id -> (max err / B over the raw conv outputs or None, largest fraction of its bound any output used)
_ERRORS = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stylemc_amd import build
    build.build(verbose=False)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False


def test_wino_case_table_is_small():
    """Every case's fp64 reference stays at or below the cap of the direct-conv table
    (test_gpu_conv_routes.test_case_table_is_small)."""
    limit = 2 * 9 * 256 * 256 * 128 * 128
    for c in wc.CASES:
        assert wc.flops(c) <= limit, (c.id, wc.flops(c))


@pytest.mark.parametrize("cid", [c.id for c in wc.CASES])
def test_wino_route_vs_fp64(cid):
    c = wc.BY_ID[cid]
    d = wc.make_inputs(c)
    u64, B = wc.conv64(c, d)
    tol = wc.TOL[c.fam]
    if cid in wc.SHORT_K:   # module docstring: twice the CPU fp32 model's error on the same inputs
        model = ((wc.model_conv(c, d).double() - u64).abs() / B).max().item()
        print(f"{cid}: CPU fp32 model max err / B {model:.3e} (recorded {wc.SHORT_K[cid][0]:.3e})")
        tol = 2 * model
    refs = wc.reference(c, d, u64, B, tol)
    outs, name, flags, ns = wc.launch(c, d)
    if cid in wc.SHORT_K:
        of_tol = max(((o.double().cpu() - r[1]).abs() / r[2]).max().item()
                     for o, r in zip(outs, wc.reference(c, d, u64, B, wc.TOL[c.fam])))
        print(f"{cid}: kernel {of_tol:.2f} x the bound with TOL (recorded {wc.SHORT_K[cid][1]:.2f})")
    assert name != "none", f"{cid}: no route recorded"
    assert (name, flags, ns) == wc.EXPECTED[cid], f"{cid}: ran {name} flags {flags} splits {ns}"
    assert len(outs) == len(refs)
    raw_ratio, used, cells = None, 0.0, []
    for got, (what, ref, bound, raw) in zip(outs, refs):
        got = got.double().cpu()
        assert torch.isfinite(got).all(), f"{cid} {what}: non-finite or unwritten outputs"
        err = (got - ref).abs()
        frac = (err / bound).max().item()
        rel = ((got - ref).norm() / ref.norm()).item()
        used = max(used, frac)
        cell = f"{what}: {frac:.2f} of bound, norm {rel:.3e}"
        if raw:
            ratio = (err / (bound / tol)).max().item()   # bound / tol = |factor| B
            raw_ratio = max(raw_ratio or 0.0, ratio)
            cell += f", max err / B {ratio:.3e}"
        cells.append((what, frac, rel, raw, cell))
    print(f"{cid}: {name} flags={flags} splits={ns}  " + "; ".join(x[4] for x in cells))
    _ERRORS[cid] = (raw_ratio, used)
    for what, frac, rel, raw, _ in cells:
        assert frac <= 1.0, f"{cid} {what} ({name}): error {frac:.3f} x its bound"
        if raw:
            assert rel <= wc.REL[c.fam], f"{cid} {what} ({name}): relative norm error {rel:.3e}"


def test_every_wino_route_covered():
    """The table reaches every route of both families but the WAIVED ones, and a waived route no case reaches.
    Launches every case itself (no reference), so it depends on no other test.  The split target is a constant and
    the plans do not depend on the CU count, so the assertions are unconditional."""
    print()
    for fam in (2, 4):
        names = wc.route_names(fam)
        assert names[0] == "none" and len(set(names)) == len(names)
        waived = {k: v for k, v in WAIVED.items() if k.startswith("wino4_") == (fam == 4)}
        assert set(waived) <= set(names), sorted(set(waived) - set(names))
        seen = {}
        for c in wc.CASES:
            if c.fam != fam:
                continue
            _, name, flags, ns = wc.launch(c, wc.make_inputs(c))
            assert (name, flags, ns) == wc.EXPECTED[c.id], f"{c.id}: ran {name} flags {flags} splits {ns}"
            seen.setdefault(name, []).append((c.id, flags, ns))
        for name in names[1:]:
            if name in seen:
                cells = []
                for cid, flags, ns in seen[name]:
                    e = _ERRORS.get(cid)
                    err = "" if e is None else (f", {e[0]:.1e} B" if e[0] is not None else "") + f", {e[1]:.2f} of bound"
                    cells.append(f"{cid}(f{flags}{'/%d' % ns if ns > 1 else ''}{err})")
                print(f"ROUTE {name}: " + " ".join(cells))
            else:
                print(f"ROUTE {name}: WAIVED {waived.get(name, '-- NOT WAIVED --')}")
        missing = set(names[1:]) - set(seen) - set(waived)
        assert not missing, f"routes no case reaches: {sorted(missing)}"
        stale = sorted(n for n in waived if n in seen)
        assert not stale, f"waived but reached by a case: {stale}"
        if fam == 2:   # both modifier flags on both block shapes, alone and together
            for tc in (16, 32):
                got = {f for n, v in seen.items() if n.startswith(f"wino_kernel<{tc},") for _, f, _ in v}
                for f in (wc.SPLIT, wc.FOLD, wc.SPLIT | wc.FOLD):
                    assert f in got, f"TC {tc}: no case with flags {f}"


def test_every_epilogue_form_on_every_block_shape():
    """Each epilogue form runs on a TC = 16, a TC = 32 and an F(4x4) case, with the EK its guard selects."""
    for form in wc.FORMS:
        for g in wc.GEOM:
            hit = [c for c in wc.CASES if c.epi == form and c.id.startswith(g + "_") and not c.id.startswith(g + "_split")]
            assert hit, (form, g)
            for c in hit:
                assert wc.EXPECTED[c.id][0].endswith(f",{wc.epilogue_body(form)}>"), c.id
    for g in ("tc16", "tc32"):   # the split form with store, modact_lrelu and PRELU
        split = {c.epi for c in wc.CASES if c.id.startswith(g + "_split")}
        assert split == {"store", "modact_lrelu", "prelu"}, (g, split)


def test_route_report_reads_none_after_a_refused_call():
    """A call that fails on the host before its launch leaves route 0 ("none")."""
    from stylemc_amd import _hip
    lib = _hip.load()
    c = wc.BY_ID["tc16_store_k1_whole"]
    _, name, _, _ = wc.launch(c, wc.make_inputs(c))
    assert name != "none"
    t = torch.zeros(64 * 64 * 64, device=wc.DEV)
    rc = lib.smc_conv3x3_wino_f32(t.data_ptr(), 1, 32, 6, 64, t.data_ptr(), 32, t.data_ptr(), None, None, _hip.stream())
    assert rc == 2   # h = 6, w = 64: no block divides the tile grid
    assert lib.smc_conv3x3_wino_last_route() == 0 and lib.smc_conv3x3_wino_last_route_flags() == 0
    assert lib.smc_conv3x3_wino_last_nsplit() == 0
    c = wc.BY_ID["f4_store_k1_whole"]
    _, name, _, _ = wc.launch(c, wc.make_inputs(c))
    assert name != "none"
    rc = lib.smc_conv3x3_wino4_f32(t.data_ptr(), 1, 32, 12, 64, t.data_ptr(), 64, t.data_ptr(), None, None, _hip.stream())
    assert rc == 2 and lib.smc_conv3x3_wino4_last_route() == 0
