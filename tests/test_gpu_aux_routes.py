"""Every kernel instantiation csrc/modconv_aux.hip and csrc/torgb.hip can launch, each through small cases that provably
run it (smc_modconv_aux_last_route / _last_route_flags / _last_nsplit), against an fp64 CPU reference of the same fp32
operands with a derived bound on every output element.  The case table, the references, the kink margins and the
derivation of the bounds are in tests/aux_cases.py.

Adjoint pad below 2 (smc_modconv_blur_act_bwd_f32).  With t smaller than u, a tile of the t grid used to add to dd only
the u positions inside its own 32 x 64 window, so u rows and columns beyond the last tile were summed by nobody.  The
*_pad11_*, *_pad01_* and *_pad00_* cases hold dd there (no-cancellation inputs: a dropped row is ~1/33 of dd); the last
tile of a grid row / column now owns what lies beyond it.  Above adjoint pad 3 a tile's haloed window ends before its
own last rows, so dd is rejected on the host there (tests/test_aux_cases_cpu.py) and the *_pad44_* / *_pad64_* cases
hold dT alone.
"""
import pytest
import torch

from tests import aux_cases as ac

pytestmark = pytest.mark.gpu

# id -> (route name, largest fraction of its bound any output used), for the table the coverage test prints
_USED = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stylemc_amd import build
    build.build(verbose=False)


def _fraction(err, bound):
    """max err / bound; a zero bound (a value no rounding touches) demands a zero error."""
    zero = bound == 0
    assert (err[zero] == 0).all(), "an output that must be exact is not"
    return (err[~zero] / bound[~zero]).max().item() if (~zero).any() else 0.0


def _run(cid):
    c = ac.BY_ID[cid]
    d = ac.make_inputs(c)
    assert ac.backward_margins(c, d), f"{cid}: kink margins"
    refs = ac.reference(c, d)
    try:
        outs, rep = ac.launch(c, d)
    except RuntimeError as e:    # a device error poisons the process: run nothing more on the GPU after it
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"{cid}: device error, stopping the session: {e}", returncode=3)
        raise
    want = ac.planned(c, ac.cu_count())
    assert (c.route, c.flags) == want[:2]
    assert rep[0] != "none", f"{cid}: no route recorded"
    assert rep == want, f"{cid}: ran {rep}, planned {want}"
    assert len(outs) == len(refs)
    used, cells = 0.0, []
    for got, (what, ref, bound) in zip(outs, refs):
        got = got.double().cpu().reshape(ref.shape)
        assert torch.isfinite(got).all(), f"{cid} {what}: non-finite or unwritten outputs"
        frac = _fraction((got - ref).abs(), bound.expand_as(ref))
        cells.append((what, frac))
        used = max(used, frac)
    print(f"{cid}: {rep[0]} flags={rep[1]} split={rep[2]}  " + "; ".join(f"{w}: {f:.3f} of bound" for w, f in cells))
    _USED[cid] = (rep[0], used)
    for what, frac in cells:
        assert frac <= 1.0, f"{cid} {what} ({rep[0]}): error {frac:.3f} x its bound"
    return c, d, outs


def _ids(ep):
    return [c.id for c in ac.cases_of(ep)]


@pytest.mark.parametrize("cid", _ids("blur"))
def test_blur_act_vs_fp64(cid):
    _run(cid)


@pytest.mark.parametrize("cid", _ids("blur_bwd"))
def test_blur_act_bwd_vs_fp64(cid):
    _run(cid)


@pytest.mark.parametrize("cid", _ids("act_bwd"))
def test_act_bwd_vs_fp64(cid):
    _run(cid)


@pytest.mark.parametrize("cid", _ids("epilogue"))
def test_epilogue_vs_fp64(cid):
    _run(cid)


@pytest.mark.parametrize("cid", _ids("torgb_fwd"))
def test_torgb_fwd_vs_fp64(cid):
    _run(cid)


@pytest.mark.parametrize("cid", _ids("torgb_bwd"))
def test_torgb_bwd_vs_fp64(cid):
    _run(cid)


@pytest.mark.parametrize("cid", _ids("torgb_act_bwd"))
def test_torgb_act_bwd_vs_fp64_and_unfused(cid):
    """Held to fp64, to the planned channel split, and bit-equal to smc_torgb_bwd_f32 + the sum +
    smc_modconv_act_bwd_f32 (grad_from_y), as the header promises."""
    c, d, (du,) = _run(cid)
    ref, _ = ac.launch_torgb_act_bwd(c, d, unfused=True)
    assert torch.equal(du, ref), f"{cid}: differs from the unfused passes at {(du != ref).sum().item()} elements"


@pytest.mark.parametrize("cid", _ids("channel_dot"))
def test_channel_dot_vs_fp64(cid):
    _run(cid)


@pytest.mark.parametrize("cid", _ids("demod") + _ids("demod_bwd"))
def test_demod_vs_fp64(cid):
    _run(cid)


def test_rsqrtf_error_is_within_the_recorded_figure():
    """aux_cases.RSQRT_REL is 2 x the measured error of rsqrtf alone: cin = 1, s = 1, eps = 0 make acc = wsq exactly,
    so d = rsqrtf(wsq) with no other rounding.  Prints the figure; it must stay within the recorded one."""
    from stylemc_amd import _hip
    gen = torch.Generator().manual_seed(7)
    w = torch.exp2(torch.rand(1 << 16, generator=gen) * 40 - 20)
    wsq, s = w.reshape(-1, 1).to(ac.DEV), torch.ones(1, 1, device=ac.DEV)
    out = torch.full((1, w.numel()), float("nan"), device=ac.DEV)
    _hip.call("smc_modconv_demod_f32", s.data_ptr(), wsq.data_ptr(), out.data_ptr(), 1, 1, w.numel(), 0.0, _hip.stream())
    torch.cuda.synchronize()
    ref = w.double().rsqrt()
    rel = ((out.cpu().double().reshape(-1) - ref).abs() / ref).max().item()
    print(f"rsqrtf: max relative error {rel:.3e} = {rel / 2.0 ** -24:.2f} x 2^-24 (recorded bound {ac.RSQRT_REL:.3e})")
    assert rel <= ac.RSQRT_REL


def test_every_aux_route_covered():
    """The table reaches every route of smc_modconv_aux_route_name, none waived, with both dd forms on every kernel
    that sums dd.  Launches every case itself (no reference), so it depends on no other test."""
    names = ac.route_names()
    assert names[0] == "none" and len(set(names)) == len(names)
    seen = {}
    cus = ac.cu_count()
    for c in ac.CASES:
        _, rep = ac.launch(c, ac.make_inputs(c))
        assert rep == ac.planned(c, cus), f"{c.id}: ran {rep}"
        seen.setdefault(rep[0], []).append((c.id, rep[1], rep[2]))
    print()
    for name in names[1:]:
        cells = []
        for cid, flags, ns in seen.get(name, []):
            u = _USED.get(cid)
            cells.append(f"{cid}(f{flags}/{ns}" + (f", {u[1]:.2f}" if u else "") + ")")
        worst = max((_USED[cid][1] for cid, _, _ in seen.get(name, []) if cid in _USED), default=None)
        print(f"ROUTE {name}: worst {'-' if worst is None else '%.3f' % worst} of bound; " + " ".join(cells))
    missing = set(names[1:]) - set(seen)
    assert not missing, f"routes no case reaches: {sorted(missing)}"
    for key in ("bwd_v4_u", "bwd_v4_us", "bwd_v2_u", "bwd_s_u", "act_v4_u", "act_u"):    # the kernels that sum dd
        runs = seen[ac.R[key]]
        assert {f for _, f, _ in runs} == {0, ac.DD}, f"{ac.R[key]}: dd direct and partials, got {runs}"
    splits = {ns for _, _, ns in seen[ac.R["rgb_ab_vec"]]}
    assert len(splits) >= 3, f"channel splits of torgb_act_bwd reached: {sorted(splits)}"


def test_report_reads_none_after_a_refused_call():
    from stylemc_amd import _hip
    lib = _hip.load()
    c = ac.BY_ID["channel_dot_v4_400_r1"]
    _, rep = ac.launch(c, ac.make_inputs(c))
    assert rep[0] == ac.R["dot_v4"]
    t = torch.zeros(64, device=ac.DEV)
    assert lib.smc_torgb_fwd_f32(t.data_ptr(), t.data_ptr(), t.data_ptr(), None, t.data_ptr(), 1, 4, 5, 2, 2, -1.0,
                                 _hip.stream()) == 2
    assert (lib.smc_modconv_aux_last_route(), lib.smc_modconv_aux_last_route_flags(),
            lib.smc_modconv_aux_last_nsplit()) == (0, 0, 1)
