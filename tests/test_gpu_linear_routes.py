"""Every launch form of the ViT GEMM (lin_launch, csrc/vit.hip) at the kernel level: each case of tests/linear_cases.py
runs in every form its shape admits -- {B as given, B transposed, split-bf16 planes} x {separate reduction kernel,
in-launch hand-off}; the tower's executor runs the transposed and planes kernels with the hand-off -- through
smc_linear_ex_f32, provably in that form (smc_linear_last_route / _last_nsplit / _last_reduce), against
A.double() @ B.double().

Bounds (the project's): exact-fp32 forms within 2e-5 of max |ref| (tests/test_gpu_vit.py); the planes form within 2x the
error of the exact-fp32 form of the same case and reduce mode (the smaller of "b" and "bt"), in max and in relative
norm.  Short-K fallback for the 2x ratio only, as tests/test_gpu_conv_routes.py: where the exact-fp32 error is already
below one ulp of the output's max (2^-23 max |ref|) the planes form is held instead elementwise to
|err| <= max err_fp32 + 2^-23 (|A| @ |B|), computed in fp64 (carried through the epilogue's derivative where there is one).
"""
import functools

import pytest
import torch

from stylemc_amd._hip import LIN_REDUCE_INLAUNCH, LIN_REDUCE_KERNEL, LIN_REDUCE_NONE
from tests import linear_cases as lc

pytestmark = pytest.mark.gpu
DEV = lc.DEV
REDUCE_NAMES = {LIN_REDUCE_NONE: "single pass", LIN_REDUCE_KERNEL: "reduction kernel", LIN_REDUCE_INLAUNCH: "hand-off"}

# errors recorded by test_linear_route_vs_fp64 for the table test_every_linear_route_covered prints:
# (case id, operand, handoff) -> [max error, norm error, passed by the fallback bound]
_ERRORS = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stylemc_amd import build
    build.build(verbose=False)
    torch.backends.cuda.matmul.allow_tf32 = False


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _run(cid, epi=None):
    """One launch of the case per form (shared by the tests below: no form runs twice)."""
    c = lc.BY_ID[cid]
    return {form: lc.launch(c, form[0], form[1], epi) for form in lc.forms(c)}


def _errs(got, ref):
    scale = max(ref.abs().max().item(), 1e-12)
    got = got.double()
    return (got - ref).abs().max().item() / scale, ((got - ref).norm() / ref.norm()).item()


def _check_records(c, runs):
    for (op, handoff), (_, rec) in runs.items():
        what = f"{c.id} {op} handoff={handoff}"
        assert rec.route != "none" and rec.nsplit >= 1, f"{what}: no route recorded"
        assert rec.route == lc.expected_route(c, op), f"{what}: ran {rec.route}"
        if rec.nsplit > 1:
            assert rec.reduce == (LIN_REDUCE_INLAUNCH if handoff else LIN_REDUCE_KERNEL), f"{what}: reduce {rec.reduce}"
        else:
            assert rec.reduce == LIN_REDUCE_NONE, f"{what}: reduce {rec.reduce}"
        if _cus() == 256:   # the plans the table was built for
            assert rec.nsplit == c.nsplit, f"{what}: nsplit {rec.nsplit}, the table expects {c.nsplit}"


def _check_bounds(c, runs, epi=None):
    refs = lc.reference(c.id, epi)
    errs = {form: [_errs(o, r) for o, r in zip(outs, refs)] for form, (outs, _) in runs.items()}
    for form, (_, rec) in runs.items():
        print(f"{c.id} {form[0]} {'hand-off' if form[1] else 'kernel'} epi={epi}: {rec.route} nsplit={rec.nsplit} "
              f"reduce={rec.reduce} " + " ".join(f"max {m:.3e} norm {q:.3e}" for m, q in errs[form]))
    for (op, handoff), e in errs.items():
        for k, (x_max, x_norm) in enumerate(e):
            what = f"{c.id}[{k}] {op} handoff={handoff} epi={epi}"
            key = (c.id, op, handoff)
            if epi is None:
                _ERRORS[key] = [x_max, x_norm, False]
            if op != "planes":
                assert x_max <= 2e-5, f"{what}: max err {x_max:.3e}"
                continue
            f_max = min(errs[(o, handoff)][k][0] for o in ("b", "bt"))
            f_norm = min(errs[(o, handoff)][k][1] for o in ("b", "bt"))
            if x_max <= 2 * f_max and x_norm <= 2 * f_norm:
                continue
            # Short-K fallback (module docstring): only where the exact-fp32 error is below one ulp of the output's max
            assert f_max < 2.0 ** -23, (f"{what}: max {x_max:.3e} norm {x_norm:.3e} > 2 x exact fp32 "
                                        f"max {f_max:.3e} norm {f_norm:.3e}")
            print(f"{what}: fallback (max {x_max:.3e} norm {x_norm:.3e}; exact fp32 max {f_max:.3e} norm {f_norm:.3e})")
            if epi is None:
                _ERRORS[key][2] = True
            ref, bound = refs[k], lc.reference(c.id, epi, bound=True)[k]
            excess = ((runs[(op, handoff)][0][k].double() - ref).abs() - bound).max().item()
            assert excess <= f_max * ref.abs().max().item(), (
                f"{what}: error exceeds exact fp32's {f_max:.3e} + 2^-23 (|A| @ |B|) by {excess:.3e}")


def test_case_table_is_small():
    """No case's fp64 reference exceeds the largest existing linear test, (200, 768, 3072)."""
    limit = 2 * 200 * 768 * 3072
    for c in lc.CASES:
        assert lc.flops(c) <= limit, (c.id, lc.flops(c))
    strided = [c for c in lc.CASES if c.strided]
    assert sum(lc.is_v2(c) for c in strided) >= 3 and sum(not lc.is_v2(c) for c in strided) >= 2
    assert any(lc.is_v2(c) and c.nsplit > 1 and c.M % 32 for c in strided)   # a strided hand-off case with tail rows
    assert set(lc.EPI_CASES) <= set(lc.BY_ID)


@pytest.mark.parametrize("cid", [c.id for c in lc.CASES])
def test_linear_route_vs_fp64(cid):
    """Every form of the case against fp64, with the route, nsplit and reduce mode it was asked for.

    This test found lin_gemm2_x3_kernel past the 2x bound on v2_33x64x128_ld4 (max 3.263e-07 of the max against exact
    fp32's 1.577e-07, 2.07x, with the exact-fp32 error at 1.3 ulp of the max, above the fallback's 1 ulp): all six
    products on one accumulator rounded the running result 96 times at K = 128 against the exact-fp32 kernel's 65.
    The kernel now keeps the five cross terms on an accumulator of their own (csrc/vit.hip); the case measures
    1.332e-07.  DESIGN.md section 3, ViT GEMM routes."""
    c = lc.BY_ID[cid]
    runs = _run(cid)
    _check_records(c, runs)
    _check_bounds(c, runs)


@pytest.mark.parametrize("cid", [c.id for c in lc.CASES if c.nsplit > 1])
def test_handoff_equals_reduction_kernel(cid):
    """Both reductions sum the same stored partial tiles in split order (lin_gemm_kernel's and lin_gemm2_kernel's
    hand-off loops, lin_splitk_epilogue_kernel), so the two results of one kernel are equal bit for bit -- in the one
    run each form gets.  A mismatch means the hand-off summed something else than the stored partials."""
    c = lc.BY_ID[cid]
    runs = _run(cid)
    compared = 0
    for op in sorted({op for op, _ in runs}):
        (sep,), rs = runs[(op, False)]
        (hand,), rh = runs[(op, True)]
        assert rs.route == rh.route and rs.nsplit == rh.nsplit
        if rs.nsplit == 1:   # a device with another CU count may plan a single pass
            continue
        assert (rs.reduce, rh.reduce) == (LIN_REDUCE_KERNEL, LIN_REDUCE_INLAUNCH)
        diff = (sep != hand)
        assert torch.equal(sep, hand), (f"{cid} {op} ({rs.route}, nsplit {rs.nsplit}): {int(diff.sum())} elements differ, "
                                        f"max {(sep.double() - hand.double()).abs().max().item():.3e}, first at "
                                        f"{diff.nonzero()[0].tolist()}")
        compared += 1
    if _cus() == 256:
        assert compared == len({op for op, _ in runs})


@pytest.mark.parametrize("cid", lc.EPI_CASES)
@pytest.mark.parametrize("epi", lc.EPI_KINDS)
def test_linear_epilogues_all_forms(cid, epi):
    """The three epilogues of test_gpu_vit.test_linear_epilogues -- bias + QuickGELU with the pre-activation saved at
    ld_pre = N + 4 (strided cases), bias + residual in place (C aliases the residual), the QuickGELU' multiply -- in
    every form and both reduce modes, against the fp64 epilogue under the bounds of the module docstring."""
    c = lc.BY_ID[cid]
    runs = _run(cid, epi)
    _check_records(c, runs)
    _check_bounds(c, runs, epi)


def _planes_model(b):
    """CPU integer model of the truncation split of a [K][N] fp32 matrix, in the planes layout (int16)."""
    K, N = b.shape
    hi = -65536   # 0xffff0000 as int32

    def trunc16(x):
        return (x.view(torch.int32) & hi).view(torch.float32)

    r1 = b - trunc16(b)
    r2 = r1 - trunc16(r1)
    terms = [(x.contiguous().view(torch.int32) >> 16).to(torch.int16) for x in (b, r1, r2)]
    k = torch.arange(K).view(K, 1).expand(K, N)
    n = torch.arange(N).view(1, N).expand(K, N)
    out = torch.zeros(K * N * 3, dtype=torch.int16)
    for s, t in enumerate(terms):
        idx = ((((k // 32) * 3 + s) * 4 + (k % 32) // 8) * N + n) * 8 + k % 8
        out[idx.reshape(-1)] = t.reshape(-1)
    return out, terms


@pytest.mark.parametrize("K,N,ldb", [(64, 64, 64), (96, 132, 136), (768, 512, 512)])
def test_x3_planes_bit_exact(K, N, ldb):
    """smc_linear_x3_planes == the truncation split (term 0 the top 16 bits of v, term 1 of r1 = v - trunc16(v), term 2
    of r1 - trunc16(r1), all in fp32) at ((((k/32) 3 + s) 4 + (k%32)/8) N + n) 8 + k%8, and t0 + t1 + t2 == v exactly."""
    from stylemc_amd import _hip
    lib = _hip.load()
    g = torch.Generator().manual_seed(K + N)
    b = torch.randn(K, N, generator=g) / K ** 0.5
    bd = torch.full((K, ldb), float("nan"), device=DEV)
    bd[:, :N] = b.to(DEV)
    nbytes = lib.smc_linear_x3_planes_bytes(K, N)
    assert nbytes == 6 * K * N
    out = lc.Guarded1d(nbytes // 2, torch.int16, -1, 12345)
    _hip.call("smc_linear_x3_planes", bd.data_ptr(), ldb, K, N, out.ptr(), _hip.stream())
    torch.cuda.synchronize()
    out.check(f"planes {K}x{N}")
    got = out.buf[lc.GUARD:lc.GUARD + out.n].cpu()
    want, _ = _planes_model(b)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} plane elements differ"
    # the three terms the GPU wrote, gathered back to [K][N], sum to the input bit for bit
    k = torch.arange(K).view(K, 1).expand(K, N)
    n = torch.arange(N).view(1, N).expand(K, N)
    t = []
    for s in range(3):
        idx = ((((k // 32) * 3 + s) * 4 + (k % 32) // 8) * N + n) * 8 + k % 8
        t.append((got[idx.reshape(-1)].to(torch.int32) << 16).view(torch.float32).reshape(K, N))
    total = (t[0] + t[1]) + t[2]
    assert torch.equal(total.view(torch.int32), b.view(torch.int32))


def test_every_linear_route_covered():
    """The table reaches every route, within every kernel every reduce mode and nsplit == 1, and in the two kernels the
    tower runs (B transposed, planes) an uneven split, one K step per split, 16 splits and a grid below 8.  Uses the
    launches of test_linear_route_vs_fp64 when that ran (launches the rest itself); the plans are those of 256 CUs."""
    if _cus() != 256:
        pytest.skip(f"the table's split-K plans are those of 256 CUs (this device has {_cus()})")
    names = lc.route_names()
    assert names[0] == "none" and len(set(names)) == len(names)
    seen = {}
    for c in lc.CASES:
        for (op, handoff), (_, rec) in _run(c.id).items():
            assert rec.route != "none"
            seen.setdefault(rec.route, []).append((c, op, handoff, rec))
    print()
    for name in names[1:]:
        for reduce in (LIN_REDUCE_NONE, LIN_REDUCE_KERNEL, LIN_REDUCE_INLAUNCH):
            rows = [(c, op, h, r) for c, op, h, r in seen.get(name, []) if r.reduce == reduce]
            es = [_ERRORS[(c.id, op, h)] for c, op, h, _ in rows if (c.id, op, h) in _ERRORS]
            print(f"ROUTE {name} / {REDUCE_NAMES[reduce]}: {len(rows)} launches, nsplit "
                  f"{sorted({r.nsplit for _, _, _, r in rows})}, worst max err "
                  f"{max((e[0] for e in es), default=float('nan')):.2e}, fallback "
                  f"{sorted({c.id for (c, op, h, _) in rows if _ERRORS.get((c.id, op, h), [0, 0, False])[2]})}")
    assert set(seen) == set(names[1:]), f"routes no case reaches: {sorted(set(names[1:]) - set(seen))}"
    for name, rows in seen.items():
        reduces = {r.reduce for _, _, _, r in rows}
        assert reduces == {LIN_REDUCE_NONE, LIN_REDUCE_KERNEL, LIN_REDUCE_INLAUNCH}, (name, reduces)
    for name in ("lin_gemm2_kernel<true>", "lin_gemm2_x3_kernel"):
        rows = seen[name]
        for handoff in (False, True):
            split = [(c, r) for c, _, h, r in rows if h == handoff and r.nsplit > 1]
            assert any(lc.k_steps(c) % r.nsplit for c, r in split), f"{name} handoff={handoff}: no uneven split"
            assert any(lc.k_steps(c) == r.nsplit for c, r in split), f"{name} handoff={handoff}: no one-step split"
            assert any(r.nsplit == 16 for _, r in split), f"{name} handoff={handoff}: no 16-way split"
        assert any(lc.grid(c, r.nsplit) < 8 for c, _, _, r in rows), f"{name}: no grid below 8"
        assert any(lc.grid(c, r.nsplit) % 8 for c, _, _, r in rows if lc.grid(c, r.nsplit) > 8), \
            f"{name}: no grid that is not a multiple of 8"


@pytest.mark.parametrize("products", [0, 1], ids=["fp32", "x3"])
def test_executor_takes_the_covered_forms(products, monkeypatch):
    """One smc_vit_forward_f32 of a seeded ViT-B/32 at batch 4 ends with the projection head, (4, 512, 768) in the
    table: the record shows the transposed-B kernel (products = 0) or the planes kernel (products = 1), and on 256 CUs
    the in-launch hand-off over 12 splits -- the forms the unit cases above hold to fp64."""
    from stylemc_amd import _hip, vit_hip
    lib = _hip.load()
    monkeypatch.setattr(vit_hip, "X3", bool(products))
    hip = vit_hip.build_visual("ViT-B/32", seed=4, device=DEV)
    assert hip.cfg.products == products
    x = torch.randn(4, 3, 224, 224, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        y = hip(x)
    name = lib.smc_linear_route_name(lib.smc_linear_last_route()).decode()
    nsplit, reduce = lib.smc_linear_last_nsplit(), lib.smc_linear_last_reduce()
    assert bool(torch.isfinite(y).all())
    assert name == ("lin_gemm2_x3_kernel" if products else "lin_gemm2_kernel<true>"), name
    assert "v2_4x512x768" in lc.BY_ID
    if nsplit > 1:
        assert reduce == LIN_REDUCE_INLAUNCH
    if _cus() == 256:
        assert (nsplit, reduce) == (12, LIN_REDUCE_INLAUNCH), (nsplit, reduce)
