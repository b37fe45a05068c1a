"""Every kernel instantiation the direct-conv dispatcher (conv_gemm_impl, csrc/conv_gemm.hip) can launch, each through
a small case that provably runs it (smc_conv_gemm_last_route) and against an fp64 CPU convolution.

Bounds (the project's): exact-fp32 MFMA within 2e-5 of max |ref|; split-bf16 within 2x the
exact-fp32 kernel's own error on the same inputs, in max and in relative norm; the epilogue outputs held to the same.
Short-K fallback for the 2x ratio only: where the exact-fp32 error is already below one ulp of the output's max
(2^-23 max |ref|) the ratio compares two roundings of the result, not two summations, and the split form is held
instead to the bound DESIGN.md section 3 derives, elementwise |err_x3| <= max err_fp32 + 2^-23 (|W| (*) |x s|), in fp64.
"""
import pytest
import torch

from stylemc_amd._hip import ROUTE_PER_SAMPLE as PER_SAMPLE
from stylemc_amd._hip import ROUTE_PRESCALE as PRESCALE
from stylemc_amd._hip import ROUTE_SPLIT_K as SPLIT_K
from stylemc_amd._hip import ROUTE_WSAMPLE as WSAMPLE
from tests import conv_cases as cc

pytestmark = pytest.mark.gpu
DEV = cc.DEV

FLAG_NAMES = {SPLIT_K: "split-K", PER_SAMPLE: "per-sample tiling", PRESCALE: "prescaled input",
              WSAMPLE: "per-sample weights"}

# Routes no table case has to reach.  One reason is admissible:
#  (a) the guard contains "input >= 2 GiB" -- all six run in test_2gib_routes / test_gpu_ops.test_conv_gemm_2gib_input_fallback
#      against the fast routes on half batches.
# (The dispatcher's route table holds no unreachable instantiation: tests/test_capi.py compares its names with this set.)
_GIB = "(a) `buf = n * cin * in_h * in_w * 4 < 2^31` false: input >= 2 GiB"
WAIVED = {
    # (a): covered by the 2 GiB tests, not by a table case
    "conv_gemm_kernel<1,4,1,1,16,false>": _GIB + " (test_gpu_ops.test_conv_gemm_2gib_input_fallback asserts it)",
    "conv_gemm_kernel<1,4,1,1,32,false>": _GIB + " (test_2gib_routes[cin512-cout32])",
    "conv_gemm_kernel<2,2,1,2,32,false>": _GIB + " (test_2gib_routes[cin512-cout64])",
    "conv_gemm_kernel<2,2,2,2,32,false>": _GIB + " (test_2gib_routes[cin512-cout128])",
    "conv_gemm_kernel<2,2,1,2,16,false>": _GIB + " (test_2gib_routes[cin256-cout64])",
    "conv_gemm_kernel<2,2,2,2,16,false>": _GIB + " (test_2gib_routes[cin256-cout128])",
}

# the families whose launches can carry each modifier flag (the kernel template name up to '<')
FAMILY_FLAGS = {
    "conv_gemm_lds_kernel": (SPLIT_K, PER_SAMPLE, PRESCALE, WSAMPLE),
    "conv_gemm_x3_kernel": (SPLIT_K, PER_SAMPLE, PRESCALE, WSAMPLE),
    "convt_lds_kernel": (SPLIT_K, PER_SAMPLE, PRESCALE, WSAMPLE),
    "convt_x3_kernel": (SPLIT_K, PER_SAMPLE, PRESCALE, WSAMPLE),
    "conv_gemm_kernel": (SPLIT_K, PRESCALE),   # register-staged: the style scale is applied in the K loop
}

# errors recorded by test_route_vs_fp64 for the table test_every_route_covered prints:
# id -> {form: (route name, max error, whether the split form passed by the short-K fallback bound)}
_ERRORS = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stylemc_amd import build
    build.build(verbose=False)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False


def _errs(got, ref):
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all(), "non-finite or unwritten outputs"
    scale = max(ref.abs().max().item(), 1e-12)
    return (got - ref).abs().max().item() / scale, ((got - ref).norm() / ref.norm()).item()


def test_case_table_is_small():
    """Every case's fp64 reference stays at or below the largest existing direct-conv case (1, 256, 256, 128)."""
    limit = 2 * 9 * 256 * 256 * 128 * 128
    for c in cc.CASES:
        assert cc.flops(c) <= limit, (c.id, cc.flops(c))


@pytest.mark.parametrize("cid", [c.id for c in cc.CASES])
def test_route_vs_fp64(cid):
    c = cc.BY_ID[cid]
    d = cc.make_inputs(c)
    refs = cc.reference(c, d)
    res = {}
    check_route = torch.cuda.get_device_properties(0).multi_processor_count == 256   # the plans the table was built for
    for form in (False, True):
        outs, route, flags, name = cc.launch(c, d, form)
        assert route != 0, f"{cid} x3={form}: no route recorded ({name})"
        if check_route:
            assert (name, flags) == cc.EXPECTED[cid][form], f"{cid} x3={form}: ran {name} flags {flags}"
        assert len(outs) == len(refs)
        res[form] = (outs, name, [_errs(o, r) for o, r in zip(outs, refs)])
        print(f"{cid} x3={form}: {name} flags={flags} " + " ".join(f"max {m:.3e} norm {q:.3e}" for m, q in res[form][2]))
    _ERRORS[cid] = {form: [res[form][1], max(m for m, _ in res[form][2]), False] for form in res}
    split_launched = res[True][1].startswith(("conv_gemm_x3_kernel", "convt_x3_kernel"))
    for k, ((f_max, f_norm), (x_max, x_norm)) in enumerate(zip(res[False][2], res[True][2])):
        what = f"{cid}[{k}]"
        assert f_max <= 2e-5, f"{what} exact fp32 ({res[False][1]}): max err {f_max:.3e}"
        if not split_launched:   # no split-bf16 form of this shape: the same exact-fp32 bound
            assert x_max <= 2e-5, f"{what} with planes ({res[True][1]}): max err {x_max:.3e}"
            continue
        if x_max <= 2 * f_max and x_norm <= 2 * f_norm:
            continue
        # Short-K fallback (module docstring): only where the exact-fp32 error is below one ulp of the output's max
        assert f_max < 2.0 ** -23, (f"{what} x3 ({res[True][1]}) max {x_max:.3e} norm {x_norm:.3e} > 2 x fp32 "
                                    f"({res[False][1]}) max {f_max:.3e} norm {f_norm:.3e}")
        _ERRORS[cid][True][2] = True
        ref, bound = refs[k], cc.reference(c, d, bound=True)[k]
        excess = ((res[True][0][k].detach().double().cpu() - ref).abs() - bound).max().item()
        assert excess <= f_max * ref.abs().max().item(), (
            f"{what} x3 ({res[True][1]}): error exceeds fp32's {f_max:.3e} + 2^-23 (|W| (*) |x s|) by {excess:.3e}")


def test_every_route_covered():
    """The table reaches every route but the WAIVED ones, and every modifier flag in every family that can set it.
    Launches every case itself (no reference), so it depends on no other test; the plans are those of 256 CUs."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip(f"the table's split-K / tile plans are those of 256 CUs (this device has {cus})")
    names = cc.route_names()
    assert names[0] == "none" and len(set(names)) == len(names)
    assert set(WAIVED) <= set(names), sorted(set(WAIVED) - set(names))
    seen, fam_flags = {}, {}
    for c in cc.CASES:
        d = cc.make_inputs(c)
        for form in (False, True):
            _, route, flags, name = cc.launch(c, d, form)
            assert route != 0, f"{c.id} x3={form}: no route recorded"
            seen.setdefault(name, []).append((c.id, form, flags))
            fam = name.split("<")[0]
            fam_flags[fam] = fam_flags.get(fam, 0) | flags
    print()
    for name in names[1:]:
        if name in seen:
            cells = []
            for cid, form, flags in seen[name]:
                e = _ERRORS.get(cid, {}).get(form)
                cells.append(f"{cid}{'/x3' if form else ''}(f{flags}{', %.1e' % e[1] if e else ''}"
                             f"{', fallback' if e and e[2] else ''})")
            print(f"ROUTE {name}: " + " ".join(cells))
        else:
            print(f"ROUTE {name}: WAIVED {WAIVED.get(name, '-- NOT WAIVED --')}")
    missing = set(names[1:]) - set(seen) - set(WAIVED)
    assert not missing, f"routes no case reaches: {sorted(missing)}"
    stale = [n for n in WAIVED if n in seen and not WAIVED[n].startswith("(a)")]
    assert not stale, f"waived as unreachable but reached: {stale}"
    for fam, flags in FAMILY_FLAGS.items():
        for f in flags:
            assert fam_flags.get(fam, 0) & f, f"{fam}: no case with {FLAG_NAMES[f]}"


@pytest.mark.parametrize("cin,cout", [(512, 32), (512, 64), (512, 128), (256, 64), (256, 128)],
                         ids=lambda v: None if v is None else (f"cin{v}" if v in (256, 512) else f"cout{v}"))
def test_2gib_routes(cin, cout):
    """Inputs of exactly 2^31 bytes (512 x 512 planes: n = 4 of 512 channels, n = 8 of 256) run the register-staged
    kernel with 64-bit addressing, in its 32-channel form from 512 channels up and its 16-channel form below.  A block
    of its output at the highest addresses (the last 16 rows of the last image) is held to the exact-fp32 bound against
    fp64, 2e-5 of the max; the whole output to the same conv on the two half batches (< 2 GiB: the LDS-DMA / row-halo
    kernels, held to that bound against fp64 by the cases above), as in
    test_gpu_ops.test_conv_gemm_2gib_input_fallback."""
    import torch.nn.functional as F
    from stylemc_amd import _hip, modconv
    lib = _hip.load()
    gen = torch.Generator().manual_seed(31)
    r = 512
    n = 2 ** 31 // (cin * r * r * 4)
    assert n * cin * r * r * 4 == 2 ** 31
    W = torch.randn(cout, cin, 3, 3, generator=gen) / (9 * cin) ** 0.5
    P = modconv.PackedConv(W.to(DEV), 1)
    P.use_x3 = False
    x = torch.randn(n, cin, r, r, device=DEV, generator=torch.Generator(device=DEV).manual_seed(37))
    ph, nph, _, _ = P.fwd_phases(r, r)
    y = torch.empty(n, cout, r, r, device=DEV)
    modconv.gemm(x, y, ph, nph, cin, cout, epi=modconv._epilogue(_hip.EPI_STORE))
    tile = {32: "1,4,1,1", 64: "2,2,1,2", 128: "2,2,2,2"}[cout]
    assert cc.route_name(lib.smc_conv_gemm_last_route()) == f"conv_gemm_kernel<{tile},{32 if cin >= 512 else 16},false>"
    # fp64 of output rows r-16 .. r-1 of the last image: input rows r-17 .. r-1 (the first output row of the strip
    # lacks its upper neighbour and is dropped)
    ref = F.conv2d(x[n - 1:, :, r - 17:].double().cpu(), W.double(), padding=1)[:, :, 1:]
    e64 = ((y[n - 1:, :, r - 16:].double().cpu() - ref).abs().max() / ref.abs().max()).item()
    y2 = torch.empty_like(y)
    h = n // 2
    for sl in (slice(0, h), slice(h, n)):
        part = torch.empty(h, cout, r, r, device=DEV)
        modconv.gemm(x[sl], part, ph, nph, cin, cout, epi=modconv._epilogue(_hip.EPI_STORE))
        assert not cc.route_name(lib.smc_conv_gemm_last_route()).startswith("conv_gemm_kernel<")
        y2[sl] = part
    err = ((y - y2).abs().max() / y2.abs().max()).item()
    print(f"2 GiB cin {cin} cout {cout}: vs fp64 {e64:.3e}, vs half batches {err:.3e}")
    assert e64 <= 2e-5, e64
    # two exact-fp32 summations of the same K = 9 cin products in different orders, each within 2e-5 of the max of
    # fp64 (the bound above, and the fast kernels' own): their difference is within the sum of the two
    assert err <= 4e-5, err
    del x, y, y2
    torch.cuda.empty_cache()
