"""The convolution weight-gradient kernel (smc_conv_wgrad_f32) against fp64, through the C ABI.

Accuracy bound: |dw - ref| <= 1e-6 * sum |grad| |inp| per element (the same index set with absolute values, in fp64).
A sequential fp32 product chain on N(0, 1) data has a worst error of 1.6e-7 .. 2.3e-7 of sum |a b| for K = 256 .. 4096
(simulated on the CPU, 512 outputs x 4 seeds per K); the exact-fp32 MFMA is such a chain (<= 3.5e-7 at K = 4096), and
split partial sums only shorten the chains.  The bound is about 3x that; every case keeps K <= 4096.
"""
import pytest
import torch

from tests import wgrad_cases as WC

pytestmark = pytest.mark.gpu

DEV = "cuda"
BOUND = 1e-6


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stylemc_amd import build
    build.build(verbose=False)


def run_kernel(c, inp, grad, extra=64):
    """dw buffer of cout*cin*k*k + extra floats, NaN-filled before the call."""
    from stylemc_amd import _hip
    lib = _hip.load()
    oh, ow = WC.out_hw(c)
    total = c.cout * c.cin * c.k * c.k
    buf = torch.full((total + extra,), float("nan"), device=DEV, dtype=torch.float32)
    nb = lib.smc_conv_wgrad_workspace_size(c.n, c.cin, c.cout, c.in_h, c.in_w, oh, ow, c.k, c.k, c.stride)
    ws = torch.full((max(nb // 4, 1),), float("nan"), device=DEV, dtype=torch.float32)
    _hip.call("smc_conv_wgrad_f32", inp.data_ptr(), c.n, c.cin, c.in_h, c.in_w, grad.data_ptr(), c.cout, oh, ow,
              c.k, c.k, c.stride, c.pad, c.pad, buf.data_ptr(), ws.data_ptr() if nb > 0 else None, nb, _hip.stream())
    torch.cuda.synchronize()
    return buf, total, lib.smc_conv_wgrad_last_nsplit(), nb


@pytest.mark.parametrize("case", [c.id for c in WC.CASES])
def test_wgrad_vs_fp64(case):
    c = WC.BY_ID[case]
    inp, grad, ref, bound = WC.reference(c)
    xi, gi = inp.to(DEV), grad.to(DEV)
    buf, total, nsplit, nb = run_kernel(c, xi, gi)
    dw = buf[:total].reshape(c.cout, c.cin, c.k, c.k)
    assert torch.isfinite(dw).all(), "dw not fully written"
    ratio = ((dw.double().cpu() - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"wgrad {case}: nsplit {nsplit}, workspace {nb} B, worst |dw - ref| / sum|g||x| = {ratio:.3e}")
    assert ratio <= BOUND, f"{case}: worst error {ratio:.3e} of sum |grad| |inp| > {BOUND:.0e}"
    # masked edges: nothing written past [cout][cin][kh][kw]
    assert torch.isnan(buf[total:]).all(), "wrote past the end of dw"
    # bit-identical from run to run
    buf2, _, nsplit2, _ = run_kernel(c, xi, gi)
    assert nsplit2 == nsplit
    assert torch.equal(buf2[:total], buf[:total]), "two calls differ"
    assert (nb > 0) == (nsplit > 1)
    if case == WC.FIRST_CASE:
        assert nsplit >= 1
    if case == WC.SPLIT_CASE and torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert nsplit > 1, "K = 4096 on one tile must split"
