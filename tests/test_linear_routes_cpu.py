"""Host-side checks of the ViT GEMM launcher (no GPU): the case table of tests/linear_cases.py carries the split-K
plans the library makes on 256 CUs (smc_linear_workspace_size is host logic, and without a device the library plans for
256 CUs), so a planner change shows up as a table diff instead of silently losing coverage in
tests/test_gpu_linear_routes.py; and the new entry points validate their arguments before any launch."""
import ctypes

import pytest
import torch

from stylemc_amd import _hip, build
from tests import linear_cases as lc


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the table's plans are those of 256 CUs")
    return _hip.load()


def test_linear_case_table_plans(lib):
    for c in lc.CASES:
        assert c.K % 32 == 0 and c.N % 4 == 0, c.id
        assert lc.is_v2(c) == (c.N % 64 == 0 and c.K % 64 == 0) and c.id.startswith("v2_" if lc.is_v2(c) else "v1_")
        assert 1 <= c.nsplit <= min(16, lc.k_steps(c)), c.id
        size = lib.smc_linear_workspace_size(c.M, c.N, c.K)
        if c.nsplit == 1:
            assert size == 0, (c.id, size)
        else:
            assert size % (4 * c.M * c.N) == 0 and size // (4 * c.M * c.N) == c.nsplit, (c.id, size / (4 * c.M * c.N))
    v2 = [c for c in lc.CASES if lc.is_v2(c)]
    # the edges the GPU coverage test asks of the kernels the tower runs
    assert any(lc.k_steps(c) % c.nsplit for c in v2 if c.nsplit > 1)
    assert any(lc.k_steps(c) == c.nsplit for c in v2 if c.nsplit > 1)
    assert any(c.nsplit == 16 for c in v2) and any(lc.grid(c, c.nsplit) < 8 for c in v2)
    assert any(c.nsplit == 1 for c in v2) and any(c.nsplit == 1 for c in lc.CASES if not lc.is_v2(c))


def test_linear_route_names(lib):
    names = lc.route_names()
    assert names == ["none", "lin_gemm_kernel", "lin_gemm2_kernel<false>", "lin_gemm2_kernel<true>",
                     "lin_gemm2_x3_kernel"]
    assert lib.smc_linear_route_name(-1) is None and lib.smc_linear_route_name(len(names)) is None
    assert {lc.expected_route(c, op) for c in lc.CASES for op, _ in lc.forms(c)} == set(names[1:])


def test_linear_host_validation_without_gpu(lib):
    assert lib.smc_linear_counter_ints(200, 768) == 7 * 12
    assert lib.smc_linear_counter_ints(1, 4) == 1
    assert lib.smc_linear_x3_planes_bytes(64, 128) == 64 * 128 * 6
    fake = ctypes.c_void_p(256)
    rc = lib.smc_linear_x3_planes(fake, 64, 48, 64, fake, None)
    assert rc == 2 and b"K % 32" in lib.smc_last_error()
    rc = lib.smc_linear_x3_planes(None, 64, 64, 64, fake, None)
    assert rc == 1 and b"null" in lib.smc_last_error()
    # a split-K call (nsplit 3) whose workspace is one float short fails on the host, in every form, and records no route
    M, N, K = 200, 768, 3072
    need = lib.smc_linear_workspace_size(M, N, K)
    assert need == 3 * M * N * 4
    for bt, planes, counters in ((None, None, None), (fake, None, fake), (None, fake, fake)):
        rc = lib.smc_linear_ex_f32(fake, K, fake, N, fake, N, M, N, K, None, fake, need - 4, bt, planes, counters, None)
        assert rc == 1 and b"workspace" in lib.smc_last_error()
        assert lib.smc_linear_last_route() == 0 and lib.smc_linear_last_nsplit() == 0
        assert lib.smc_linear_last_reduce() == 0
    rc = lib.smc_linear_ex_f32(fake, K, fake, N, fake, N, M, N, K, None, fake, need, ctypes.c_void_p(260), None, None, None)
    assert rc == 1 and b"aligned" in lib.smc_last_error()
