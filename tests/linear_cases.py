"""Shared helpers of tests/test_gpu_linear_routes.py and tests/test_linear_routes_cpu.py: the case table of the ViT GEMM
launcher (lin_launch in csrc/vit.hip), one launch of a case through smc_linear_ex_f32 in a given form, and its fp64 CPU
reference.

A case is (id, M, N, K, nsplit, strided):
  M, N, K   C[M][N] = A[M][K] . B[K][N]
  nsplit    the split-K factor the launcher plans on 256 CUs (lin_nsplit2 on 128 CUs for the 32 x 64-tile kernels,
            N % 64 == 0 and K % 64 == 0; lin_nsplit on 256 CUs for the 32 x 128-tile kernel).  test_linear_routes_cpu
            holds the column to smc_linear_workspace_size, which is host logic and plans for 256 CUs without a device.
  strided   lda = K + 4, ldb = N + 4, ldc = N + 4 (and the epilogue operands' pitches N + 4) instead of the dense pitches
A form is (operand, handoff):
  operand   "b": B as given [K][N]; "bt": B transposed [N][K] as well (the executor's exact-fp32 form); "planes": B's
            split-bf16 planes as well (the executor's products = 1 form).  The 32 x 128-tile kernel has "b" only.
  handoff   True: zeroed counters, the in-launch split-K hand-off (the executor's); False: the separate reduction kernel
"""
import collections
import ctypes
import functools

import torch

DEV = "cuda"
PAD_ROWS = 32        # sentinel rows before and after an output: a whole tile of rows past M
GUARD = 64           # sentinel elements before and after the workspace and the counters (keeps 16-B alignment)
SENTINEL = -1234.5
ISENTINEL = -7777

Case = collections.namedtuple("Case", "id M N K nsplit strided")


def _c(M, N, K, nsplit, strided=False):
    v2 = N % 64 == 0 and K % 64 == 0
    return Case(f"{'v2' if v2 else 'v1'}_{M}x{N}x{K}{'_ld4' if strided else ''}", M, N, K, nsplit, strided)


CASES = [
    # ---- 32 x 64 tiles (N % 64 == 0, K % 64 == 0): grid = ceil(M / 32) (N / 64) nsplit, K steps of 64
    _c(1, 64, 64, 1),                      # one tile, one K step, grid 1
    _c(33, 64, 128, 1, strided=True),      # one tail row; grid 2
    _c(200, 2304, 768, 1),                 # the qkv product: 252 tiles, grid % 8 = 4
    _c(400, 768, 768, 2),                  # grid 312
    _c(200, 768, 3072, 3),                 # c_proj: 16 K steps per split; M tail of 8
    _c(70, 192, 320, 5),                   # one K step per split; grid 45
    _c(31, 128, 448, 7),                   # one K step per split; grid 14
    _c(97, 320, 704, 6, strided=True),     # 11 K steps over 6 splits: uneven ranges; one tail row
    _c(200, 64, 1088, 9, strided=True),    # 17 K steps over 9 splits: uneven; grid 63; M tail of 8
    _c(17, 64, 1344, 11, strided=True),    # 21 K steps over 11 splits: uneven; one tile; grid 11
    _c(4, 512, 768, 12),                   # the tower's projection head at batch 4: one K step per split
    _c(50, 192, 1024, 16),                 # the cap of 16 splits: one K step per split
    # ---- 32 x 128 tiles (the rest): grid = ceil(M / 32) x ceil(N / 128) x nsplit, K steps of 32
    _c(1, 4, 32, 1),
    _c(37, 132, 64, 1, strided=True),      # N tail inside a 128-wide tile
    _c(50, 256, 96, 3),                    # one K step per split
    _c(33, 100, 160, 5, strided=True),     # one K step per split; one tail row
    _c(40, 68, 1056, 11),                  # 33 K steps over 11 splits
    _c(70, 132, 992, 16, strided=True),    # 31 K steps over 16 splits: uneven
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

EPI_KINDS = ("gelu_pre", "residual_inplace", "dact")
EPI_CASES = ["v2_33x64x128_ld4", "v2_200x64x1088_ld4", "v2_4x512x768", "v1_37x132x64_ld4", "v1_33x100x160_ld4"]


def is_v2(c):
    return c.N % 64 == 0 and c.K % 64 == 0


def k_steps(c):
    return c.K // (64 if is_v2(c) else 32)


def grid(c, nsplit):
    """Workgroups of the launch (the 32 x 64-tile kernels' flat grid; the 32 x 128-tile kernel's x * y * z)."""
    mt = (c.M + 31) // 32
    return mt * (c.N // 64 if is_v2(c) else (c.N + 127) // 128) * nsplit


def forms(c):
    ops = ("b", "bt", "planes") if is_v2(c) else ("b",)
    return [(op, handoff) for op in ops for handoff in (False, True)]


def expected_route(c, op):
    if not is_v2(c):
        return "lin_gemm_kernel"
    return {"b": "lin_gemm2_kernel<false>", "bt": "lin_gemm2_kernel<true>", "planes": "lin_gemm2_x3_kernel"}[op]


def flops(c):
    return 2 * c.M * c.N * c.K


def route_names():
    from stylemc_amd import _hip
    lib = _hip.load()
    return [lib.smc_linear_route_name(i).decode() for i in range(lib.smc_linear_route_count())]


def qgelu(x):
    return x * torch.sigmoid(1.702 * x)


def qgelu_grad(x):
    s = torch.sigmoid(1.702 * x)
    return s + 1.702 * x * s * (1 - s)


@functools.lru_cache(maxsize=None)
def host_inputs(cid):
    """Seeded CPU operands of a case and its fp64 references, computed once and shared (read-only)."""
    c = BY_ID[cid]
    g = torch.Generator().manual_seed(c.M * 7 + c.N + c.K)
    d = {"a": torch.randn(c.M, c.K, generator=g), "b": torch.randn(c.K, c.N, generator=g) / c.K ** 0.5,
         "bias": torch.randn(c.N, generator=g), "res": torch.randn(c.M, c.N, generator=g),
         "pre_in": torch.randn(c.M, c.N, generator=g)}
    d["ref"] = d["a"].double() @ d["b"].double()
    return d


def reference(cid, epi=None, bound=False):
    """fp64 outputs of a case under an epilogue kind (a list: the output, and the saved pre-activation for gelu_pre).
    bound: instead the elementwise split-bf16 product bound 2^-23 (|A| @ |B|) carried through the epilogue's
    derivative (bias and residual: 1; QuickGELU: sup |QuickGELU'| < 1.1; dact: |QuickGELU'(pre)|)."""
    d = host_inputs(cid)
    acc = d["ref"]
    if bound:
        bd = 2.0 ** -23 * (d["a"].double().abs() @ d["b"].double().abs())
        if epi == "gelu_pre":
            return [1.1 * bd, bd]
        if epi == "dact":
            return [bd * qgelu_grad(d["pre_in"].double()).abs()]
        return [bd]
    if epi is None:
        return [acc]
    if epi == "gelu_pre":
        z = acc + d["bias"].double()
        return [qgelu(z), z]
    if epi == "residual_inplace":
        return [acc + d["bias"].double() + d["res"].double()]
    if epi == "dact":
        return [acc * qgelu_grad(d["pre_in"].double())]
    raise ValueError(epi)


class Guarded2d:
    """An [M][N] matrix of row pitch ld inside a larger buffer: PAD_ROWS sentinel rows before and after, the pad columns
    sentinel too; the real elements NaN (or `fill`)."""

    def __init__(self, M, N, ld, fill=None):
        self.M, self.N = M, N
        self.buf = torch.full((M + 2 * PAD_ROWS, ld), SENTINEL, device=DEV)
        self.real = self.buf[PAD_ROWS:PAD_ROWS + M, :N]
        if fill is None:
            self.real.fill_(float("nan"))
        else:
            self.real.copy_(fill)

    def ptr(self):
        return self.real.data_ptr()

    def check(self, what):
        out = self.real.cpu()
        rest = self.buf.cpu().clone()
        rest[PAD_ROWS:PAD_ROWS + self.M, :self.N] = SENTINEL
        assert bool((rest == SENTINEL).all()), f"{what}: wrote outside its [M][N] block"
        assert bool(torch.isfinite(out).all()), f"{what}: non-finite or unwritten outputs"
        return out


class Guarded1d:
    """n elements (exactly the size a query returned) between GUARD sentinels."""

    def __init__(self, n, dtype, fill, sentinel):
        self.n, self.sentinel = n, sentinel
        self.buf = torch.full((n + 2 * GUARD,), sentinel, device=DEV, dtype=dtype)
        self.buf[GUARD:GUARD + n] = fill

    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.buf.element_size() if self.n else None

    def check(self, what):
        b = self.buf.cpu()
        assert bool((b[:GUARD] == self.sentinel).all() and (b[GUARD + self.n:] == self.sentinel).all()), \
            f"{what}: wrote outside the queried size"


@functools.lru_cache(maxsize=None)
def device_inputs(cid):
    """The case's operands on the device at the case's pitches; "bt" and "planes" are built from the (strided) B."""
    from stylemc_amd import _hip
    lib = _hip.load()
    c, h = BY_ID[cid], host_inputs(cid)
    pad = 4 if c.strided else 0
    d = {"ld_n": c.N + pad}
    a = torch.zeros(c.M, c.K + pad, device=DEV)
    a[:, :c.K] = h["a"].to(DEV)
    b = torch.zeros(c.K, c.N + pad, device=DEV)
    b[:, :c.N] = h["b"].to(DEV)
    d["a"], d["b"] = a, b
    d["bias"] = h["bias"].to(DEV)
    d["pre_in"] = torch.zeros(c.M, c.N + pad, device=DEV)
    d["pre_in"][:, :c.N] = h["pre_in"].to(DEV)
    if is_v2(c):
        d["bt"] = b[:, :c.N].t().contiguous()
        nbytes = lib.smc_linear_x3_planes_bytes(c.K, c.N)
        assert nbytes == c.K * c.N * 6
        d["planes"] = torch.empty(nbytes // 2, device=DEV, dtype=torch.int16)
        _hip.call("smc_linear_x3_planes", b.data_ptr(), b.stride(0), c.K, c.N, d["planes"].data_ptr(), _hip.stream())
    return d


Record = collections.namedtuple("Record", "route nsplit reduce")


def launch(c, op, handoff, epi=None):
    """One smc_linear_ex_f32 call of the case in a form, with the workspace and the counters sized exactly by the
    queries and every written buffer between sentinels.  Returns (outputs on the CPU as reference() lists them,
    Record(route name, nsplit, reduce mode))."""
    from stylemc_amd import _hip
    lib = _hip.load()
    d, h = device_inputs(c.id), host_inputs(c.id)
    ld = d["ld_n"]
    out = Guarded2d(c.M, c.N, ld, fill=h["res"].to(DEV) if epi == "residual_inplace" else None)
    pre = None
    e = _hip.LinearEpilogue()
    if epi == "gelu_pre":
        pre = Guarded2d(c.M, c.N, ld)
        e.bias, e.act, e.pre_save, e.ld_pre = d["bias"].data_ptr(), _hip.LIN_ACT_QUICKGELU, pre.ptr(), ld
    elif epi == "residual_inplace":
        e.bias, e.residual, e.ld_res = d["bias"].data_ptr(), out.ptr(), ld
    elif epi == "dact":
        e.dact_pre, e.ld_dact = d["pre_in"].data_ptr(), ld
    wsb = lib.smc_linear_workspace_size(c.M, c.N, c.K)
    ws = Guarded1d(wsb // 4, torch.float32, float("nan"), SENTINEL)
    nctr = lib.smc_linear_counter_ints(c.M, c.N)
    ctr = Guarded1d(nctr if handoff else 0, torch.int32, 0, ISENTINEL)
    _hip.call("smc_linear_ex_f32", d["a"].data_ptr(), d["a"].stride(0), d["b"].data_ptr(), d["b"].stride(0), out.ptr(),
              ld, c.M, c.N, c.K, ctypes.byref(e) if epi is not None else None, ws.ptr(), wsb,
              d["bt"].data_ptr() if op == "bt" else None, d["planes"].data_ptr() if op == "planes" else None,
              ctr.ptr(), _hip.stream())
    rec = Record(lib.smc_linear_route_name(lib.smc_linear_last_route()).decode(), lib.smc_linear_last_nsplit(),
                 lib.smc_linear_last_reduce())
    torch.cuda.synchronize()
    what = f"{c.id} {op} handoff={handoff} epi={epi}"
    outs = [out.check(what + " C")]
    if pre is not None:
        outs.append(pre.check(what + " pre_save"))
    ws.check(what + " workspace")
    ctr.check(what + " counters")
    return outs, rec
