"""Shared helpers of tests/test_gpu_conv_routes.py: the case table of the direct-conv dispatcher (conv_gemm_impl in
csrc/conv_gemm.hip), one launch of a case through the C ABI, and its fp64 CPU reference.

A case is (id, kind, n, cin, cout, h, w, style, tag, epi, plan, misalign):
  kind      same3x3 / stride2: the pad-1 3x3 conv at stride 1 / 2 of an [n, cin, h, w] input (irse_hip.fwd_taps +
            modconv._phase); stride2_gather: the up = 2 layers' data gradient, a stride-2 3x3 gather over an
            [n, cin, 2h+1, 2w+1] input onto [n, cout, h, w] (modconv.PackedConv.bwd_phases); transposed: the stride-2
            transposed 3x3 conv of an [n, cin, h, w] input onto [n, cout, 2h+1, 2w+1] (PackedConv.fwd_phases)
  cin, cout the GEMM's K channels and output channels
  style     a per-sample input scale s[n, cin]
  tag       0: smc_conv_gemm_f32, 1: smc_conv_gemm_aux_f32 (the IR-SE50 executor's planning)
  epi       store / prelu / prelu_grad / affine_res (the epilogues of test_gpu_irse.test_conv_epilogue_modes)
  plan      None or (plan, local) for _hip.plan_batch
  misalign  the input 4 B past a 16-B boundary
The shapes are the smallest that reach their route on 256 CUs (the guards are quoted in the table's comments).
"""
import collections
import ctypes

import torch

DEV = "cuda"

Case = collections.namedtuple("Case", "id kind n cin cout h w style tag epi plan misalign")


def _c(id, kind, n, cin, cout, h, w, style=False, tag=0, epi="store", plan=None, misalign=False):
    return Case(id, kind, n, cin, cout, h, w, style, tag, epi, plan, misalign)


CASES = [
    # ---- 128 x 128 tile (cout % 128 == 0, >= 128 tiles so the 64 x 64 tile does not take it)
    _c("t128_k16", "same3x3", 1, 48, 128, 64, 256),                        # 16-channel K steps, split-K
    _c("t128_k16_style", "same3x3", 2, 48, 128, 64, 128, style=True),      # per-sample weights, tiles within images
    _c("t128_k32_plan16", "same3x3", 1, 512, 128, 32, 32, plan=(16, 1)),   # cin >= 512: lds_bk32; planned as 16 images
    _c("t128_k16_aux", "same3x3", 1, 48, 128, 64, 256, tag=1, epi="prelu"),
    _c("t128_k32_aux_plan16", "same3x3", 1, 512, 128, 32, 32, tag=1, epi="affine_res", plan=(16, 1)),
    _c("t128_k32x3_aux", "stride2", 4, 64, 128, 128, 128, tag=1, epi="prelu_grad"),   # cin % 32, < 512
    # ---- 64 x 128 tile (cout 64 / 192, >= 128 tiles)
    _c("t64_k16", "same3x3", 1, 48, 64, 96, 192),
    _c("t64_k32", "same3x3", 1, 64, 192, 64, 128),
    _c("t64_stem_aux", "same3x3", 2, 16, 64, 112, 112, tag=1, epi="prelu"),           # the IR-SE50 stem (cin 16)
    _c("t64_k32_aux", "same3x3", 2, 64, 64, 112, 112, tag=1, epi="affine_res"),
    _c("t64_k16_aux", "same3x3", 1, 48, 64, 96, 192, tag=1),
    # ---- 32 x 128 tile (cout 32 / 96)
    _c("t32_k16", "same3x3", 2, 48, 96, 24, 40),
    _c("t32_k32", "same3x3", 3, 64, 32, 40, 24),
    _c("t32_k16_aux", "same3x3", 2, 48, 96, 24, 40, tag=1, epi="prelu_grad"),
    _c("t32_style_wsample", "same3x3", 2, 32, 32, 32, 24, style=True),                # h w % 128 == 0, 9 cout <= h w
    _c("t32_style_misaligned", "same3x3", 2, 32, 32, 16, 16, style=True, misalign=True),   # no prescale: wsample
    _c("t32_per_sample", "same3x3", 3, 48, 32, 20, 30, style=True),                   # h w % 128 != 0, 9 cout <= h w
    _c("t32_prescale", "same3x3", 2, 64, 32, 16, 12, style=True),                     # h w <= 9 cout, h w % 4 == 0
    # ---- 64 x 64 small tile (cout % 64 == 0, < 128 tiles)
    _c("s64_k32", "same3x3", 2, 64, 64, 16, 16),
    _c("s64_k16", "same3x3", 2, 48, 128, 16, 24),
    _c("s64_prescale", "same3x3", 2, 512, 512, 8, 8, style=True),
    _c("s64_per_sample", "same3x3", 3, 32, 64, 25, 24, style=True),                   # 9 cout <= h w, h w % 64 != 0
    _c("s64_k32_aux_7", "same3x3", 2, 512, 512, 7, 7, tag=1, epi="prelu"),            # the IR-SE50 planes
    _c("s64_k32_aux_14", "stride2", 4, 128, 256, 28, 28, tag=1, epi="affine_res"),
    _c("s64_k32_aux_28", "same3x3", 2, 128, 128, 28, 28, tag=1, epi="prelu_grad"),
    _c("s64_k32_aux_56", "same3x3", 4, 64, 64, 56, 56, tag=1, epi="prelu"),
    _c("s64_k16_aux", "same3x3", 2, 48, 64, 16, 24, tag=1, epi="affine_res"),
    # ---- row-halo (exact fp32 only: cout 32 / 64, w % 256 == 0, unsplit -> >= 512 tiles)
    _c("row32", "same3x3", 1, 16, 32, 128, 512),
    _c("row64", "same3x3", 1, 16, 64, 256, 256),
    _c("row32_aux", "same3x3", 1, 16, 32, 256, 256, tag=1),
    # ---- split-bf16 wide tile (cout % 256 == 0, unsplit at 256 x 128: one image planned as 16)
    _c("wide_gather", "stride2_gather", 1, 128, 256, 64, 64, plan=(16, 1)),
    # ---- stride-2 gather (the up = 2 data gradient)
    _c("gather_t32", "stride2_gather", 2, 32, 32, 20, 28),
    _c("gather_s64", "stride2_gather", 3, 64, 128, 8, 12),
    # ---- register-staged below 2 GiB: style, tiles straddling images (h w % 128 != 0), 9 cout > h w, h w % 4 != 0
    _c("reg128_k16", "same3x3", 3, 48, 128, 9, 9, style=True),
    _c("reg128_k32", "same3x3", 3, 512, 128, 9, 9, style=True),
    _c("reg64_k16", "same3x3", 3, 48, 64, 9, 9, style=True),
    _c("reg64_k32", "same3x3", 3, 512, 64, 9, 9, style=True),
    _c("reg32_k16", "same3x3", 3, 48, 32, 9, 7, style=True),
    _c("reg32_k32", "same3x3", 3, 512, 32, 9, 9, style=True),
    _c("reg128_k16_aux", "same3x3", 3, 48, 128, 9, 9, style=True, tag=1),
    _c("reg128_k32_aux", "same3x3", 3, 512, 128, 9, 9, style=True, tag=1, epi="prelu"),
    _c("reg64_k16_aux", "same3x3", 3, 48, 64, 9, 9, style=True, tag=1, epi="affine_res"),
    _c("reg64_k32_aux", "same3x3", 3, 512, 64, 9, 9, style=True, tag=1),
    _c("reg32_k16_aux", "same3x3", 3, 48, 32, 9, 7, style=True, tag=1, epi="prelu_grad"),
    _c("reg32_k32_aux", "same3x3", 3, 512, 32, 9, 9, style=True, tag=1),
    # ... and cout 16 (half-empty 32-channel tile, masked): no LDS-DMA form
    _c("cout16", "same3x3", 2, 32, 16, 40, 24),
    _c("cout16_prescale", "same3x3", 2, 32, 16, 8, 12, style=True),
    _c("cout16_stem_adjoint_aux", "same3x3", 2, 64, 16, 112, 112, tag=1),
    # ---- transposed conv, phase-fused (cout 32 / 64), and the per-phase kernels from 128 channels up
    _c("convt32_per_sample", "transposed", 2, 64, 32, 33, 20, style=True),            # (h+1)(w+1) % 128 != 0
    _c("convt32_prescale", "transposed", 2, 64, 32, 8, 12, style=True),
    _c("convt32_shared", "transposed", 2, 32, 32, 15, 31),                            # no style: shared weights
    _c("convt64_per_sample", "transposed", 2, 64, 64, 33, 20, style=True),
    _c("convt64_prescale", "transposed", 3, 128, 64, 8, 12, style=True),
    _c("convt32_wsample", "transposed", 1, 64, 32, 31, 31, style=True),               # (h+1)(w+1) % 128 == 0
    _c("convt64_wsample", "transposed", 1, 64, 64, 31, 31, style=True),
    _c("convt128_phases", "transposed", 1, 48, 128, 16, 12, style=True),
    _c("convt16_fused", "transposed", 2, 32, 16, 9, 7, style=True),                   # cout 16: convt_gemm_kernel
]

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# The route and modifier flags (SMC_ROUTE_*: 1 split-K, 2 per-sample tiling, 4 prescaled input, 8 per-sample weights)
# each case is built to reach on 256 CUs, read off the dispatcher's guards: id -> ((exact-fp32 form), (with split-bf16
# planes)).  Asserted by test_route_vs_fp64 on a 256-CU device, so a case that drifts onto another kernel fails by itself.
EXPECTED = {
    "t128_k16": (("conv_gemm_lds_kernel<2,2,2,2,16,2>", 1), ("conv_gemm_x3_kernel<1,4,4,1,16>", 1)),
    "t128_k16_style": (("conv_gemm_lds_kernel<2,2,2,2,16,2>", 9), ("conv_gemm_x3_kernel<1,4,4,1,16>", 9)),
    "t128_k32_plan16": (("conv_gemm_lds_kernel<2,2,2,2,32,2>", 1), ("conv_gemm_x3_kernel<1,4,4,1,16>", 1)),
    "t128_k16_aux": (("conv_gemm_lds_kernel<2,2,2,2,16,2,1>", 1), ("conv_gemm_x3_kernel<2,2,2,2,16,NST,1>", 1)),
    "t128_k32_aux_plan16": (("conv_gemm_lds_kernel<2,2,2,2,32,2,1>", 1), ("conv_gemm_x3_kernel<2,2,2,2,32,NST,1>", 1)),
    "t128_k32x3_aux": (("conv_gemm_lds_kernel<2,2,2,2,16,2,1>", 1), ("conv_gemm_x3_kernel<2,2,2,2,32,NST,1>", 1)),
    "t64_k16": (("conv_gemm_lds_kernel<2,2,1,2,16,2>", 1), ("conv_gemm_x3_kernel<1,4,2,1,16>", 1)),
    "t64_k32": (("conv_gemm_lds_kernel<2,2,1,2,16,2>", 1), ("conv_gemm_x3_kernel<1,4,2,1,16>", 1)),
    "t64_stem_aux": (("conv_gemm_lds_kernel<2,2,1,2,16,2,1>", 1), ("conv_gemm_x3_kernel<2,2,1,2,16>", 1)),
    "t64_k32_aux": (("conv_gemm_lds_kernel<2,2,1,2,16,2,1>", 1), ("conv_gemm_x3_kernel<2,2,1,2,32>", 1)),
    "t64_k16_aux": (("conv_gemm_lds_kernel<2,2,1,2,16,2,1>", 1), ("conv_gemm_x3_kernel<2,2,1,2,16>", 1)),
    "t32_k16": (("conv_gemm_lds_kernel<1,4,1,1,16,2>", 1), ("conv_gemm_x3_kernel<1,4,1,1,16>", 1)),
    "t32_k32": (("conv_gemm_lds_kernel<1,4,1,1,16,2>", 1), ("conv_gemm_x3_kernel<1,4,1,1,32>", 1)),
    "t32_k16_aux": (("conv_gemm_lds_kernel<1,4,1,1,16,2,1>", 1), ("conv_gemm_x3_kernel<1,4,1,1,16>", 1)),
    "t32_style_wsample": (("conv_gemm_lds_kernel<1,4,1,1,16,2>", 9), ("conv_gemm_x3_kernel<1,4,1,1,32>", 9)),
    "t32_style_misaligned": (("conv_gemm_lds_kernel<1,4,1,1,16,2>", 9), ("conv_gemm_x3_kernel<1,4,1,1,32>", 9)),
    "t32_per_sample": (("conv_gemm_lds_kernel<1,4,1,1,16,2>", 11), ("conv_gemm_x3_kernel<1,4,1,1,16>", 11)),
    "t32_prescale": (("conv_gemm_lds_kernel<1,4,1,1,16,2>", 5), ("conv_gemm_x3_kernel<1,4,1,1,32>", 5)),
    "s64_k32": (("conv_gemm_lds_kernel<2,2,1,1,16,2>", 1), ("conv_gemm_x3_kernel<2,2,1,1,32>", 1)),
    "s64_k16": (("conv_gemm_lds_kernel<2,2,1,1,16,2>", 1), ("conv_gemm_x3_kernel<2,2,1,1,16>", 1)),
    "s64_prescale": (("conv_gemm_lds_kernel<2,2,1,1,16,2>", 5), ("conv_gemm_x3_kernel<2,2,1,1,32>", 5)),
    "s64_per_sample": (("conv_gemm_lds_kernel<2,2,1,1,16,2>", 11), ("conv_gemm_x3_kernel<2,2,1,1,32>", 11)),
    "s64_k32_aux_7": (("conv_gemm_lds_kernel<2,2,1,1,32,2,1>", 1), ("conv_gemm_x3_kernel<2,2,1,1,32,NST,1>", 1)),
    "s64_k32_aux_14": (("conv_gemm_lds_kernel<2,2,1,1,32,2,1>", 1), ("conv_gemm_x3_kernel<2,2,1,1,32,NST,1>", 1)),
    "s64_k32_aux_28": (("conv_gemm_lds_kernel<2,2,1,1,32,2,1>", 1), ("conv_gemm_x3_kernel<2,2,1,1,32,NST,1>", 1)),
    "s64_k32_aux_56": (("conv_gemm_lds_kernel<2,2,1,1,32,2,1>", 1), ("conv_gemm_x3_kernel<2,2,1,1,32,NST,1>", 1)),
    "s64_k16_aux": (("conv_gemm_lds_kernel<2,2,1,1,16,2,1>", 1), ("conv_gemm_x3_kernel<2,2,1,1,16,NST,1>", 1)),
    "row32": (("conv_row_kernel<1,4,1,2,8>", 0), ("conv_gemm_x3_kernel<1,4,1,1,16>", 0)),
    "row64": (("conv_row_kernel<1,4,2,2,8>", 0), ("conv_gemm_x3_kernel<1,4,2,1,16>", 0)),
    "row32_aux": (("conv_row_kernel<1,4,1,2,8>", 0), ("conv_gemm_x3_kernel<1,4,1,1,16>", 0)),
    "wide_gather": (("conv_gemm_lds_kernel<2,2,2,2,16,2>", 0), ("conv_gemm_x3_kernel<1,4,8,1,16,2,0,true>", 0)),
    "gather_t32": (("conv_gemm_lds_kernel<1,4,1,1,16,2>", 1), ("conv_gemm_x3_kernel<1,4,1,1,32>", 1)),
    "gather_s64": (("conv_gemm_lds_kernel<2,2,1,1,16,2>", 1), ("conv_gemm_x3_kernel<2,2,1,1,32>", 1)),
    "reg128_k16": (("conv_gemm_kernel<2,2,2,2,16,true>", 1), ("conv_gemm_kernel<2,2,2,2,16,true>", 1)),
    "reg128_k32": (("conv_gemm_kernel<2,2,2,2,32,true>", 1), ("conv_gemm_kernel<2,2,2,2,32,true>", 1)),
    "reg64_k16": (("conv_gemm_kernel<2,2,1,2,16,true>", 1), ("conv_gemm_kernel<2,2,1,2,16,true>", 1)),
    "reg64_k32": (("conv_gemm_kernel<2,2,1,2,32,true>", 1), ("conv_gemm_kernel<2,2,1,2,32,true>", 1)),
    "reg32_k16": (("conv_gemm_kernel<1,4,1,1,16,true>", 1), ("conv_gemm_kernel<1,4,1,1,16,true>", 1)),
    "reg32_k32": (("conv_gemm_kernel<1,4,1,1,32,true>", 1), ("conv_gemm_kernel<1,4,1,1,32,true>", 1)),
    "reg128_k16_aux": (("conv_gemm_kernel<2,2,2,2,16,true,1>", 1), ("conv_gemm_kernel<2,2,2,2,16,true,1>", 1)),
    "reg128_k32_aux": (("conv_gemm_kernel<2,2,2,2,32,true,1>", 1), ("conv_gemm_kernel<2,2,2,2,32,true,1>", 1)),
    "reg64_k16_aux": (("conv_gemm_kernel<2,2,1,2,16,true,1>", 1), ("conv_gemm_kernel<2,2,1,2,16,true,1>", 1)),
    "reg64_k32_aux": (("conv_gemm_kernel<2,2,1,2,32,true,1>", 1), ("conv_gemm_kernel<2,2,1,2,32,true,1>", 1)),
    "reg32_k16_aux": (("conv_gemm_kernel<1,4,1,1,16,true,1>", 1), ("conv_gemm_kernel<1,4,1,1,16,true,1>", 1)),
    "reg32_k32_aux": (("conv_gemm_kernel<1,4,1,1,32,true,1>", 1), ("conv_gemm_kernel<1,4,1,1,32,true,1>", 1)),
    "cout16": (("conv_gemm_kernel<1,4,1,1,16,true>", 1), ("conv_gemm_kernel<1,4,1,1,16,true>", 1)),
    "cout16_prescale": (("conv_gemm_kernel<1,4,1,1,16,true>", 5), ("conv_gemm_kernel<1,4,1,1,16,true>", 5)),
    "cout16_stem_adjoint_aux": (("conv_gemm_kernel<1,4,1,1,16,true,1>", 1), ("conv_gemm_kernel<1,4,1,1,16,true,1>", 1)),
    "convt32_per_sample": (("convt_lds_kernel<1,4,1,1,16>", 11), ("convt_x3_kernel<1,4,1,1>", 11)),
    "convt32_prescale": (("convt_lds_kernel<1,4,1,1,16>", 5), ("convt_x3_kernel<1,4,1,1>", 5)),
    "convt32_shared": (("convt_lds_kernel<1,4,1,1,16>", 0), ("convt_x3_kernel<1,4,1,1>", 0)),
    "convt64_per_sample": (("convt_lds_kernel<2,2,1,2,16>", 11), ("convt_x3_kernel<1,4,2,1>", 11)),
    "convt64_prescale": (("convt_lds_kernel<2,2,1,2,16>", 5), ("convt_x3_kernel<1,4,2,1>", 5)),
    "convt32_wsample": (("convt_lds_kernel<1,4,1,1,16>", 9), ("convt_x3_kernel<1,4,1,1>", 9)),
    "convt64_wsample": (("convt_lds_kernel<2,2,1,2,16>", 9), ("convt_x3_kernel<1,4,2,1>", 9)),
    "convt128_phases": (("conv_gemm_lds_kernel<2,2,1,1,16,2>", 4), ("conv_gemm_x3_kernel<2,2,1,1,16>", 4)),
    "convt16_fused": (("convt_gemm_kernel<1,4,1,1,16>", 1), ("convt_gemm_kernel<1,4,1,1,16>", 1)),
}
assert set(EXPECTED) == set(BY_ID)


def flops(c):
    """FLOP of the case's fp64 reference (2 x 9 taps x n cin cout x output positions)."""
    oh, ow = out_hw(c)
    return 2 * 9 * c.n * c.cin * c.cout * oh * ow


def in_hw(c):
    return (2 * c.h + 1, 2 * c.w + 1) if c.kind == "stride2_gather" else (c.h, c.w)


def out_hw(c):
    if c.kind == "transposed":
        return 2 * c.h + 1, 2 * c.w + 1
    if c.kind == "stride2":
        return c.h // 2, c.w // 2
    return c.h, c.w


def make_inputs(c):
    """The case's CPU fp32 operands, seeded by its id: W in the layout of its reference call, x, s (or None) and the
    epilogue's per-channel / per-element operands."""
    gen = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id)))
    ih, iw = in_hw(c)
    oh, ow = out_hw(c)
    d = {}
    if c.kind == "stride2_gather":   # the forward conv's weight [cin_fwd = cout][cout_fwd = cin]
        d["W"] = torch.randn(c.cin, c.cout, 3, 3, generator=gen) / (9 * c.cin) ** 0.5
    else:
        d["W"] = torch.randn(c.cout, c.cin, 3, 3, generator=gen) / (9 * c.cin) ** 0.5
    d["x"] = torch.randn(c.n, c.cin, ih, iw, generator=gen)
    d["s"] = torch.randn(c.n, c.cin, generator=gen) * 0.5 + 1 if c.style else None
    d["a"] = torch.rand(c.cout, generator=gen) + 0.5
    d["b"] = torch.randn(c.cout, generator=gen)
    d["al"] = torch.rand(c.cout, generator=gen) * 0.5
    d["act_ref"] = torch.randn(c.n, c.cout, oh, ow, generator=gen)
    rs = 2 if oh % 2 == 0 and ow % 2 == 0 else 1
    d["rs"] = rs
    d["res"] = torch.randn(c.n, c.cout, oh // rs, ow // rs, generator=gen)
    return d


def _conv64(c, x, W):
    import torch.nn.functional as F
    if c.kind == "transposed":
        return F.conv_transpose2d(x, W.transpose(0, 1), stride=2)
    if c.kind == "stride2_gather":
        return F.conv2d(x, W.transpose(0, 1), stride=2)
    return F.conv2d(x, W, stride=2 if c.kind == "stride2" else 1, padding=1)


def reference(c, d, bound=False):
    """fp64 CPU outputs of the case, in launch()'s order.  bound=True: instead, per output, the fp64 tensor
    2^-23 (|W| (*) |x s|) (times the epilogue's |scale|) that DESIGN.md section 3 derives for the split-bf16 form's
    dropped cross terms."""
    xs = d["x"].double()
    if d["s"] is not None:
        xs = xs * d["s"].double()[:, :, None, None]
    W = d["W"].double()
    a = d["a"].double()[None, :, None, None]
    if bound:
        acc = _conv64(c, xs.abs(), W.abs()) * 2.0 ** -23
        return {"store": [acc], "prelu": [acc * a, acc * a], "prelu_grad": [acc], "affine_res": [acc * a]}[c.epi]
    acc = _conv64(c, xs, W)
    b = d["b"].double()[None, :, None, None]
    al = d["al"].double()[None, :, None, None]
    if c.epi == "store":
        return [acc]
    z = acc * a + b
    if c.epi == "prelu":
        return [z, torch.where(z >= 0, z, z * al)]
    if c.epi == "prelu_grad":
        return [torch.where(d["act_ref"].double() >= 0, acc, acc * al)]
    full = torch.zeros_like(z)
    full[:, :, ::d["rs"], ::d["rs"]] = d["res"].double()
    return [z + full]


def _misaligned(t):
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def launch(c, d, x3):
    """One launch of the case through its entry point, with split-bf16 planes (x3) or without.  Returns
    (outputs, route, flags, route name); the outputs are in reference()'s order."""
    from stylemc_amd import _hip, modconv
    from stylemc_amd.irse_hip import fwd_taps
    lib = _hip.load()
    oh, ow = out_hw(c)
    keep = []
    if c.kind in ("same3x3", "stride2"):
        taps, wk = fwd_taps(d["W"])
        wk = wk.contiguous().to(DEV)
        planes = modconv.x3_planes(wk, c.cin, c.cout, enabled=x3)
        assert (planes is not None) == x3
        stride = 2 if c.kind == "stride2" else 1
        ph, nph = (_hip.ConvPhase * 1)(modconv._phase(taps, stride, oh, ow, 0, 0, 1, 1, wk, planes)), 1
        keep += [wk, planes]
    else:
        P = modconv.PackedConv(d["W"].to(DEV), 2)
        P.use_x3 = x3
        if c.kind == "transposed":
            ph, nph, th, tw = P.fwd_phases(c.h, c.w)
            assert (th, tw) == (oh, ow) and all((w is not None) == x3 for w in P.x3_phases)
        else:
            ph, nph = P.bwd_phases(c.h, c.w)
            assert (P.x3_bwd is not None) == x3
        keep.append(P)
    x = d["x"].to(DEV)
    if c.misalign:
        x = _misaligned(x)
    s = d["s"].to(DEV) if d["s"] is not None else None
    y = torch.full((c.n, c.cout, oh, ow), float("nan"), device=DEV)
    e = _hip.ConvEpilogue()
    e.mode, e.act, e.gain, e.clamp = _hip.EPI_STORE, _hip.ACT_CODES["linear"], 1.0, -1.0
    outs = [y]
    if c.epi == "prelu":
        z = torch.full_like(y, float("nan"))
        ad, bd, ald = d["a"].to(DEV), d["b"].to(DEV), d["al"].to(DEV)
        e.mode, e.scale_c, e.bias, e.alpha_c, e.u_save = (_hip.EPI_PRELU, ad.data_ptr(), bd.data_ptr(), ald.data_ptr(),
                                                          z.data_ptr())
        keep += [ad, bd, ald]
        outs = [z, y]
    elif c.epi == "prelu_grad":
        ald, ref = d["al"].to(DEV), d["act_ref"].to(DEV)
        e.mode, e.alpha_c, e.act_ref = _hip.EPI_PRELU_GRAD, ald.data_ptr(), ref.data_ptr()
        keep += [ald, ref]
    elif c.epi == "affine_res":
        ad, bd, resd = d["a"].to(DEV), d["b"].to(DEV), d["res"].to(DEV)
        e.mode, e.scale_c, e.bias, e.residual, e.residual_stride = (_hip.EPI_AFFINE, ad.data_ptr(), bd.data_ptr(),
                                                                    resd.data_ptr(), d["rs"])
        keep += [ad, bd, resd]
    entry, query = (("smc_conv_gemm_aux_f32", "smc_conv_gemm_aux_workspace_size") if c.tag else
                    ("smc_conv_gemm_f32", "smc_conv_gemm_workspace_size"))
    ih, iw = in_hw(c)
    with _hip.plan_batch(*(c.plan or (0, 0))):
        wsb = getattr(lib, query)(c.n, c.cin, c.cout, oh, ow, ph, nph)
        ws = torch.empty(max(wsb // 4, 1), device=DEV)
        _hip.call(entry, x.data_ptr(), c.n, c.cin, ih, iw, y.data_ptr(), c.cout, oh, ow, ph, nph, _hip.ptr(s),
                  ctypes.byref(e), ws.data_ptr(), wsb, _hip.stream())
        route, flags = lib.smc_conv_gemm_last_route(), lib.smc_conv_gemm_last_route_flags()
    torch.cuda.synchronize()
    del keep
    return outs, route, flags, route_name(route)


def route_name(route):
    from stylemc_amd import _hip
    name = _hip.load().smc_conv_gemm_route_name(route)
    return name.decode() if name is not None else f"<route {route}>"


def route_names():
    from stylemc_amd import _hip
    return [route_name(r) for r in range(_hip.load().smc_conv_gemm_route_count())]
