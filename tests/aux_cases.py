"""Shared helpers of tests/test_gpu_aux_routes.py and tests/test_aux_cases_cpu.py: the case table of the memory-bound
companion kernels (csrc/modconv_aux.hip, csrc/torgb.hip), one launch of a case through the C ABI, its fp64 CPU
reference with a bound for every output element, and a Python statement of the dispatchers' guards from which the
expected route (smc_modconv_aux_last_route), flags and channel split of a case are read.

A case is (id, ep, p, route, flags): ep the entry point's key in ENTRY, p its parameters (a dict, defaults in _DEFAULTS),
route / flags the kernel and SMC_ROUTE_DD_PARTIALS the case is built to reach (literal; planned() must agree).

The guards (modconv_aux.hip, torgb.hip), "al" = the OR of the named pointers:
  blur_act       `fh == 4 && fw == 4` else blur_act_kernel;  `v4 = split_stride % 4 == 0 && (al(t, y, u_save, noise) & 15)
                 == 0 && y_w % 2 == 0 && noise_nstride % 2 == 0 && padx0 <= 4 && fw - 1 - padx0 <= 4`; v4 and
                 `!f && fgain == 4.f` -> blur_act_v4<..,true>, v4 -> blur_act_v4<..>, else blur_act_fast
  blur_act_bwd   `nstr = from_y ? 0 : noise_nstride`, al(g, u, from_y ? 0 : noise);  `u_w % 4 == 0 && nstr % 4 == 0 &&
                 (al & 15) == 0 && padx0 <= 4 && fw - 1 - padx0 <= 4` -> blur_act_bwd_v4<4,4,FROMY[,true when !f &&
                 fgain == 4.f]>;  else `u_w % 2 == 0 && padx0 % 2 == 0 && nstr % 2 == 0 && (al & 7) == 0` ->
                 blur_act_bwd_fast<4,4,true,FROMY>;  else blur_act_bwd_fast<4,4,false,FROMY>.
                 dd partials: `dd && ceil(u_h / 32) * ceil(u_w / 64) > 2`, one slot per tile of the t grid
  act_bwd        `vec4 = hw % 4 == 0 && (from_y || !noise || noise_nstride % 4 == 0) && al(g, u, du, from_y ? 0 : noise)
                 % 16 == 0`; workgroups per plane `vec4 ? ceil(hw / 4 / 1024) : max(1, ceil(hw / 2048))`; dd partials:
                 `dd && blocks_per_plane > 2`
  channel_dot    `len % 4 == 0 && (al(a, b, a_scaled) & 15) == 0` -> channel_dot_v4_kernel
  torgb fwd      `hw <= 4096` -> small;  `hw % 4 == 0 && x, y 16-B aligned` -> <true>;  else <false>
  torgb bwd      `hw <= 4096` -> small;  `hw % 4 == 0 && dx 16-B aligned` -> <true>;  else <false>
  torgb_act_bwd  `vec = hw % 4 == 0 && (al(g_next, y, du) & 15) == 0`;  `grid.x = ceil((vec ? hw / 4 : hw) / 256)`;
                 `plan_wg = grid.x * plan_batch(n)`; `while (plan_wg * nz < 4 * CUs && cin % (16 * nz) == 0) nz *= 2`
                 (nz from the device's CU count, never a literal)

References are fp64 torch on the fp32 operands: F.conv2d with the explicitly flipped (flip = 0) or unflipped filter
for the FIR, the header's epilogue formula z = u d + noise strength + bias, y = clamp(act(z) gain), and
torch.autograd.grad of sum(g y) for du, dT, dd (of sum(g y_rgb) for dx).  The grad_from_y forms, which have no u to
differentiate, take bias_act's y-referenced gradient formula (tests/test_aux_cases_cpu.py holds it to autograd and to
oracle/ops.py).

Kinks.  Every backward case moves the elements whose fp64 pre-activation z lies within MARGIN = 1e-3 of 0, or whose
|act(z) gain| lies within MARGIN of the clamp, out of the margin before the launch (push_margins; a given y likewise),
and margins_ok() asserts it: the activation mask of every element is then the same in fp32 and fp64 and no element is
excluded from any bound.

Bounds: K roundings x EPS = 2^-24 x B, B the same expression in fp64 with every operand replaced by its magnitude.
  u of the FIR       K = 17 (runtime taps: f * fgain rounds once, then 16 fma), 16 with the built-in taps, 2 + fh fw for
                     the generic kernel (unfused product and add per tap), + nsplit - 1;  B = FIR(sum |T_k|, |taps|)
  y from u           gain L (|d| err_u + Ke EPS S), S = |u64 d| + |noise strength| + |bias|: the activation and the clamp
                     are L-Lipschitz, L = max(1, alpha) (1 for every form but lrelu_a15), and the epilogue's own roundings
                     (noise strength, the fma, the bias add, z alpha, the gain) are Ke = 4 relative roundings of values
                     no larger than S while alpha <= 1/2 (the two on the negative branch are scaled by alpha), 5 for
                     lrelu_a15.  STORE: err_u
  du                 K = 3 (alpha, gain, d), B = |du64|
  dT                 K = 3 + 17 (3 + 16 built-in), B = FIR^T(|du64|, |taps|)
  torgb forward      K = cin + 3, B = sum |w s x| + |b|
  torgb backward     K = cout + 2 (+ 1 with accumulate), B = sum |w s g| (+ |dx before|)
  torgb_act_bwd du   K = cout + 2 + 1 (the sum with g_next) + 3, B = slope gain |d| (|g_next| + sum |w s g|)
  reductions         K = 2 + the longest chain of dependent additions: the per-thread count, 6 butterfly steps, 3 LDS
                     adds, then 2 atomic adds or the partial pass (ceil(tiles / 64) + 6 + 1); chain() states it per case
  demod              d = rsqrtf(acc + eps): relative (K_acc EPS) / 2 + RSQRT_REL, K_acc = 2 + ceil(cin / 64) + 6 + 1 (every
                     term s^2 wsq is non-negative, so B = acc)
RSQRT_REL is rsqrtf's own relative error.  The ROCm install carries no ULP table, so it is 2 x the largest error
measured against fp64 on an MI355X over exact arguments (cin = 1, s = 1, eps = 0: d = rsqrtf(wsq) with nothing else
rounding; tests/test_gpu_aux_routes.py::test_rsqrtf_error_is_within_the_recorded_figure re-measures it); DESIGN.md
"Companion-kernel launch forms" records the figure.

No-cancellation cases (nocancel): g takes the sign that makes every term dz u >= 0 (a = b for the dot), so B equals the
result and a dropped row or tile is a fixed fraction of it, far above K EPS.
"""
import collections
import ctypes

import torch
import torch.nn.functional as F

DEV = "cuda"
EPS = 2.0 ** -24
DD = 32          # _hip.ROUTE_DD_PARTIALS
MARGIN = 1e-3
# rsqrtf: 2 x the measured 9.063e-8 (1.52 x 2^-24, over 65536 arguments in 2^-20 .. 2^20; module docstring)
RSQRT_REL = 2 * 9.063e-8

Case = collections.namedtuple("Case", "id ep p route flags")

SQ2 = 2 ** 0.5
_L = dict(act="lrelu", alpha=0.2, gain=SQ2, clamp=1.0)
_FULL = dict(mode="MODACT", d=True, noise="const", strength=True, bias=True, u_save=True)
# epilogue forms: the smc_conv_epilogue fields a launch sets (everything else NULL / 0)
FORMS = {
    "store": dict(mode="STORE"),
    "lrelu_clamp": dict(_FULL, **_L),                                   # the compile-time modact2 body
    "relu_clamp": dict(_FULL, act="relu", alpha=0.0, gain=SQ2, clamp=1.0),
    "lrelu_noclamp": dict(_FULL, **dict(_L, clamp=-1.0)),
    "linear_clamp": dict(_FULL, act="linear", alpha=0.0, gain=SQ2, clamp=1.0),
    "lrelu_a15": dict(_FULL, **dict(_L, alpha=1.5)),
    "no_d": dict(_FULL, **_L) | dict(d=False),
    "no_noise": dict(_FULL, **_L) | dict(noise=None),
    "no_strength": dict(_FULL, **_L) | dict(strength=False),
    "no_bias": dict(_FULL, **_L) | dict(bias=False),
    "no_usave": dict(_FULL, **_L) | dict(u_save=False),
    "noise_img": dict(_FULL, **_L) | dict(noise="img"),                 # per sample, nstride = h w
    "noise_odd": dict(_FULL, **_L) | dict(noise="odd"),                 # per sample, odd nstride
    "relu_nulls": dict(mode="MODACT", act="relu", alpha=0.0, gain=SQ2, clamp=-1.0, u_save=True),
}

# kernel names as the route table spells them
R = dict(
    epi="epilogue_kernel", blur_g="blur_act_kernel", blur_f="blur_act_fast<4,4>",
    blur_v4="blur_act_v4<4,4,kBlurTPB,kBlurNT>", blur_v4s="blur_act_v4<4,4,kBlurTPB,kBlurNT,true>",
    bwd_v4_u="blur_act_bwd_v4<4,4,false>", bwd_v4_us="blur_act_bwd_v4<4,4,false,true>",
    bwd_v4_y="blur_act_bwd_v4<4,4,true>", bwd_v4_ys="blur_act_bwd_v4<4,4,true,true>",
    bwd_v2_u="blur_act_bwd_fast<4,4,true,false>", bwd_v2_y="blur_act_bwd_fast<4,4,true,true>",
    bwd_s_u="blur_act_bwd_fast<4,4,false,false>", bwd_s_y="blur_act_bwd_fast<4,4,false,true>",
    demod="demod_kernel", act_v4_u="act_bwd_vec4_kernel<false>", act_v4_y="act_bwd_vec4_kernel<true>",
    act_u="act_bwd_kernel<false>", act_y="act_bwd_kernel<true>", dot_v4="channel_dot_v4_kernel",
    dot="channel_dot_kernel", demod_bwd="demod_bwd_kernel", rgb_f_small="torgb_fwd_small_kernel",
    rgb_f_vec="torgb_fwd_kernel<true>", rgb_f="torgb_fwd_kernel<false>", rgb_b_small="torgb_bwd_small_kernel",
    rgb_b_vec="torgb_bwd_kernel<true>", rgb_b="torgb_bwd_kernel<false>", rgb_ab_vec="torgb_act_bwd_kernel<true>",
    rgb_ab="torgb_act_bwd_kernel<false>",
)

_DEFAULTS = {
    # t: [n, c, th, tw] at row pitch `pitch` (0: tw), nsplit planes at stride n c th pitch + sextra; y: yh x yw (None: the
    # full output); filt: "std" (f = NULL, built-in), "std_rt" (the same taps passed), "asym" (random 4x4), "kHxW"; mis:
    # misalignment of t in floats
    "blur": dict(n=1, c=2, th=9, tw=9, pitch=0, yh=None, yw=None, filt="std", fgain=4.0, pad=(1, 1), flip=0,
                 form="lrelu_clamp", nsplit=1, sextra=0, mis=0),
    # u, g: [n, c, uh, uw]; pad: the adjoint's (padx0, pady0); mis: misalignment of u and g in floats
    "blur_bwd": dict(n=1, c=2, uh=8, uw=8, pad=(2, 2), pitch=0, filt="std", fgain=4.0, flip=1, form="lrelu_clamp",
                     from_y=0, dd=True, mis=0, nocancel=False),
    "act_bwd": dict(n=2, c=3, h=7, w=9, form="lrelu_clamp", from_y=0, dd=True, mis=0, nocancel=False),
    "epilogue": dict(n=1, c=3, h=6, w=10, form="lrelu_clamp", nsplit=1),
    "torgb_fwd": dict(n=2, cin=12, cout=3, h=4, w=4, bias=True, clamp=0.3, mis=0),
    "torgb_bwd": dict(n=2, cin=12, cout=3, h=4, w=4, clamp=0.3, scale=1, acc=0, mis=0),
    "torgb_act_bwd": dict(n=2, cin=24, cout=3, h=16, w=16, g_next=True, mis=0, plan=None, clamp_rgb=0.3),
    "channel_dot": dict(rows=1, len=400, scaled=False, acc=0, mis=0, nocancel=False),
    "demod": dict(n=3, cin=64, cout=5),
    "demod_bwd": dict(n=2, cin=33, cout=20),
}

CASES = []


def _case(ep, cid, route, flags=0, **p):
    unknown = set(p) - set(_DEFAULTS[ep])
    assert not unknown, (cid, unknown)
    CASES.append(Case(f"{ep}_{cid}", ep, dict(_DEFAULTS[ep], **p), R[route], flags))


# ---- smc_modconv_blur_act_f32.  Tile 32 x 64; the v4 kernels walk four row tiles per workgroup.
_case("blur", "v4s_8x8", "blur_v4s", th=9, tw=9)                                    # one partial tile
_case("blur", "v4s_66x130", "blur_v4s", th=67, tw=131)                              # 3 x 3 tiles, edges in both axes
_case("blur", "v4s_130x66", "blur_v4s", c=1, th=131, tw=67)        # 5 row tiles: a second workgroup of one tile
_case("blur", "v4s_pitch12", "blur_v4s", th=9, tw=9, pitch=12)                      # pitch % 4 == 0
_case("blur", "v4s_pitch11_n2", "blur_v4s", n=2, th=9, tw=9, pitch=11)              # planes at every offset mod 4
_case("blur", "v4s_store", "blur_v4s", th=35, tw=67, form="store")
_case("blur", "v4s_cropped", "blur_v4s", th=40, tw=70, yh=33, yw=66)                # y smaller than the full output
_case("blur", "v4s_noise_img", "blur_v4s", n=2, th=9, tw=9, form="noise_img")
_case("blur", "v4s_nsplit3", "blur_v4s", th=35, tw=67, nsplit=3, sextra=2)          # 4690 + 2: stride % 4 == 0
_case("blur", "v4_std_rt", "blur_v4", th=35, tw=67, filt="std_rt")                  # the same taps at run time
_case("blur", "v4_asym_flip0", "blur_v4", th=35, tw=67, filt="asym", fgain=1.0, flip=0)
_case("blur", "v4_asym_flip1", "blur_v4", th=35, tw=67, filt="asym", fgain=1.0, flip=1)
_case("blur", "v4_pad00", "blur_v4", th=36, tw=69, filt="asym", fgain=1.0, pad=(0, 0))
_case("blur", "v4_pad21", "blur_v4", th=35, tw=65, filt="asym", fgain=1.0, pad=(2, 1))
_case("blur", "v4_pad33", "blur_v4", th=30, tw=63, filt="asym", fgain=1.0, pad=(3, 3))
_case("blur", "v4_pad44", "blur_v4", th=28, tw=61, filt="asym", fgain=1.0, pad=(4, 4))
_case("blur", "v4_nsplit3", "blur_v4", th=35, tw=67, filt="asym", fgain=2.0, nsplit=3, sextra=6)
for _form in ("relu_clamp", "lrelu_noclamp", "linear_clamp", "lrelu_a15", "no_d", "no_noise", "no_strength", "no_bias",
              "no_usave", "relu_nulls"):
    _case("blur", f"v4s_{_form}", "blur_v4s", th=9, tw=11, form=_form)
_case("blur", "fast_mis_t", "blur_f", th=35, tw=67, mis=1)                          # t 4 B off 16-B alignment
_case("blur", "fast_sstride", "blur_f", th=35, tw=67, nsplit=3, sextra=3)           # split_stride % 4 != 0
_case("blur", "fast_mis_t_nsplit3", "blur_f", th=35, tw=67, nsplit=3, sextra=2, mis=1)   # split_stride % 4 == 0
_case("blur", "fast_odd_7x9", "blur_f", th=8, tw=10)                              # odd y_w: the per-column stores
_case("blur", "fast_pad5", "blur_f", th=26, tw=58, filt="asym", fgain=1.0, pad=(5, 3))
_case("blur", "fast_noise_odd", "blur_f", n=2, th=9, tw=9, form="noise_odd")        # leaves the 16-B and pair paths
_case("blur", "fast_66x130_flip1", "blur_f", th=67, tw=131, filt="asym", fgain=1.0, flip=1, mis=1)
_case("blur", "fast_store", "blur_f", th=9, tw=9, form="store", mis=2)
for _k, _hw in (("k3x3", (34, 34)), ("k6x6", (37, 37)), ("k8x8", (39, 39)), ("k1x4", (33, 36)), ("k4x1", (36, 33))):
    _case("blur", f"generic_{_k}", "blur_g", th=_hw[0], tw=_hw[1], filt=_k, fgain=1.0, pad=(1, 1), flip=0)
_case("blur", "generic_k3x3_flip1_nsplit3", "blur_g", th=9, tw=9, filt="k3x3", fgain=2.0, flip=1, nsplit=3, sextra=1)
_case("blur", "generic_k4x1_nsplit3_stride164", "blur_g", th=9, tw=9, filt="k4x1", fgain=1.0, nsplit=3, sextra=2)
_case("blur", "generic_k6x6_store", "blur_g", th=12, tw=12, filt="k6x6", fgain=1.0, pad=(2, 2), form="store")

# ---- smc_modconv_blur_act_bwd_f32.  dd: direct (at most two 32 x 64 tiles of u) and SMC_ROUTE_DD_PARTIALS.
for _fy, _tag in ((0, "u"), (1, "y")):
    _dd = not _fy
    _pf = DD if _dd else 0
    _case("blur_bwd", f"v4s_{_tag}_32x128", f"bwd_v4_{_tag}s", uh=32, uw=128, from_y=_fy, dd=_dd)
    _case("blur_bwd", f"v4s_{_tag}_66x132", f"bwd_v4_{_tag}s", _pf, uh=66, uw=132, from_y=_fy, dd=_dd, pitch=136)
    _case("blur_bwd", f"v4_{_tag}_34x64_flip0", f"bwd_v4_{_tag}", uh=34, uw=64, filt="asym", fgain=1.0, flip=0,
          from_y=_fy, dd=_dd)
    _case("blur_bwd", f"v4_{_tag}_66x132_flip1", f"bwd_v4_{_tag}", _pf, uh=66, uw=132, filt="asym", fgain=1.0,
          flip=1, from_y=_fy, dd=_dd)
    _case("blur_bwd", f"v2_{_tag}_32x66", f"bwd_v2_{_tag}", uh=32, uw=66, from_y=_fy, dd=_dd)
    _case("blur_bwd", f"v2_{_tag}_66x130", f"bwd_v2_{_tag}", _pf, uh=66, uw=130, filt="asym", fgain=1.0, flip=0,
          from_y=_fy, dd=_dd, pitch=135)
    _case("blur_bwd", f"v2_{_tag}_34x194", f"bwd_v2_{_tag}", _pf, c=1, uh=34, uw=194, from_y=_fy, dd=_dd)
    _case("blur_bwd", f"s_{_tag}_7x9", f"bwd_s_{_tag}", uh=7, uw=9, from_y=_fy, dd=_dd)
    _case("blur_bwd", f"s_{_tag}_66x129", f"bwd_s_{_tag}", _pf, uh=66, uw=129, filt="asym", fgain=1.0, flip=1,
          from_y=_fy, dd=_dd)
    _case("blur_bwd", f"s_{_tag}_mis_34x64", f"bwd_s_{_tag}", uh=34, uw=64, mis=1, from_y=_fy, dd=_dd)
_case("blur_bwd", "v2_u_mis8_32x64", "bwd_v2_u", uh=32, uw=64, mis=2)              # 8-B aligned only
_case("blur_bwd", "v2_u_noise_img", "bwd_v2_u", n=2, uh=9, uw=10, form="noise_img")          # nstride % 4 == 2
_case("blur_bwd", "s_u_noise_odd", "bwd_s_u", n=2, uh=8, uw=8, form="noise_odd")
_case("blur_bwd", "v4s_u_nocancel_128x128", "bwd_v4_us", DD, c=1, uh=128, uw=128, nocancel=True)
_case("blur_bwd", "s_u_nocancel_97x129", "bwd_s_u", DD, c=1, uh=97, uw=129, nocancel=True)
for _form in ("relu_clamp", "lrelu_noclamp", "linear_clamp", "no_d", "no_noise", "no_bias"):
    _case("blur_bwd", f"v4s_u_{_form}", "bwd_v4_us", uh=12, uw=12, form=_form)
# adjoint pad (3, 3): forward pad 0, t three larger than u (t tiles that own nothing)
_case("blur_bwd", "v4_u_pad33_32x64", "bwd_v4_u", uh=32, uw=64, pad=(3, 3), filt="asym", fgain=1.0)
_case("blur_bwd", "s_u_pad33_33x65", "bwd_s_u", DD, uh=33, uw=65, pad=(3, 3), filt="asym", fgain=1.0, flip=0)
# adjoint pad below 2: t smaller than u, u rows / columns beyond the last tile's 32 x 64 window
_case("blur_bwd", "s_u_pad11_33x65", "bwd_s_u", DD, uh=33, uw=65, pad=(1, 1), nocancel=True)
_case("blur_bwd", "s_u_pad11_33x130", "bwd_s_u", DD, uh=33, uw=130, pad=(1, 1), nocancel=True)
_case("blur_bwd", "s_u_pad11_34x129", "bwd_s_u", DD, uh=34, uw=129, pad=(1, 1), filt="asym", fgain=1.0, nocancel=True)
_case("blur_bwd", "v4s_u_pad11_33x64", "bwd_v4_us", uh=33, uw=64, pad=(1, 1), nocancel=True)     # dd direct
_case("blur_bwd", "v4_u_pad11_33x132", "bwd_v4_u", DD, uh=33, uw=132, pad=(1, 1), filt="asym", fgain=1.0,
      nocancel=True)
_case("blur_bwd", "v2_u_pad01_33x130", "bwd_v2_u", DD, uh=33, uw=130, pad=(0, 1), nocancel=True)
_case("blur_bwd", "v4s_u_pad00_35x68", "bwd_v4_us", DD, uh=35, uw=68, pad=(0, 0), nocancel=True)   # t 32 x 65
_case("blur_bwd", "v4s_y_pad11_33x64", "bwd_v4_ys", uh=33, uw=64, pad=(1, 1), from_y=1, dd=False)
# adjoint pad 4 (forward pad -1): dT only -- beyond pad 3 a tile's window lacks part of its own 32 x 64 and dd is
# rejected on the host (tests/test_aux_cases_cpu.py); 2 x 2 tiles of t
_case("blur_bwd", "v4_u_pad44_40x68_dt_only", "bwd_v4_u", uh=40, uw=68, pad=(4, 4), filt="asym", fgain=1.0, dd=False)
_case("blur_bwd", "s_u_pad44_33x65_dt_only", "bwd_s_u", uh=33, uw=65, pad=(4, 4), filt="asym", fgain=1.0, flip=0,
      dd=False)
_case("blur_bwd", "v2_y_pad64_34x66", "bwd_v2_y", uh=34, uw=66, pad=(6, 4), from_y=1, dd=False)

# ---- smc_modconv_act_bwd_f32.  Scalar: 2048 elements per workgroup; vec4: 1024 float4.
for _fy, _tag in ((0, "u"), (1, "y")):
    _dd = not _fy
    _pf = DD if _dd else 0
    _case("act_bwd", f"s_{_tag}_7x9", f"act_{_tag}", h=7, w=9, from_y=_fy, dd=_dd)                  # one workgroup
    _case("act_bwd", f"s_{_tag}_45x47", f"act_{_tag}", h=45, w=47, from_y=_fy, dd=_dd)              # two: atomics
    _case("act_bwd", f"s_{_tag}_65x65", f"act_{_tag}", _pf, h=65, w=65, from_y=_fy, dd=_dd)         # three: partials
    _case("act_bwd", f"v4_{_tag}_10x10", f"act_v4_{_tag}", h=10, w=10, from_y=_fy, dd=_dd)          # a tail
    _case("act_bwd", f"v4_{_tag}_64x64", f"act_v4_{_tag}", h=64, w=64, from_y=_fy, dd=_dd)
    _case("act_bwd", f"v4_{_tag}_92x92", f"act_v4_{_tag}", _pf, n=1, h=92, w=92, from_y=_fy, dd=_dd)
    _case("act_bwd", f"s_{_tag}_mis_64x64", f"act_{_tag}", n=1, h=64, w=64, mis=1, from_y=_fy, dd=_dd)   # two workgroups
    _case("act_bwd", f"s_{_tag}_mis_72x72", f"act_{_tag}", _pf, n=1, h=72, w=72, mis=1, from_y=_fy, dd=_dd)
for _form in ("relu_clamp", "linear_clamp", "lrelu_noclamp", "no_d", "no_noise", "no_bias", "noise_img"):
    _case("act_bwd", f"v4_u_{_form}", "act_v4_u", h=8, w=8, form=_form)
    _case("act_bwd", f"s_u_{_form}", "act_u", h=7, w=9, form=_form)
_case("act_bwd", "s_u_noise_odd_8x8", "act_u", h=8, w=8, form="noise_odd")          # nstride % 4 != 0 leaves vec4
_case("act_bwd", "v4_u_nocancel_128x128", "act_v4_u", DD, n=1, c=2, h=128, w=128, nocancel=True)
_case("act_bwd", "s_u_nocancel_127x129", "act_u", DD, n=1, c=2, h=127, w=129, nocancel=True)

# ---- smc_modconv_epilogue_f32: the partials are summed eight at a time
for _ns in (1, 2, 9, 10, 17):
    _case("epilogue", f"nsplit{_ns}", "epi", nsplit=_ns)
_case("epilogue", "store_nsplit9", "epi", nsplit=9, form="store")
_case("epilogue", "gridstride_512x512", "epi", c=5, h=512, w=512, nsplit=2, form="store")   # > 16 CUs 256 elements

# ---- smc_torgb_fwd_f32
_case("torgb_fwd", "small_16_cin512", "rgb_f_small", cin=512, h=4, w=4)
_case("torgb_fwd", "small_16_cin7_cout1", "rgb_f_small", cin=7, cout=1, h=4, w=4, clamp=-1.0)
_case("torgb_fwd", "small_16_cin20_cout4", "rgb_f_small", cin=20, cout=4, h=4, w=4, bias=False)
_case("torgb_fwd", "small_64x64_cin136", "rgb_f_small", n=1, cin=136, h=64, w=64)
_case("torgb_fwd", "small_5x7_cin12", "rgb_f_small", cin=12, h=5, w=7)
_case("torgb_fwd", "vec_66x64_cin12", "rgb_f_vec", cin=12, h=66, w=64)
_case("torgb_fwd", "vec_66x64_cin7_cout4", "rgb_f_vec", n=1, cin=7, cout=4, h=66, w=64, bias=False, clamp=-1.0)
_case("torgb_fwd", "vec_66x64_cin136_cout1", "rgb_f_vec", n=1, cin=136, cout=1, h=66, w=64)
_case("torgb_fwd", "scalar_65x65_cin20", "rgb_f", cin=20, h=65, w=65)
_case("torgb_fwd", "scalar_65x65_cin7_cout4", "rgb_f", n=1, cin=7, cout=4, h=65, w=65, clamp=-1.0)
_case("torgb_fwd", "scalar_mis_66x64_cin12_cout1", "rgb_f", cin=12, cout=1, h=66, w=64, mis=1, bias=False)

# ---- smc_torgb_bwd_f32
for _sc, _acc in ((1, 0), (0, 0), (1, 1), (0, 1)):
    _t = f"scale{_sc}_acc{_acc}"
    _case("torgb_bwd", f"small_16_cin40_{_t}", "rgb_b_small", cin=40, h=4, w=4, scale=_sc, acc=_acc)
    _case("torgb_bwd", f"vec_66x64_cin12_{_t}", "rgb_b_vec", n=1, cin=12, h=66, w=64, scale=_sc, acc=_acc)
    _case("torgb_bwd", f"scalar_65x65_cin12_{_t}", "rgb_b", n=1, cin=12, h=65, w=65, scale=_sc, acc=_acc)
_case("torgb_bwd", "small_64x64_cin7_cout4", "rgb_b_small", n=1, cin=7, cout=4, h=64, w=64, clamp=-1.0)
_case("torgb_bwd", "small_5x7_cin20_cout1", "rgb_b_small", cin=20, cout=1, h=5, w=7)
_case("torgb_bwd", "vec_66x64_cin20_cout4", "rgb_b_vec", cin=20, cout=4, h=66, w=64, clamp=-1.0)
_case("torgb_bwd", "scalar_mis_66x64_cin7_cout1", "rgb_b", cin=7, cout=1, h=66, w=64, mis=1)

# ---- smc_torgb_act_bwd_f32: the channel split (grid.z) is planned(), never a literal
for _cin in (64, 48, 24, 20):
    _case("torgb_act_bwd", f"vec_cin{_cin}", "rgb_ab_vec", cin=_cin)
    _case("torgb_act_bwd", f"scalar_cin{_cin}", "rgb_ab", cin=_cin, h=15, w=17, g_next=(_cin != 48))
_case("torgb_act_bwd", "vec_cin64_last_block", "rgb_ab_vec", cin=64, g_next=False)
_case("torgb_act_bwd", "vec_cin64_cout4", "rgb_ab_vec", cin=64, cout=4, clamp_rgb=-1.0)
_case("torgb_act_bwd", "scalar_mis_cin64_cout1", "rgb_ab", cin=64, cout=1, mis=1)
_case("torgb_act_bwd", "vec_cin64_planned_large", "rgb_ab_vec", cin=64, plan=(4096, 2))   # the split stops early
_case("torgb_act_bwd", "vec_cin512_66x64", "rgb_ab_vec", n=1, cin=512, h=66, w=64)

# ---- smc_channel_dot_f32
for _rows in (1, 5):
    _case("channel_dot", f"v4_400_r{_rows}", "dot_v4", rows=_rows, len=400)              # the tail loop only
    _case("channel_dot", f"v4_4120_r{_rows}", "dot_v4", rows=_rows, len=4120, scaled=True)    # a four-deep trip + tail
    _case("channel_dot", f"s_63_r{_rows}", "dot", rows=_rows, len=63, scaled=True)
    _case("channel_dot", f"s_1001_r{_rows}", "dot", rows=_rows, len=1001, acc=1)
    _case("channel_dot", f"s_mis_400_r{_rows}", "dot", rows=_rows, len=400, mis=1, scaled=True, acc=1)
_case("channel_dot", "v4_4120_acc", "dot_v4", rows=5, len=4120, acc=1)
_case("channel_dot", "v4_nocancel_16384", "dot_v4", rows=2, len=16384, nocancel=True)
_case("channel_dot", "s_nocancel_16385", "dot", rows=2, len=16385, nocancel=True)

# ---- demodulation
for _cin in (1, 63, 64, 65, 512):
    _case("demod", f"cin{_cin}", "demod", cin=_cin)                                      # n cout = 15 rows: 3 + 3/4 blocks
_case("demod_bwd", "cin33_cout20", "demod_bwd")                    # two column blocks, the second with one live lane
_case("demod_bwd", "cin33_cout7", "demod_bwd", cout=7)                                   # an empty output group
_case("demod_bwd", "cin64_cout64", "demod_bwd", cin=64, cout=64)

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
ENTRY = {"blur": "smc_modconv_blur_act_f32", "blur_bwd": "smc_modconv_blur_act_bwd_f32",
         "act_bwd": "smc_modconv_act_bwd_f32", "epilogue": "smc_modconv_epilogue_f32", "torgb_fwd": "smc_torgb_fwd_f32",
         "torgb_bwd": "smc_torgb_bwd_f32", "torgb_act_bwd": "smc_torgb_act_bwd_f32",
         "channel_dot": "smc_channel_dot_f32", "demod": "smc_modconv_demod_f32",
         "demod_bwd": "smc_modconv_demod_bwd_f32"}


def cases_of(ep):
    return [c for c in CASES if c.ep == ep]


def cdiv(a, b):
    return -(-a // b)


# --------------------------------------------------------------------------------- the dispatchers' guards, restated

def noise_nstride(form, hw):
    kind = FORMS[form].get("noise")
    return {None: 0, "const": 0, "img": hw, "odd": hw + 1 - hw % 2}[kind]


def taps_of(filt):
    """(f or None, fh, fw) of a filter key: f the fp32 [fh, fw] taps the call passes."""
    if filt in ("std", "std_rt"):
        k = torch.tensor([1.0, 3.0, 3.0, 1.0])
        return (None if filt == "std" else torch.outer(k, k) / 64), 4, 4
    gen = torch.Generator().manual_seed(sum(map(ord, filt)))
    fh, fw = (4, 4) if filt == "asym" else map(int, filt[1:].split("x"))
    return torch.rand(fh, fw, generator=gen) / (fh * fw) + torch.randn(fh, fw, generator=gen) * 0.05, fh, fw


def blur_geometry(p):
    _, fh, fw = taps_of(p["filt"])
    px, py = p["pad"]
    full = (p["th"] + 2 * py - fh + 1, p["tw"] + 2 * px - fw + 1)
    return (p["yh"] or full[0], p["yw"] or full[1]), full


def split_stride(p):
    """The split_stride a blur case passes: 0 with one plane (as the product's caller), else the plane set + sextra."""
    return p["n"] * p["c"] * p["th"] * (p["pitch"] or p["tw"]) + p["sextra"] if p["nsplit"] > 1 else 0


def bwd_geometry(p):
    px, py = p["pad"]
    return p["uh"] + 2 * py - 3, p["uw"] + 2 * px - 3


def planned(c, cus=None):
    """(route name, flags, channel split) of a case by the guards in the module docstring.  cus: the device's CU count
    (smc_torgb_act_bwd_f32 only)."""
    p, ep = c.p, c.ep
    if ep == "blur":
        f, fh, fw = taps_of(p["filt"])
        if (fh, fw) != (4, 4):
            return R["blur_g"], 0, 1
        (yh, yw), _ = blur_geometry(p)
        form = FORMS[p["form"]]
        stride = split_stride(p)
        aligned = p["mis"] % 4 == 0     # y, u_save and noise are allocations of their own: 16-B aligned or NULL
        px = p["pad"][0]
        v4 = (stride % 4 == 0 and aligned and yw % 2 == 0 and noise_nstride(p["form"], yh * yw) % 2 == 0 and px <= 4 and
              fw - 1 - px <= 4)
        if not v4:
            return R["blur_f"], 0, 1
        return R["blur_v4s" if f is None and p["fgain"] == 4.0 else "blur_v4"], 0, 1
    if ep == "blur_bwd":
        f, _, fw = taps_of(p["filt"])
        y = "y" if p["from_y"] else "u"
        nstr = 0 if p["from_y"] else noise_nstride(p["form"], p["uh"] * p["uw"])
        px = p["pad"][0]
        flags = DD if p["dd"] and cdiv(p["uh"], 32) * cdiv(p["uw"], 64) > 2 else 0
        if p["uw"] % 4 == 0 and nstr % 4 == 0 and p["mis"] % 4 == 0 and px <= 4 and fw - 1 - px <= 4:
            return R[f"bwd_v4_{y}" + ("s" if f is None and p["fgain"] == 4.0 else "")], flags, 1
        if p["uw"] % 2 == 0 and px % 2 == 0 and nstr % 2 == 0 and p["mis"] % 2 == 0:
            return R[f"bwd_v2_{y}"], flags, 1
        return R[f"bwd_s_{y}"], flags, 1
    if ep == "act_bwd":
        hw = p["h"] * p["w"]
        has_noise = FORMS[p["form"]].get("noise") is not None
        vec4 = (hw % 4 == 0 and (p["from_y"] or not has_noise or noise_nstride(p["form"], hw) % 4 == 0) and
                p["mis"] % 4 == 0)
        blocks = act_bwd_blocks(hw, vec4)
        y = "y" if p["from_y"] else "u"
        return R[("act_v4_" if vec4 else "act_") + y], DD if p["dd"] and blocks > 2 else 0, 1
    if ep == "epilogue":
        return R["epi"], 0, 1
    if ep in ("torgb_fwd", "torgb_bwd"):
        hw = p["h"] * p["w"]
        k = "rgb_f" if ep == "torgb_fwd" else "rgb_b"
        if hw <= 4096:
            return R[k + "_small"], 0, 1
        return R[k + "_vec" if hw % 4 == 0 and p["mis"] % 4 == 0 else k], 0, 1
    if ep == "torgb_act_bwd":
        hw = p["h"] * p["w"]
        vec = hw % 4 == 0 and p["mis"] % 4 == 0
        gx = cdiv(hw // 4 if vec else hw, 256)
        n_plan = p["n"]
        if p["plan"]:
            plan, local = p["plan"]
            n_plan = max(1, (p["n"] * plan + local // 2) // local)       # smc::plan_rows
        nz = 1
        if cus is not None:
            while gx * n_plan * nz < 4 * cus and p["cin"] % (16 * nz) == 0:
                nz *= 2
        return R["rgb_ab_vec" if vec else "rgb_ab"], 0, (nz if cus is not None else None)
    if ep == "channel_dot":
        return R["dot_v4" if p["len"] % 4 == 0 and p["mis"] % 4 == 0 else "dot"], 0, 1
    return R[ep], 0, 1


def act_bwd_blocks(hw, vec4):
    return cdiv(hw // 4, 1024) if vec4 else max(1, cdiv(hw, 2048))


def chain(c):
    """The longest chain of dependent additions a term of the case's reduction passes through (module docstring)."""
    p, ep = c.p, c.ep
    block = 6 + 3
    if ep == "blur_bwd":
        # elements of the haloed 35 x 67 tile per thread: 10 scalar loads, 5 pairs, 3 float4 groups
        per = 12 if "bwd_v4" in c.route else 10
        th, tw = bwd_geometry(p)
        tiles = cdiv(th, 32) * cdiv(tw, 64)
        return per + block + (cdiv(tiles, 64) + 6 + 1 if c.flags & DD else 2)
    if ep == "act_bwd":
        hw = p["h"] * p["w"]
        vec4 = "vec4" in c.route
        blocks = act_bwd_blocks(hw, vec4)
        per = 16 if vec4 else cdiv(hw, blocks * 256)
        return per + block + (cdiv(blocks, 64) + 6 + 1 if c.flags & DD else 2)
    if ep == "channel_dot":
        if c.route == R["dot_v4"]:
            len4 = p["len"] // 4
            # 3 adds inside a float4's dot, one per trip of its accumulator (tail trips go to acc[0]), 2 to fold the four
            return 3 + cdiv(len4, 1024) + 4 + 2 + block + p["acc"]
        return cdiv(p["len"], 256) + block + p["acc"]
    if ep == "demod":
        return cdiv(p["cin"], 64) + 6 + 1          # + eps
    if ep == "demod_bwd":
        return cdiv(p["cout"], 8) + 8 + 1          # per thread, the 8 LDS partials, ds +=
    raise KeyError(ep)


# --------------------------------------------------------------------------------- fp64 pieces

def fir64(x, taps, pad, flip, gain):
    """upfirdn2d(x, taps, padding = pad on both sides, flip_filter = flip, gain) at up = down = 1, in x's dtype:
    F.conv2d correlates, so the taps are flipped unless flip."""
    k = taps.to(x.dtype) * gain
    if not flip:
        k = k.flip(0, 1)
    px, py = pad
    n, c, h, w = x.shape
    xp = F.pad(x, [px, px, py, py])
    return F.conv2d(xp.reshape(n * c, 1, h + 2 * py, w + 2 * px), k[None, None]).reshape(n, c, h + 2 * py - k.shape[0] + 1,
                                                                                        w + 2 * px - k.shape[1] + 1)


def act64(name, z, alpha):
    if name == "relu":
        return z.clamp(min=0)
    if name == "lrelu":
        return torch.where(z >= 0, z, z * alpha)
    assert name == "linear"
    return z


def epi64(u, dten, ops, form, h, w):
    """The header's MODACT formula in fp64.  u: [n, c, h, w]; dten: [n, c] (ones where the form has no d).  Returns
    (y, z, act(z) gain before the clamp, S)."""
    f = FORMS[form]
    n = u.shape[0]
    dd = dten[:, :, None, None]
    nz = torch.zeros(1, 1, 1, 1, dtype=torch.float64)
    if f.get("noise"):
        nst = ops["nstride"]
        t = ops["noise"].double()
        nz = t[:h * w].reshape(1, 1, h, w) if nst == 0 else t.reshape(n, nst)[:, :h * w].reshape(n, 1, h, w)
        if f.get("strength"):
            nz = nz * ops["strength"].double().item()
    b = ops["bias"].double()[None, :, None, None] if f.get("bias") else torch.zeros(1, 1, 1, 1, dtype=torch.float64)
    z = u * dd + nz + b
    pre = act64(f["act"], z, f["alpha"]) * f["gain"]
    y = pre.clamp(-f["clamp"], f["clamp"]) if f["clamp"] >= 0 else pre
    return y, z, pre, (u * dd).abs() + nz.abs() + b.abs()


def act_grad64(form, g, y):
    """bias_act's y-referenced gradient (bias_act.cu:51-142) of a form in fp64: g gain act'(y), 0 where |y| >= clamp."""
    f = FORMS[form]
    r = g
    if f["act"] == "relu":
        r = torch.where(y > 0, g, torch.zeros_like(g))
    elif f["act"] == "lrelu":
        r = torch.where(y > 0, g, g * f["alpha"])
    r = r * f["gain"]
    if f["clamp"] >= 0:
        r = torch.where((y > -f["clamp"]) & (y < f["clamp"]), r, torch.zeros_like(r))
    return r


def y_bound(form, dten, err_u, S):
    f = FORMS[form]
    lip = max(1.0, f["alpha"]) if f["act"] == "lrelu" else 1.0
    ke = 4 if f["alpha"] <= 0.5 else 5
    return f["gain"] * lip * (dten.abs()[:, :, None, None] * err_u + ke * EPS * S)


def epi_ops(gen, form, n, c, hw):
    nst = noise_nstride(form, hw)
    return dict(d=torch.rand(n, c, generator=gen) + 0.5, nstride=nst,
                noise=torch.randn(n * nst if nst else hw, generator=gen), strength=torch.tensor([0.3]),
                bias=torch.randn(c, generator=gen) * 0.3)


def dten64(form, ops, n, c):
    return ops["d"].double() if FORMS[form].get("d") else torch.ones(n, c, dtype=torch.float64)


def margins_ok(z, pre, clamp):
    ok = bool((z.abs() >= MARGIN).all())
    if clamp >= 0:
        ok = ok and bool(((pre.abs() - clamp).abs() >= MARGIN).all())
    return ok


def push_margins(u, ops, form, h, w):
    """Move the elements of the fp32 u whose z or |act(z) gain| lies inside a kink margin out of it (in place)."""
    f = FORMS[form]
    dten = dten64(form, ops, u.shape[0], u.shape[1])
    for _ in range(16):
        _, z, pre, _ = epi64(u.double(), dten, ops, form, h, w)
        bad = z.abs() < MARGIN
        if f["clamp"] >= 0:
            bad |= (pre.abs() - f["clamp"]).abs() < MARGIN
        if not bad.any():
            return
        u += (bad * (0.01 / dten[:, :, None, None])).float()
    raise AssertionError("margins not reached")


def push_y(y, clamp):
    for _ in range(16):
        bad = y.abs() < MARGIN
        if clamp >= 0:
            bad |= (y.abs() - clamp).abs() < MARGIN
        if not bad.any():
            return
        y += bad.float() * 0.01
    raise AssertionError("margins not reached")


def _gen(c):
    return torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id)))


# --------------------------------------------------------------------------------- inputs and references per entry
# make_inputs(c) -> dict of CPU fp32 operands; reference(c, d) -> [(name, fp64 value, elementwise bound)] in launch()'s
# output order; backward_margins(c, d) -> True when the case's kink margins hold (forward cases: True).

def make_inputs(c):
    gen, p, ep = _gen(c), c.p, c.ep
    d = {}
    if ep == "blur":
        n, ch, th, tw, ns = p["n"], p["c"], p["th"], p["tw"], p["nsplit"]
        pitch = p["pitch"] or tw
        stride = n * ch * th * pitch + p["sextra"]
        assert ns > 1 or p["sextra"] == 0
        flat = torch.full((ns * stride,), float("nan"))
        d["Tv"] = torch.randn(ns, n, ch, th, tw, generator=gen)
        for s in range(ns):
            flat[s * stride: s * stride + n * ch * th * pitch].view(n, ch, th, pitch)[..., :tw] = d["Tv"][s]
        d["T"], d["stride"] = flat, split_stride(p)
        (yh, yw), _ = blur_geometry(p)
        d["ops"] = epi_ops(gen, p["form"], n, ch, yh * yw)
    elif ep in ("blur_bwd", "act_bwd"):
        n, ch = p["n"], p["c"]
        h, w = (p["uh"], p["uw"]) if ep == "blur_bwd" else (p["h"], p["w"])
        f = FORMS[p["form"]]
        d["ops"] = epi_ops(gen, p["form"], n, ch, h * w)
        d["g"] = torch.randn(n, ch, h, w, generator=gen)
        u = torch.randn(n, ch, h, w, generator=gen)
        if p["from_y"]:
            u = u * 0.8
            push_y(u, f["clamp"])
        else:
            push_margins(u, d["ops"], p["form"], h, w)
        d["u"] = u
        if p["nocancel"]:     # dz = g gain act'(.), act' >= 0: dz u >= 0 with the sign of u (u = 0 has measure 0)
            d["g"] = d["g"].abs() * torch.where(u >= 0, 1.0, -1.0)
        d["dd0"] = torch.randn(n, ch, generator=gen) if c.flags & DD else torch.zeros(n, ch)
    elif ep == "epilogue":
        n, ch, h, w, ns = p["n"], p["c"], p["h"], p["w"], p["nsplit"]
        d["src"] = torch.randn(ns, n, ch, h, w, generator=gen)
        d["ops"] = epi_ops(gen, p["form"], n, ch, h * w)
    elif ep in ("torgb_fwd", "torgb_bwd", "torgb_act_bwd"):
        n, cin, cout, hw = p["n"], p["cin"], p["cout"], p["h"] * p["w"]
        d["w"] = torch.randn(cout, cin, generator=gen) / cin ** 0.5
        d["s"] = torch.rand(n, cin, generator=gen) + 0.5
        if ep == "torgb_fwd":
            d["x"] = torch.randn(n, cin, hw, generator=gen) * 0.3
            d["b"] = torch.randn(cout, generator=gen) * 0.1
        else:
            clamp = p["clamp"] if ep == "torgb_bwd" else p["clamp_rgb"]
            d["g"] = torch.randn(n, cout, hw, generator=gen)
            y = torch.randn(n, cout, hw, generator=gen) * 0.3
            push_y(y, clamp)
            d["y_rgb"] = y
        if ep == "torgb_bwd":
            d["dx0"] = torch.randn(n, cin, hw, generator=gen)
        if ep == "torgb_act_bwd":
            d["g_next"] = torch.randn(n, cin, hw, generator=gen)
            d["d"] = torch.rand(n, cin, generator=gen) + 0.5
            y = torch.randn(n, cin, hw, generator=gen) * 0.8
            push_y(y, _L["clamp"])
            d["y"] = y
    elif ep == "channel_dot":
        rows, ln = p["rows"], p["len"]
        d["a"] = torch.randn(rows, ln, generator=gen)
        d["b"] = d["a"].clone() if p["nocancel"] else torch.randn(rows, ln, generator=gen)
        d["scale"] = torch.rand(rows, generator=gen) + 0.5
        d["out0"] = torch.randn(rows, generator=gen)
    elif ep == "demod":
        d["s"] = torch.randn(p["n"], p["cin"], generator=gen)
        d["wsq"] = torch.rand(p["cout"], p["cin"], generator=gen) + 0.01
    elif ep == "demod_bwd":
        n, cin, cout = p["n"], p["cin"], p["cout"]
        d["s"] = torch.randn(n, cin, generator=gen)
        d["d"] = torch.rand(n, cout, generator=gen) + 0.5
        d["dd"] = torch.randn(n, cout, generator=gen)
        d["wsq"] = torch.rand(cout, cin, generator=gen)
        d["ds0"] = torch.randn(n, cin, generator=gen)
    return d


def backward_margins(c, d):
    p, ep = c.p, c.ep
    if ep in ("blur_bwd", "act_bwd"):
        f = FORMS[p["form"]]
        h, w = d["u"].shape[2:]
        if p["from_y"]:
            return margins_ok(d["u"].double(), d["u"].double(), f["clamp"])
        _, z, pre, _ = epi64(d["u"].double(), dten64(p["form"], d["ops"], p["n"], p["c"]), d["ops"], p["form"], h, w)
        return margins_ok(z, pre, f["clamp"])
    if ep == "torgb_bwd":
        return margins_ok(d["y_rgb"].double(), d["y_rgb"].double(), p["clamp"])
    if ep == "torgb_act_bwd":
        return (margins_ok(d["y_rgb"].double(), d["y_rgb"].double(), p["clamp_rgb"]) and
                margins_ok(d["y"].double(), d["y"].double(), _L["clamp"]))
    return True


def fir_k(p):
    """Roundings of one FIR output of the case's kernel (module docstring)."""
    f, fh, fw = taps_of(p["filt"])
    if (fh, fw) != (4, 4):
        return 2 + fh * fw
    return 16 if f is None and p["fgain"] == 4.0 else 17


def taps64(p):
    f, _, _ = taps_of(p["filt"])
    return (taps_of("std_rt")[0] if f is None else f).double()


def bwd_grads(c, d):
    """(du64, dd64 without dd0, dz64 u64 magnitudes summed per plane) of an epilogue backward case."""
    p = c.p
    n, ch, h, w = d["u"].shape
    g = d["g"].double()
    if p["from_y"]:
        dten = dten64(p["form"], d["ops"], n, ch)
        return act_grad64(p["form"], g, d["u"].double()) * dten[:, :, None, None], None, None
    u = d["u"].double().requires_grad_()
    dten = dten64(p["form"], d["ops"], n, ch).requires_grad_()
    y, _, _, _ = epi64(u, dten, d["ops"], p["form"], h, w)
    du, dd = torch.autograd.grad((y * g).sum(), (u, dten))
    dz_u = (du / dten.detach()[:, :, None, None]) * d["u"].double()
    return du, dd, dz_u.abs().sum((2, 3))


def reference(c, d):
    p, ep = c.p, c.ep
    if ep == "blur":
        form = p["form"]
        (yh, yw), _ = blur_geometry(p)
        taps = taps64(p)
        crop = lambda t: t[:, :, :yh, :yw]
        u64 = crop(fir64(d["Tv"].double().sum(0), taps, p["pad"], p["flip"], p["fgain"]))
        B = crop(fir64(d["Tv"].double().abs().sum(0), taps.abs(), p["pad"], p["flip"], abs(p["fgain"])))
        err_u = (fir_k(p) + p["nsplit"] - 1) * EPS * B
        if FORMS[form]["mode"] == "STORE":
            return [("y", u64, err_u)]
        dten = dten64(form, d["ops"], p["n"], p["c"])
        y, _, _, S = epi64(u64, dten, d["ops"], form, yh, yw)
        outs = [("y", y, y_bound(form, dten, err_u, S))]
        return outs + ([("u_save", u64, err_u)] if FORMS[form].get("u_save") else [])
    if ep == "act_bwd":
        du, dd, B = bwd_grads(c, d)
        outs = [("du", du, 3 * EPS * du.abs())]
        if p["dd"]:
            outs.append(("dd", dd + d["dd0"].double(), (2 + chain(c)) * EPS * (B + d["dd0"].double().abs())))
        return outs
    if ep == "blur_bwd":
        du, dd, B = bwd_grads(c, d)
        taps = taps64(p)
        th, tw = bwd_geometry(p)
        if p["from_y"]:
            dt = fir64(du, taps, p["pad"], p["flip"], p["fgain"])
        else:   # autograd through the forward FIR (pad 3 - adjoint pad, the other flip): U = u + FIR(T), T = 0
            n, ch, h, w = d["u"].shape
            T = torch.zeros(n, ch, th, tw, dtype=torch.float64, requires_grad=True)
            fwd_pad = (3 - p["pad"][0], 3 - p["pad"][1])
            U = d["u"].double() + fir64(T, taps, fwd_pad, 1 - p["flip"], p["fgain"])
            y, _, _, _ = epi64(U, dten64(p["form"], d["ops"], n, ch), d["ops"], p["form"], h, w)
            (dt,) = torch.autograd.grad((y * d["g"].double()).sum(), T)
        Bt = fir64(du.abs(), taps.abs(), p["pad"], p["flip"], abs(p["fgain"]))
        assert dt.shape[2:] == (th, tw)
        outs = [("dt", dt, (3 + fir_k(p)) * EPS * Bt)]
        if p["dd"]:
            outs.append(("dd", dd + d["dd0"].double(), (2 + chain(c)) * EPS * (B + d["dd0"].double().abs())))
        return outs
    if ep == "epilogue":
        form = p["form"]
        u64, B = d["src"].double().sum(0), d["src"].double().abs().sum(0)
        err_u = (p["nsplit"] - 1) * EPS * B
        if FORMS[form]["mode"] == "STORE":
            return [("y", u64, err_u)]
        dten = dten64(form, d["ops"], p["n"], p["c"])
        y, _, _, S = epi64(u64, dten, d["ops"], form, p["h"], p["w"])
        return [("y", y, y_bound(form, dten, err_u, S)), ("u_save", u64, err_u)]
    if ep == "torgb_fwd":
        ws = d["w"].double()[None] * d["s"].double()[:, None, :]                 # [n, cout, cin]
        b = d["b"].double()[None, :, None] if p["bias"] else torch.zeros(1, 1, 1, dtype=torch.float64)
        y = torch.einsum("noi,nip->nop", ws, d["x"].double()) + b
        B = torch.einsum("noi,nip->nop", ws.abs(), d["x"].double().abs()) + b.abs()
        if p["clamp"] >= 0:
            y = y.clamp(-p["clamp"], p["clamp"])
        return [("y", y, (p["cin"] + 3) * EPS * B)]
    if ep == "torgb_bwd":
        s = d["s"].double() if p["scale"] else torch.ones_like(d["s"].double())
        ws = d["w"].double()[None] * s[:, None, :]
        x = torch.zeros(p["n"], p["cin"], p["h"] * p["w"], dtype=torch.float64, requires_grad=True)
        # x = 0 plus the given y as a constant: autograd's clamp mask is then the given one
        y = torch.einsum("noi,nip->nop", ws, x) + d["y_rgb"].double()
        yc = y.clamp(-p["clamp"], p["clamp"]) if p["clamp"] >= 0 else y
        (dx,) = torch.autograd.grad((yc * d["g"].double()).sum(), x)
        gm = act_grad64_linear(d["g"].double(), d["y_rgb"].double(), p["clamp"])
        B = torch.einsum("noi,nop->nip", ws.abs(), gm.abs())
        k = p["cout"] + 2
        if p["acc"]:
            dx, B, k = dx + d["dx0"].double(), B + d["dx0"].double().abs(), k + 1
        return [("dx", dx, k * EPS * B)]
    if ep == "torgb_act_bwd":
        ws = d["w"].double()[None] * d["s"].double()[:, None, :]
        gm = act_grad64_linear(d["g"].double(), d["y_rgb"].double(), p["clamp_rgb"])
        t = torch.einsum("noi,nop->nip", ws, gm)
        Bt = torch.einsum("noi,nop->nip", ws.abs(), gm.abs())
        gy, By = t, Bt
        if p["g_next"]:
            gy, By = gy + d["g_next"].double(), By + d["g_next"].double().abs()
        dk = d["d"].double()[:, :, None]
        du = act_grad64("lrelu_clamp", gy, d["y"].double()) * dk
        Bdu = act_grad64("lrelu_clamp", By, d["y"].double()) * dk
        return [("du", du, (p["cout"] + 2 + 1 + 3) * EPS * Bdu)]
    if ep == "channel_dot":
        a, b = d["a"].double(), d["b"].double()
        out, B = (a * b).sum(1), (a * b).abs().sum(1)
        if p["acc"]:
            out, B = out + d["out0"].double(), B + d["out0"].double().abs()
        outs = [("out", out, (2 + chain(c)) * EPS * B)]
        if p["scaled"]:
            sc = a * d["scale"].double()[:, None]
            outs.append(("a_scaled", sc, EPS * sc.abs()))
        return outs
    if ep == "demod":
        acc = torch.einsum("ni,oi->no", d["s"].double() ** 2, d["wsq"].double()) + DEMOD_EPS
        dref = acc.rsqrt()
        return [("d", dref, dref * ((2 + chain(c)) * EPS / 2 * 1.001 + RSQRT_REL))]
    if ep == "demod_bwd":
        s, dv, dd, wsq = (d[k].double() for k in ("s", "d", "dd", "wsq"))
        t = torch.einsum("no,oi->ni", dd * dv ** 3, wsq)
        Bt = torch.einsum("no,oi->ni", (dd * dv ** 3).abs(), wsq.abs())
        ds0 = d["ds0"].double()
        return [("ds", ds0 - s * t, (2 + chain(c)) * EPS * (ds0.abs() + s.abs() * Bt))]
    raise KeyError(ep)


DEMOD_EPS = 1e-8


def act_grad64_linear(g, y, clamp):
    """ToRGB's linear bias_act gradient mask: g where |y| < clamp (everywhere without a clamp)."""
    return g if clamp < 0 else torch.where((y > -clamp) & (y < clamp), g, torch.zeros_like(g))


# --------------------------------------------------------------------------------- launch

def dev(t, mis=0):
    """A device copy of t that starts `mis` floats past a 256-B aligned address (and has 8 floats of slack behind)."""
    buf = torch.empty(t.numel() + 8 + mis, device=DEV)
    assert buf.data_ptr() % 256 == 0
    v = buf[mis: mis + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def nan_like(shape, mis=0):
    return dev(torch.full(tuple(shape), float("nan")), mis)


def build_epilogue(form, ops, keep, from_y=0):
    from stylemc_amd import _hip
    f = FORMS[form]
    e = _hip.ConvEpilogue()
    e.mode = getattr(_hip, "EPI_" + f["mode"])
    if f["mode"] == "STORE":
        return e
    e.act, e.alpha, e.gain, e.clamp = _hip.ACT_CODES[f["act"]], f["alpha"], f["gain"], f["clamp"]
    e.grad_from_y = from_y

    def put(name):
        t = dev(ops[name])
        keep.append(t)
        return t.data_ptr()
    if f.get("d"):
        e.d = put("d")
    if f.get("noise"):
        e.noise, e.noise_nstride = put("noise"), ops["nstride"]
    if f.get("strength"):
        e.noise_strength = put("strength")
    if f.get("bias"):
        e.bias = put("bias")
    return e


def report():
    from stylemc_amd import _hip
    lib = _hip.load()
    r = lib.smc_modconv_aux_last_route()
    name = lib.smc_modconv_aux_route_name(r)
    return (name.decode() if name is not None else f"<route {r}>", lib.smc_modconv_aux_last_route_flags(),
            lib.smc_modconv_aux_last_nsplit())


def route_names():
    from stylemc_amd import _hip
    lib = _hip.load()
    return [lib.smc_modconv_aux_route_name(i).decode() for i in range(lib.smc_modconv_aux_route_count())]


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def launch(c, d):
    """One launch of the case through its entry point.  Returns (outputs in reference()'s order, (route name, flags,
    split)); every output buffer was filled with NaN (or the case's prefill) before the launch."""
    from stylemc_amd import _hip
    lib = _hip.load()
    p, ep = c.p, c.ep
    keep, st = [], _hip.stream()
    if ep == "blur":
        f, fh, fw = taps_of(p["filt"])
        form = FORMS[p["form"]]
        (yh, yw), _ = blur_geometry(p)
        T = dev(d["T"], p["mis"])
        fd = dev(f) if f is not None else None
        y = nan_like((p["n"], p["c"], yh, yw))
        e = build_epilogue(p["form"], d["ops"], keep)
        u = None
        if form.get("u_save"):
            u = nan_like(y.shape)
            e.u_save = u.data_ptr()
        _hip.call(ENTRY[ep], T.data_ptr(), p["nsplit"], d["stride"], y.data_ptr(), p["n"], p["c"], p["th"], p["tw"],
                  p["pitch"], yh, yw, _hip.ptr(fd), fh, fw, p["pad"][0], p["pad"][1], p["fgain"], p["flip"],
                  ctypes.byref(e), st)
        outs = [y] + ([u] if u is not None else [])
    elif ep in ("blur_bwd", "act_bwd"):
        g, u = dev(d["g"], p["mis"]), dev(d["u"], p["mis"])
        e = build_epilogue(p["form"], d["ops"], keep, p["from_y"])
        dd = dev(d["dd0"]) if p["dd"] else None
        n, ch, h, w = d["u"].shape
        if ep == "act_bwd":
            du = nan_like(d["u"].shape)
            nb = lib.smc_modconv_act_bwd_workspace_size(n, ch, h, w)
            ws = nan_like((max(nb // 4, 1),))
            _hip.call(ENTRY[ep], g.data_ptr(), u.data_ptr(), du.data_ptr(), _hip.ptr(dd), n, ch, h, w, ctypes.byref(e),
                      ws.data_ptr() if nb else None, nb, st)
            outs = [du]
        else:
            f, fh, fw = taps_of(p["filt"])
            fd = dev(f) if f is not None else None
            th, tw = bwd_geometry(p)
            dt = nan_like((n, ch, th, p["pitch"] or tw))
            nb = lib.smc_modconv_blur_act_bwd_workspace_size(n, ch, h, w, th, tw)
            ws = nan_like((max(nb // 4, 1),))
            _hip.call(ENTRY[ep], g.data_ptr(), u.data_ptr(), dt.data_ptr(), _hip.ptr(dd), n, ch, h, w, th, tw,
                      p["pitch"], _hip.ptr(fd), fh, fw, p["pad"][0], p["pad"][1], p["fgain"], p["flip"],
                      ctypes.byref(e), ws.data_ptr() if nb else None, nb, st)
            torch.cuda.synchronize()
            assert torch.isnan(dt[..., tw:]).all(), f"{c.id}: columns beyond t_w were written"
            outs = [dt[..., :tw]]
        outs += [dd] if dd is not None else []
    elif ep == "epilogue":
        src = dev(d["src"])
        n, ch, h, w = d["src"].shape[1:]
        y = nan_like((n, ch, h, w))
        e = build_epilogue(p["form"], d["ops"], keep)
        outs = [y]
        if FORMS[p["form"]].get("u_save"):
            u = nan_like(y.shape)
            e.u_save = u.data_ptr()
            outs.append(u)
        _hip.call(ENTRY[ep], src.data_ptr(), p["nsplit"], n * ch * h * w, y.data_ptr(), n, ch, h, w, ctypes.byref(e), st)
    elif ep == "torgb_fwd":
        x, w, s = dev(d["x"], p["mis"]), dev(d["w"]), dev(d["s"])
        b = dev(d["b"]) if p["bias"] else None
        y = nan_like((p["n"], p["cout"], p["h"] * p["w"]), p["mis"])
        _hip.call(ENTRY[ep], x.data_ptr(), w.data_ptr(), s.data_ptr(), _hip.ptr(b), y.data_ptr(), p["n"], p["cin"],
                  p["cout"], p["h"], p["w"], p["clamp"], st)
        outs = [y]
    elif ep == "torgb_bwd":
        g, y, w, s = dev(d["g"]), dev(d["y_rgb"]), dev(d["w"]), dev(d["s"])
        dx = dev(d["dx0"], p["mis"]) if p["acc"] else nan_like(d["dx0"].shape, p["mis"])
        _hip.call(ENTRY[ep], g.data_ptr(), y.data_ptr(), w.data_ptr(), s.data_ptr() if p["scale"] else None,
                  dx.data_ptr(), p["n"], p["cin"], p["cout"], p["h"], p["w"], p["clamp"], p["scale"], p["acc"], st)
        outs = [dx]
    elif ep == "torgb_act_bwd":
        du, rep_ = launch_torgb_act_bwd(c, d)
        return [du], rep_
    elif ep == "channel_dot":
        a, b, sc = dev(d["a"], p["mis"]), dev(d["b"], p["mis"]), dev(d["scale"])
        out = dev(d["out0"]) if p["acc"] else nan_like(d["out0"].shape)
        asc = nan_like(d["a"].shape, p["mis"]) if p["scaled"] else None
        _hip.call(ENTRY[ep], a.data_ptr(), b.data_ptr(), sc.data_ptr() if p["scaled"] else None, out.data_ptr(),
                  _hip.ptr(asc), p["rows"], p["len"], p["acc"], st)
        outs = [out] + ([asc] if asc is not None else [])
    elif ep == "demod":
        s, wsq = dev(d["s"]), dev(d["wsq"])
        out = nan_like((p["n"], p["cout"]))
        _hip.call(ENTRY[ep], s.data_ptr(), wsq.data_ptr(), out.data_ptr(), p["n"], p["cin"], p["cout"], DEMOD_EPS, st)
        outs = [out]
    elif ep == "demod_bwd":
        s, dv, dd, wsq, ds = (dev(d[k]) for k in ("s", "d", "dd", "wsq", "ds0"))
        _hip.call(ENTRY[ep], s.data_ptr(), dv.data_ptr(), dd.data_ptr(), wsq.data_ptr(), ds.data_ptr(), p["n"],
                  p["cin"], p["cout"], st)
        outs = [ds]
    else:
        raise KeyError(ep)
    rep_ = report()
    torch.cuda.synchronize()
    del keep
    return outs, rep_


def _conv1_epilogue(dten):
    from stylemc_amd import _hip
    e = _hip.ConvEpilogue()
    e.mode, e.grad_from_y = _hip.EPI_MODACT, 1
    e.act, e.alpha, e.gain, e.clamp = _hip.ACT_CODES[_L["act"]], _L["alpha"], _L["gain"], _L["clamp"]
    e.d = dten.data_ptr()
    return e


def launch_torgb_act_bwd(c, d, unfused=False):
    """smc_torgb_act_bwd_f32 of the case, or (unfused) the three passes its header promises bit-equality with:
    smc_torgb_bwd_f32 (scale = 1), the sum with g_next, smc_modconv_act_bwd_f32 (grad_from_y)."""
    from stylemc_amd import _hip
    p, st = c.p, _hip.stream()
    n, cin, cout, h, w = p["n"], p["cin"], p["cout"], p["h"], p["w"]
    g, yr, wt, s, dk = (dev(d[k]) for k in ("g", "y_rgb", "w", "s", "d"))
    gn = dev(d["g_next"], p["mis"]) if p["g_next"] else None
    y, du = dev(d["y"], p["mis"]), nan_like(d["y"].shape, p["mis"])
    e = _conv1_epilogue(dk)
    if unfused:
        t = nan_like(d["y"].shape)
        _hip.call("smc_torgb_bwd_f32", g.data_ptr(), yr.data_ptr(), wt.data_ptr(), s.data_ptr(), t.data_ptr(), n, cin,
                  cout, h, w, p["clamp_rgb"], 1, 0, st)
        gy = dev(torch.zeros(d["y"].shape))
        torch.add(gn, t, out=gy) if gn is not None else gy.copy_(t)
        _hip.call("smc_modconv_act_bwd_f32", gy.data_ptr(), y.data_ptr(), du.data_ptr(), None, n, cin, h, w,
                  ctypes.byref(e), None, 0, st)
        torch.cuda.synchronize()
        return du, None
    with _hip.plan_batch(*(p["plan"] or (0, 0))):
        _hip.call("smc_torgb_act_bwd_f32", g.data_ptr(), yr.data_ptr(), wt.data_ptr(), s.data_ptr(), p["clamp_rgb"],
                  _hip.ptr(gn), y.data_ptr(), du.data_ptr(), n, cin, cout, h, w, ctypes.byref(e), st)
        rep_ = report()
    torch.cuda.synchronize()
    return du, rep_
