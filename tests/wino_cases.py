"""Shared helpers of tests/test_gpu_wino_routes.py and tests/test_wino_predicates.py: the case table of the two
Winograd dispatchers (smc_conv3x3_wino_ws_f32 in csrc/wino.hip, smc_conv3x3_wino4_f32 in csrc/wino4.hip), one launch of
a case through the C ABI, its fp64 CPU reference with the error bound of every output, a Python statement of the
host-side rules (tile block, split plan, fold, epilogue body), and a CPU fp32 model of the Winograd arithmetic.

A case is (id, fam, n, cin, cout, h, w, epi, style, flip, ws):
  fam       2: F(2x2), smc_conv3x3_wino_ws_f32;  4: F(4x4), smc_conv3x3_wino4_f32
  cin, cout the call's K channels and output channels of the [n, cin, h, w] -> [n, cout, h, w] pad-1 3x3 conv
  epi       a key of FORMS (the smc_conv_epilogue the launch carries)
  style     a per-sample input scale s[n, cin]
  flip      1: the taps of the data gradient (smc_wino*_weights_f32 flip = 1 of a [cin][cout][3][3] forward weight)
  ws        F(2x2) only: the call passes the workspace smc_conv3x3_wino_workspace_size() asks for

The guards the routes are read off (plan_wino() in wino.hip; SMC_WINO_FOLD 1, split target 512):
  TC     wino_tc(): `for (tc = 32; tc >= 16; tc /= 2) if ((w / 2) % tc == 0 && (h / 2) % (WBT / tc) == 0)`
         -> 32 where w % 64 == 0 and h % 4 == 0, else 16 where w % 32 == 0 and h % 8 == 0 (so TC 16 means w % 64 == 32)
  fold   `pl.fold = has_s && pl.fold_bytes > 0 && ws_ok`, fold_bytes > 0 iff cin * cout <= 128 * 128: the launch then
         runs SM = 2 with SMC_ROUTE_WINO_FOLD
  SM     `pl.sm = has_s && !pl.fold ? 1 : 2`
  split  `if (pl.split_bytes > 0 && ws_ok)` -> EK 3, SMC_ROUTE_SPLIT_K; the split count: `while (items * ns < 512 &&
         nsteps % (2 * ns) == 0 && nsteps / (2 * ns) >= 8) ns *= 2` -- cin >= 128 for two splits of 8 steps
  EK     smc::epi_body() (wino_host.hpp): `modact_plain = mode == MODACT && !residual`; 1 where `modact_plain && act ==
         LRELU && 0 <= alpha <= 1 && clamp >= 0`; 2 where `modact_plain && act == LINEAR && clamp < 0`; else 0.
         (Neither scale_c nor a NULL operand is
         part of the guard: MODACT lrelu + clamp with scale_c, or with d = bias = strength = NULL, runs EK 1;
         the table holds each of the two both ways, with the clamp (EK 1) and with clamp = -1 (the generic body).)
F(4x4) has the SM and EK guards only (plan_wino4() in wino4.hip; the same epi_body()).

Reference and bounds.  u64 is the fp64 conv of the fp32 operands (x s, W), B = conv(|W|, |x s|) the sum of the
magnitudes of its products, TOL / REL the project's Winograd bounds (F(2x2): 2e-6 B elementwise, 1e-6 relative norm,
tests/test_gpu_wino.py; F(4x4): 8e-6 / 1e-5, tests/test_gpu_wino4.py):
  raw conv outputs (y of STORE, u_save of MODACT; y of modact_linear_bwd = u d gain):  |err| <= |factor| TOL B and the
    relative norm <= REL.
  epilogue outputs.  z = u d scale_c + noise strength + bias and y = clamp(act(z) gain) + residual.  Every activation
    here (lrelu with 0 <= alpha <= 1, relu, PReLU with |alpha_c| <= 1, linear) and the clamp are 1-Lipschitz and
    continuous, so |act(z) - act(z64)| <= |z - z64| at every element, kinks included: no exclusions.  z - z64 has the
    conv error scaled by |d scale_c| and the roundings of the epilogue's own fp32 arithmetic (the product d scale_c, the
    product noise strength, the fma, the bias add, the gain: each relative 2^-24 of a value no larger than
    S = |u64 d scale_c| + |noise strength| + |bias|; 4 of them are allowed), and the final residual add rounds once:
      |y - y64| <= gain (|d scale_c| TOL B + 4 2^-24 S) + |residual| 2^-24
    PRELU (z = u scale_c + bias in u_save, y = PReLU(z)) and AFFINE take it with d = 1, gain = 1, no noise.
    PRELU_GRAD multiplies by a factor chosen by the given act_ref (drawn away from 0): |factor| TOL B.
"""
import collections
import ctypes

import torch

DEV = "cuda"
FOLD = 16        # _hip.ROUTE_WINO_FOLD
SPLIT = 1        # _hip.ROUTE_SPLIT_K
TOL = {2: 2e-6, 4: 8e-6}
REL = {2: 1e-6, 4: 1e-5}
EPS = 2.0 ** -24

Case = collections.namedtuple("Case", "id fam n cin cout h w epi style flip ws")

_L = dict(act="lrelu", alpha=0.2, gain=2 ** 0.5, clamp=1.5)
_FULL = dict(mode="MODACT", d=True, noise="img", strength=True, bias=True, u_save=True)
# epilogue forms: the smc_conv_epilogue fields a launch sets (everything else NULL / 0)
FORMS = {
    "store": dict(mode="STORE"),
    "modact_lrelu": dict(_FULL, **_L),
    "modact_lrelu_const": dict(_FULL, **_L, noise="const"),
    # what modconv._modconv_bwd issues: d = styles, linear, gain 1, clamp -1, u_save = dxs, no noise, no bias
    "modact_linear_bwd": dict(mode="MODACT", d=True, act="linear", alpha=0.0, gain=1.0, clamp=-1.0, u_save=True),
    "modact_linear": dict(_FULL, act="linear", alpha=0.0, gain=2 ** 0.5, clamp=-1.0),
    "modact_lrelu_scale_c": dict(_FULL, **_L, scale_c=True),          # EK 1: scale_c is not in the guard
    "modact_lrelu_nulls": dict(mode="MODACT", noise="img", u_save=True, **_L),     # EK 1 with d, bias, strength NULL
    # ---- the generic body (EK 0)
    "g_relu_clamp": dict(_FULL, act="relu", alpha=0.0, gain=2 ** 0.5, clamp=1.5),
    "g_lrelu_noclamp": dict(_FULL, **dict(_L, clamp=-1.0)),
    "g_linear_clamp": dict(_FULL, act="linear", alpha=0.0, gain=2 ** 0.5, clamp=1.5),
    "g_lrelu_nulls": dict(mode="MODACT", noise="img", u_save=True, **dict(_L, clamp=-1.0)),   # d, bias, strength NULL
    "g_lrelu_scale_c": dict(_FULL, **dict(_L, clamp=-1.0), scale_c=True),
    "g_lrelu_residual": dict(_FULL, **_L, residual=1),
    "prelu": dict(mode="PRELU", scale_c=True, bias=True, alpha_c=True, u_save=True),
    "prelu_grad": dict(mode="PRELU_GRAD", alpha_c=True, act_ref=True),
    "affine_res1": dict(mode="AFFINE", scale_c=True, bias=True, residual=1),
    "affine_res2": dict(mode="AFFINE", scale_c=True, bias=True, residual=2),
}

# Geometry per block shape: [whole image = one block, both borders in one staged patch; two row blocks; interior
# column and row blocks (3 x 3 blocks)], the K ladder (1 / 2 / 3 steps, and a ring that wraps many times) and the
# output-channel blocks (1 / 2 / 3).
GEOM = {
    "tc16": dict(fam=2, hw=[(8, 32), (16, 32), (24, 96)], cin=[8, 16, 24, 64], cout=[32, 64, 96]),
    "tc32": dict(fam=2, hw=[(4, 64), (8, 64), (12, 192)], cin=[8, 16, 24, 64], cout=[32, 64, 96]),
    "f4": dict(fam=4, hw=[(8, 64), (16, 64), (24, 192)], cin=[4, 8, 12, 64], cout=[64, 128, 192]),
}

# One row per launch form, run on every block shape: (key, n, K-ladder index, cout index, geometry index, epi, style,
# flip, ws, (SM, EK, flags) of F(2x2), SM of F(4x4)).  ws is dropped for F(4x4) (no workspace, no fold: a style runs
# SM 1).  n = 3 with three output-channel blocks gives item counts that are no multiple of 8 (the XCD order's
# remainder branch): 18 and 81 items in both families.
_ROWS = [
    ("store_k1_whole", 1, 0, 0, 0, "store", False, 0, False, (2, 0, 0), 2),            # 1 K step: no `ks + 1 < nsteps` issue
    ("store_style_k3_interior", 2, 2, 1, 2, "store", True, 0, False, (1, 0, 0), 1),    # cin != cout, left / top halos
    ("store_flip_k64", 1, 3, 0, 1, "store", False, 1, False, (2, 0, 0), 2),            # ring wraps; flipped taps
    ("modact_lrelu", 2, 1, 1, 2, "modact_lrelu", True, 0, False, (1, 1, 0), 1),
    ("modact_lrelu_k64", 1, 3, 0, 1, "modact_lrelu", True, 0, False, (1, 1, 0), 1),    # the style of every step of a long K
    ("modact_lrelu_fold", 2, 1, 0, 1, "modact_lrelu", True, 0, True, (2, 1, FOLD), 1),
    ("modact_lrelu_const_n3", 3, 2, 2, 1, "modact_lrelu_const", False, 0, False, (2, 1, 0), 2),
    ("modact_linear_bwd", 2, 3, 0, 2, "modact_linear_bwd", False, 1, False, (2, 2, 0), 2),
    ("modact_linear_style_k1", 1, 0, 0, 0, "modact_linear", True, 0, False, (1, 2, 0), 1),
    ("modact_lrelu_scale_c", 2, 1, 0, 0, "modact_lrelu_scale_c", True, 0, True, (2, 1, FOLD), 1),
    ("modact_lrelu_nulls", 1, 0, 1, 1, "modact_lrelu_nulls", False, 0, False, (2, 1, 0), 2),
    ("g_relu_clamp", 1, 1, 0, 1, "g_relu_clamp", True, 0, False, (1, 0, 0), 1),
    ("g_lrelu_noclamp", 2, 2, 0, 0, "g_lrelu_noclamp", False, 0, False, (2, 0, 0), 2),
    ("g_linear_clamp_fold", 2, 1, 0, 0, "g_linear_clamp", True, 0, True, (2, 0, FOLD), 1),
    ("g_lrelu_nulls", 1, 0, 1, 1, "g_lrelu_nulls", False, 0, False, (2, 0, 0), 2),
    ("g_lrelu_scale_c", 1, 1, 0, 1, "g_lrelu_scale_c", True, 0, False, (1, 0, 0), 1),
    ("g_lrelu_residual", 1, 1, 0, 1, "g_lrelu_residual", False, 0, False, (2, 0, 0), 2),
    ("prelu_n3_interior", 3, 0, 2, 2, "prelu", False, 0, False, (2, 0, 0), 2),
    ("prelu_grad", 1, 1, 0, 1, "prelu_grad", False, 0, False, (2, 0, 0), 2),
    ("affine_res1", 1, 2, 0, 0, "affine_res1", False, 1, False, (2, 0, 0), 2),
    ("affine_res2", 2, 1, 1, 1, "affine_res2", True, 0, False, (1, 0, 0), 1),
]

# F(2x2) split-K (EK 3 + smc_modconv_epilogue_f32): (key, block shape, n, cin, cout, geometry index, epi, style,
# (SM, flags), nsplit).  cin = 128 is 16 steps = 2 splits of 8; cin = 256 is 32 steps = 4 splits of 8; every grid here
# is far below 512 items.  cin * cout = 128 * 96 <= 128 * 128 folds; 128 * 160 does not.
_SPLIT_ROWS = [
    ("split_store", "tc16", 1, 128, 32, 0, "store", False, (2, SPLIT), 2),
    ("split_lrelu_fold_n3", "tc16", 3, 128, 96, 0, "modact_lrelu", True, (2, SPLIT | FOLD), 2),
    ("split_prelu_style", "tc16", 1, 128, 160, 1, "prelu", True, (1, SPLIT), 2),
    ("split4_prelu", "tc32", 1, 256, 32, 0, "prelu", False, (2, SPLIT), 4),
    ("split_store_fold_n3", "tc32", 3, 128, 96, 1, "store", True, (2, SPLIT | FOLD), 2),
    ("split_lrelu_style", "tc32", 1, 128, 160, 0, "modact_lrelu", True, (1, SPLIT), 2),
]

CASES = []
# id -> (route name, flags, K splits) each case is built to reach, from the literal (SM, EK, flags) of its row
EXPECTED = {}
for _g, _geo in GEOM.items():
    for _key, _n, _ki, _oi, _gi, _epi, _style, _flip, _ws, (_sm, _ek, _fl), _sm4 in _ROWS:
        _h, _w = _geo["hw"][_gi]
        _c = Case(f"{_g}_{_key}", _geo["fam"], _n, _geo["cin"][_ki], _geo["cout"][_oi], _h, _w, _epi, _style, _flip,
                  _ws and _geo["fam"] == 2)
        CASES.append(_c)
        EXPECTED[_c.id] = ((f"wino4_kernel<{_sm4},{_ek}>", 0, 1) if _geo["fam"] == 4 else
                           (f"wino_kernel<{_g[2:]},{_sm},{_ek}>", _fl, 1))
for _key, _g, _n, _cin, _cout, _gi, _epi, _style, (_sm, _fl), _ns in _SPLIT_ROWS:
    _h, _w = GEOM[_g]["hw"][_gi]
    _c = Case(f"{_g}_{_key}", 2, _n, _cin, _cout, _h, _w, _epi, _style, 0, True)
    CASES.append(_c)
    EXPECTED[_c.id] = (f"wino_kernel<{_g[2:]},{_sm},3>", _fl, _ns)

# w = 128: two 32-column blocks per tile row -- and the width a wino_tc() that offered 64 columns would run as one
# 64-column block (`(w / 2) % 64 == 0`), so that knob cannot change without this case's route assertion failing
CASES.append(Case("tc32_store_w128", 2, 1, 16, 32, 4, 128, "store", False, 0, False))
EXPECTED["tc32_store_w128"] = ("wino_kernel<32,2,0>", 0, 1)

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES) == len(EXPECTED)

# Bounds taken from the CPU fp32 model instead of TOL (module docstring of test_gpu_wino_routes.py, "Short K"; cin = 4
# or 8 only): id -> (max err / B of model_conv() on the case's inputs, the kernel's largest error as a multiple of the
# bound computed with TOL, measured on an MI355X).  The case is held to the bounds computed with 2 x the model's figure
# in TOL's place.
#   f4_prelu_n3_interior (cin = 4, one K step; 2.65 M outputs of 36 products each): the model misses TOL = 8e-6 by
#   itself, 1.458e-5 B, and wino4_kernel<2,0> measures 1.78 x the TOL bound = 1.42e-5 B, 0.50 of the 2 x model bound.
#   The other thirteen cin = 4 / 8 F(4x4) cases meet TOL (0.34 .. 0.97 of their bounds) and stay on it.
SHORT_K = {"f4_prelu_n3_interior": (1.458e-5, 1.78)}


def flops(c):
    """FLOP of the case's fp64 reference (2 x 9 taps x n cin cout h w)."""
    return 2 * 9 * c.n * c.cin * c.cout * c.h * c.w


# --------------------------------------------------------------------------------- the host-side rules, restated

def wino_tc(h, w):
    """Tile columns of the F(2x2) block (include/stylemc_hip.h, smc_conv3x3_wino_supported): 2 tile rows x 32 columns
    where w % 64 == 0 and h % 4 == 0, else 4 x 16 where w % 32 == 0 and h % 8 == 0, else none."""
    if h <= 0 or w <= 0:
        return 0
    if w % 64 == 0 and h % 4 == 0:
        return 32
    if w % 32 == 0 and h % 8 == 0:
        return 16
    return 0


def wino_supported(n, cin, cout, h, w):
    return int(n >= 1 and cin >= 8 and cin % 8 == 0 and cout >= 32 and cout % 32 == 0 and
               n * cin * h * w * 4 < 2 ** 31 and wino_tc(h, w) != 0)


def wino4_supported(n, cin, cout, h, w):
    return int(n >= 1 and cin >= 4 and cin % 4 == 0 and w >= 64 and w % 64 == 0 and h >= 8 and h % 8 == 0 and
               cout >= 64 and cout % 64 == 0 and
               n * cin * h * w * 4 < 2 ** 31 and cin * 36 * cout * 4 < 2 ** 31)


def wino_nsplit(n, cin, cout, h, w):
    items, steps, ns = n * (h * w // 256) * (cout // 32), cin // 8, 1
    while items * ns < 512 and steps % (2 * ns) == 0 and steps // (2 * ns) >= 8:
        ns *= 2
    return ns


def wino_workspace(n, cin, cout, h, w):
    """(split bytes, fold bytes) of smc_conv3x3_wino_workspace_size (their sum; the split-bf16 mode off)."""
    if not wino_supported(n, cin, cout, h, w):
        return 0, 0
    ns = wino_nsplit(n, cin, cout, h, w)
    split = (ns * n * cout * h * w * 4 + 255) // 256 * 256 if ns > 1 else 0
    fold = n * cin * cout * 64 if cin * cout <= 128 * 128 else 0
    return split, fold


def epilogue_body(form):
    """EK of a form by the dispatchers' guards (ek1 / ek2 above; the split form's 3 is decided by the plan)."""
    f = FORMS[form]
    plain = f["mode"] == "MODACT" and not f.get("residual")
    if plain and f["act"] == "lrelu" and 0 <= f["alpha"] <= 1 and f["clamp"] >= 0:
        return 1
    if plain and f["act"] == "linear" and f["clamp"] < 0:
        return 2
    return 0


def planned_route(c):
    """(route name, flags, K splits) of a case by the rules above -- the CPU check of the EXPECTED table."""
    ek = epilogue_body(c.epi)
    if c.fam == 4:
        return f"wino4_kernel<{1 if c.style else 2},{ek}>", 0, 1
    split, fold = wino_workspace(c.n, c.cin, c.cout, c.h, c.w)
    folded = c.ws and c.style and fold > 0
    flags = (FOLD if folded else 0) | (SPLIT if c.ws and split > 0 else 0)
    ns = wino_nsplit(c.n, c.cin, c.cout, c.h, c.w) if flags & SPLIT else 1
    sm = 1 if c.style and not folded else 2
    return f"wino_kernel<{wino_tc(c.h, c.w)},{sm},{3 if flags & SPLIT else ek}>", flags, ns


# --------------------------------------------------------------------------------- inputs, reference, bounds

def make_inputs(c):
    """The case's CPU fp32 operands, seeded by its id."""
    gen = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id)))
    f = FORMS[c.epi]
    d = {}
    wshape = (c.cin, c.cout, 3, 3) if c.flip else (c.cout, c.cin, 3, 3)
    d["W"] = torch.randn(wshape, generator=gen) / (9 * c.cin) ** 0.5
    d["x"] = torch.randn(c.n, c.cin, c.h, c.w, generator=gen)
    d["s"] = torch.rand(c.n, c.cin, generator=gen) + 0.5 if c.style else None
    d["d"] = torch.rand(c.n, c.cout, generator=gen) + 0.5
    d["noise"] = torch.randn((c.n, c.h * c.w) if f.get("noise") == "img" else (c.h * c.w,), generator=gen)
    d["strength"] = torch.tensor([0.3])
    d["bias"] = torch.randn(c.cout, generator=gen)
    d["scale_c"] = torch.rand(c.cout, generator=gen) + 0.5
    d["alpha_c"] = torch.rand(c.cout, generator=gen) * 0.5                  # [0, 0.5)
    r = torch.randn(c.n, c.cout, c.h, c.w, generator=gen)
    d["act_ref"] = torch.where(r >= 0, r + 0.1, r - 0.1)                    # away from 0
    rs = f.get("residual") or 1
    d["residual"] = torch.randn(c.n, c.cout, c.h // rs, c.w // rs, generator=gen)
    return d


def conv_weight64(c, d):
    """The fp64 [cout][cin][3][3] cross-correlation weight of the call (flip = 1: the forward weight's adjoint)."""
    W = d["W"].double()
    return W.flip(2, 3).transpose(0, 1).contiguous() if c.flip else W


def conv64(c, d):
    """(u64, B): the fp64 conv of the fp32 operands and the conv of their magnitudes."""
    import torch.nn.functional as F
    xs = d["x"].double()
    if d["s"] is not None:
        xs = xs * d["s"].double()[:, :, None, None]
    W = conv_weight64(c, d)
    return F.conv2d(xs, W, padding=1), F.conv2d(xs.abs(), W.abs(), padding=1)


def _act64(name, z, alpha):
    if name == "relu":
        return z.clamp(min=0)
    if name == "lrelu":
        return torch.where(z >= 0, z, z * alpha)
    assert name == "linear"
    return z


def reference(c, d, u64, B, tol):
    """Any smc_conv_epilogue form in fp64 from u64: a list of (name, fp64 value, elementwise bound, raw) per output the
    launch writes, in launch()'s order.  raw: a conv output (times a per-channel factor), held to the relative norm
    too.  tol: the elementwise factor of the conv error (TOL[c.fam], or a case's SHORT_K bound)."""
    f = FORMS[c.epi]
    ch = lambda t: t.double()[None, :, None, None]
    res, res_abs = 0.0, 0.0
    if f.get("residual"):
        rs = f["residual"]
        res = torch.zeros_like(u64)
        res[:, :, ::rs, ::rs] = d["residual"].double()
        res_abs = res.abs() * EPS
    sc = ch(d["scale_c"]) if f.get("scale_c") else torch.ones(1, 1, 1, 1, dtype=torch.float64)
    b = ch(d["bias"]) if f.get("bias") else torch.zeros(1, 1, 1, 1, dtype=torch.float64)
    mode = f["mode"]
    if mode == "STORE":
        return [("y", u64 + res, tol * B + res_abs, True)]
    if mode == "PRELU_GRAD":
        fac = torch.where(d["act_ref"].double() >= 0, torch.ones_like(u64), ch(d["alpha_c"]).expand_as(u64))
        return [("y", u64 * fac + res, fac.abs() * tol * B + res_abs, False)]
    if mode == "MODACT":
        dd = d["d"].double()[:, :, None, None] if f.get("d") else torch.ones(1, 1, 1, 1, dtype=torch.float64)
        dsc = dd * sc
        nz = 0.0
        if f.get("noise"):
            nz = d["noise"].double().reshape(-1, 1, c.h, c.w) * (d["strength"].double().item() if f.get("strength") else 1.0)
        z = u64 * dsc + nz + b
        y = _act64(f["act"], z, f["alpha"]) * f["gain"]
        if f["clamp"] >= 0:
            y = y.clamp(-f["clamp"], f["clamp"])
        S = (u64 * dsc).abs() + (nz.abs() if f.get("noise") else 0.0) + b.abs()
        if c.epi == "modact_linear_bwd":   # a raw conv times d gain
            outs = [("y", y, (dsc * f["gain"]).abs() * tol * B, True)]
        else:
            outs = [("y", y + res, f["gain"] * (dsc.abs() * tol * B + 4 * EPS * S) + res_abs, False)]
        if f.get("u_save"):
            outs.append(("u_save", u64, tol * B, True))
        return outs
    z = u64 * sc + b
    zb = sc.abs() * tol * B + 4 * EPS * ((u64 * sc).abs() + b.abs())
    if mode == "AFFINE":
        return [("y", z + res, zb + res_abs, False)]
    assert mode == "PRELU"
    y = torch.where(z >= 0, z, z * ch(d["alpha_c"]))
    return [("y", y + res, zb + res_abs, False), ("u_save", z, zb, False)]


# --------------------------------------------------------------------------------- launch

def build_epilogue(c, d, y, keep):
    """The ConvEpilogue of the case's form (device operands appended to `keep`) and its u_save tensor (or None)."""
    from stylemc_amd import _hip
    f = FORMS[c.epi]
    e = _hip.ConvEpilogue()
    e.mode = getattr(_hip, "EPI_" + f["mode"])
    e.act, e.alpha, e.gain, e.clamp = _hip.ACT_CODES[f.get("act", "linear")], f.get("alpha", 0.0), f.get("gain", 1.0), \
        f.get("clamp", -1.0)

    def dev(name):
        t = d[name].to(DEV)
        keep.append(t)
        return t.data_ptr()
    if f.get("d"):
        e.d = dev("d")
    if f.get("noise"):
        e.noise, e.noise_nstride = dev("noise"), c.h * c.w if f["noise"] == "img" else 0
    if f.get("strength"):
        e.noise_strength = dev("strength")
    if f.get("bias"):
        e.bias = dev("bias")
    for k in ("scale_c", "alpha_c", "act_ref"):
        if f.get(k):
            setattr(e, k, dev(k))
    if f.get("residual"):
        e.residual, e.residual_stride = dev("residual"), f["residual"]
    u = None
    if f.get("u_save"):
        u = torch.full_like(y, float("nan"))
        e.u_save = u.data_ptr()
    return e, u


def launch(c, d):
    """One launch of the case through its entry point.  Returns (outputs, route name, flags, K splits); the outputs
    (y, then u_save where the form has one) were filled with NaN before the launch."""
    from stylemc_amd import _hip
    lib = _hip.load()
    keep = []
    x, W = d["x"].to(DEV), d["W"].to(DEV)
    s = d["s"].to(DEV) if d["s"] is not None else None
    wout, win = (c.cin, c.cout) if c.flip else (c.cout, c.cin)    # the [cout][cin][3][3] shape of W as stored
    uw = torch.empty((16 if c.fam == 2 else 36) * c.cin * c.cout, device=DEV)
    _hip.call("smc_wino_weights_f32" if c.fam == 2 else "smc_wino4_weights_f32", W.data_ptr(), wout, win, c.flip,
              uw.data_ptr(), _hip.stream())
    y = torch.full((c.n, c.cout, c.h, c.w), float("nan"), device=DEV)
    e, u = build_epilogue(c, d, y, keep)
    if c.fam == 2:
        nb = lib.smc_conv3x3_wino_workspace_size(c.n, c.cin, c.cout, c.h, c.w) if c.ws else 0
        ws = torch.full((max(nb // 4, 1),), float("nan"), device=DEV)
        _hip.call("smc_conv3x3_wino_ws_f32", x.data_ptr(), c.n, c.cin, c.h, c.w, y.data_ptr(), c.cout, uw.data_ptr(),
                  _hip.ptr(s), ctypes.byref(e), ws.data_ptr() if nb else None, nb, _hip.stream())
        route, flags, ns = (lib.smc_conv3x3_wino_last_route(), lib.smc_conv3x3_wino_last_route_flags(),
                            lib.smc_conv3x3_wino_last_nsplit())
    else:
        _hip.call("smc_conv3x3_wino4_f32", x.data_ptr(), c.n, c.cin, c.h, c.w, y.data_ptr(), c.cout, uw.data_ptr(),
                  _hip.ptr(s), ctypes.byref(e), _hip.stream())
        route, flags, ns = lib.smc_conv3x3_wino4_last_route(), 0, 1
    torch.cuda.synchronize()
    del keep
    return [y] + ([u] if u is not None else []), route_name(c.fam, route), flags, ns


def route_name(fam, route):
    from stylemc_amd import _hip
    lib = _hip.load()
    name = (lib.smc_conv3x3_wino_route_name if fam == 2 else lib.smc_conv3x3_wino4_route_name)(route)
    return name.decode() if name is not None else f"<route {route}>"


def route_names(fam):
    from stylemc_amd import _hip
    lib = _hip.load()
    count = lib.smc_conv3x3_wino_route_count() if fam == 2 else lib.smc_conv3x3_wino4_route_count()
    return [route_name(fam, r) for r in range(count)]


# --------------------------------------------------------------------------------- CPU fp32 model of the arithmetic

def _bt6(x):
    """B^T x along dim 0 of a [6, ...] fp32 tensor, in the order of wino4.hip's bt6 (without its fused roundings)."""
    p, q, r, s = x[1] + x[2], x[3] + x[4], x[1] - x[2], x[4] - x[3]
    u, w = x[3] - x[1], x[4] - x[2]
    return torch.stack([4 * x[0] + (-5 * x[2] + x[4]), -4 * p + q, 4 * r + s, 2 * u + w, -2 * u + w,
                        4 * x[1] + (-5 * x[3] + x[5])])


def _at6(m):
    s12, d12, s34, d34 = m[1] + m[2], m[1] - m[2], m[3] + m[4], m[3] - m[4]
    return torch.stack([m[0] + s12 + s34, 2 * d34 + d12, 4 * s34 + s12, 8 * d34 + d12 + m[5]])


def _bt4(x):
    return torch.stack([x[0] - x[2], x[1] + x[2], x[2] - x[1], x[1] - x[3]])


def _at4(m):
    return torch.stack([m[0] + m[1] + m[2], m[1] - m[2] - m[3]])


def model_conv(c, d):
    """The case's raw conv by the same Winograd arithmetic in torch fp32 on the CPU: the kernels' transforms in their
    order (bt6 / at6; F(2x2)'s adds), U by the weight kernels' rules (F(4x4): G g G^T in fp64, rounded once; F(2x2):
    fp32 with the 1/2 factors), the per-point channel sums as fp32 matmuls.  Never the kernel under test: the yardstick
    of a short-K case whose error the algorithm, not the kernel, produces."""
    t = 4 if c.fam == 4 else 2
    a = t + 2
    W64 = conv_weight64(c, d)                                            # [cout][cin][3][3]
    if c.fam == 4:
        G = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
                          [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=torch.float64)
        U = torch.einsum("ai,ocij,bj->aboc", G, W64, G).float()
    else:
        G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
        U = torch.einsum("ai,ocij,bj->aboc", G, W64.float(), G)
    x = torch.nn.functional.pad(d["x"], (1, 1, 1, 1))
    # patches [a, a, n, cin, th, tw]: rows i, columns j of every tile's input patch
    P = x.unfold(2, a, t).unfold(3, a, t).permute(4, 5, 0, 1, 2, 3).contiguous()
    bt, at = (_bt6, _at6) if c.fam == 4 else (_bt4, _at4)
    if c.fam == 4:
        V = bt(bt(P.transpose(0, 1)).transpose(0, 1))                    # d B first, then B^T (d B), as wino4_kernel
    else:
        V = bt(bt(P).transpose(0, 1)).transpose(0, 1)                    # B^T d first, then (B^T d) B, as wino_kernel
    if d["s"] is not None:
        V = V * d["s"][None, None, :, :, None, None]
    M = torch.einsum("aboc,abnchw->abnohw", U, V)
    Y = at(at(M).transpose(0, 1)).transpose(0, 1)                         # [t, t, n, cout, th, tw]
    return Y.permute(2, 3, 4, 0, 5, 1).reshape(c.n, c.cout, c.h, c.w)
