"""Shared helpers of tests/test_gpu_irse_stages.py and tests/test_irse_cases_cpu.py: the case tables of the IR-SE50
executor's own kernels (csrc/irse.hip), one launch of a case, its fp64 CPU reference, and a bound for every output element.

Stage cases (STAGE_CASES) run the squeeze-and-excite launch pairs through smc_irse_se_fwd_f32 / smc_irse_se_bwd_f32, the
same host code the executor runs per unit.  Every output is compared with fp64 computed from the operands the device
itself read -- each link of the chain m -> h -> g -> out -> xbn and dg -> dr takes the device's value of the link before
(rounded fp32, widened exactly), so no bound has to carry another link's error and the ReLU kink of h (continuous) and
the h > 0 mask of the backward (read from the device's h, exact) cost nothing.

Bounds: K roundings x EPS = 2^-24 x B, B the same expression in fp64 with every operand replaced by its magnitude.  With
hw = oh ow, L(x) = ceil(x / 64) the additions one lane makes (the + 0 past the end is exact) and 6 the butterfly steps:
  m      K = L(hw) + 6 + 2 (1 / hw rounds, then the scale),              B = mean |r|
  dg     K = L(hw) + 6 + 1 (each product rounds before it is added),      B = sum |dout r|
  h      K = L(C) + 6 (at most 8 fma per lane),                           B = sum_c |w1| |m|;  relu is 1-Lipschitz
  g      t = sum_j w2 h: K_t = hid fma, B_t = sum_j |w2| |h|, e_t = K_t EPS B_t.  g = 1 / (1 + expf(-t)):
         |g - g64| <= g (1 - g) exp(e_t) e_t + g ((1 - g) EXPF_REL + 2 EPS)     (sigmoid' = g (1 - g) moves by at most
         exp(e_t) over e_t; expf's relative error reaches g through E / (1 + E) = 1 - g; the add and the divide round)
  out    K = 2,  B = |r g| + |shortcut|
  xbn    K = 2,  B = |out a| + |b|
  dr     dz = dg g (1 - g): 3 roundings;  dh = (h > 0) sum_c w2 dz: K_dh = 3 + L(C) + 6, B_dh = sum_c |w2| |dz|;
         dm = sum_j w1 dh / hw: K_dm = K_dh + hid + 2, B_dm = sum_j |w1| B_dh / hw;  dr = dout g + dm:
         (K_dm + 2) EPS B_dm + 2 EPS |dout g|
EXPF_REL is expf's own relative error.  The ROCm install carries no ULP table, so, as for RSQRT_REL of
tests/aux_cases.py, it is 2 x the largest error measured against fp64 on an MI355X over exact arguments
(expf_probe(): hid = 1, h = 1 exactly, t = w2 <= -8, where g = 1 / (1 + E) with E >= 2980 carries expf's error whole and
the add and the divide add at most 2 EPS, which the figure therefore includes;
tests/test_gpu_irse_stages.py::test_expf_error_is_within_the_recorded_figure re-measures it); DESIGN.md "IR-SE50 executor
stages" records the figure.

No-cancellation cases (nocancel): r, dout, w1 and w2 are >= 0, so every term of m, dg and of the h and dh dots is >= 0,
B equals the result and a dropped pixel, hidden row or channel is a fixed fraction of it.

Executor cases (NETS) run small networks of the Backbone's shape through irse_hip._Packed and smc_irse_forward_f32 /
smc_irse_backward_f32 / smc_irse_trunk_f32, with the small-plane Winograd switch on and off.  Forward: feat and every
saved segment (z; u1, r, h, g per unit; located by saved_layout(), a restatement of the executor's 64-float rounding)
against net_forward() in fp64.  Backward: dimg against net_backward() in fp64, a restatement of the executor's backward
that takes the masks (z >= 0, u1 >= 0, h > 0) and r, g, h from the device's own saved buffer: it is linear in dfeat and
has no kink.  The magnitude bound B across three or more convolutions is 600 .. 3600 x max |ref| and would hide an SE
mistake, so these cases take the reference's own fp32 error as the yardstick, both sides scaled by max |ref|:
  e_ref32 = error of the same restatement evaluated in fp32 torch on the CPU, against fp64;  e_hip <= MARGIN e_ref32,
MARGIN = 8 for every case (the MFMA kernels add the 9 cin products of a 3x3 conv in one sequential fp32 chain where the
CPU conv blocks the sum).

MUTATIONS lists the mistakes every case must be able to tell from rounding (tests/test_irse_cases_cpu.py): applied to
the reference, each moves some checked output of every case it applies to (applies()) by at least 8 x that output's
bound (for a net: POWER x MARGIN x e_ref32, in the forward and, where the mistake has a backward form, in dimg too).
The seeds in the tables were chosen until that held; the no-cancellation weights are scaled by the full fan-in and two
nets scale their SE weights (se_gain) for the same reason.  NET_WAIVED lists the one (net, mutation) pair for which no
inputs tried give power, with the stage case that tests that mistake at the same plane instead.
"""
import collections
import ctypes
import math

import torch
import torch.nn.functional as F
from torch import nn

DEV = "cuda"
EPS = 2.0 ** -24
MARGIN = 8.0
POWER = 8.0
# expf: 2 x the measured 9.885e-8 (1.66 x 2^-24, over 2048 arguments in -80 .. -8; module docstring)
EXPF_REL = 2 * 9.885e-8
KSE_CPB = 16        # channels per workgroup of the SE kernels (kSeCpb)
SE_MAXQ = 8

MUTATIONS = ("dm_dropped", "inv_hw", "last_pixel", "last_chunk", "last_hidden", "mask_ignored", "gate_block",
             "gate_sample", "sc_stride1", "sc_pitch", "xbn_bn", "pingpong")


def cdiv(a, b):
    return -(-a // b)


def zsplit(hw):
    """(workgroups per plane, pixels per workgroup) of the SE kernels (se_zsplit, `chunk`)."""
    z = max(1, cdiv(hw, 256))
    return z, cdiv(hw, z)


# ------------------------------------------------------------------------------------------------- stage cases

Stage = collections.namedtuple("Stage", "id C hid oh ow n short xbn nocancel seed forms")
STAGE_CASES = []


def _stage(cid, C, hid, oh, ow, n=1, short="conv", xbn=True, nocancel=False, seed=0, forms=""):
    STAGE_CASES.append(Stage(cid, C, hid, oh, ow, n, short, xbn, nocancel, seed, forms))


# short: "conv" (sc given), "id1" (x at stride 1), "id2" (x [2 oh][2 ow] read at stride 2).
# forms: what the case is for -- L = per-lane additions of plane_dot, z = pixel split, q = ceil(C / 64) C-dot terms per
# lane with or without a ragged last term, hid passes of the `j0 += 16` loop.
_stage("c16_h1_1x1", 16, 1, 1, 1, n=3, short="id1", xbn=False, seed=2,
       forms="hw 1: one live lane, one live thread; hid 1: rows 1..3 of the first pass clamped; C 16: one lane quarter")
_stage("c32_h3_7x7", 32, 3, 7, 7, n=1, seed=2, forms="hw 49 < 64: L = 1 with dead lanes; two channel blocks; n = 1")
_stage("c96_h16_3x5", 96, 16, 3, 5, n=3, short="id2", seed=0,
       forms="C 96: second lane term ragged (lane + 64 < 96); hid 16: one full pass; id2 at 6 x 10 (in_w != in_h)")
_stage("c160_h17_5x3", 160, 17, 5, 3, n=1, short="id2", xbn=False, seed=0,
       forms="C 160: three lane terms, the last ragged; hid 17: a second pass of one row; id2 at 10 x 6; no xbn")
_stage("c512_h33_15x17", 512, 33, 15, 17, n=1, short="id1", seed=0,
       forms="C 512 = 64 SE_MAXQ; hid 33: third pass; hw 255: L = 4, last lane short, z = 1 with one dead thread")
_stage("c32_h256_16x16", 32, 256, 16, 16, n=3, seed=0,
       forms="hid 256: the limit, 16 passes, every thread stores h; hw 256: z = 1, all threads live")
_stage("c16_h3_257x1", 16, 3, 257, 1, n=1, short="id1", xbn=False, seed=3,
       forms="hw 257: z = 2 of 129 + 128; ow 1; L = 5 with one lane at 5")
_stage("c32_h17_17x17", 32, 17, 17, 17, n=3, short="id2", seed=0,
       forms="hw 289: z = 2, 145 + 144; id2 at 34 x 34 across chunks")
_stage("c16_h16_16x32", 16, 16, 16, 32, n=1, seed=0, forms="hw 512: z = 2 of 256, the 8-deep load group exactly full")
_stage("c16_h1_19x27", 16, 1, 19, 27, n=3, short="id1", seed=3,
       forms="hw 513: z = 3 of 171; a second trip of the 8-deep load loop with one live load")
_stage("c32_h3_56x56", 32, 3, 56, 56, n=1, short="id2", seed=0,
       forms="hw 3136: the product's 13-way split of 242 (last chunk 232); id2 at 112 x 112")
_stage("c16_h3_128x128", 16, 3, 128, 128, n=1, seed=6, forms="hw 16384: the e4e planes, z = 64 of 256, L = 256")
_stage("nc_c96_h17_5x3", 96, 17, 5, 3, n=3, nocancel=True, seed=0,
       forms="no cancellation: a dropped channel of the ragged lane term or the 17th hidden row is a fixed fraction of B")
_stage("nc_c16_h33_19x27", 16, 33, 19, 27, n=1, short="id1", nocancel=True, seed=0,
       forms="no cancellation at hw 513: a dropped pixel is 1 / 513 of B")
_stage("nc_c32_h3_56x56", 32, 3, 56, 56, n=3, nocancel=True, xbn=False, seed=0,
       forms="no cancellation on the 13-way split, n = 3")
_stage("nc_c16_h1_128x128", 16, 1, 128, 128, n=1, nocancel=True, seed=0, forms="no cancellation at z = 64")

STAGE_BY_ID = {c.id: c for c in STAGE_CASES}
assert len(STAGE_BY_ID) == len(STAGE_CASES)


def stage_validate(n, C, hid, s, in_h, in_w):
    """se_validate of csrc/irse.hip: the message fragment of the first check that fails, None when the shape passes."""
    if n < 1:
        return "batch"
    if C < KSE_CPB or C % KSE_CPB:
        return "not a multiple of 16"
    if C > 64 * SE_MAXQ:
        return "> 512"
    if not 1 <= hid <= 256:
        return "SE hidden width"
    if s not in (1, 2):
        return "stride"
    if in_h < s or in_w < s or in_h % s or in_w % s:
        return "odd size"
    if (in_h // s) * (in_w // s) * n * C >= 2 ** 31:
        return "2^31"
    return None


def stage_geometry(c):
    s = 2 if c.short == "id2" else 1
    return s, s * c.oh, s * c.ow


def stage_inputs(c):
    """fp32 CPU operands of a stage case (forward and backward)."""
    gen = torch.Generator().manual_seed(1000 + c.seed)
    s, in_h, in_w = stage_geometry(c)

    def rn(*shape):
        return torch.randn(*shape, generator=gen)

    pos = (lambda t: t.abs()) if c.nocancel else (lambda t: t)
    # (all-positive weights scaled by the full fan-in, or the gate saturates at 1 and g (1 - g) vanishes)
    s1, s2 = (1.0 / c.C, 1.0 / c.hid) if c.nocancel else (c.C ** -0.5, 2.0 * c.hid ** -0.5)
    I = dict(r=pos(rn(c.n, c.C, c.oh, c.ow)), w1=pos(rn(c.hid, c.C)) * s1, w2=pos(rn(c.C, c.hid)) * s2,
             dout=pos(rn(c.n, c.C, c.oh, c.ow)),
             a=torch.rand(c.C, generator=gen) + 0.5, b=rn(c.C))
    I["sc" if c.short == "conv" else "x"] = rn(c.n, c.C, in_h, in_w)
    return I


def _sub(x, s, oh, ow, mut):
    """The identity shortcut's read x[s y][s x] (MaxPool2d(1, s)), and two ways to get its index wrong."""
    if mut == "sc_stride1":
        return x[:, :, :oh, :ow]
    if mut == "sc_pitch":        # row pitch ow in place of in_w
        yy, xx = torch.meshgrid(torch.arange(oh), torch.arange(ow), indexing="ij")
        return x.flatten(2)[:, :, (s * yy * ow + s * xx).flatten()].reshape(x.shape[0], x.shape[1], oh, ow)
    return x[:, :, ::s, ::s]


def _zero_last_chunk(t):
    hw = t.shape[2] * t.shape[3]
    z, chunk = zsplit(hw)
    t = t.clone()
    t.flatten(2)[:, :, (z - 1) * chunk:] = 0
    return t


def _mut_gate(g, mut):
    if mut == "gate_block":
        g = g.clone()
        g[:, -KSE_CPB:] = g[:, :KSE_CPB]
    if mut == "gate_sample":
        g = g.clone()
        g[1] = g[0]
    return g


def stage_fwd_ref(c, I, dev=None, mut=None):
    """{name: (fp64 reference, bound)} of m, h, g, out (and xbn).  dev: the device's outputs (fp32 CPU tensors) that
    the later links are computed from; None: this function's own, rounded to fp32."""
    s, in_h, in_w = stage_geometry(c)
    hw = c.oh * c.ow
    r, w1, w2 = I["r"].double(), I["w1"].double(), I["w2"].double()
    out = {}

    def link(name, val):
        return (dev[name] if dev is not None else val.float()).double()

    rr = r.flatten(2)
    if mut == "last_pixel":
        rr = rr.clone()
        rr[:, :, -1] = 0
    m = rr.sum(-1) / (hw + 1 if mut == "inv_hw" else hw)
    out["m"] = (m, (cdiv(hw, 64) + 8) * EPS * r.flatten(2).abs().sum(-1) / hw)
    md = link("m", m)
    h = torch.relu(md @ w1.t())
    if mut == "last_hidden":
        h = h.clone()
        h[:, -1] = 0
    out["h"] = (h, (cdiv(c.C, 64) + 6) * EPS * (md.abs() @ w1.abs().t()))
    hd = link("h", h)
    g = torch.sigmoid(hd @ w2.t())
    et = c.hid * EPS * (hd.abs() @ w2.abs().t())
    out["g"] = (g, g * (1 - g) * torch.exp(et) * et + g * ((1 - g) * EXPF_REL + 2 * EPS))
    gd = _mut_gate(link("g", g), mut)[:, :, None, None]
    short = I["sc"].double() if c.short == "conv" else _sub(I["x"].double(), s, c.oh, c.ow, mut)
    o = r * gd + short
    if mut == "last_chunk":
        o = _zero_last_chunk(o)
    out["out"] = (o, 2 * EPS * ((r * gd).abs() + short.abs()))
    if c.xbn:
        od = link("out", o)
        a, b = I["a"].double()[None, :, None, None], I["b"].double()[None, :, None, None]
        out["xbn"] = (od * a + b, 2 * EPS * ((od * a).abs() + b.abs()))
    return out


def stage_bwd_ref(c, I, fwd, dev=None, mut=None):
    """{name: (fp64 reference, bound)} of dg, dr from dout and the forward's r, g, h (fwd: fp32 CPU tensors)."""
    hw = c.oh * c.ow
    dout, r, w1, w2 = I["dout"].double(), I["r"].double(), I["w1"].double(), I["w2"].double()
    g, h = fwd["g"].double(), fwd["h"].double()
    out = {}
    prod = (dout * r).flatten(2)
    pm = prod
    if mut == "last_pixel":
        pm = prod.clone()
        pm[:, :, -1] = 0
    dg = pm.sum(-1)
    out["dg"] = (dg, (cdiv(hw, 64) + 7) * EPS * prod.abs().sum(-1))
    dgd = (dev["dg"] if dev is not None else dg.float()).double()
    dz = dgd * g * (1 - g)
    mask = torch.ones_like(h) if mut == "mask_ignored" else (h > 0).double()
    dh = (dz @ w2) * mask
    b_dh = (dz.abs() @ w2.abs()) * mask
    if mut == "last_hidden":
        dh = dh.clone()
        dh[:, -1] = 0
    k_dh = 3 + cdiv(c.C, 64) + 6
    dm = dh @ w1 / (hw + 1 if mut == "inv_hw" else hw)
    if mut == "dm_dropped":
        dm = torch.zeros_like(dm)
    b_dm = b_dh @ w1.abs() / hw
    gm = _mut_gate(g, mut)[:, :, None, None]
    dr = dout * gm + dm[:, :, None, None]
    if mut == "last_chunk":
        dr = _zero_last_chunk(dr)
    bound = ((k_dh + c.hid + 2 + 2) * EPS * b_dm)[:, :, None, None] + 2 * EPS * (dout * gm).abs()
    out["dr"] = (dr, bound.expand_as(dr))
    return out


def stage_applies(c, mut):
    """Whether a mutation names something a stage case has (a second channel block, a second sample, ...)."""
    return {"dm_dropped": True, "inv_hw": True, "last_pixel": True, "last_chunk": True, "last_hidden": True,
            "mask_ignored": not c.nocancel, "gate_block": c.C >= 2 * KSE_CPB, "gate_sample": c.n >= 2,
            "sc_stride1": c.short == "id2", "sc_pitch": c.short == "id2", "xbn_bn": False, "pingpong": False}[mut]


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def run_stage_fwd(c, I):
    """One smc_irse_se_fwd_f32 launch pair into NaN-filled outputs; {name: fp32 CPU tensor}."""
    from stylemc_amd import _hip
    s, in_h, in_w = stage_geometry(c)
    d = {k: v.to(DEV).contiguous() for k, v in I.items()}
    o = dict(out=_nan(c.n, c.C, c.oh, c.ow), h=_nan(c.n, c.hid), g=_nan(c.n, c.C), m=_nan(c.n, c.C))
    if c.xbn:
        o["xbn"] = _nan(c.n, c.C, c.oh, c.ow)
    _hip.call("smc_irse_se_fwd_f32", d["r"].data_ptr(), _hip.ptr(d.get("sc")), _hip.ptr(d.get("x")), s, in_h, in_w,
              c.n, c.C, d["w1"].data_ptr(), d["w2"].data_ptr(), c.hid, d["a"].data_ptr() if c.xbn else None,
              d["b"].data_ptr() if c.xbn else None, o["out"].data_ptr(), _hip.ptr(o.get("xbn")), o["h"].data_ptr(),
              o["g"].data_ptr(), o["m"].data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def run_stage_bwd(c, I, fwd):
    from stylemc_amd import _hip
    d = {k: I[k].to(DEV).contiguous() for k in ("dout", "r", "w1", "w2")}
    g, h = fwd["g"].to(DEV), fwd["h"].to(DEV)
    o = dict(dg=_nan(c.n, c.C), dr=_nan(c.n, c.C, c.oh, c.ow))
    _hip.call("smc_irse_se_bwd_f32", d["dout"].data_ptr(), d["r"].data_ptr(), g.data_ptr(), h.data_ptr(),
              d["w1"].data_ptr(), d["w2"].data_ptr(), c.n, c.C, c.hid, c.oh, c.ow, o["dg"].data_ptr(),
              o["dr"].data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def expf_probe():
    """(case, operands, t) of the expf measurement: C = 16, hid = 1, r = 1 on 8 x 8 planes and w1 = e_0, so m = h = 1
    exactly and t = w2 exactly; n = 1, 16 arguments per launch, `rows` launches."""
    c = Stage("expf_probe", 16, 1, 8, 8, 1, "conv", False, False, 0, "")
    I = dict(r=torch.ones(1, 16, 8, 8), w1=torch.zeros(1, 16), sc=torch.zeros(1, 16, 8, 8), dout=torch.zeros(1, 16, 8, 8),
             a=torch.ones(16), b=torch.zeros(16))
    I["w1"][0, 0] = 1.0
    gen = torch.Generator().manual_seed(7)
    t = -(8 + 72 * torch.rand(128, 16, generator=gen))        # expf(-t) in e^8 .. e^80, all finite, normal results
    return c, I, t.float()


# ------------------------------------------------------------------------------------------------ executor cases

Net = collections.namedtuple("Net", "id units hw n seed se_gain forms")
NETS = []


def _net(nid, units, hw, n=2, seed=0, se_gain=1.0, forms=""):
    NETS.append(Net(nid, tuple(units), hw, n, seed, se_gain, forms))


# units: (cin, depth, stride, SE hidden width); the stem is 3 -> units[0].cin, the output layer flat -> 32.  Weights are
# synthetic.seeded_state_dict(seed) with both SE layers scaled by se_gain: at 1 the gate of a plane of 289 or more pixels
# barely moves with its input and the SE backward is too small a share of dimg for the power condition.
_net("u1_16_32_s2_12", [(16, 32, 2, 4)], 12,
     forms="conv shortcut; c1_fwd eligible for small-plane Winograd, its adjoint (32 -> 16) not")
_net("u1_32_32_s1_7_h5", [(32, 32, 1, 5)], 7, seed=3, forms="identity shortcut at stride 1, odd plane, hid 5")
_net("u1_32_32_s2_34_h3", [(32, 32, 2, 3)], 34, seed=2, se_gain=4.0, forms="subsampled identity shortcut, ohw 289 (two ragged chunks), hid 3")
_net("u2_16_96_160_8", [(16, 96, 2, 17), (96, 160, 1, 33)], 8, forms="C 96 and 160, hid 17 and 33; xbn between units")
_net("u1_16_512_s2_4", [(16, 512, 2, 32)], 4, forms="C 512: the SE_MAXQ limit")
_net("u1_16_32_s2_2", [(16, 32, 2, 4)], 2, forms="2 x 2 -> 1 x 1: one-pixel planes")
_net("u1_16_32_s2_112", [(16, 32, 2, 4)], 112, n=1, seed=2, se_gain=4.0, forms="the product's 13-way split (56 x 56)")
_net("u4_24", [(16, 32, 2, 4), (32, 32, 1, 4), (32, 64, 2, 8), (64, 64, 1, 8)], 24, n=3,
     forms="xa / xb ping-pong, the xbn chain, n_saved 3 with n 1..3, trunk taps (0, 1, 3), (1,), (3,)")
NET_BY_ID = {c.id: c for c in NETS}
# (net, mutation) pairs no choice of inputs gives power: the reason, and the stage case that is the test of it instead
NET_WAIVED = {
    ("u1_16_32_s2_112", "inv_hw"): ("1 / 3137 for 1 / 3136 moves dm, itself a few percent of dimg, by 3e-4 of itself: at most 10 "
                                    "e_ref32 over seeds 0..9 and se_gain 1, 4, 16 where 64 is asked; in the forward the same "
                                    "mistake moves h by thousands of e_ref32", "nc_c32_h3_56x56"),
}
U4_TAPS = ((0, 1, 3), (1,), (3,))
FEAT = 32


class SmallNet(nn.Module):
    """input_layer / body / output_layer of the Backbone's shape over a free list of units."""

    def __init__(self, units, in_hw, feat=FEAT):
        super().__init__()
        from stylemc_amd.id_loss import model_irse as M
        stem = units[0][0]
        self.input_layer = nn.Sequential(nn.Conv2d(3, stem, (3, 3), 1, 1, bias=False), nn.BatchNorm2d(stem),
                                         M.PReLU(stem))
        blocks, hw = [], in_hw
        for cin, depth, s, hid in units:
            blk = M.BottleneckIRSE(cin, depth, s)
            se = M.SEModule(depth, 1)
            se.fc1 = nn.Conv2d(depth, hid, kernel_size=1, bias=False)
            se.fc2 = nn.Conv2d(hid, depth, kernel_size=1, bias=False)
            blk.res_layer[5] = se
            blocks.append(blk)
            hw //= s
        self.body = nn.Sequential(*blocks)
        d = units[-1][1]
        self.output_layer = nn.Sequential(nn.BatchNorm2d(d), nn.Dropout(0.4), M._Flatten(),
                                          nn.Linear(d * hw * hw, feat), nn.BatchNorm1d(feat))

    def forward(self, x):
        return self.output_layer(self.body(self.input_layer(x)))


def build_net(c):
    from stylemc_amd import synthetic
    net = SmallNet(c.units, c.hw)
    net.load_state_dict(synthetic.seeded_state_dict(net, seed=c.seed))
    net = net.eval().requires_grad_(False)
    for blk in net.body:
        blk.res_layer[5].fc1.weight.mul_(c.se_gain)
        blk.res_layer[5].fc2.weight.mul_(c.se_gain)
    return net


def net_inputs(c):
    gen = torch.Generator().manual_seed(2000 + c.seed)
    return torch.randn(c.n, 3, c.hw, c.hw, generator=gen), torch.randn(c.n, FEAT, generator=gen)


def net_params(mod, dtype):
    """The network as the executor sees it (BatchNorms as fp64 (a, b), the output layer folded in fp64), cast to dtype."""
    from stylemc_amd.irse_hip import bn_affine

    def c(t):
        return t.detach().double().cpu().to(dtype)

    def aff(bn):
        a, b = bn_affine(bn)
        return c(a)[None, :, None, None], c(b)[None, :, None, None]

    conv, bn, pr = mod.input_layer[0], mod.input_layer[1], mod.input_layer[2]
    P = dict(stem=dict(W=c(conv.weight), ab=aff(bn), alpha=c(pr.weight)[None, :, None, None]), units=[])
    for blk in mod.body:
        res = blk.res_layer
        u = dict(ab1=aff(res[0]), W1=c(res[1].weight), alpha=c(res[2].weight)[None, :, None, None], W2=c(res[3].weight),
                 s=res[3].stride[0], ab2=aff(res[4]), w1=c(res[5].fc1.weight).flatten(1), w2=c(res[5].fc2.weight).flatten(1),
                 sc=None)
        if isinstance(blk.shortcut_layer, nn.Sequential):
            u["sc"] = (c(blk.shortcut_layer[0].weight), aff(blk.shortcut_layer[1]))
        P["units"].append(u)
    if hasattr(mod, "output_layer"):
        bno, fc, bnf = mod.output_layer[0], mod.output_layer[3], mod.output_layer[4]
        ao, bo = bn_affine(bno)
        af, bf = bn_affine(bnf)
        Wl = fc.weight.detach().double().cpu()
        rep = Wl.shape[1] // ao.numel()
        P["Wf"] = (Wl * ao.repeat_interleave(rep)[None, :] * af[:, None]).to(dtype)
        P["fb"] = ((fc.bias.detach().double().cpu() + Wl @ bo.repeat_interleave(rep)) * af + bf).to(dtype)
    return P


def _prelu(z, alpha):
    return torch.where(z >= 0, z, z * alpha)


def net_forward(P, x, mut=None):
    """Restated forward in the dtype of P: (feat, z, [per unit dict(u1, r, h, g, out)])."""
    x = x.to(P["stem"]["W"].dtype)
    a, b = P["stem"]["ab"]
    z = F.conv2d(x, P["stem"]["W"], padding=1) * a + b
    cur = _prelu(z, P["stem"]["alpha"])
    S = []
    for k, u in enumerate(P["units"]):
        a1, b1 = u["ab1"]
        if mut == "xbn_bn" and k >= 1 and P["units"][k - 1]["ab1"][0].shape == a1.shape:
            a1, b1 = P["units"][k - 1]["ab1"]          # the combine of unit k - 1 took its own BN1
        u1 = F.conv2d(cur * a1 + b1, u["W1"], padding=1)
        a2, b2 = u["ab2"]
        r = F.conv2d(_prelu(u1, u["alpha"]), u["W2"], stride=u["s"], padding=1) * a2 + b2
        oh, ow = r.shape[2:]
        hw = oh * ow
        rr = r.flatten(2)
        if mut == "last_pixel":
            rr = rr.clone()
            rr[:, :, -1] = 0
        m = rr.sum(-1) / (hw + 1 if mut == "inv_hw" else hw)
        h = torch.relu(m @ u["w1"].t())
        if mut == "last_hidden":
            h = h.clone()
            h[:, -1] = 0
        g = torch.sigmoid(h @ u["w2"].t())
        xs = cur
        if mut == "pingpong" and k >= 2 and S[k - 2]["out"].numel() == cur.numel():
            xs = S[k - 2]["out"].reshape(cur.shape)    # the buffer still holds unit k - 2's output
        if u["sc"] is not None:
            Ws, (sa, sb) = u["sc"]
            short = F.conv2d(xs, Ws, stride=u["s"]) * sa + sb
        else:
            short = _sub(xs, u["s"], oh, ow, mut)
        gm = g if x.shape[0] < 2 and mut == "gate_sample" else _mut_gate(g, mut)
        out = r * gm[:, :, None, None] + short
        if mut == "last_chunk":
            out = _zero_last_chunk(out)
        S.append(dict(u1=u1, r=r, h=h, g=g, out=out))
        cur = out
    feat = cur.flatten(1) @ P["Wf"].t() + P["fb"] if "Wf" in P else None
    return feat, z, S


def net_backward(P, z, S, dfeat, mut=None):
    """Restated backward in the dtype of P over the unit list: dimg from dfeat, the masks z >= 0, u1 >= 0, h > 0 and
    r, g, h of S (the device's saved buffer, or a reference's own activations).  Linear in dfeat; no kink."""
    dt = P["stem"]["W"].dtype
    n = dfeat.shape[0]
    last = S[-1]["r"]
    dx = (dfeat.to(dt) @ P["Wf"]).reshape(n, *last.shape[1:])
    for k in range(len(S) - 1, -1, -1):
        u, sv = P["units"][k], S[k]
        r, g, h, u1 = (sv[key][:n].to(dt) for key in ("r", "g", "h", "u1"))
        s = u["s"]
        hw = r.shape[2] * r.shape[3]
        dout = dx
        prod = (dout * r).flatten(2)
        if mut == "last_pixel":
            prod = prod.clone()
            prod[:, :, -1] = 0
        dz = prod.sum(-1) * g * (1 - g)
        dh = dz @ u["w2"]
        if mut != "mask_ignored":
            dh = dh * (h > 0).to(dt)
        if mut == "last_hidden":
            dh = dh.clone()
            dh[:, -1] = 0
        dm = dh @ u["w1"] / (hw + 1 if mut == "inv_hw" else hw)
        if mut == "dm_dropped":
            dm = torch.zeros_like(dm)
        gm = g if n < 2 and mut == "gate_sample" else _mut_gate(g, mut)
        dr = dout * gm[:, :, None, None] + dm[:, :, None, None]
        if mut == "last_chunk":
            dr = _zero_last_chunk(dr)
        dy1 = F.conv_transpose2d(dr * u["ab2"][0], u["W2"], stride=s, padding=1, output_padding=s - 1)
        du1 = dy1 * torch.where(u1 >= 0, torch.ones_like(u1), u["alpha"].expand_as(u1))
        dxk = F.conv_transpose2d(du1, u["W1"], padding=1) * u["ab1"][0]
        if u["sc"] is not None:
            Ws, (sa, _) = u["sc"]
            dxk = dxk + F.conv_transpose2d(dout * sa, Ws, stride=s, output_padding=s - 1)
        else:
            dxk = dxk.clone()
            dxk[:, :, ::s, ::s] += dout
        dx = dxk
    zz = z[:n].to(dt)
    dy0 = dx * torch.where(zz >= 0, torch.ones_like(zz), P["stem"]["alpha"].expand_as(zz))
    return F.conv_transpose2d(dy0 * P["stem"]["ab"][0], P["stem"]["W"], padding=1)


FWD_MUTS = ("inv_hw", "last_pixel", "last_chunk", "last_hidden", "gate_block", "gate_sample", "sc_stride1", "sc_pitch",
            "xbn_bn", "pingpong")
BWD_MUTS = ("dm_dropped", "inv_hw", "last_pixel", "last_chunk", "last_hidden", "mask_ignored", "gate_block",
            "gate_sample")


def net_applies(c, mut):
    ident2 = any(ci == d and s == 2 for ci, d, s, _ in c.units)
    return {"dm_dropped": True, "inv_hw": True, "last_pixel": True, "last_chunk": True, "last_hidden": True,
            "mask_ignored": True, "gate_block": True, "gate_sample": c.n >= 2, "sc_stride1": ident2, "sc_pitch": ident2,
            "xbn_bn": any(c.units[k - 1][0] == c.units[k][0] for k in range(1, len(c.units))),
            "pingpong": len(c.units) >= 3}[mut]


def rnd64(k):
    return (k + 63) & ~63


def saved_layout(c, n):
    """Offsets of the saved segments for n faces (saved_floats of csrc/irse.hip: each segment rounded up to 64 floats):
    ({'z': (off, shape)}, [per unit {'u1' | 'r' | 'h' | 'g': (off, shape)}], total floats)."""
    off = 0

    def seg(*shape):
        nonlocal off
        o = off
        off += rnd64(math.prod(shape))
        return o, shape

    hw = c.hw
    z = seg(n, c.units[0][0], hw, hw)
    per = []
    for cin, depth, s, hid in c.units:
        d = dict(u1=seg(n, depth, hw, hw))
        hw //= s
        d["r"] = seg(n, depth, hw, hw)
        d["h"] = seg(n, hid)
        d["g"] = seg(n, depth)
        per.append(d)
    return dict(z=z), per, off


def split_saved(c, n, saved):
    """(z, [per unit dict(u1, r, h, g)]) views of a flat saved buffer (CPU tensor)."""
    zl, per, total = saved_layout(c, n)
    assert saved.numel() == total, (saved.numel(), total)

    def view(o_shape):
        o, shape = o_shape
        return saved[o:o + math.prod(shape)].reshape(shape)

    return view(zl["z"]), [{k: view(v) for k, v in d.items()} for d in per]


def rel_err(a, ref):
    """max |a - ref| / max |ref|; NaN (an unwritten element) counts as infinite."""
    a, ref = a.double(), ref.double()
    e = (a - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)
    return float("inf") if math.isnan(e) else e


def run_net(c, mod, x, dfeat, wino_sp, n_grads=None, taps=()):
    """The network on the device: feat, the saved buffer, dimg for each n of n_grads, and the trunk's tap outputs
    for each tap tuple -- all into NaN-filled buffers, all returned as CPU tensors."""
    from stylemc_amd import _hip, irse_hip
    old = irse_hip.WINO_SP
    irse_hip.WINO_SP = wino_sp
    try:
        pk = irse_hip._Packed(mod, DEV, c.hw)
    finally:
        irse_hip.WINO_SP = old
    lib = _hip.load()
    net = ctypes.byref(pk.net)
    n = x.shape[0]
    xd = x.to(DEV).contiguous()
    feat = _nan(n, pk.net.feat)
    nsv = lib.smc_irse_saved_floats(net, n)
    assert nsv == saved_layout(c, n)[2], (nsv, saved_layout(c, n)[2])
    saved = _nan(nsv)
    wsb = lib.smc_irse_workspace_bytes(net, n)
    ws = _nan(wsb // 4)
    _hip.call("smc_irse_forward_f32", net, xd.data_ptr(), n, feat.data_ptr(), saved.data_ptr(), ws.data_ptr(), wsb,
              _hip.stream())
    res = dict(feat=feat.cpu(), saved=saved.cpu(), dimg={}, taps={})
    for ng in n_grads or (n,):
        dimg = _nan(ng, 3, c.hw, c.hw)
        wsb = lib.smc_irse_workspace_bytes(net, ng)
        ws = _nan(wsb // 4)
        df = dfeat[:ng].to(DEV).contiguous()
        _hip.call("smc_irse_backward_f32", net, df.data_ptr(), n, ng, saved.data_ptr(), dimg.data_ptr(), ws.data_ptr(),
                  wsb, _hip.stream())
        res["dimg"][ng] = dimg.cpu()
    for tp in taps:
        hw, shapes = c.hw, []
        for cin, depth, s, hid in c.units:
            hw //= s
            shapes.append((n, depth, hw, hw))
        outs = [_nan(*shapes[k]) for k in tp]
        wsb = lib.smc_irse_trunk_workspace_bytes(net, n)
        ws = _nan(wsb // 4)
        tu = (ctypes.c_int * len(tp))(*tp)
        to = (ctypes.c_void_p * len(tp))(*[o.data_ptr() for o in outs])
        _hip.call("smc_irse_trunk_f32", net, xd.data_ptr(), n, tu, to, len(tp), ws.data_ptr(), wsb, _hip.stream())
        res["taps"][tp] = [o.cpu() for o in outs]
    torch.cuda.synchronize()
    return res
