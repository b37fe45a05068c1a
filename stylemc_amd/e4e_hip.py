"""e4e / pSp real-image inversion (image -> W+) on the gfx950 kernel library.

Drop-in for the reference's ``Encoder4Editing`` / ``GradualStyleEncoder`` (encoder4editing/models/encoders/
psp_encoders.py:58-200) as ``pSp.forward`` runs them at inference (models/psp.py:57-68): same state_dict, eval mode,
frozen, fp32, square inputs (256 x 256 is the workload).  Forward:

  trunk    smc_irse_trunk_f32: the IR-SE50 stem + body of the native executor (irse_hip._Packed without the output
           layer) with the outputs of units 6 / 20 / 23 tapped (c1, c2, c3)
  FPN      latlayer{1,2} as 1-tap smc_conv_gemm_f32 calls with a bias epilogue, then smc_upsample_add_f32 (p2, p1)
  heads    the 18 GradualStyleBlocks, family by family (coarse on c3, middle on p2, fine on p1): level l of every
           head of a family is one smc_conv_s2_grouped_f32 launch (level 0 with group stride 0: all heads read the
           same feature map); the taps that only touch padding at a level's plane size are dropped when packing
  linear   the 18 EqualLinears as one grouped 1-tap launch with alpha = 1 (scale and lr_mul folded on the host)
  W+       w0 + deltas (e4e) or the stacked rows (pSp), + latent_avg when given (psp.py:62-68)

``GROUPED = False`` runs the heads as per-conv calls of the existing entry points instead (smc_conv_gemm_f32 with a
bias + lrelu SMC_EPI_MODACT epilogue, smc_linear_f32) on the same packed weights: the A/B baseline of
tools/bench_e4e.py and a second implementation for the tests.
"""
import ctypes

import torch
from torch import nn

from . import _hip, modconv
from .encoder4editing.models.encoders.psp_encoders import ENCODERS, TAP_UNITS
from .irse_hip import _Packed

# Heads through the grouped kernel (csrc/e4e.hip); False: composed from smc_conv_gemm_f32 / smc_linear_f32 calls.
GROUPED = True
# First fine level (11 heads on the same p1, M = n * 32 * 32 at 256 px: the one compute-bound level) as one
# smc_conv_gemm_f32 call with the heads' weights concatenated to cout = 11 * 512 instead of the grouped kernel; the
# next level then reads its channel slices through the strides.  On by measurement (DESIGN.md section 11,
# profiles/e4e/: 554 us against 845 us for that level at one photograph, 1.92 against 2.51 ms at four).
FINE0_GEMM = True
LRELU_ALPHA = 0.01  # nn.LeakyReLU() default (psp_encoders.py:42,46)


def live_taps(h, w):
    """Taps ky*3 + kx of a 3x3 stride-2 pad-1 conv that touch the h x w plane for at least one output position."""
    def live(size):
        out = (size - 1) // 2 + 1
        return [k for k in range(3) if any(0 <= 2 * a - 1 + k < size for a in range(out))]
    return [ky * 3 + kx for ky in live(h) for kx in live(w)]


def out_size(h):
    return (h - 1) // 2 + 1


def pack_taps(weights, taps, device):
    """[G][len(taps)][cin][cout] fp32 from G conv weights [cout][cin][3][3], head by head (a permutation: exact)."""
    cout, cin = weights[0].shape[:2]
    out = torch.empty(len(weights), len(taps), cin, cout, device=device, dtype=torch.float32)
    for g, W in enumerate(weights):
        W = W.detach().to(device, torch.float32).reshape(cout, cin, 9)
        out[g] = W[:, :, taps].permute(2, 1, 0)
    return out


class _Level:
    """One level of a head family: G convs on h x w planes."""

    def __init__(self, convs, h, device, concat=False):
        self.h = h
        self.oh = out_size(h)
        self.taps = live_taps(h, h)
        self.taps_c = (ctypes.c_int * len(self.taps))(*self.taps)
        self.groups = len(convs)
        self.cout, self.cin = convs[0].weight.shape[:2]
        self.wk = pack_taps([c.weight for c in convs], self.taps, device)
        self.bias = torch.stack([c.bias.detach().to(device, torch.float32) for c in convs]).contiguous()
        # composed path: one gather-GEMM phase per head on its slice of the same packed weights
        offs = [(t // 3 - 1, t % 3 - 1) for t in self.taps]
        self.phases = [(_hip.ConvPhase * 1)(modconv._phase(offs, 2, self.oh, self.oh, 0, 0, 1, 1, self.wk[g]))
                       for g in range(self.groups)]
        self.wk_cat = self.bias_cat = self.phase_cat = None
        if concat:  # [tap][cin][G * cout] for the one-call form of the first fine level
            self.wk_cat = self.wk.permute(1, 2, 0, 3).reshape(len(self.taps), self.cin, -1).contiguous()
            self.bias_cat = self.bias.reshape(-1)
            self.phase_cat = (_hip.ConvPhase * 1)(modconv._phase(offs, 2, self.oh, self.oh, 0, 0, 1, 1, self.wk_cat))
            self.wk = None  # (the grouped copy is not kept beside it)
            self.phases = None


class _PackedE4E:
    """Packed trunk, laterals and heads of one encoder for one input size."""

    def __init__(self, enc, device, in_hw, trunk):
        dev = torch.device(device)
        self.in_hw = in_hw
        self.grouped, self.fine0_gemm = GROUPED, FINE0_GEMM
        self.trunk = trunk
        sizes = []
        hw = in_hw
        for k, unit in enumerate(enc.body):
            hw //= unit.res_layer[3].stride[0]
            if k in TAP_UNITS:
                sizes.append((unit.res_layer[3].weight.shape[0], hw))
        self.tap_shapes = sizes  # (channels, size) of c1, c2, c3
        self.tap_units = (ctypes.c_int * 3)(*TAP_UNITS)

        def lateral(conv):
            wk = conv.weight.detach().to(dev, torch.float32)[:, :, 0, 0].t().contiguous().unsqueeze(0)
            return wk, conv.bias.detach().to(dev, torch.float32).contiguous()

        self.lat1, self.lat2 = lateral(enc.latlayer1), lateral(enc.latlayer2)
        (_, s1), (_, s2), (_, s3) = sizes
        bounds = [(0, enc.coarse_ind, s3), (enc.coarse_ind, enc.middle_ind, s2), (enc.middle_ind, enc.style_count, s1)]
        self.families = []
        for fi, (lo, hi, size) in enumerate(bounds):
            heads = [enc.styles[j] for j in range(lo, hi)]
            nconv = len(heads[0].convs) // 2
            levels, h = [], size
            for l in range(nconv):
                concat = self.grouped and self.fine0_gemm and fi == 2 and l == 0 and nconv > 1
                levels.append(_Level([hd.convs[2 * l] for hd in heads], h, dev, concat))
                h = out_size(h)
            if h != 1:
                raise ValueError(f"HipE4E: a {in_hw}-px input leaves {h}x{h} planes at the heads' linear layers")
            self.families.append((lo, hi, levels))
        # the EqualLinears as 1-tap 'convs' on 1x1 planes: weight * scale and bias * lr_mul folded (stylegan2/model.py:
        # 144-155), [18][1][cin][cout]
        lin = [s.linear for s in enc.styles]
        self.lin_wk = torch.stack([(l.weight.detach().to(dev, torch.float32) * l.scale).t() for l in lin]) \
            .unsqueeze(1).contiguous()
        self.lin_bias = torch.stack([l.bias.detach().to(dev, torch.float32) * l.lr_mul for l in lin]).contiguous()
        self.lin_taps = (ctypes.c_int * 1)(4)
        if dev.type == "cuda":
            torch.cuda.current_stream(dev).synchronize()


def grouped_conv(x, sample_stride, group_stride, groups, n, cin, h, w, wk, taps_c, bias, alpha, y, cout):
    """One smc_conv_s2_grouped_f32 launch (x: any tensor whose storage holds the strided blocks, y [G][n][cout][oh][ow])."""
    lib = _hip.load()
    nt = len(taps_c)
    wsb = lib.smc_conv_s2_grouped_workspace_size(groups, n, cin, cout, h, w, nt)
    if wsb < 0:
        raise RuntimeError(f"smc_conv_s2_grouped_f32 has no kernel for G {groups} n {n} {cin}->{cout} {h}x{w}")
    ws = torch.empty(wsb // 4, device=y.device, dtype=torch.float32) if wsb > 0 else None
    _hip.call("smc_conv_s2_grouped_f32", _hip.ptr(x), sample_stride, group_stride, groups, n, cin, h, w, _hip.ptr(wk),
              taps_c, nt, _hip.ptr(bias), float(alpha), _hip.ptr(y), cout, _hip.ptr(ws), wsb, _hip.stream())


def upsample_add(x, lat):
    """bilinear(x -> lat's size, align_corners) + lat (helpers.py:123-140) in one launch."""
    x, lat = x.contiguous(), lat.contiguous()
    n, c, ih, iw = x.shape
    y = torch.empty_like(lat)
    _hip.call("smc_upsample_add_f32", _hip.ptr(x), n * c, ih, iw, _hip.ptr(lat), _hip.ptr(y), lat.shape[2],
              lat.shape[3], _hip.stream())
    return y


def _bias_epi(bias, act="linear", alpha=0.0):
    return modconv._epilogue(_hip.EPI_MODACT, bias=bias, act=act, alpha=alpha)


class HipE4E(nn.Module):
    """Encoder4Editing / GradualStyleEncoder (state_dict-compatible with the reference) on the gfx950 kernels."""

    def __init__(self, encoder_type="Encoder4Editing", num_layers=50, mode="ir_se", stylegan_size=1024):
        super().__init__()
        if encoder_type not in ENCODERS:
            raise ValueError(f"{encoder_type} is not a valid encoder (psp.py:30-39); have {sorted(ENCODERS)}")
        self.encoder = ENCODERS[encoder_type](num_layers, mode, stylegan_size)
        self.encoder_type = encoder_type
        self.latent_avg = None  # [style_count, 512] when the checkpoint starts from the average latent
        self._packed = None
        self._trunks = {}       # input size -> packed trunk (kept across the GROUPED / FINE0_GEMM switches)

    def state_dict(self, *args, **kwargs):
        return self.encoder.state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        r = self.encoder.load_state_dict(state_dict, strict=strict, assign=assign)
        self._packed, self._trunks = None, {}
        return r

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        if self.latent_avg is not None:
            self.latent_avg = fn(self.latent_avg)
        self._packed, self._trunks = None, {}
        return self

    def packed(self, in_hw):
        pk = self._packed
        if pk is None or pk.in_hw != in_hw or (pk.grouped, pk.fine0_gemm) != (GROUPED, FINE0_GEMM):
            self._packed = None  # (release the previous size's 0.9 GB before packing the next)
            dev = next(self.encoder.parameters()).device
            if in_hw not in self._trunks:
                self._trunks[in_hw] = _Packed(self.encoder.eval(), dev, in_hw, output_layer=False)
            self._packed = _PackedE4E(self.encoder.eval(), dev, in_hw, self._trunks[in_hw])
        return self._packed

    # ---- the three timed parts (tools/bench_e4e.py times them separately)

    def trunk(self, x, pk):
        n = x.shape[0]
        lib = _hip.load()
        net = ctypes.byref(pk.trunk.net)
        taps = [torch.empty(n, c, s, s, device=x.device, dtype=torch.float32) for c, s in pk.tap_shapes]
        outs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in taps])
        wsb = lib.smc_irse_trunk_workspace_bytes(net, n)
        if wsb < 0:
            _hip.check(1, "smc_irse_trunk_workspace_bytes")
        ws = torch.empty(wsb // 4, device=x.device, dtype=torch.float32)
        _hip.call("smc_irse_trunk_f32", net, x.data_ptr(), n, pk.tap_units, outs, 3, ws.data_ptr(), wsb, _hip.stream())
        return taps

    def fpn(self, c1, c2, c3, pk):
        def lateral(c, packed):
            wk, bias = packed
            n, cin, h, w = c.shape
            cout = wk.shape[2]
            y = torch.empty(n, cout, h, w, device=c.device, dtype=torch.float32)
            ph = (_hip.ConvPhase * 1)(modconv._phase([(0, 0)], 1, h, w, 0, 0, 1, 1, wk))
            modconv.gemm(c, y, ph, 1, cin, cout, epi=_bias_epi(bias))
            return y

        p2 = upsample_add(c3, lateral(c2, pk.lat1))
        p1 = upsample_add(p2, lateral(c1, pk.lat2))
        return p2, p1

    def heads(self, c3, p2, p1, pk):
        """The 18 head outputs [style_count][n][512]."""
        n = c3.shape[0]
        dev = c3.device
        count = pk.lin_wk.shape[0]
        feats = torch.empty(count, n, 512, device=dev, dtype=torch.float32)
        for (lo, hi, levels), feat in zip(pk.families, (c3, p2, p1)):
            G = hi - lo
            x, ss, gs = feat, feat.shape[1] * feat.shape[2] * feat.shape[3], 0
            for li, lv in enumerate(levels):
                last = li == len(levels) - 1
                y = feats[lo:hi] if last else torch.empty(G, n, lv.cout, lv.oh, lv.oh, device=dev, dtype=torch.float32)
                if lv.wk_cat is not None:
                    # one gather GEMM with cout = G * 512: y [n][G*512][oh][ow], read below as channel slices
                    y = torch.empty(n, G * lv.cout, lv.oh, lv.oh, device=dev, dtype=torch.float32)
                    modconv.gemm(x, y, lv.phase_cat, 1, lv.cin, G * lv.cout,
                                 epi=_bias_epi(lv.bias_cat, "lrelu", LRELU_ALPHA))
                    x, ss, gs = y, G * lv.cout * lv.oh * lv.oh, lv.cout * lv.oh * lv.oh
                    continue
                if pk.grouped:
                    grouped_conv(x, ss, gs, G, n, lv.cin, lv.h, lv.h, lv.wk, lv.taps_c, lv.bias, LRELU_ALPHA, y, lv.cout)
                else:
                    for g in range(G):
                        xg = x if gs == 0 else x[g]
                        modconv.gemm(xg, y[g].view(n, lv.cout, lv.oh, lv.oh), lv.phases[g], 1, lv.cin, lv.cout,
                                     epi=_bias_epi(lv.bias[g], "lrelu", LRELU_ALPHA))
                x, ss, gs = y, lv.cout * lv.oh * lv.oh, n * lv.cout * lv.oh * lv.oh
        out = torch.empty_like(feats)
        if pk.grouped:
            grouped_conv(feats, 512, n * 512, count, n, 512, 1, 1, pk.lin_wk, pk.lin_taps, pk.lin_bias, 1.0, out, 512)
        else:
            lib = _hip.load()
            wsb = max(lib.smc_linear_workspace_size(n, 512, 512), 0)
            ws = torch.empty(max(wsb // 4, 1), device=dev, dtype=torch.float32)
            for g in range(count):
                le = _hip.LinearEpilogue()
                le.bias = pk.lin_bias[g].data_ptr()
                _hip.call("smc_linear_f32", feats[g].data_ptr(), 512, pk.lin_wk[g].data_ptr(), 512, out[g].data_ptr(),
                          512, n, 512, 512, ctypes.byref(le), ws.data_ptr(), wsb, _hip.stream())
        return out

    @torch.no_grad()
    def forward(self, x, latent_avg=None):
        """x [n, 3, S, S] in [-1, 1] -> W+ [n, style_count, 512] (+ latent_avg [style_count, 512] when given or set)."""
        if not x.is_cuda:
            raise RuntimeError("HipE4E runs on the GPU only (got a CPU tensor)")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
            raise ValueError(f"HipE4E expects square [n, 3, S, S] images, got {tuple(x.shape)}")
        x = x.to(torch.float32).contiguous()
        pk = self.packed(x.shape[2])
        c1, c2, c3 = self.trunk(x, pk)
        p2, p1 = self.fpn(c1, c2, c3, pk)
        heads = self.heads(c3, p2, p1, pk).permute(1, 0, 2).contiguous()
        w = ENCODERS[self.encoder_type].combine(heads)
        avg = self.latent_avg if latent_avg is None else latent_avg
        if avg is not None:
            w = w + avg.to(w.device, torch.float32)  # psp.py:64-68: latent_avg.repeat(n, 1, 1)
        return w


def build_e4e(state_dict=None, seed=5, device="cuda", encoder_type="Encoder4Editing", stylegan_size=1024,
              latent_avg=None):
    from . import synthetic
    net = HipE4E(encoder_type=encoder_type, stylegan_size=stylegan_size)
    net.encoder.load_state_dict(state_dict if state_dict is not None else
                                synthetic.e4e_state_dict(net.encoder, seed=seed))
    net.latent_avg = latent_avg
    return net.eval().requires_grad_(False).to(device)
