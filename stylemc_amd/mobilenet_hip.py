"""MobileNet-GDConv landmark regressor (mobilenet_facial.MobileNet_GDConv / _56) on the gfx950 kernel library.

Eval mode, frozen, fp32.  Every BatchNorm is folded at load into a per-channel scale / shift (computed in fp64).

  stem, every 1x1   smc_conv_gemm_f32 (the gather GEMM on the exact-fp32 MFMA).  BN + ReLU6 is its SMC_EPI_MODACT
                    epilogue with scale_c = the BN scale, bias = the BN shift, act relu, gain 1, clamp 6
                    (y = clamp(relu(acc * scale + shift), +-6) = ReLU6); the linear projection is SMC_EPI_AFFINE, with
                    ``residual`` = the block's input where the block has a skip.  No new epilogue mode is needed.
  depthwise 3x3     smc_dwconv_f32 (BN + ReLU6 in its own epilogue)
  linear7           smc_dwconv_f32, global form (7x7 on 7x7 / 2x2 on 2x2), BN folded, linear
  linear1           1x1 GEMM on the 1x1 planes, SMC_EPI_AFFINE

The gather GEMM wants cin % 16 == 0 and cout == 16 or cout % 32 == 0, so every activation is carried at its channel
count rounded up to 32 (3 -> 16 for the image, 24 -> 32, 144 -> 160, 136 -> 160): the padded weights, scales and shifts
are zero, so the padded channels hold exact zeros through ReLU6, the depthwise layers and the residual adds, and the
real channels see the same sums.
"""
import ctypes

import torch
from torch import nn

from . import _hip, mobilenet_facial, modconv


def padded(c):
    return 16 if c <= 16 else (c + 31) // 32 * 32


def fold_bn(bn):
    """(scale, shift) of an eval-mode BatchNorm2d, in fp64."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return scale, bn.bias.detach().double() - bn.running_mean.detach().double() * scale


def _pad1(v, c, dev):
    out = torch.zeros(c, dtype=torch.float32, device=dev)
    out[:v.numel()] = v.to(dev, torch.float32)
    return out


class _Gemm:
    """A dense conv (1x1, or the 3x3 stride-2 stem) + folded BN [+ ReLU6] as one smc_conv_gemm_f32 call."""

    def __init__(self, conv, bn, relu6, dev):
        W = conv.weight.detach().to(dev, torch.float32)
        cout, cin, k, _ = W.shape
        self.cin, self.cout, self.k, self.stride = padded(cin), padded(cout), k, conv.stride[0]
        wk = torch.zeros(k * k, self.cin, self.cout, dtype=torch.float32, device=dev)
        wk[:, :cin, :cout] = W.reshape(cout, cin, k * k).permute(2, 1, 0)
        self.wk = wk
        scale, shift = fold_bn(bn)
        self.scale, self.shift = _pad1(scale, self.cout, dev), _pad1(shift, self.cout, dev)
        self.relu6 = relu6
        self.offs = [(ky - k // 2, kx - k // 2) for ky in range(k) for kx in range(k)]

    def out_hw(self, h, w):
        return (h - 1) // self.stride + 1, (w - 1) // self.stride + 1

    def __call__(self, x, residual=None):
        n, _, h, w = x.shape
        oh, ow = self.out_hw(h, w)
        y = torch.empty(n, self.cout, oh, ow, device=x.device, dtype=torch.float32)
        ph = (_hip.ConvPhase * 1)(modconv._phase(self.offs, self.stride, oh, ow, 0, 0, 1, 1, self.wk))
        if self.relu6:
            e = modconv._epilogue(_hip.EPI_MODACT, bias=self.shift, act="relu", gain=1.0, clamp=6.0)
        else:
            e = modconv._epilogue(_hip.EPI_AFFINE, bias=self.shift)
            if residual is not None:
                e.residual = _hip.ptr(residual)
                e.residual_stride = 1
        e.scale_c = _hip.ptr(self.scale)
        modconv.gemm(x, y, ph, 1, self.cin, self.cout, epi=e)
        return y


class _Depthwise:
    """A depthwise conv + folded BN [+ ReLU6] as one smc_dwconv_f32 call (3x3 pad 1, or the global form)."""

    def __init__(self, conv, bn, relu6, dev):
        W = conv.weight.detach().to(dev, torch.float32)
        c, _, k, _ = W.shape
        self.c, self.k, self.stride, self.pad = padded(c), k, conv.stride[0], conv.padding[0]
        self.w = torch.zeros(self.c, k, k, dtype=torch.float32, device=dev)
        self.w[:c] = W[:, 0]
        scale, shift = fold_bn(bn)
        self.scale, self.shift = _pad1(scale, self.c, dev), _pad1(shift, self.c, dev)
        self.act = _hip.DW_ACT_RELU6 if relu6 else _hip.DW_ACT_LINEAR

    def __call__(self, x):
        return dwconv(x, self.w, self.stride, self.pad, self.scale, self.shift, self.act)


def dwconv(x, w, stride=1, pad=1, scale=None, shift=None, act=0):
    """One smc_dwconv_f32 launch: x [n, c, h, w], w [c, k, k]."""
    n, c, h, wd = x.shape
    k = w.shape[-1]
    if not _hip.load().smc_dwconv_supported(n, c, h, wd, k, stride, pad):
        raise RuntimeError(f"smc_dwconv_f32 has no kernel for {tuple(x.shape)} k {k} stride {stride} pad {pad}")
    oh, ow = ((h - 1) // stride + 1, (wd - 1) // stride + 1) if pad == 1 else (1, 1)
    y = torch.empty(n, c, oh, ow, device=x.device, dtype=torch.float32)
    _hip.call("smc_dwconv_f32", _hip.ptr(x), n, c, h, wd, _hip.ptr(w), k, stride, pad, _hip.ptr(scale), _hip.ptr(shift),
              act, _hip.ptr(y), _hip.stream())
    return y


def maxpool2d(x, k, stride=2):
    """One smc_maxpool2d_f32 launch (ceil mode, pad 0): x [n, c, h, w]."""
    n, c, h, w = x.shape
    oh, ow = -((h - k) // -stride) + 1, -((w - k) // -stride) + 1
    y = torch.empty(n, c, oh, ow, device=x.device, dtype=torch.float32)
    _hip.call("smc_maxpool2d_f32", _hip.ptr(x), n * c, h, w, k, stride, _hip.ptr(y), _hip.stream())
    return y


def crop_bilinear_norm(img, boxes, out_size, mean=None, std=None, denorm=True):
    """One smc_crop_bilinear_norm_f32 launch: img [n, 3, H, W] (in [-1, 1] with ``denorm``, else 0..255 values), boxes
    [n, 4] int32 on the device (x1, y1, x2, y2; exclusive ends), mean / std sequences of 3 floats (both None: no
    normalise, the resized 0..255 crop) -> [n, 3, out_size, out_size]."""
    n, c, h, w = img.shape
    if c != 3 or boxes.dtype != torch.int32 or tuple(boxes.shape) != (n, 4) or not boxes.is_cuda:
        raise ValueError("crop_bilinear_norm: img [n, 3, H, W] and int32 device boxes [n, 4] expected")
    img, boxes = img.contiguous(), boxes.contiguous()
    y = torch.empty(n, 3, out_size, out_size, device=img.device, dtype=torch.float32)
    m3 = (ctypes.c_float * 3)(*[float(v) for v in mean]) if mean is not None else None
    s3 = (ctypes.c_float * 3)(*[float(v) for v in std]) if std is not None else None
    _hip.call("smc_crop_bilinear_norm_f32", _hip.ptr(img), n, h, w, boxes.data_ptr(), out_size, int(bool(denorm)), m3, s3,
              _hip.ptr(y), _hip.stream())
    return y


class _Packed:
    def __init__(self, net, dev):
        feats = net.base_net[0]
        self.stem = _Gemm(feats[0][0], feats[0][1], True, dev)
        self.blocks = []
        for blk in feats[1:-1]:
            layers = list(blk.conv)
            expand = _Gemm(layers[0][0], layers[0][1], True, dev) if len(layers) == 4 else None
            dw = _Depthwise(layers[-3][0], layers[-3][1], True, dev)
            project = _Gemm(layers[-2], layers[-1], False, dev)
            self.blocks.append((expand, dw, project, blk.use_res_connect))
        self.last = _Gemm(feats[-1][0], feats[-1][1], True, dev)
        self.linear7 = _Depthwise(net.linear7.conv, net.linear7.bn, False, dev)
        self.linear1 = _Gemm(net.linear1.conv, net.linear1.bn, False, dev)
        self.num_classes = net.linear1.conv.weight.shape[0]
        if torch.device(dev).type == "cuda":
            torch.cuda.current_stream(dev).synchronize()


class HipMobileNetGDConv(nn.Module):
    """MobileNet_GDConv (``input_size`` 224) or MobileNet_GDConv_56 (56), state_dict-compatible with the
    mobilenet_facial modules."""

    def __init__(self, num_classes=136, input_size=224):
        super().__init__()
        cls = {224: mobilenet_facial.MobileNet_GDConv, 56: mobilenet_facial.MobileNet_GDConv_56}.get(input_size)
        if cls is None:
            raise ValueError(f"MobileNet-GDConv exists for 224 and 56 px inputs, not {input_size}")
        self.net = cls(num_classes)
        self.input_size = input_size
        self._packed = None

    def state_dict(self, *args, **kwargs):
        return self.net.state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        r = self.net.load_state_dict(state_dict, strict=strict, assign=assign)
        self._packed = None
        return r

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self._packed = None
        return self

    def packed(self):
        if self._packed is None:
            self._packed = _Packed(self.net.eval(), next(self.net.parameters()).device)
        return self._packed

    def trunk(self, x, pk, on_depthwise=None):
        """features[0..18] on the channel-padded input.  on_depthwise(layer, x): called before each depthwise launch
        (tools/bench_landmarks.py collects the layers' shapes with it)."""
        x = pk.stem(x)
        for expand, dw, project, skip in pk.blocks:
            h = expand(x) if expand is not None else x
            if on_depthwise is not None:
                on_depthwise(dw, h)
            x = project(dw(h), residual=x if skip else None)
        return pk.last(x)

    @torch.no_grad()
    def forward(self, x):
        """x [n, 3, S, S] normalised crops -> [n, num_classes]."""
        if not x.is_cuda:
            raise RuntimeError("HipMobileNetGDConv runs on the GPU only (got a CPU tensor)")
        s = self.input_size
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, s, s):
            raise ValueError(f"HipMobileNetGDConv expects [n, 3, {s}, {s}] crops, got {tuple(x.shape)}")
        pk = self.packed()
        xp = torch.zeros(x.shape[0], pk.stem.cin, s, s, device=x.device, dtype=torch.float32)
        xp[:, :3] = x
        y = pk.linear1(pk.linear7(self.trunk(xp, pk)))
        return y[:, :pk.num_classes, 0, 0].contiguous()


def build_mobilenet(state_dict=None, seed=7, device="cuda", input_size=224, num_classes=136):
    """The executor with a checkpoint's state_dict (mobilenet_facial.load_checkpoint) or the seeded synthetic weights."""
    from . import synthetic
    net = HipMobileNetGDConv(num_classes=num_classes, input_size=input_size)
    net.net.load_state_dict(state_dict if state_dict is not None else synthetic.mobilenet_state_dict(net.net, seed=seed))
    return net.eval().requires_grad_(False).to(device)
