"""conv2d / conv_transpose2d on gfx950 with weight gradients -- drop-in for the reference's
torch_utils/ops/conv2d_gradfix.py.

Public surface kept: ``conv2d``, ``conv_transpose2d``, the module flags ``enabled`` and
``weight_gradients_disabled`` and the context manager ``no_weight_gradients()``.

Forward and data gradient are one ``smc_conv_gemm_f32`` launch each (the direct implicit GEMM of the synthesis
layers, exact-fp32 products: the weights are not frozen here, so they are packed per call and carry no split-bf16
planes); the weight gradient is ``smc_conv_wgrad_f32``.  What has no kernel raises ``NotImplementedError``:
dilation, kernels other than 1x1 / 3x3, stride > 2, padding outside 0..2, ``conv_transpose2d`` other than 3x3
stride 2 padding 0 output_padding 0, and double backward.  CPU tensors raise ``RuntimeError`` (no CPU fallback),
non-fp32 tensors ``NotImplementedError``; ``enabled = False`` (the reference's switch to the stock torch ops) raises
``RuntimeError`` on the next call instead of silently changing nothing.
"""
import contextlib

import torch
from torch.autograd.function import once_differentiable

from ... import _hip
from ... import modconv

enabled = True                      # the reference's switch to the stock torch ops: False raises here (no fallback)
weight_gradients_disabled = False   # forcefully skip the weight gradient (see no_weight_gradients)

# How many launches had to zero-pad their channels to the direct GEMM's granularity (cin % 16, cout 16 or a multiple
# of 32) since import.  The synthesis widths need none (tests assert it).
channel_pad_count = 0


@contextlib.contextmanager
def no_weight_gradients():
    global weight_gradients_disabled
    old = weight_gradients_disabled
    weight_gradients_disabled = True
    try:
        yield
    finally:
        weight_gradients_disabled = old


def _check_enabled():
    if not enabled:
        raise RuntimeError("stylemc_amd.conv2d_gradfix: enabled = False selects the stock torch.nn.functional ops in the "
                           "reference; this build has no such fallback, the HIP path is the only one")


def _pair(v, what):
    if isinstance(v, int):
        return v, v
    v = tuple(int(e) for e in v)
    if len(v) == 1:
        return v[0], v[0]
    if len(v) != 2:
        raise ValueError(f"conv2d_gradfix: {what} must be an int or a pair (got {v})")
    return v


def _check_tensors(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("stylemc_amd.conv2d_gradfix: tensors must be on the GPU (no CPU fallback)")
        if t.dtype != torch.float32:
            raise NotImplementedError(f"stylemc_amd.conv2d_gradfix: fp32 only (got {t.dtype})")


def _pad_cin(c):
    return (c + 15) // 16 * 16


def _pad_cout(c):
    return 16 if c <= 16 else (c + 31) // 32 * 32


def _gemm(x, wk_list, phases_geom, cin, cout, yh, yw, zero_fill=False):
    """One smc_conv_gemm_f32 launch (SMC_EPI_STORE) of x [n, cin, h, w] with per-phase packed weights
    wk_list[p] [taps][cin][cout] and geometry phases_geom[p] = (taps, in_stride, out_h, out_w, oy, ox, sy, sx).
    Channels are zero-padded to the GEMM's granularity where needed.  Returns y [n, cout, yh, yw]."""
    global channel_pad_count
    n = x.shape[0]
    ci, co = _pad_cin(cin), _pad_cout(cout)
    if ci != cin or co != cout:
        channel_pad_count += 1
        if ci != cin:
            x = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, ci - cin))
        wk_list = [torch.nn.functional.pad(wk, (0, co - cout, 0, ci - cin)) for wk in wk_list]
    x = x.contiguous()
    wk_list = [wk.contiguous() for wk in wk_list]
    y = (torch.zeros if zero_fill else torch.empty)(n, co, yh, yw, device=x.device, dtype=torch.float32)
    arr = (_hip.ConvPhase * len(wk_list))(*[modconv._phase(g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], wk)
                                            for g, wk in zip(phases_geom, wk_list)])
    epi = modconv._epilogue(_hip.EPI_STORE)
    modconv.gemm(x, y, arr, len(wk_list), ci, co, epi=epi)
    return y if co == cout else y[:, :cout].contiguous()


def _wgrad(inp, grad, kh, kw, stride, pad):
    """smc_conv_wgrad_f32: dw [grad channels][inp channels][kh][kw]."""
    inp, grad = inp.contiguous(), grad.contiguous()
    n, cin, ih, iw = inp.shape
    _, cout, oh, ow = grad.shape
    lib = _hip.load()
    nb = lib.smc_conv_wgrad_workspace_size(n, cin, cout, ih, iw, oh, ow, kh, kw, stride)
    ws = torch.empty(nb // 4, device=inp.device, dtype=torch.float32) if nb > 0 else None
    dw = torch.empty(cout, cin, kh, kw, device=inp.device, dtype=torch.float32)
    _hip.call("smc_conv_wgrad_f32", inp.data_ptr(), n, cin, ih, iw, grad.data_ptr(), cout, oh, ow, kh, kw, stride,
              pad[0], pad[1], dw.data_ptr(), _hip.ptr(ws), nb, _hip.stream())
    return dw


# ------------------------------------------------------------------------------------------- conv2d, one group

def _conv_fwd(x, w, stride, pad):
    cout, cin, kh, kw = w.shape
    _, _, ih, iw = x.shape
    oh = (ih + 2 * pad[0] - kh) // stride + 1
    ow = (iw + 2 * pad[1] - kw) // stride + 1
    assert oh >= 1 and ow >= 1, "conv2d_gradfix: empty output"
    taps = [(ky - pad[0], kx - pad[1]) for ky in range(kh) for kx in range(kw)]
    wk = w.permute(2, 3, 1, 0).reshape(kh * kw, cin, cout)   # [t][i][o]
    return _gemm(x, [wk], [(taps, stride, oh, ow, 0, 0, 1, 1)], cin, cout, oh, ow)


def _conv_dgrad(dy, w, stride, pad, ih, iw):
    """Adjoint of _conv_fwd through the same GEMM: flipped taps on [t][o][i] (stride 1), or the polyphase transposed
    form with the padding folded into each phase's taps (stride 2)."""
    cout, cin, kh, kw = w.shape
    wb = w.permute(2, 3, 0, 1)   # [ky][kx][o][i]
    if stride == 1:
        taps = [(pad[0] - ky, pad[1] - kx) for ky in range(kh) for kx in range(kw)]
        return _gemm(dy, [wb.reshape(kh * kw, cout, cin)], [(taps, 1, ih, iw, 0, 0, 1, 1)], cout, cin, ih, iw)
    # dx[2a+qy, 2b+qx] = sum over the taps with (qy + pad - ky) even of W[o,i,ky,kx] dy[a + (qy + pad - ky)/2, ...]
    wks, geom = [], []
    for qy in range(min(2, ih)):
        for qx in range(min(2, iw)):
            sel = [(ky, kx) for ky in range(kh) for kx in range(kw)
                   if (qy + pad[0] - ky) % 2 == 0 and (qx + pad[1] - kx) % 2 == 0]
            if not sel:
                continue
            wks.append(torch.stack([wb[ky, kx] for ky, kx in sel]))
            geom.append(([((qy + pad[0] - ky) // 2, (qx + pad[1] - kx) // 2) for ky, kx in sel], 1,
                         (ih - qy + 1) // 2, (iw - qx + 1) // 2, qy, qx, 2, 2))
    # a 1x1 kernel reaches one phase only: the other input positions get no gradient
    return _gemm(dy, wks, geom, cout, cin, ih, iw, zero_fill=len(wks) < 4)


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, pad):
        ctx.stride, ctx.pad = stride, pad
        ctx.save_for_backward(x, w)
        return _conv_fwd(x, w, stride, pad)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = _conv_dgrad(dy, w, ctx.stride, ctx.pad, x.shape[2], x.shape[3])
        if ctx.needs_input_grad[1] and not weight_gradients_disabled:
            dw = _wgrad(x, dy, w.shape[2], w.shape[3], ctx.stride, ctx.pad)
        return dx, dw, None, None


# ------------------------------------------------------- conv_transpose2d (3x3, stride 2, padding 0), one group

def _convt_fwd(x, w):
    """T[n, o, 2a+ky, 2b+kx] += x[n, i, a, b] w[i, o, ky, kx] as the 4 polyphase phases of modconv.PackedConv."""
    cin, cout, kh, kw = w.shape
    _, _, h, wd = x.shape
    th, tw = 2 * h + 1, 2 * wd + 1
    wks, geom = [], []
    for py in (0, 1):
        for px in (0, 1):
            sel = [(ky, kx) for ky in range(kh) for kx in range(kw) if ky % 2 == py and kx % 2 == px]
            wks.append(torch.stack([w[:, :, ky, kx] for ky, kx in sel]))   # [t][i][o]
            geom.append(([(-(ky - py) // 2, -(kx - px) // 2) for ky, kx in sel], 1, (th - py + 1) // 2,
                         (tw - px + 1) // 2, py, px, 2, 2))
    return _gemm(x, wks, geom, cin, cout, th, tw)


def _convt_dgrad(dt, w, h, wd):
    """dx[n, i, a, b] = sum w[i, o, ky, kx] dT[n, o, 2a+ky, 2b+kx]: the stride-2 gather."""
    cin, cout, kh, kw = w.shape
    taps = [(ky, kx) for ky in range(kh) for kx in range(kw)]
    wk = w.permute(2, 3, 1, 0).reshape(kh * kw, cout, cin)   # [t][o][i]
    return _gemm(dt, [wk], [(taps, 2, h, wd, 0, 0, 1, 1)], cout, cin, h, wd)


class _ConvTranspose2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return _convt_fwd(x, w)

    @staticmethod
    @once_differentiable
    def backward(ctx, dt):
        x, w = ctx.saved_tensors
        dt = dt.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = _convt_dgrad(dt, w, x.shape[2], x.shape[3])
        if ctx.needs_input_grad[1] and not weight_gradients_disabled:
            # roles swapped: the "input" is dT, the "gradient" is x -> [cin][cout][kh][kw], this op's weight layout
            dw = _wgrad(dt, x, w.shape[2], w.shape[3], 2, (0, 0))
        return dx, dw


# ------------------------------------------------------------------------------------------------ public ops

def _grouped(fn, x, w, groups):
    """Run fn(x_g, w_g) group by group on channel slices.  Both weight layouts keep the group as the leading factor
    of dim 0.  For one image the input slices are contiguous views; otherwise they are copied."""
    if groups == 1:
        return fn(x, w)
    if x.shape[1] % groups or w.shape[0] % groups:
        raise ValueError(f"conv2d_gradfix: channels ({x.shape[1]}, {w.shape[0]}) not divisible by groups={groups}")
    cpg = x.shape[1] // groups
    wpg = w.shape[0] // groups
    ys = []
    for g in range(groups):
        xg = x[:, g * cpg:(g + 1) * cpg]
        if x.shape[0] != 1:
            xg = xg.contiguous()
        ys.append(fn(xg, w[g * wpg:(g + 1) * wpg]))
    return torch.cat(ys, dim=1)


def conv2d(input, weight, bias=None, stride=1, padding=0, dilation=1, groups=1):
    if _pair(dilation, "dilation") != (1, 1):
        raise NotImplementedError("stylemc_amd.conv2d_gradfix.conv2d: dilation != 1 has no gfx950 kernel")
    _check_enabled()
    _check_tensors(input, weight, bias)
    sy, sx = _pair(stride, "stride")
    if sy != sx or sy not in (1, 2):
        raise NotImplementedError(f"stylemc_amd.conv2d_gradfix.conv2d: stride {(sy, sx)} (only 1 and 2)")
    kh, kw = weight.shape[2], weight.shape[3]
    if not (kh == kw and kh in (1, 3)):
        raise NotImplementedError(f"stylemc_amd.conv2d_gradfix.conv2d: kernel {kh}x{kw} (only 1x1 and 3x3)")
    pad = _pair(padding, "padding")
    if not all(0 <= p <= 2 for p in pad):
        raise NotImplementedError(f"stylemc_amd.conv2d_gradfix.conv2d: padding {pad} (only 0..2)")
    if input.shape[1] != weight.shape[1] * groups:
        raise ValueError(f"conv2d_gradfix.conv2d: input has {input.shape[1]} channels, weight expects "
                         f"{weight.shape[1] * groups}")
    y = _grouped(lambda xg, wg: _Conv2d.apply(xg, wg, sy, pad), input, weight, groups)
    if bias is not None:
        y = y + bias.reshape(1, -1, 1, 1)
    return y


def conv_transpose2d(input, weight, bias=None, stride=1, padding=0, output_padding=0, groups=1, dilation=1):
    if _pair(dilation, "dilation") != (1, 1):
        raise NotImplementedError("stylemc_amd.conv2d_gradfix.conv_transpose2d: dilation != 1 has no gfx950 kernel")
    _check_enabled()
    _check_tensors(input, weight, bias)
    kh, kw = weight.shape[2], weight.shape[3]
    if not (kh == 3 and kw == 3 and _pair(stride, "stride") == (2, 2) and _pair(padding, "padding") == (0, 0)
            and _pair(output_padding, "output_padding") == (0, 0)):
        raise NotImplementedError("stylemc_amd.conv2d_gradfix.conv_transpose2d: only the 3x3 stride-2 transposed conv "
                                  "with padding 0 and output_padding 0 has a gfx950 kernel")
    if input.shape[1] != weight.shape[0]:
        raise ValueError(f"conv2d_gradfix.conv_transpose2d: input has {input.shape[1]} channels, weight expects "
                         f"{weight.shape[0]}")
    y = _grouped(_ConvTranspose2d.apply, input, weight, groups)
    if bias is not None:
        y = y + bias.reshape(1, -1, 1, 1)
    return y
