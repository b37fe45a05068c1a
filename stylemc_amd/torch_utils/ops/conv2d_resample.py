"""2-D convolution with optional FIR up/down-sampling on gfx950 -- drop-in for the reference's
torch_utils/ops/conv2d_resample.py.

``conv2d_resample(x, w, f, up, down, padding, groups, flip_weight, flip_filter)`` keeps the reference's signature and
padding arithmetic (conv2d_resample.py:58-154; the routes as restated in oracle/ops.py).  It composes the HIP
``conv2d_gradfix`` ops (direct implicit GEMM forward / data gradient, ``smc_conv_wgrad_f32`` weight gradient) with the
HIP ``upfirdn2d``; both carry their own autograd, so gradients with respect to x and w follow.  ``up`` and ``down``
are restricted to {1, 2}; what ``conv2d_gradfix`` has no kernel for raises ``NotImplementedError``.
"""
import torch

from . import conv2d_gradfix
from . import upfirdn2d
from .upfirdn2d import _get_filter_size, _parse_padding


def conv2d_resample(x, w, f=None, up=1, down=1, padding=0, groups=1, flip_weight=True, flip_filter=False):
    """x [n, cin, h, w], w [cout, cin // groups, kh, kw], f: a setup_filter() FIR or None."""
    assert isinstance(x, torch.Tensor) and x.ndim == 4
    assert isinstance(w, torch.Tensor) and w.ndim == 4
    assert f is None or (isinstance(f, torch.Tensor) and f.ndim in (1, 2) and f.dtype == torch.float32)
    if not isinstance(up, int) or not isinstance(down, int) or up not in (1, 2) or down not in (1, 2):
        raise NotImplementedError(f"stylemc_amd.conv2d_resample: up={up}, down={down} (only 1 and 2)")
    conv2d_gradfix._check_tensors(x, w)   # GPU fp32 only: no CPU fallback
    assert isinstance(groups, int) and groups >= 1
    oc, icpg, kh, kw = w.shape
    fw, fh = _get_filter_size(f)
    px0, px1, py0, py1 = _parse_padding(padding)

    def conv(x, w, stride=1, pad=0, transpose=False, flip=True):
        # the conv kernels correlate (flip=True, the reference's flip_weight); a true convolution flips the taps
        if not flip:
            w = torch.flip(w, [2, 3])
        if transpose:
            return conv2d_gradfix.conv_transpose2d(x, w, stride=stride, padding=pad, groups=groups)
        return conv2d_gradfix.conv2d(x, w, stride=stride, padding=pad, groups=groups)

    # padding that keeps the image centred through the resampling filters
    if up > 1:
        px0 += (fw + up - 1) // 2
        px1 += (fw - up) // 2
        py0 += (fh + up - 1) // 2
        py1 += (fh - up) // 2
    if down > 1:
        px0 += (fw - down + 1) // 2
        px1 += (fw - down) // 2
        py0 += (fh - down + 1) // 2
        py1 += (fh - down) // 2

    # 1x1 kernel with downsampling: FIR first, so the conv runs on the small image
    if kh == 1 and kw == 1 and down > 1 and up == 1:
        x = upfirdn2d.upfirdn2d(x, f, down=down, padding=[px0, px1, py0, py1], flip_filter=flip_filter)
        return conv(x, w, flip=flip_weight)

    # 1x1 kernel with upsampling: conv first, for the same reason
    if kh == 1 and kw == 1 and up > 1 and down == 1:
        x = conv(x, w, flip=flip_weight)
        return upfirdn2d.upfirdn2d(x, f, up=up, padding=[px0, px1, py0, py1], gain=up ** 2, flip_filter=flip_filter)

    # downsampling only: FIR, then the strided conv
    if down > 1 and up == 1:
        x = upfirdn2d.upfirdn2d(x, f, padding=[px0, px1, py0, py1], flip_filter=flip_filter)
        return conv(x, w, stride=down, flip=flip_weight)

    # upsampling: stride-`up` transposed conv, FIR with gain up^2, optional downsampling FIR
    if up > 1:
        # [groups * oc/g, icpg, kh, kw] -> [groups * icpg, oc/g, kh, kw], conv_transpose2d's weight layout
        wt = w.reshape(groups, oc // groups, icpg, kh, kw).transpose(1, 2).reshape(groups * icpg, oc // groups, kh, kw)
        px0 -= kw - 1
        px1 -= kw - up
        py0 -= kh - 1
        py1 -= kh - up
        pxt = max(min(-px0, -px1), 0)
        pyt = max(min(-py0, -py1), 0)
        x = conv(x, wt, stride=up, pad=[pyt, pxt], transpose=True, flip=not flip_weight)
        x = upfirdn2d.upfirdn2d(x, f, padding=[px0 + pxt, px1 + pxt, py0 + pyt, py1 + pyt], gain=up ** 2,
                                flip_filter=flip_filter)
        if down > 1:
            x = upfirdn2d.upfirdn2d(x, f, down=down, flip_filter=flip_filter)
        return x

    # no resampling left here (up == down == 1).  Symmetric non-negative padding: the conv pads by itself
    if px0 == px1 and py0 == py1 and px0 >= 0 and py0 >= 0:
        return conv(x, w, pad=[py0, px0], flip=flip_weight)

    # asymmetric or negative padding: pad / crop explicitly (a 1x1 identity FIR), then an unpadded conv
    x = upfirdn2d.upfirdn2d(x, None, padding=[px0, px1, py0, py1])
    return conv(x, w, flip=flip_weight)
