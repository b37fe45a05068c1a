"""Cases of the convolution weight-gradient kernel (smc_conv_wgrad_f32) and their fp64 references.

Each case is the smallest instance of something the kernel can get wrong (32 x 32-channel tiles, 16-position K
chunks over the flattened (n, a, b) index, masked tile edges, split K).  Every case keeps n * out_h * out_w <= 4096.

Reference: torch.nn.grad.conv2d_weight on the CPU in float64; for the role-swapped case (the weight gradient of the
stride-2 transposed conv) the fp64 autograd of F.conv_transpose2d.  `bound` is the same sum over the same index set
with absolute values, sum |grad| |inp|, the scale of the accuracy bound.
"""
import collections

import torch
import torch.nn.functional as F

Case = collections.namedtuple("Case", "id n cin cout in_h in_w k stride pad swap")


def _c(id, n, cin, cout, in_h, in_w, k, stride, pad, swap=False):
    return Case(id, n, cin, cout, in_h, in_w, k, stride, pad, swap)


# cin / cout / in_h / in_w are the kernel's arguments: for the role-swapped case `inp` is the transposed conv's
# output gradient dT (5 channels, 9 x 9) and `grad` the layer input x (4 channels, 4 x 4).
CASES = [
    _c("tiny_4to5_7x7", 2, 4, 5, 7, 7, 3, 1, 1),          # far below a tile, odd plane, chunks cross image boundaries
    _c("edge_17to33_9x5", 1, 17, 33, 9, 5, 3, 1, 1),      # one channel over a tile edge on both sides, rows < a chunk
    _c("tiles_48to96_16x16", 2, 48, 96, 16, 16, 3, 1, 1),  # several tiles, the last partly filled
    _c("k1_6to3_5x5", 2, 6, 3, 5, 5, 1, 1, 0),             # one tap
    _c("stride2_4to5_8x8", 2, 4, 5, 8, 8, 3, 2, 1),        # strided reads (the down2 golden's conv)
    _c("swap_convT_4x4", 2, 5, 4, 9, 9, 3, 2, 0, swap=True),   # transposed-conv weight gradient (up2_plain golden)
    _c("pad2_16to16_4x4", 3, 16, 16, 4, 4, 3, 1, 2),       # pad 2: whole tap rows out of range
    _c("split_32to32_32x32", 4, 32, 32, 32, 32, 3, 1, 1),  # one tile, K = 4096: the planner must split
]
BY_ID = {c.id: c for c in CASES}
SPLIT_CASE = "split_32to32_32x32"   # asserts nsplit > 1 on a 256-CU device
FIRST_CASE = "tiny_4to5_7x7"        # asserts nsplit >= 1


def out_hw(c):
    return (c.in_h + 2 * c.pad - c.k) // c.stride + 1, (c.in_w + 2 * c.pad - c.k) // c.stride + 1


def inputs(c):
    """Seeded N(0, 1) operands (CPU fp32): inp [n, cin, in_h, in_w], grad [n, cout, out_h, out_w]."""
    gen = torch.Generator().manual_seed(1000 + CASES.index(c))
    oh, ow = out_hw(c)
    inp = torch.randn(c.n, c.cin, c.in_h, c.in_w, generator=gen)
    grad = torch.randn(c.n, c.cout, oh, ow, generator=gen)
    return inp, grad


def _ref(c, inp, grad):
    inp, grad = inp.double(), grad.double()
    if c.swap:
        # inp = dT, grad = x: dw [x channels][dT channels][k][k], conv_transpose2d's weight layout
        w = torch.zeros(c.cout, c.cin, c.k, c.k, dtype=torch.float64, requires_grad=True)
        (dw,) = torch.autograd.grad(F.conv_transpose2d(grad, w, stride=2), w, inp)
        return dw
    return torch.nn.grad.conv2d_weight(inp, (c.cout, c.cin, c.k, c.k), grad, stride=c.stride, padding=c.pad)


_cache = {}


def reference(c):
    """(inp, grad, dw_ref fp64, bound fp64) of a case, computed once and shared (do not modify)."""
    if c.id not in _cache:
        inp, grad = inputs(c)
        _cache[c.id] = (inp, grad, _ref(c, inp, grad), _ref(c, inp.abs(), grad.abs()))
    return _cache[c.id]
