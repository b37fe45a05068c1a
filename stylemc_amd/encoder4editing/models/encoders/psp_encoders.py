"""Torch restatement of the reference's e4e / pSp encoders (encoder4editing/models/encoders/psp_encoders.py).

``Encoder4Editing`` (psp_encoders.py:124-200) and ``GradualStyleEncoder`` (psp_encoders.py:58-121) share everything
but the last step: both run the IR-SE50 body, tap units 6 / 20 / 23 (c1, c2, c3), build the FPN maps p2 and p1 and run
18 ``GradualStyleBlock`` heads (3 coarse on c3, 4 middle on p2, 11 fine on p1); e4e returns w0 + deltas
(psp_encoders.py:186-200, ``ProgressiveStage.Inference``: every delta applied), pSp the stacked head outputs
(psp_encoders.py:120).  state_dict names match the reference (``input_layer``, ``body.K.{shortcut_layer,res_layer}``,
``styles.K.convs.M``, ``styles.K.linear``, ``latlayer{1,2}``), so ``e4e_ffhq_encode.pt``'s ``encoder.*`` loads unchanged.

Inference only: the progressive training stages (psp_encoders.py:12-31,165-171) are not restated.  These modules are
the CPU / float64 yardstick of ``stylemc_amd.e4e_hip.HipE4E``, which runs the same state_dict on the HIP kernels.
"""
import math

import torch
from torch import nn

from ....id_loss.model_irse import PReLU
from .helpers import _upsample_add, get_units

TAP_UNITS = (6, 20, 23)      # psp_encoders.py:102-107,179-184: c1, c2, c3
COARSE_IND, MIDDLE_IND = 3, 7  # psp_encoders.py:82-83,148-149


class EqualLinear(nn.Module):
    """models/stylegan2/model.py:128-157 without an activation (the heads use none): weight * (lr_mul / sqrt(in_dim)),
    bias * lr_mul."""

    def __init__(self, in_dim, out_dim, bias=True, bias_init=0, lr_mul=1):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(out_dim, in_dim).div_(lr_mul))
        self.bias = nn.Parameter(torch.zeros(out_dim).fill_(bias_init)) if bias else None
        self.scale = (1 / math.sqrt(in_dim)) * lr_mul
        self.lr_mul = lr_mul

    def forward(self, input):
        return nn.functional.linear(input, self.weight * self.scale,
                                    bias=None if self.bias is None else self.bias * self.lr_mul)


class GradualStyleBlock(nn.Module):
    """psp_encoders.py:34-55: log2(spatial) stride-2 3x3 convs, each followed by LeakyReLU(0.01), down to 1x1, then
    an EqualLinear."""

    def __init__(self, in_c, out_c, spatial):
        super().__init__()
        self.out_c = out_c
        self.spatial = spatial
        num_pools = int(math.log2(spatial))
        modules = [nn.Conv2d(in_c, out_c, kernel_size=3, stride=2, padding=1), nn.LeakyReLU()]
        for _ in range(num_pools - 1):
            modules += [nn.Conv2d(out_c, out_c, kernel_size=3, stride=2, padding=1), nn.LeakyReLU()]
        self.convs = nn.Sequential(*modules)
        self.linear = EqualLinear(out_c, out_c, lr_mul=1)

    def forward(self, x):
        x = self.convs(x)
        x = x.view(-1, self.out_c)
        return self.linear(x)


class _StyleEncoder(nn.Module):
    """What both encoders share: psp_encoders.py:59-93 == 125-161."""

    def __init__(self, num_layers=50, mode="ir_se", stylegan_size=1024):
        super().__init__()
        self.input_layer = nn.Sequential(nn.Conv2d(3, 64, (3, 3), 1, 1, bias=False), nn.BatchNorm2d(64), PReLU(64))
        self.body = nn.Sequential(*get_units(num_layers, mode))
        self.styles = nn.ModuleList()
        log_size = int(math.log(stylegan_size, 2))
        self.style_count = 2 * log_size - 2
        self.coarse_ind = COARSE_IND
        self.middle_ind = MIDDLE_IND
        for i in range(self.style_count):
            spatial = 16 if i < self.coarse_ind else 32 if i < self.middle_ind else 64
            self.styles.append(GradualStyleBlock(512, 512, spatial))
        self.latlayer1 = nn.Conv2d(256, 512, kernel_size=1, stride=1, padding=0)
        self.latlayer2 = nn.Conv2d(128, 512, kernel_size=1, stride=1, padding=0)

    def features(self, x):
        """c1, c2, c3: the outputs of body units 6, 20 and 23."""
        x = self.input_layer(x)
        taps = []
        for i, unit in enumerate(self.body):
            x = unit(x)
            if i in TAP_UNITS:
                taps.append(x)
        return taps

    def head_outputs(self, x):
        """The 18 head outputs [n, 512] in style order (the part both forwards share)."""
        c1, c2, c3 = self.features(x)
        p2 = _upsample_add(c3, self.latlayer1(c2))
        p1 = _upsample_add(p2, self.latlayer2(c1))
        out = []
        for j in range(self.style_count):
            feat = c3 if j < self.coarse_ind else p2 if j < self.middle_ind else p1
            out.append(self.styles[j](feat))
        return out

    @staticmethod
    def combine(heads):
        raise NotImplementedError

    def forward(self, x):
        return self.combine(torch.stack(self.head_outputs(x), dim=1))


class GradualStyleEncoder(_StyleEncoder):
    """pSp: W+ row i is head i's output (psp_encoders.py:109-121)."""

    @staticmethod
    def combine(heads):
        return heads


class Encoder4Editing(_StyleEncoder):
    """e4e at ProgressiveStage.Inference: row 0 is w0 = head 0, row i > 0 is w0 + head i (psp_encoders.py:186-200)."""

    @staticmethod
    def combine(heads):
        w = heads.clone()
        w[:, 1:] += heads[:, :1]
        return w


ENCODERS = {"Encoder4Editing": Encoder4Editing, "GradualStyleEncoder": GradualStyleEncoder}
