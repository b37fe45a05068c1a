"""MobileNet-GDConv 68-point face-landmark regressor (drop-in for the reference's ``mobilenet_facial.py``).

``MobileNet_GDConv`` (224 x 224 input) and ``MobileNet_GDConv_56`` (56 x 56) of the reference (mobilenet_facial.py:
55-85) are torchvision's MobileNetV2 feature trunk, then ``linear7`` (a depthwise convolution whose kernel covers the
whole 7 x 7 / 2 x 2 plane, + BatchNorm) and ``linear1`` (1 x 1 conv 1280 -> num_classes, + BatchNorm); the output is
``[n, num_classes]`` (136 = 68 points x 2, in units of the crop's side).

torchvision is not installed where this project is built, so the trunk is restated here from the MobileNetV2 paper's
table (inverted-residual settings (t, c, n, s) below, stem 3x3 stride 2 -> 32, last 1x1 -> 1280) with the module
nesting torchvision uses, so that a checkpoint's names load: ``features.{i}.conv.{j}...`` inside ``base_net.0``
(mobilenet_facial.py:58-59 wraps ``children()[:-1]``, i.e. the ``features`` Sequential, in another Sequential).
KEY-NAME PARITY WITH TORCHVISION IS UNPINNED HERE: no torchvision and no published checkpoint is available to compare
against.  The reference also registers the same trunk a second time as ``pretrain_net.features.*`` (with the unused
classifier); ``load_checkpoint_state`` drops those duplicate keys.
"""
import torch
from torch import nn

# (expansion t, output channels c, repeats n, stride s of the first repeat)
INVERTED_RESIDUAL_SETTINGS = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2),
                              (6, 320, 1, 1))
STEM_CHANNELS, LAST_CHANNELS = 32, 1280


class ConvBNReLU(nn.Sequential):
    """conv (no bias) + BatchNorm + ReLU6, as children 0 / 1 / 2."""

    def __init__(self, inp, oup, k=3, stride=1, groups=1):
        super().__init__(nn.Conv2d(inp, oup, k, stride, (k - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(oup),
                         nn.ReLU6(inplace=False))


class InvertedResidual(nn.Module):
    """[1x1 expand + BN + ReLU6 (absent at t = 1)], 3x3 depthwise + BN + ReLU6, 1x1 project + BN (linear); the input is
    added when stride is 1 and the channel counts agree."""

    def __init__(self, inp, oup, stride, t):
        super().__init__()
        hidden = inp * t
        self.use_res_connect = stride == 1 and inp == oup
        layers = [ConvBNReLU(inp, hidden, k=1)] if t != 1 else []
        layers += [ConvBNReLU(hidden, hidden, stride=stride, groups=hidden), nn.Conv2d(hidden, oup, 1, 1, 0, bias=False),
                   nn.BatchNorm2d(oup)]
        self.conv = nn.Sequential(*layers)

    def forward(self, x):
        return x + self.conv(x) if self.use_res_connect else self.conv(x)


def mobilenet_v2_features():
    feats = [ConvBNReLU(3, STEM_CHANNELS, stride=2)]
    inp = STEM_CHANNELS
    for t, c, n, s in INVERTED_RESIDUAL_SETTINGS:
        for i in range(n):
            feats.append(InvertedResidual(inp, c, s if i == 0 else 1, t))
            inp = c
    feats.append(ConvBNReLU(inp, LAST_CHANNELS, k=1))
    return nn.Sequential(*feats)


class ConvBlock(nn.Module):
    """conv (no bias) + BatchNorm [+ PReLU] (mobilenet_facial.py:9-27); the two blocks of the nets here are linear."""

    def __init__(self, inp, oup, k, s, p, dw=False, linear=False):
        super().__init__()
        self.linear = linear
        self.conv = nn.Conv2d(inp, oup, k, s, p, groups=inp if dw else 1, bias=False)
        self.bn = nn.BatchNorm2d(oup)
        if not linear:
            self.prelu = nn.PReLU(oup)

    def forward(self, x):
        x = self.bn(self.conv(x))
        return x if self.linear else self.prelu(x)


class MobileNet_GDConv(nn.Module):
    """224 x 224 input: the trunk leaves 7 x 7 planes, linear7 is a 7 x 7 depthwise conv."""
    GLOBAL_K = 7
    INPUT_SIZE = 224

    def __init__(self, num_classes=136):
        super().__init__()
        self.base_net = nn.Sequential(mobilenet_v2_features())
        self.linear7 = ConvBlock(LAST_CHANNELS, LAST_CHANNELS, (self.GLOBAL_K, self.GLOBAL_K), 1, 0, dw=True, linear=True)
        self.linear1 = ConvBlock(LAST_CHANNELS, num_classes, 1, 1, 0, linear=True)

    def forward(self, x):
        x = self.linear1(self.linear7(self.base_net(x)))
        return x.view(x.size(0), -1)


class MobileNet_GDConv_56(MobileNet_GDConv):
    """56 x 56 input: 2 x 2 planes, linear7 is a 2 x 2 depthwise conv (mobilenet_facial.py:72-85)."""
    GLOBAL_K = 2
    INPUT_SIZE = 56


def load_checkpoint_state(checkpoint):
    """The regressor's state_dict out of a checkpoint as the reference saves it (find_direction.py:275-278: a dict with
    ``state_dict`` of a DataParallel-wrapped net): strips ``module.``, drops the duplicate ``pretrain_net.*`` entries
    (the trunk registered a second time, and its unused classifier), keeps ``base_net.0.*`` / ``linear7.*`` /
    ``linear1.*``."""
    sd = checkpoint["state_dict"] if isinstance(checkpoint, dict) and "state_dict" in checkpoint else checkpoint
    out = {}
    for k, v in sd.items():
        k = k[7:] if k.startswith("module.") else k
        if k.startswith("pretrain_net."):
            continue
        out[k] = v
    return out


def load_checkpoint(path, map_location="cpu"):
    """torch.load(weights_only=True) + load_checkpoint_state."""
    return load_checkpoint_state(torch.load(path, map_location=map_location, weights_only=True))
