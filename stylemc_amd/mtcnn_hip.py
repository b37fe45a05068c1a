"""MTCNN's P-Net / R-Net / O-Net (MTCNN/get_nets.py) on the gfx950 kernel library.

  convs    the valid 3x3 / 2x2 convolutions with bias + PReLU: smc_conv_gemm_f32 gather convs (taps (ky, kx) at stride 1,
           no tap ever leaves the plane) with the SMC_EPI_PRELU epilogue (scale_c NULL, bias, alpha_c)
  pools    smc_maxpool2d_f32 (ceil mode)
  FC       the same GEMM as a 1-tap conv on 1 x 1 planes (cin = 576 / 1152).  Flatten's transpose(3, 2) quirk
           (get_nets.py:21-24) is folded into the packed FC weight: its columns are permuted from (c, x, y) to (c, y, x)
           order once at load, so the activations are read as they lie in memory
  heads    the 2-way class head, the 4 box offsets (and O-Net's 10 landmark coordinates) as ONE GEMM with the heads'
           weights concatenated (6 / 16 outputs, SMC_EPI_AFFINE with the bias); the 2-way softmax is torch's

The GEMM wants cin % 16 == 0 and cout == 16 or cout % 32 == 0: channels are carried rounded up (3 -> 16, 10 -> 16,
28 -> 32, 48 -> 64) with zero weights, biases and slopes, so the padded channels hold exact zeros.

The nets are packed once (the reference rebuilds them and rereads the weight files on every detect_faces call,
detector.py:28-31).  Interface: float32 numpy batch in, numpy arrays out, as MTCNN.detector.detect_faces calls them.
"""
import numpy as np
import torch

from . import _hip, modconv
from .MTCNN import get_nets
from .mobilenet_hip import maxpool2d, padded


class _Conv:
    """Valid k x k conv (or an FC as a 1-tap conv on 1 x 1 planes) + bias [+ PReLU]."""

    def __init__(self, weight, bias, alpha, dev):
        W = torch.as_tensor(weight, dtype=torch.float32)
        if W.dim() == 2:
            W = W[:, :, None, None]
        cout, cin, k, _ = W.shape
        self.k, self.cin, self.cout = k, padded(cin), padded(cout)
        wk = torch.zeros(k * k, self.cin, self.cout, dtype=torch.float32)
        wk[:, :cin, :cout] = W.reshape(cout, cin, k * k).permute(2, 1, 0)
        self.wk = wk.to(dev)
        self.bias = torch.zeros(self.cout, dtype=torch.float32)
        self.bias[:cout] = torch.as_tensor(bias, dtype=torch.float32)
        self.bias = self.bias.to(dev)
        self.alpha = None
        if alpha is not None:
            a = torch.zeros(self.cout, dtype=torch.float32)
            a[:cout] = torch.as_tensor(alpha, dtype=torch.float32)
            self.alpha = a.to(dev)
        self.offs = [(ky, kx) for ky in range(k) for kx in range(k)]

    def __call__(self, x):
        n, _, h, w = x.shape
        oh, ow = h - self.k + 1, w - self.k + 1
        y = torch.empty(n, self.cout, oh, ow, device=x.device, dtype=torch.float32)
        ph = (_hip.ConvPhase * 1)(modconv._phase(self.offs, 1, oh, ow, 0, 0, 1, 1, self.wk))
        if self.alpha is not None:
            e = modconv._epilogue(_hip.EPI_PRELU, bias=self.bias)
            e.alpha_c = _hip.ptr(self.alpha)
        else:
            e = modconv._epilogue(_hip.EPI_AFFINE, bias=self.bias)
        modconv.gemm(x, y, ph, 1, self.cin, self.cout, epi=e)
        return y


def fold_flatten(weight, c, h, w):
    """FC weight [out, c * w * h] for inputs flattened after transpose(3, 2), i.e. in (c, x, y) order, re-ordered for
    inputs flattened as they lie in memory, (c, y, x): a permutation of columns, exact."""
    W = torch.as_tensor(weight, dtype=torch.float32)
    return W.reshape(W.shape[0], c, w, h).transpose(2, 3).reshape(W.shape[0], c * h * w)


def _pad_rows(weight, c_real, c_pad, hw):
    """FC weight [out, c_real * hw] -> [out, c_pad * hw] with zero columns for the padded channels."""
    W = torch.zeros(weight.shape[0], c_pad, hw, dtype=torch.float32)
    W[:, :c_real] = weight.reshape(weight.shape[0], c_real, hw)
    return W.reshape(weight.shape[0], c_pad * hw)


class _Net:
    def __init__(self, name, wts, dev):
        f = lambda k: wts["features." + k]  # noqa: E731
        conv = lambda i: _Conv(f(f"conv{i}.weight"), f(f"conv{i}.bias"), f(f"prelu{i}.weight"), dev)  # noqa: E731
        self.name = name
        if name == "pnet":
            self.body = [conv(1), ("pool", 2), conv(2), conv(3)]
            heads, self.fc = ("conv4_1", "conv4_2"), None
        else:
            if name == "rnet":
                self.body = [conv(1), ("pool", 3), conv(2), ("pool", 3), conv(3)]
                fc, c, side, heads = 4, 64, 3, ("conv5_1", "conv5_2")
            else:
                self.body = [conv(1), ("pool", 3), conv(2), ("pool", 3), conv(3), ("pool", 2), conv(4)]
                fc, c, side, heads = 5, 128, 3, ("conv6_1", "conv6_2", "conv6_3")
            Wfc = _pad_rows(fold_flatten(f(f"conv{fc}.weight"), c, side, side), c, padded(c), side * side)
            self.fc = _Conv(Wfc, f(f"conv{fc}.bias"), f(f"prelu{fc}.weight"), dev)
            self.flat = (padded(c), side)
        Wh = torch.cat([torch.as_tensor(wts[h + ".weight"], dtype=torch.float32).flatten(1) for h in heads])
        bh = torch.cat([torch.as_tensor(wts[h + ".bias"], dtype=torch.float32) for h in heads])
        self.heads = _Conv(Wh, bh, None, dev)
        self.head_sizes = [int(np.asarray(wts[h + ".bias"]).shape[0]) for h in heads]

    def __call__(self, x):
        for layer in self.body:
            x = maxpool2d(x, layer[1]) if isinstance(layer, tuple) else layer(x)
        if self.fc is not None:
            c, side = self.flat
            if tuple(x.shape[1:]) != (c, side, side):
                raise ValueError(f"{self.name}: {tuple(x.shape[2:])} planes at the FC layer, expected {side} x {side}")
            x = self.fc(x.reshape(x.shape[0], c * side * side, 1, 1))
        y = self.heads(x)
        outs, lo = [], 0
        for size in self.head_sizes:
            outs.append(y[:, lo:lo + size])
            lo += size
        probs = torch.softmax(outs[0], dim=1)
        if self.fc is not None:
            outs = [o[:, :, 0, 0] for o in outs]
            probs = probs[:, :, 0, 0]
        # (offsets, probs) / (landmarks, offsets, probs), the nets' output order (get_nets.py:72,117,170)
        return tuple(reversed([probs] + outs[1:]))


MIN_INPUT = {"pnet": 12, "rnet": 24, "onet": 48}


class HipMTCNN:
    """The three nets, packed once for ``device``.  weights: {'pnet' | 'rnet' | 'onet': {parameter name: array}}."""

    def __init__(self, weights, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("HipMTCNN runs on the GPU only")
        self.nets = {n: _Net(n, weights[n], self.device) for n in get_nets.NAMES}
        torch.cuda.current_stream(self.device).synchronize()

    @torch.no_grad()
    def run(self, name, x):
        """x: float32 numpy or tensor [n, 3, h, w] -> tuple of device tensors."""
        x = torch.as_tensor(x, dtype=torch.float32)
        s = MIN_INPUT[name]
        ok = x.dim() == 4 and x.shape[1] == 3 and (min(x.shape[2:]) >= s if name == "pnet" else tuple(x.shape[2:]) == (s, s))
        if not ok:
            raise ValueError(f"{name}: input {tuple(x.shape)}")
        if x.shape[0] == 0:
            raise ValueError(f"{name}: empty batch")
        xp = torch.zeros(x.shape[0], 16, x.shape[2], x.shape[3], device=self.device, dtype=torch.float32)
        xp[:, :3] = x.to(self.device)
        with torch.cuda.device(self.device):
            return self.nets[name](xp)

    def _numpy(self, name, x):
        return tuple(o.contiguous().cpu().numpy() for o in self.run(name, x))

    def pnet(self, x):
        return self._numpy("pnet", x)

    def rnet(self, x):
        return self._numpy("rnet", x)

    def onet(self, x):
        return self._numpy("onet", x)


def build_mtcnn(weights="synthetic", device="cuda", seed=11):
    """HipMTCNN from a weights directory (pnet.npy, rnet.npy, onet.npy in the reference's format), a dict of the three
    nets' weights, or 'synthetic' (seeded stand-ins, synthetic.mtcnn_weights)."""
    if isinstance(weights, str):
        if weights == "synthetic":
            from . import synthetic
            weights = synthetic.mtcnn_weights(seed=seed)
        else:
            weights = get_nets.load_weights(weights)
    return HipMTCNN(weights, device=device)
