"""P-Net, R-Net and O-Net as torch modules with the reference's parameter names (MTCNN/get_nets.py:27-170), and their
weight files.

The modules are the CPU / float64 restatement the GPU executor (mtcnn_hip.HipMTCNN) is tested against; they do not read
weight files in their constructors (the reference's do, from CWD-relative paths).  All convolutions are valid (no
padding) with a bias and a per-channel PReLU; the pools are ceil-mode max-pools.  ``Flatten`` swaps height and width
before flattening (get_nets.py:21-24: the weights were converted from a column-major framework).  The 2-way softmax is
part of the nets' outputs.  O-Net's Dropout is the identity in eval mode and is left out (it has no parameters).

Weight files: ``pnet.npy`` / ``rnet.npy`` / ``onet.npy`` in one directory, each np.save of a dict
{named_parameters() name: array}, which numpy stores as a pickled 0-d object array.  ``load_weights`` reads them through
an unpickler that resolves only numpy's own array-rebuilding callables (the allow-list approach of legacy.py): nothing in
the file is imported or executed, and a payload that is not a dict of numeric arrays is refused.
"""
import collections
import os
import pickle

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

NAMES = ("pnet", "rnet", "onet")


class Flatten(nn.Module):
    def forward(self, x):
        return x.transpose(3, 2).contiguous().view(x.size(0), -1)


def _features(spec):
    """spec: (name, 'conv', cin, cout, k) | (name, 'pool', k) | (name, 'flatten') | (name, 'fc', cin, cout); a PReLU
    named prelu<i> follows every conv<i> / fc."""
    layers = collections.OrderedDict()
    for item in spec:
        name, kind = item[0], item[1]
        if kind == "conv":
            layers[name] = nn.Conv2d(item[2], item[3], item[4], 1)
            layers["prelu" + name[4:]] = nn.PReLU(item[3])
        elif kind == "pool":
            layers[name] = nn.MaxPool2d(item[2], 2, ceil_mode=True)
        elif kind == "flatten":
            layers[name] = Flatten()
        else:
            layers[name] = nn.Linear(item[2], item[3])
            layers["prelu" + name[4:]] = nn.PReLU(item[3])
    return nn.Sequential(layers)


class PNet(nn.Module):
    """Fully convolutional, 12-px receptive field, stride 2: [n, 3, h, w] -> (offsets [n, 4, h', w'], probs [n, 2, h', w'])
    with h' = ceil((h - 2) / 2) - 4."""

    def __init__(self):
        super().__init__()
        self.features = _features([("conv1", "conv", 3, 10, 3), ("pool1", "pool", 2), ("conv2", "conv", 10, 16, 3),
                                   ("conv3", "conv", 16, 32, 3)])
        self.conv4_1 = nn.Conv2d(32, 2, 1, 1)
        self.conv4_2 = nn.Conv2d(32, 4, 1, 1)

    def forward(self, x):
        x = self.features(x)
        return self.conv4_2(x), F.softmax(self.conv4_1(x), dim=1)


class RNet(nn.Module):
    """[n, 3, 24, 24] -> (offsets [n, 4], probs [n, 2])."""

    def __init__(self):
        super().__init__()
        self.features = _features([("conv1", "conv", 3, 28, 3), ("pool1", "pool", 3), ("conv2", "conv", 28, 48, 3),
                                   ("pool2", "pool", 3), ("conv3", "conv", 48, 64, 2), ("flatten", "flatten"),
                                   ("conv4", "fc", 576, 128)])
        self.conv5_1 = nn.Linear(128, 2)
        self.conv5_2 = nn.Linear(128, 4)

    def forward(self, x):
        x = self.features(x)
        return self.conv5_2(x), F.softmax(self.conv5_1(x), dim=1)


class ONet(nn.Module):
    """[n, 3, 48, 48] -> (landmarks [n, 10], offsets [n, 4], probs [n, 2])."""

    def __init__(self):
        super().__init__()
        self.features = _features([("conv1", "conv", 3, 32, 3), ("pool1", "pool", 3), ("conv2", "conv", 32, 64, 3),
                                   ("pool2", "pool", 3), ("conv3", "conv", 64, 64, 3), ("pool3", "pool", 2),
                                   ("conv4", "conv", 64, 128, 2), ("flatten", "flatten"), ("conv5", "fc", 1152, 256)])
        self.conv6_1 = nn.Linear(256, 2)
        self.conv6_2 = nn.Linear(256, 4)
        self.conv6_3 = nn.Linear(256, 10)

    def forward(self, x):
        x = self.features(x)
        return self.conv6_3(x), self.conv6_2(x), F.softmax(self.conv6_1(x), dim=1)


NETS = {"pnet": PNet, "rnet": RNet, "onet": ONet}


# ------------------------------------------------------------------------------------------------ weight files

def _numpy_callable(*paths):
    for path in paths:
        mod, _, name = path.rpartition(".")
        try:
            return getattr(__import__(mod, fromlist=[name]), name)
        except (ImportError, AttributeError):
            continue
    raise ImportError(paths[0])


class _ArrayUnpickler(pickle.Unpickler):
    """Resolves numpy's array-rebuilding callables and nothing else (numpy < 2 names the module numpy.core, >= 2
    numpy._core)."""
    _ALLOWED = {}
    for _mod in ("numpy.core.multiarray", "numpy._core.multiarray"):
        _ALLOWED[(_mod, "_reconstruct")] = _numpy_callable("numpy._core.multiarray._reconstruct",
                                                           "numpy.core.multiarray._reconstruct")
        _ALLOWED[(_mod, "scalar")] = _numpy_callable("numpy._core.multiarray.scalar", "numpy.core.multiarray.scalar")
    _ALLOWED[("numpy", "ndarray")] = np.ndarray
    _ALLOWED[("numpy", "dtype")] = np.dtype

    def find_class(self, module, name):
        fn = self._ALLOWED.get((module, name))
        if fn is None:
            raise pickle.UnpicklingError(f"MTCNN weight file references {module}.{name}: not on the allow-list (loading "
                                         f"never imports or executes code from the file)")
        return fn

    def persistent_load(self, pid):
        raise pickle.UnpicklingError("persistent ids are not used by MTCNN weight files")


def load_weight_file(path):
    """{name: float32 array} from one .npy written by np.save(path, dict)."""
    with open(path, "rb") as f:
        version = np.lib.format.read_magic(f)
        if version == (1, 0):
            shape, _, dtype = np.lib.format.read_array_header_1_0(f)
        elif version == (2, 0):
            shape, _, dtype = np.lib.format.read_array_header_2_0(f)
        else:
            raise ValueError(f"{path}: npy format version {version}")
        if not dtype.hasobject or shape != ():
            raise ValueError(f"{path}: expected a pickled dict (0-d object array), got shape {shape} dtype {dtype}")
        obj = _ArrayUnpickler(f).load()
    if isinstance(obj, np.ndarray) and obj.dtype == object and obj.shape == ():
        obj = obj[()]
    if not isinstance(obj, dict):
        raise ValueError(f"{path}: payload is {type(obj).__name__}, not a dict of arrays")
    out = {}
    for k, v in obj.items():
        if not isinstance(k, str) or not isinstance(v, np.ndarray) or v.dtype.kind not in "fiu":
            raise ValueError(f"{path}: entry {k!r} is not a numeric array")
        out[k] = np.ascontiguousarray(v, dtype=np.float32)
    return out


def save_weight_file(path, weights):
    """The reference's format: np.save of a dict of arrays (written with open(): np.save would append '.npy')."""
    with open(path, "wb") as f:
        np.save(f, {k: np.asarray(v, dtype=np.float32) for k, v in weights.items()}, allow_pickle=True)


def load_weights(directory):
    """{'pnet': {...}, 'rnet': {...}, 'onet': {...}} from <directory>/{pnet,rnet,onet}.npy."""
    return {n: load_weight_file(os.path.join(directory, n + ".npy")) for n in NAMES}


def build_net(name, weights):
    """The torch module ``name`` with ``weights`` ({parameter name: array}), eval mode, frozen."""
    net = NETS[name]()
    params = dict(net.named_parameters())
    if sorted(params) != sorted(weights):
        raise ValueError(f"{name}: weight names {sorted(weights)} do not match the net's {sorted(params)}")
    for k, p in params.items():
        w = torch.as_tensor(np.asarray(weights[k]), dtype=torch.float32)
        if w.shape != p.shape:
            raise ValueError(f"{name}.{k}: shape {tuple(w.shape)}, expected {tuple(p.shape)}")
        p.data = w.clone()
    return net.eval().requires_grad_(False)


class TorchMTCNN:
    """The three torch nets behind detect_faces' net interface (numpy in, numpy out), on the CPU."""

    def __init__(self, weights, dtype=torch.float32):
        self.dtype = dtype
        self.nets = {n: build_net(n, weights[n]).to(dtype) for n in NAMES}

    def _run(self, name, x):
        with torch.no_grad():
            out = self.nets[name](torch.as_tensor(x).to(self.dtype))
        return tuple(o.float().numpy() for o in out)

    def pnet(self, x):
        return self._run("pnet", x)

    def rnet(self, x):
        return self._run("rnet", x)

    def onet(self, x):
        return self._run("onet", x)
