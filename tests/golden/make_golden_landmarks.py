"""Generate tests/golden/landmarks.npz by running the REFERENCE's own MTCNN package and crop_face on the CPU.

Run where the reference tree is present, never on the GPU box:

    python tests/golden/make_golden_landmarks.py

What is imported from the reference (read-only, CPU): ``MTCNN`` (detector, first_stage, box_utils, get_nets) and
``warp_images.crop_face`` and ``align_faces.align_face``.  warp_images and align_faces import cv2, matplotlib, torchvision, utils and mobilenet_facial at module level;
none is installed / needed for crop_face's tensor path, so they are import-only stubs (nothing stubbed is called).  The
reference's nets read ``MTCNN/weights/{pnet,rnet,onet}.npy`` relative to the working directory in their constructors:
the seeded synthetic weights (synthetic.mtcnn_weights) are written into a temporary directory in that layout and the
script changes into it, so the unmodified classes load them.

Recorded: the host functions' outputs on the seeded inputs of landmarks_inputs.py (nms in both modes, calibrate_box,
convert_to_square, correct_bboxes, _generate_bboxes), the pyramid's scale list, the three nets' outputs on seeded
inputs, one end-to-end detect_faces run (every net call's outputs in call order, and the result), crop_face on the
tensor path, and ``align_faces.align_face`` on seeded photographs with seeded 68 points at output_size 64,
transform_size 256: one case that pads and one that does not (with the Pillow version that resized them).

Condition (asserted; the seed of weights and image is searched until it holds): in the end-to-end run every thresholded
probability and every NMS overlap is at least 1e-3 from its threshold, every value passed to np.round is at least 1e-3
from a tie, every ceil argument at least 1e-3 from an integer, and at least three faces come out.  The GPU nets differ
from the reference's by about 1e-6, so the end-to-end GPU test may skip no box.
"""
import math
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.append(REF)   # after the repository: only names the repository lacks (MTCNN, warp_images) resolve there


class _Absent:
    def __init__(self, *a, **k):
        raise RuntimeError("import-only stub: not available offline")


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


_stub("cv2")
_stub("matplotlib").pyplot = _stub("matplotlib.pyplot")
_tv = _stub("torchvision")
_tv.transforms = _stub("torchvision.transforms", Compose=_Absent, Resize=_Absent, CenterCrop=_Absent)
_tv.models = _stub("torchvision.models", mobilenet_v2=_Absent)
_stub("utils", get_mean_std=_Absent)
_stub("mobilenet_facial", MobileNet_GDConv=_Absent)

import landmarks_inputs as LI                       # noqa: E402
from stylemc_amd import synthetic                   # noqa: E402
from stylemc_amd.MTCNN import get_nets as own_nets  # noqa: E402


def write_weights(seed, root):
    d = os.path.join(root, "MTCNN", "weights")
    os.makedirs(d, exist_ok=True)
    for name, wts in synthetic.mtcnn_weights(seed=seed).items():
        own_nets.save_weight_file(os.path.join(d, name + ".npy"), wts)


class _NumpyProbe:
    """numpy with round() recording how far its arguments are from a tie."""

    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        return getattr(np, name)

    def round(self, x, *a, **k):
        v = np.asarray(x, dtype=np.float64)
        if v.size:
            self._log.append(float(np.abs(np.abs(v - np.floor(v)) - 0.5).min()))
        return np.round(x, *a, **k)


class _MathProbe:
    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        return getattr(math, name)

    def ceil(self, x):
        self._log.append(abs(x - round(x)))
        return math.ceil(x)


def nms_margin(boxes, thr, mode):
    """The greedy loop of nms once more, returning min |overlap - threshold| over every comparison it makes."""
    x1, y1, x2, y2, score = (boxes[:, i] for i in range(5))
    area = (x2 - x1 + 1.0) * (y2 - y1 + 1.0)
    ids, margin = np.argsort(score), np.inf
    while len(ids) > 0:
        i, rest = ids[-1], ids[:-1]
        w = np.maximum(0.0, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + 1.0)
        h = np.maximum(0.0, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + 1.0)
        inter = w * h
        ov = inter / (np.minimum(area[i], area[rest]) if mode == "min" else area[i] + area[rest] - inter)
        if ov.size:
            margin = min(margin, float(np.abs(ov - thr).min()))
        ids = rest[~(ov > thr)]
    return margin


def end_to_end(seed, root):
    """One reference detect_faces run with seeded weights and image; returns (record dict, margins dict) or None."""
    write_weights(seed, root)
    os.chdir(root)
    import MTCNN.box_utils as rb
    import MTCNN.detector as rd
    import MTCNN.first_stage as rf
    calls, rounds, ceils, nms_m, scales = [], [], [], [], []

    def recording(cls, tag):
        class Rec(cls):
            def forward(self, x):
                out = super().forward(x)
                calls.append((tag, [o.detach().numpy().copy() for o in out]))
                return out
        return Rec

    orig = (rd.PNet, rd.RNet, rd.ONet, rd.nms, rf.nms, rd.run_first_stage, rd.np, rf.np, rf.math)
    ref_nms = rb.nms

    def nms_probe(boxes, overlap_threshold=0.5, mode="union"):
        if len(boxes):
            nms_m.append(nms_margin(np.asarray(boxes, dtype=np.float64), overlap_threshold, mode))
        return ref_nms(boxes, overlap_threshold, mode)

    def first_stage_probe(image, net, scale, threshold, device="cuda"):
        scales.append(scale)
        return orig[5](image, net, scale=scale, threshold=threshold, device=device)

    rd.PNet, rd.RNet, rd.ONet = recording(orig[0], "pnet"), recording(orig[1], "rnet"), recording(orig[2], "onet")
    rd.nms = rf.nms = nms_probe
    rd.run_first_stage = first_stage_probe
    rd.np, rf.np, rf.math = _NumpyProbe(rounds), _NumpyProbe(rounds), _MathProbe(ceils)
    try:
        img = torch.from_numpy(LI.detect_image(seed).astype(np.float32))
        try:
            boxes, lms = rd.detect_faces(img, thresholds=list(LI.THRESHOLDS), nms_thresholds=list(LI.NMS_THRESHOLDS),
                                         device="cpu")
        except ValueError:
            return None
    finally:
        rd.PNet, rd.RNet, rd.ONet, rd.nms, rf.nms, rd.run_first_stage, rd.np, rf.np, rf.math = orig
    if len(boxes) < 3:
        return None
    thr_m = []
    for tag, outs in calls:
        p = outs[-1][:, 1]
        thr_m.append(float(np.abs(p - LI.THRESHOLDS[("pnet", "rnet", "onet").index(tag)]).min()))
    margins = {"threshold": min(thr_m), "nms": min(nms_m), "round": min(rounds), "ceil": min(ceils)}
    rec = {"e2e/seed": np.array(seed), "e2e/boxes": np.asarray(boxes), "e2e/landmarks": np.asarray(lms),
           "e2e/scales": np.array(scales), "e2e/ncalls": np.array(len(calls))}
    for i, (tag, outs) in enumerate(calls):
        rec[f"e2e/call{i}/net"] = np.array(tag)
        for j, o in enumerate(outs):
            rec[f"e2e/call{i}/out{j}"] = o
    return rec, margins


def main():
    out = {}
    root = tempfile.mkdtemp(prefix="landmarks_golden_")
    cwd = os.getcwd()
    try:
        found = None
        for seed in range(200):
            res = end_to_end(seed, root)
            if res is None:
                continue
            rec, margins = res
            print(f"seed {seed}: {len(rec['e2e/boxes'])} faces, margins {margins}")
            if min(margins.values()) >= LI.MARGIN:
                found = rec
                break
        assert found is not None, "no seed satisfies the margin condition"
        assert min(margins.values()) >= LI.MARGIN and len(found["e2e/boxes"]) >= 3
        out.update(found)
        seed = int(found["e2e/seed"])
        out["e2e/margins"] = np.array([margins[k] for k in ("threshold", "nms", "round", "ceil")])

        import MTCNN.box_utils as rb
        import MTCNN.first_stage as rf
        import MTCNN.get_nets as rn
        from warp_images import crop_face

        # host functions on seeded inputs (each gets its own copy: several of them write into their argument)
        boxes, offs = LI.host_boxes(), LI.host_offsets()
        out["host/nms_union"] = np.array(rb.nms(boxes.copy(), 0.5, "union"))
        out["host/nms_min"] = np.array(rb.nms(boxes.copy(), 0.7, "min"))
        out["host/calibrate_box"] = rb.calibrate_box(boxes.copy(), offs)
        out["host/convert_to_square"] = rb.convert_to_square(boxes.copy())
        b = np.round(boxes.copy())
        out["host/correct_bboxes"] = np.stack(rb.correct_bboxes(b, 128, 96))
        out["host/correct_bboxes_arg"] = b   # the clipping writes through to the argument
        probs, poffs = LI.pnet_maps()
        out["host/generate_bboxes"] = rf._generate_bboxes(probs, poffs, 0.6 * 0.707, 0.55)
        assert out["host/generate_bboxes"].shape[0] > 10

        # the three nets (the weights of the end-to-end seed are still in place)
        with torch.no_grad():
            pnet, rnet, onet = rn.PNet().eval(), rn.RNet().eval(), rn.ONet().eval()
            for key, hw in LI.PNET_SHAPES.items():
                for j, o in enumerate(pnet(torch.from_numpy(LI.net_input("pnet", hw=hw)))):
                    out[f"nets/pnet/{key}/out{j}"] = o.numpy()
            for name, net in (("rnet", rnet), ("onet", onet)):
                for j, o in enumerate(net(torch.from_numpy(LI.net_input(name)))):
                    out[f"nets/{name}/out{j}"] = o.numpy()
        out["nets/seed"] = np.array(seed)

        # crop_face, tensor path
        img, faces = LI.crop_case()
        for key, f in faces.items():
            face, side, bbox = crop_face(img, f, 32)
            out[f"crop/{key}/face"] = face.numpy()
            out[f"crop/{key}/meta"] = np.array([side] + list(bbox))

        # align_face on seeded photographs and landmarks: one case that pads (and shrinks), one that does not.
        # align_faces.py names Image.ANTIALIAS, which current Pillow spells Image.LANCZOS (the same filter)
        from PIL import Image
        if not hasattr(Image, "ANTIALIAS"):
            Image.ANTIALIAS = Image.LANCZOS
        import PIL
        from align_faces import align_face
        for key in ("nopad", "pad"):
            img, lm = LI.align_case(key)
            out[f"align/{key}"] = np.asarray(align_face(img, lm, **LI.ALIGN_KW))
            assert out[f"align/{key}"].shape == (64, 64, 3)
        out["align/pillow"] = np.array(PIL.__version__)
    finally:
        os.chdir(cwd)
    out["versions"] = np.array(f"numpy {np.__version__} torch {torch.__version__}")
    path = os.path.join(HERE, "landmarks.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
