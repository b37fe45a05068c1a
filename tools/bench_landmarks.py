"""Timing of the face-landmark stack on the GPU.  A report, not a gate.

    python tools/bench_landmarks.py [--batches 1,8] [--reps 7] [--iters 20] [--out profiles/landmarks/bench_landmarks.txt]

Seeded synthetic nets (synthetic.mobilenet_state_dict seed 7, synthetic.mtcnn_weights seed 11) and seeded inputs.  Per
batch, with device events around `iters` back-to-back calls (host launch overhead inside the window), `reps` repetitions,
variants interleaved within a repetition:

  * every depthwise layer of the 224-px regressor (its real, channel-padded shapes, collected from one forward):
    smc_dwconv_f32 (conv + folded BN + ReLU6 in one launch) against the byte floor (input + output activations and
    weights once) / 6.29 TB/s -- the copy rate profiles/e4e/README.md uses -- and against the stock op of the installed
    torch, F.conv2d(groups=C) ALONE (without the BN and ReLU6 that the HIP launch includes), as a ratio per repetition;
  * the global depthwise layer (linear7) the same way;
  * the whole regressor;
and once: detect_faces on a 1024 x 1024 image, the device part (the nets' calls, device events summed) and the host part
(wall time minus the device part: pyramid resizes, box arithmetic, cut-outs, copies).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylemc_amd import build, mobilenet_hip, mtcnn_hip  # noqa: E402
from stylemc_amd.MTCNN import detector                   # noqa: E402

COPY_TBS = 6.29


def time_calls(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / iters  # us per call


def med(v):
    return f"{statistics.median(v):9.1f} ({min(v):.1f}..{max(v):.1f})"


class TimedNets:
    """HipMTCNN with device events around every net call."""

    def __init__(self, nets):
        self.nets, self.events, self.calls = nets, [], {"pnet": 0, "rnet": 0, "onet": 0}

    def _run(self, name, x):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = self.nets.run(name, x)
        e.record()
        self.events.append((s, e))
        self.calls[name] += x.shape[0]
        return tuple(o.contiguous().cpu().numpy() for o in out)

    def pnet(self, x):
        return self._run("pnet", x)

    def rnet(self, x):
        return self._run("rnet", x)

    def onet(self, x):
        return self._run("onet", x)

    def device_ms(self):
        torch.cuda.synchronize()
        return sum(s.elapsed_time(e) for s, e in self.events)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    build.build(verbose=False)
    dev = "cuda"
    lines = [f"# bench_landmarks: {args.reps} repetitions x {args.iters} calls, device events, interleaved; "
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    net = mobilenet_hip.build_mobilenet(None, seed=7, device=dev, input_size=224)
    pk = net.packed()
    for n in [int(b) for b in args.batches.split(",")]:
        g = torch.Generator().manual_seed(n)
        x = torch.randn(n, 3, 224, 224, generator=g).to(dev)
        layers = []
        xp = torch.zeros(n, pk.stem.cin, 224, 224, device=dev)
        xp[:, :3] = x
        feat = net.trunk(xp, pk, on_depthwise=lambda dw, h: layers.append((dw, h.clone())))
        layers.append((pk.linear7, feat.clone()))
        net(x)
        torch.cuda.synchronize()
        emit(f"\n## n = {n}")
        emit(f"# {'depthwise layer':34s} {'HIP us':>26s} {'floor us':>9s} {'floor/HIP':>9s} {'torch conv2d us':>26s} "
             f"{'HIP/torch per rep':>24s}")
        hip_t, ref_t = [[] for _ in layers], [[] for _ in layers]
        w4 = [dw.w.unsqueeze(1).contiguous() for dw, _ in layers]
        for i, (dw, h) in enumerate(layers):   # warm-up
            dw(h)
            F.conv2d(h, w4[i], stride=dw.stride, padding=dw.pad, groups=dw.c)
        for _ in range(args.reps):
            for i, (dw, h) in enumerate(layers):
                hip_t[i].append(time_calls(lambda: dw(h), args.iters))
                ref_t[i].append(time_calls(lambda: F.conv2d(h, w4[i], stride=dw.stride, padding=dw.pad, groups=dw.c),
                                           args.iters))
        tot_hip = tot_ref = tot_floor = 0.0
        for i, (dw, h) in enumerate(layers):
            oh = 1 if dw.pad == 0 else (h.shape[2] - 1) // dw.stride + 1
            nbytes = 4 * (h.numel() + n * dw.c * oh * oh + dw.w.numel() + 2 * dw.c)
            floor = nbytes / (COPY_TBS * 1e12) * 1e6
            ratio = [a / b for a, b in zip(hip_t[i], ref_t[i])]
            name = f"C{dw.c} {h.shape[2]}x{h.shape[3]} k{dw.k} s{dw.stride}" + (" global" if dw.pad == 0 else "")
            emit(f"  {name:34s} {med(hip_t[i]):>26s} {floor:9.2f} {floor / statistics.median(hip_t[i]):9.3f} "
                 f"{med(ref_t[i]):>26s} {statistics.median(ratio):8.3f} ({min(ratio):.3f}..{max(ratio):.3f})")
            tot_hip += statistics.median(hip_t[i])
            tot_ref += statistics.median(ref_t[i])
            tot_floor += floor
        emit(f"  {'all depthwise layers':34s} {tot_hip:9.1f} us HIP, {tot_ref:.1f} us torch conv2d alone, floor {tot_floor:.1f} us")
        whole = [time_calls(lambda: net(x), max(args.iters // 4, 3)) for _ in range(args.reps)]
        emit(f"  {'whole regressor (224 px)':34s} {med(whole):>26s} us / call")

    # detect_faces at 1024 x 1024
    rng = np.random.RandomState(0)
    yy, xx = np.mgrid[:1024, :1024]
    img = 127.5 + 80 * np.sin(xx / 37.0)[..., None] * np.cos(yy / 29.0)[..., None] + rng.normal(0, 20, (1024, 1024, 3))
    img = torch.from_numpy(np.clip(img, 0, 255).astype(np.float32)).to(dev)
    nets = mtcnn_hip.build_mtcnn("synthetic", device=dev, seed=11)
    thr = dict(thresholds=(0.6, 0.6, 0.6))  # (with the seeded nets: about 2000 boxes reach R-Net and 20 O-Net)
    detector.detect_faces(img, nets=nets, **thr)   # warm-up
    emit("\n## detect_faces, 1024 x 1024 (seeded nets: the box counts are not those of a trained detector)")
    for _ in range(3):
        timed = TimedNets(nets)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        boxes, _ = detector.detect_faces(img, nets=timed, **thr)
        wall = (time.perf_counter() - t0) * 1e3
        d = timed.device_ms()
        emit(f"  wall {wall:8.1f} ms, device part {d:7.1f} ms ({len(timed.events)} net calls; P-Net levels "
             f"{timed.calls['pnet']}, R-Net boxes {timed.calls['rnet']}, O-Net boxes {timed.calls['onet']}), host part "
             f"{wall - d:8.1f} ms, {len(boxes)} boxes")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
