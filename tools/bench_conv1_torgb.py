"""Layer-level timing of a 32-channel block's conv1 + ToRGB forward, from x to (y, rgb): the two launches
(smc_conv3x3_wino_ws_f32 + smc_torgb_fwd_f32) against the fused launch (smc_modconv_conv1_torgb_f32) with y stored
(the edited branch: the backward reads y) and without (the no-grad original-image branch), at the FFHQ-1024 shape
(r = 1024, 32 -> 32 channels, 3 image channels).

    python tools/bench_conv1_torgb.py [--batch 4] [--reps 5] [--iters 20] [--res 1024]
Every repetition times `iters` back-to-back forwards of each path in turn (interleaved, same process); prints each
repetition's per-forward time and whether the paths' y / rgb are bit-equal.  On a tree from before the fused route it
times the pair alone (an A/B on one box).
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylemc_amd import build, modconv  # noqa: E402


class _Ctx:
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--channels", type=int, default=32)
    args = ap.parse_args()
    build.build(verbose=False)
    dev = "cuda"
    n, r, c = args.batch, args.res, args.channels
    W = torch.randn(c, c, 3, 3, device=dev)
    x = torch.randn(n, c, r, r, device=dev)
    s = torch.randn(n, c, device=dev) * 0.5 + 1
    noise = torch.randn(r, r, device=dev)
    strength = torch.tensor(0.1, device=dev)
    bias = torch.randn(c, device=dev) * 0.1
    w_rgb = torch.randn(3, c, device=dev) / math.sqrt(c)
    s_rgb = torch.randn(n, c, device=dev) * 0.5 + 1
    b_rgb = torch.randn(3, device=dev) * 0.1
    spec = modconv.LayerSpec(W, bias, 1, None, resolution=r)
    has_fused = hasattr(modconv, "fused_torgb_ok")

    def pair():
        y = modconv._modconv_fwd(_Ctx(), x, s, spec, noise, strength, math.sqrt(2), 256.0, True, False)[0]
        return y, modconv._torgb_fwd(y, s_rgb, w_rgb, b_rgb, 256.0)

    def fused(keep_y):
        # keep_y: the edited branch (dx needed: y saved); else no gradient and need_y False
        y, _, rgb = modconv._modconv_fwd(_Ctx(), x, s, spec, noise, strength, math.sqrt(2), 256.0, keep_y, False,
                                         torgb=(s_rgb, w_rgb, b_rgb, 256.0, False))
        assert rgb is not None and (y is not None) == keep_y, "the fused route did not take the layer"
        return y, rgb

    paths = [("pair", pair)]
    if has_fused:
        modconv.FUSED_TORGB = True
        paths += [("fused+y", lambda: fused(True)), ("fused", lambda: fused(False))]
    outs = {name: f() for name, f in paths}
    torch.cuda.synchronize()
    if has_fused:
        print(f"conv1_torgb r={r} y bit-equal: {torch.equal(outs['pair'][0], outs['fused+y'][0])}  rgb bit-equal: "
              f"{torch.equal(outs['pair'][1], outs['fused+y'][1])} / {torch.equal(outs['pair'][1], outs['fused'][1])}")
    del outs
    times = {name: [] for name, _ in paths}
    for _ in range(args.reps):
        for name, f in paths:
            f()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.iters)
    for name, _ in paths:
        t = times[name]
        print(f"conv1_torgb r={r:5d} n={n} c={c:3d} {name:8s} {' '.join(f'{v:7.1f}' for v in t)} us  "
              f"(min {min(t):.1f}, max {max(t):.1f})")


if __name__ == "__main__":
    main()
