"""Layer-level timing of the up=2 modconv forward, from x to y, on both paths: the fused launch
(smc_modconv_up2_f32) against the transposed conv + FIR/epilogue pair, at the FFHQ-1024 conv0 shapes that take the
4-phase kernel (r = 512: 128 -> 64 channels, r = 1024: 64 -> 32), both product forms (the exact-fp32 form has no
fused kernel: its rows show the pair alone).  tools/bench_gemm.py's fwd_conv0 row times the GEMM alone.

    python tools/bench_up2.py [--batch 4] [--reps 5] [--iters 20] [--res 512,1024]
Every repetition times `iters` back-to-back layer forwards of each path in turn (interleaved, same process); prints
each repetition's per-launch time and whether the two paths' y are bit-equal.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylemc_amd import _hip, build, modconv  # noqa: E402


class _Ctx:
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--res", default="512,1024")
    args = ap.parse_args()
    build.build(verbose=False)
    saved = (getattr(modconv, "FUSED_UP", None), modconv.X3, getattr(modconv, "FUSED_UP_COUT", None))
    dev = "cuda"
    n = args.batch
    k = torch.tensor([1.0, 3.0, 3.0, 1.0])
    filt = torch.outer(k, k) / 64.0
    for r in [int(v) for v in args.res.split(",")]:
        cin, cout, h = min(32768 // (r // 2), 512), min(32768 // r, 512), r // 2
        W = torch.randn(cout, cin, 3, 3, device=dev)
        x = torch.randn(n, cin, h, h, device=dev)
        s = torch.randn(n, cin, device=dev) * 0.5 + 1
        noise = torch.randn(r, r, device=dev)
        strength = torch.tensor(0.1, device=dev)
        bias = torch.randn(cout, device=dev) * 0.1
        for x3 in (True, False):
            modconv.X3 = x3
            spec = modconv.LayerSpec(W, bias, 2, filt, resolution=r)

            def fwd(fused):
                modconv.FUSED_UP = fused
                # the frozen-style layers of the step: dx needed, styles not (no u store)
                return modconv._modconv_fwd(_Ctx(), x, s, spec, noise, strength, math.sqrt(2), 256.0, True, False)[0]

            # (a tree from before the fused route has no fused_up_ok: its pair alone, for an A/B on one box)
            modconv.FUSED_UP = True
            if saved[2] is not None:
                modconv.FUSED_UP_COUT = (32, 64)   # time both widths, whichever the routing takes by default
            ok = getattr(modconv, "fused_up_ok", None)
            paths = [("pair", False)] + ([("fused", True)] if ok is not None and ok(spec, n, cin, h, h) else [])
            ys = {name: fwd(f) for name, f in paths}
            torch.cuda.synchronize()
            same = torch.equal(ys["pair"], ys["fused"]) if "fused" in ys else None
            del ys
            times = {name: [] for name, _ in paths}
            for _ in range(args.reps):
                for name, f in paths:
                    fwd(f)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.iters):
                        fwd(f)
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / args.iters)
            form = "x3" if x3 else "fp32"
            for name, _ in paths:
                t = times[name]
                print(f"up2_fwd r={r:5d} cin={cin:4d} cout={cout:4d} {form:4s} {name:5s} "
                      f"{' '.join(f'{v:7.1f}' for v in t)} us  (min {min(t):.1f}, max {max(t):.1f})")
            if same is not None:
                print(f"up2_fwd r={r:5d} {form:4s} y bit-equal: {same}")
    modconv.X3 = saved[1]
    if saved[2] is not None:
        modconv.FUSED_UP = saved[0]
        modconv.FUSED_UP_COUT = saved[2]


if __name__ == "__main__":
    main()
