"""Timing of the convolution weight gradient: smc_conv_wgrad_f32 against torch.nn.grad.conv2d_weight (MIOpen) on the
GPU, at the FFHQ-1024 conv1 shapes from 64 px up and the two transposed pairs of the 512 / 1024-px conv0.  A report,
not a gate.

    python tools/bench_wgrad.py [--batch 4] [--reps 5] [--iters 20] [--out profiles/wgrad/bench_wgrad.txt]

Both paths run interleaved in one process on seeded N(0, 1) operands: per shape one warm-up call of each, then `reps`
repetitions that time `iters` back-to-back calls of each path in turn with device events.  Per shape it prints the
per-call time of every repetition's median and range, TF/s on 2 n cin cout out_h out_w taps, the share of the
157.3 TF/s fp32 MFMA peak, the split count, the ratio to MIOpen and the largest |ours - MIOpen| / max |MIOpen|.
The transposed pairs call both paths with the roles swapped (inp = dT, grad = x, stride 2, pad 0): the result
[x channels][dT channels][3][3] is the transposed conv's weight gradient in its own layout, and MIOpen is timed on
the same one backward-weight call as in the conv1 rows.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylemc_amd import _hip, build  # noqa: E402

PEAK_TF = 157.3

# (name, cin, cout, in_h, k, stride, pad, swap): cin / cout / in_h are the kernel's arguments
SHAPES = [
    ("conv1 512->512 64px", 512, 512, 64, 3, 1, 1, False),
    ("conv1 256->256 128px", 256, 256, 128, 3, 1, 1, False),
    ("conv1 128->128 256px", 128, 128, 256, 3, 1, 1, False),
    ("conv1 64->64 512px", 64, 64, 512, 3, 1, 1, False),
    ("conv1 32->32 1024px", 32, 32, 1024, 3, 1, 1, False),
    ("convT 128->64 256->512px", 64, 128, 513, 3, 2, 0, True),
    ("convT 64->32 512->1024px", 32, 64, 1025, 3, 2, 0, True),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wgrad: needs a GPU (no number is produced without one)")
    build.build(verbose=False)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    lib = _hip.load()
    dev, n = "cuda", args.batch
    lines = [f"# bench_wgrad: batch {n}, {args.reps} repetitions x {args.iters} calls, device events, interleaved; "
             f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs",
             f"# {'shape':26s} {'ours us (min..max)':>26s} {'TF/s':>6s} {'%peak':>6s} {'nsplit':>6s} "
             f"{'MIOpen us (min..max)':>28s} {'ours/MIOpen':>11s} {'max diff/max':>12s}"]
    print("\n".join(lines), flush=True)
    gen = torch.Generator().manual_seed(0)
    for name, cin, cout, ih, k, stride, pad, swap in SHAPES:
        oh = (ih + 2 * pad - k) // stride + 1
        inp = torch.randn(n, cin, ih, ih, generator=gen).to(dev)
        grad = torch.randn(n, cout, oh, oh, generator=gen).to(dev)
        nb = lib.smc_conv_wgrad_workspace_size(n, cin, cout, ih, ih, oh, oh, k, k, stride)
        ws = torch.empty(max(nb // 4, 1), device=dev)
        dw = torch.empty(cout, cin, k, k, device=dev)

        def ours():
            _hip.call("smc_conv_wgrad_f32", inp.data_ptr(), n, cin, ih, ih, grad.data_ptr(), cout, oh, oh, k, k,
                      stride, pad, pad, dw.data_ptr(), ws.data_ptr() if nb > 0 else None, nb, _hip.stream())
            return dw

        # the same single backward-weight call for every row: with the roles swapped the kernel computes exactly the
        # weight gradient of a stride-2 conv of dT whose output gradient is x
        def miopen():
            return torch.nn.grad.conv2d_weight(inp, (cout, cin, k, k), grad, stride=stride, padding=pad)

        a, b = ours().clone(), miopen()
        torch.cuda.synchronize()
        diff = ((a - b).abs().max() / b.abs().max()).item()
        nsplit = lib.smc_conv_wgrad_last_nsplit()
        times = {"ours": [], "miopen": []}
        for _ in range(args.reps):
            for key, fn in (("ours", ours), ("miopen", miopen)):
                fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) * 1e3 / args.iters)
        flops = 2.0 * n * cin * cout * oh * oh * k * k
        to, tm = statistics.median(times["ours"]), statistics.median(times["miopen"])
        tf = flops / (to * 1e-6) / 1e12
        line = (f"  {name:26s} {to:9.1f} ({min(times['ours']):7.1f}..{max(times['ours']):7.1f}) {tf:6.1f} "
                f"{100 * tf / PEAK_TF:6.1f} {nsplit:6d} {tm:11.1f} ({min(times['miopen']):7.1f}..{max(times['miopen']):7.1f}) "
                f"{to / tm:11.2f} {diff:12.2e}")
        print(line, flush=True)
        lines.append(line)
        del inp, grad, ws, dw, a, b
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
