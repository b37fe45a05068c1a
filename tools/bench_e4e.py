"""Timing of the e4e encoder (image -> W+) on the GPU at 256 px: trunk, FPN and heads separately, the heads as the
grouped kernel (smc_conv_s2_grouped_f32) against the composed per-conv calls (smc_conv_gemm_f32 / smc_linear_f32) and
against the grouped heads with the first fine level routed through one smc_conv_gemm_f32 call.  A report, not a gate.

    python tools/bench_e4e.py [--batches 1,4] [--reps 7] [--iters 20] [--out profiles/e4e/bench_e4e.txt]

Seeded synthetic encoder (synthetic.e4e_state_dict, seed 5) and seeded inputs.  All variants run interleaved in one
process: per batch one warm-up call of each, then `reps` repetitions, each timing `iters` back-to-back calls of every
variant in turn with device events (host launch overhead is inside the window: that is what a user waits for).  Per
variant: the median over repetitions of the per-call time and its min..max; for the heads also the ratio to the
grouped heads per repetition (median, min..max): a difference counts when it exceeds that spread.  Every launch of
the default heads is also timed alone (recorded from one pass, replayed) against its own floor.

Algorithmic bytes and FLOPs come from the shapes (live taps only: the taps that touch the plane; weights once,
activations in and out once).  The heads' floor is, per launch, the larger of bytes / 6.29 TB/s (the measured copy
rate) and FLOPs / 157.3 TF/s (the fp32 MFMA peak), summed over the launches; the report says which bound holds where.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylemc_amd import build, e4e_hip, modconv  # noqa: E402

PEAK_TF, COPY_TBS = 157.3, 6.29
SIZE = 256


def make_pack(net, grouped, fine0_gemm):
    """A packed encoder for one setting of the module switches (the product keeps one at a time; the bench keeps all)."""
    old = e4e_hip.GROUPED, e4e_hip.FINE0_GEMM
    e4e_hip.GROUPED, e4e_hip.FINE0_GEMM = grouped, fine0_gemm
    try:
        net.packed(SIZE)  # (packs the trunk once)
        return e4e_hip._PackedE4E(net.encoder, next(net.encoder.parameters()).device, SIZE, net._trunks[SIZE])
    finally:
        e4e_hip.GROUPED, e4e_hip.FINE0_GEMM = old


def head_launches(pk, n):
    """(name, weight bytes, activation bytes, flops) of every head launch of the grouped form, from the shapes."""
    out = []
    for fi, (lo, hi, levels) in enumerate(pk.families):
        G = hi - lo
        for li, lv in enumerate(levels):
            T = len(lv.taps)
            wb = 4 * G * T * lv.cin * lv.cout
            ab = 4 * n * ((1 if li == 0 else G) * lv.cin * lv.h * lv.h + G * lv.cout * lv.oh * lv.oh)
            fl = 2.0 * G * n * lv.oh * lv.oh * lv.cout * lv.cin * T
            out.append((f"{('coarse', 'middle', 'fine')[fi]} L{li} G{G} {lv.h}->{lv.oh} T{T}", wb, ab, fl))
    count = pk.lin_wk.shape[0]
    out.append((f"linear G{count}", 4 * count * 512 * 512, 4 * 2 * count * n * 512, 2.0 * count * n * 512 * 512))
    return out


def time_calls(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / iters  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_e4e: needs a GPU (no number is produced without one)")
    build.build(verbose=False)
    dev = "cuda"
    net = e4e_hip.build_e4e(seed=5, device=dev)
    packs = {"grouped": make_pack(net, True, False), "composed": make_pack(net, False, False),
             "grouped+fine0 gemm": make_pack(net, True, True)}
    lines = [f"# bench_e4e: {SIZE} px, {args.reps} repetitions x {args.iters} calls, device events, interleaved; "
             f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs",
             f"# floors: bytes / {COPY_TBS} TB/s (measured copy rate), FLOPs / {PEAK_TF} TF/s (fp32 MFMA peak); "
             "all times measured here, all bytes / FLOPs computed from shapes"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    print("\n".join(lines), flush=True)
    for n in [int(b) for b in args.batches.split(",")]:
        x = torch.randn(n, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(n)).clamp_(-1, 1).to(dev)
        pk0 = packs["grouped"]
        c1, c2, c3 = net.trunk(x, pk0)
        p2, p1 = net.fpn(c1, c2, c3, pk0)
        fine0 = pk0.families[2][2][0]
        cat = packs["grouped+fine0 gemm"].families[2][2][0]
        G = fine0.groups
        y_g = torch.empty(G, n, fine0.cout, fine0.oh, fine0.oh, device=dev)
        y_c = torch.empty(n, G * fine0.cout, fine0.oh, fine0.oh, device=dev)
        plane = fine0.cin * fine0.h * fine0.h
        variants = {
            "trunk": lambda: net.trunk(x, pk0),
            "fpn": lambda: net.fpn(c1, c2, c3, pk0),
            "heads grouped": lambda: net.heads(c3, p2, p1, packs["grouped"]),
            "heads composed": lambda: net.heads(c3, p2, p1, packs["composed"]),
            "heads grouped+fine0 gemm": lambda: net.heads(c3, p2, p1, packs["grouped+fine0 gemm"]),
            "fine L0 grouped kernel": lambda: e4e_hip.grouped_conv(p1, plane, 0, G, n, fine0.cin, fine0.h, fine0.h,
                                                                   fine0.wk, fine0.taps_c, fine0.bias, 0.01, y_g,
                                                                   fine0.cout),
            "fine L0 conv_gemm cout=5632": lambda: modconv.gemm(p1, y_c, cat.phase_cat, 1, cat.cin, G * cat.cout,
                                                                epi=e4e_hip._bias_epi(cat.bias_cat, "lrelu", 0.01)),
        }
        for fn in variants.values():  # warm-up: code objects, allocator
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                times[k].append(time_calls(fn, args.iters))
        # outputs of the three head forms agree (reordered fp32 sums only)
        h = {k: net.heads(c3, p2, p1, pk) for k, pk in packs.items()}
        torch.cuda.synchronize()
        scale = h["grouped"].abs().max().item()
        diffs = {k: (v - h["grouped"]).abs().max().item() / scale for k, v in h.items() if k != "grouped"}

        launches = head_launches(pk0, n)
        wb = sum(l[1] for l in launches)
        ab = sum(l[2] for l in launches)
        fl = sum(l[3] for l in launches)
        floor = 0.0
        emit(f"\n## batch {n}")
        emit(f"# heads, algorithmic: {len(launches)} launches, weights {wb / 1e6:.1f} MB, activations {ab / 1e6:.1f} MB, "
             f"{fl / 1e9:.2f} GFLOP")
        for name, w_, a_, f_ in launches:
            tb, tf = (w_ + a_) / (COPY_TBS * 1e12) * 1e6, f_ / (PEAK_TF * 1e12) * 1e6
            floor += max(tb, tf)
            emit(f"#   {name:32s} {(w_ + a_) / 1e6:8.1f} MB {f_ / 1e9:8.2f} GFLOP  floor {max(tb, tf):7.1f} us "
                 f"({'bytes' if tb >= tf else 'FLOPs'})")
        emit(f"# heads floor (sum of per-launch floors): {floor:.1f} us")
        emit(f"# {'part':30s} {'us / call median (min..max)':>34s}")
        for k, v in times.items():
            emit(f"  {k:30s} {statistics.median(v):12.1f} ({min(v):.1f}..{max(v):.1f})")
        base = times["heads grouped"]
        for k in ("heads composed", "heads grouped+fine0 gemm"):
            r = [a / b for a, b in zip(times[k], base)]
            emit(f"  {k + ' / heads grouped':44s} {statistics.median(r):6.3f} ({min(r):.3f}..{max(r):.3f}) per repetition")
        r = [a / b for a, b in zip(times["fine L0 conv_gemm cout=5632"], times["fine L0 grouped kernel"])]
        emit(f"  {'fine L0 conv_gemm / grouped kernel':44s} {statistics.median(r):6.3f} ({min(r):.3f}..{max(r):.3f}) "
             "per repetition")
        l0 = launches[[l[0].startswith("fine L0") for l in launches].index(True)]
        emit(f"  fine L0: {l0[3] / 1e9:.2f} GFLOP -> grouped kernel {l0[3] / statistics.median(times['fine L0 grouped kernel']) / 1e6:.1f} "
             f"TF/s, conv_gemm {l0[3] / statistics.median(times['fine L0 conv_gemm cout=5632']) / 1e6:.1f} TF/s "
             f"(peak {PEAK_TF})")
        for k in ("heads grouped", "heads composed", "heads grouped+fine0 gemm"):
            emit(f"  {k:30s} floor / time = {floor / statistics.median(times[k]):.3f}")
        # every launch of the default heads (grouped + fine L0 through conv_gemm) on its own: the calls are recorded
        # from one pass through net.heads and replayed, each timed over `iters` back-to-back calls
        calls = []
        orig_g, orig_m = e4e_hip.grouped_conv, modconv.gemm
        e4e_hip.grouped_conv = lambda *a, **k: (calls.append(lambda: orig_g(*a, **k)), orig_g(*a, **k))
        modconv.gemm = lambda *a, **k: (calls.append(lambda: orig_m(*a, **k)), orig_m(*a, **k))
        try:
            net.heads(c3, p2, p1, packs["grouped+fine0 gemm"])
        finally:
            e4e_hip.grouped_conv, modconv.gemm = orig_g, orig_m
        assert len(calls) == len(launches), (len(calls), len(launches))
        emit(f"# per launch (default heads), us / call median of 3 x {args.iters} (floor, floor / time)")
        total = 0.0
        for (name, w_, a_, f_), fn in zip(launches, calls):
            t = statistics.median(time_calls(fn, args.iters) for _ in range(3))
            fl_ = max((w_ + a_) / (COPY_TBS * 1e12), f_ / (PEAK_TF * 1e12)) * 1e6
            total += t
            emit(f"  {name:32s} {t:8.1f} us  (floor {fl_:6.1f} us, {fl_ / t:.2f})")
        emit(f"  sum of the launches timed alone: {total:.1f} us")
        emit(f"  max |heads - grouped heads| / max: " + ", ".join(f"{k} {d:.1e}" for k, d in diffs.items()))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
