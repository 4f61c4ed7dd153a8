"""Time kmers-color and component-colored (mf_color.hip, mf_cc.hip) on a synthetic cohort, next to their yardsticks: kmers-samples-counter
on the same tables (the same union with one word instead of three fields) and the component cutter on a table of as many k-mers with one
threshold level (one adjacency, one union-find pass).

The cohort is tools/stats_rate.py's: --n samples of --reads reads each, counted by the library at -k, classes dealt round-robin.  Every
stage runs on data resident in HBM: one warm-up, then --steps repeats, device-synchronised wall time, the median is reported; the
per-kernel times ([launches, total ms]) are the library's HIP-event timers (option profile = 1) over one more repeat of all stages.

    python tools/color_rate.py --n 64 --reads 400000 --out profiles/color_rate.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=16)
ap.add_argument("--reads", type=int, default=400_000)
ap.add_argument("--read-len", type=int, default=100)
ap.add_argument("-k", type=int, default=31)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--perc", type=float, default=0.9)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metafast_amd import lib as L  # noqa: E402


def synth_table(ctx, j, group):
    n1 = args.reads * 4 // 5
    n2 = args.reads - n1
    rl = args.read_len
    bases = torch.zeros(args.reads * rl + 64, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(args.reads + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads_device(0x5354415453, j, 0, n1, rl, 1_000_000, bases.data_ptr(), offs.data_ptr())
    ctx.synth_reads_device(0x41414141 + group, 0, j * n2, n2, rl, 100_000, bases.data_ptr() + n1 * rl, offs[n1:].data_ptr())
    offs[n1:] += n1 * rl
    t = ctx.count_device(bases.data_ptr(), offs.data_ptr(), args.reads, args.reads * rl, args.k, 0)
    torch.cuda.synchronize()
    return t


def timed(fn, steps):
    fn()                                                       # warm-up (arena, code objects)
    times = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return round(statistics.median(times), 4)


def main():
    ctx = L.Context(0, stream=torch.cuda.current_stream())
    classes = [j % 3 for j in range(args.n)]
    tabs = [synth_table(ctx, j, classes[j]) for j in range(args.n)]
    res = dict(samples=args.n, reads_per_sample=args.reads, k=args.k, steps=args.steps, entries=sum(len(t) for t in tabs))
    ct = ctx.kmers_color(tabs, classes, 1, False)
    keys, vals = ct.export()
    res["colored_kmers"] = len(ct)
    # the graph the driver would load: values above k
    keep = vals.astype(np.int64) > args.k
    graph = ctx.ctable_from_host(keys[keep], vals[keep], args.k)
    res["graph_kmers"] = len(graph)
    cutter = ctx.table_from_host(keys[keep], np.ones(int(keep.sum()), np.uint16), args.k)
    stages = {
        "kmers_color_s": lambda: ctx.kmers_color(tabs, classes, 1, False).close(),
        "kmers_color_val_s": lambda: ctx.kmers_color(tabs, classes, 1, True).close(),
        "yardstick_kmers_samples_count_s": lambda: ctx.kmers_samples_count(tabs, 1).close(),
        "component_colored_s": lambda: [c.close() for c in ctx.colored_components(graph, 3, False, args.perc)],
        "component_colored_separate_s": lambda: [c.close() for c in ctx.colored_components(graph, 3, True, args.perc)],
        "yardstick_cut_components_one_level_s": lambda: ctx.cut_components(cutter, 1, 1 << 30).close(),
    }
    for name, fn in stages.items():
        res[name] = timed(fn, args.steps)
    res["components"] = [len(c) for c in ctx.colored_components(graph, 3, False, args.perc)]
    ctx.set_option("profile", 1)                               # one more repeat under the event timers (they are off for the wall times)
    res["kernel_ms"] = {}
    for name, fn in stages.items():
        ctx.reset_timers()
        fn()
        torch.cuda.synchronize()
        res["kernel_ms"][name] = {kn: [n, round(ms, 3)] for kn, (n, ms, mx) in sorted(ctx.kernel_report().items()) if n}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
