"""Time specific-kmers and specific-kmers-3 next to stats-kmers and stats-kmers-3 on one resident synthetic cohort.  All four stream the
same samples through the same union pass; they differ in the select and row kernels and in how many k-mers reach the gather and row
passes (specific-kmers sends the k-mers of all samples on, and finds its scarce k-mers only in the row pass).

The cohort is tools/stats3_rate.py's: 32 samples of --reads reads each, counted by the library at k = 31; two groups are the halves
(16 + 16), three groups are --n3 (11 11 10).  Device-synchronised wall time, best of --steps after a warm-up; one more repeat under the
per-kernel event timers.  --root <checkout of another commit> measures that commit's stats-kmers / stats-kmers-3 (the yardsticks).

    python tools/specific_rate.py --what specific
    python tools/specific_rate.py --what specific3
    python tools/specific_rate.py --what stats --root ../parent
    python tools/specific_rate.py --what stats3 --root ../parent
Each run prints one JSON line; collect them in profiles/specific_rate.txt.
"""
import argparse
import json
import os
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--what", choices=("specific", "specific3", "stats", "stats3"), required=True)
ap.add_argument("--n3", type=int, nargs=3, default=(11, 11, 10))
ap.add_argument("--reads", type=int, default=2_000_000)
ap.add_argument("--read-len", type=int, default=100)
ap.add_argument("-k", type=int, default=31)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from metafast_amd import lib as L  # noqa: E402

SEEDS = (0x41414141, 0x42424242, 0x43434343)


def synth_table(ctx, j, group, n_reads, k, rl):
    n1 = n_reads * 4 // 5
    n2 = n_reads - n1
    bases = torch.zeros(n_reads * rl + 64, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(n_reads + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads_device(0x5354415453, j, 0, n1, rl, 1_000_000, bases.data_ptr(), offs.data_ptr())
    ctx.synth_reads_device(SEEDS[group], 0, j * n2, n2, rl, 100_000, bases.data_ptr() + n1 * rl, offs[n1:].data_ptr())
    offs[n1:] += n1 * rl
    t = ctx.count_device(bases.data_ptr(), offs.data_ptr(), n_reads, n_reads * rl, k, 0)
    torch.cuda.synchronize()
    return t


def main():
    ctx = L.Context(0, stream=torch.cuda.current_stream())
    N = sum(args.n3)
    group_of = [0] * args.n3[0] + [1] * args.n3[1] + [2] * args.n3[2]
    tabs = [synth_table(ctx, j, group_of[j], args.reads, args.k, args.read_len) for j in range(N)]
    a, b = args.n3[0], args.n3[0] + args.n3[1]
    fn = {"specific": lambda: ctx.specific_kmers(tabs[:N // 2], tabs[N // 2:])[-1],
          "specific3": lambda: ctx.specific_kmers3(tabs[:a], tabs[a:b], tabs[b:])[-1],
          "stats": lambda: ctx.stats_kmers(tabs[:N // 2], tabs[N // 2:])[-1],
          "stats3": lambda: ctx.stats_kmers3(tabs[:a], tabs[a:b], tabs[b:])[-1]}[args.what]
    fn()                                                       # warm-up (arena, code objects)
    times = []
    for _ in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctr = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    res = dict(what=args.what, root=os.path.abspath(args.root), samples=N, groups=list(args.n3) if args.what.endswith("3") else [N // 2, N - N // 2],
               reads_per_sample=args.reads, k=args.k, entries=sum(len(t) for t in tabs), counters=ctr, wall_s=[round(t, 4) for t in times],
               wall_s_best=round(min(times), 4))
    ctx.set_option("profile", 1)                               # one more repeat under the event timers (they are off for the wall times)
    ctx.reset_timers()
    fn()
    torch.cuda.synchronize()
    res["kernel_ms"] = {name: [n, round(ms, 3)] for name, (n, ms, mx) in sorted(ctx.kernel_report().items()) if n}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
