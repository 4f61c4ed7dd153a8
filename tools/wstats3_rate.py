"""Time the wide stats-kmers-3 (mf_stats_kmers3_wide_tables, mf_wstats.hip) on a synthetic cohort at k = 33 and k = 63, next to the wide two-group
stats-kmers (mf_stats_kmers_wide_tables) on the SAME samples: groups A and B of the three-group run against A and B + C of the two-group run, so
both calls read every sample.

The cohort is tools/wstats_rate.py's with a third group: --n samples a group of --reads reads each (four fifths from a genome all samples share,
one fifth from the group's own genome), counted by the library; both calls run on the tables resident in HBM.  One warm-up, then --steps repeats,
device-synchronised wall time, the median is reported.  The per-kernel times ([launches, total ms]) are the library's HIP-event timers (option
profile = 1) over one more repeat.  Every row is printed as soon as it is measured.

    python tools/wstats3_rate.py --n 5 --reads 1000000 > profiles/wstats3_rate.txt
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=5, help="samples in each of the three groups")
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--read-len", type=int, default=100)
ap.add_argument("--ks", type=int, nargs="+", default=[33, 63])
ap.add_argument("--max-bad", type=int, default=1)
ap.add_argument("--steps", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metafast_amd import lib as L  # noqa: E402

GENOMES = (0x41414141, 0x42424242, 0x43434343)


def synth_table(ctx, j, group, k):
    n1 = args.reads * 4 // 5
    n2 = args.reads - n1
    rl = args.read_len
    bases = torch.zeros(args.reads * rl + 64, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(args.reads + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads_device(0x5354415453, j, 0, n1, rl, 1_000_000, bases.data_ptr(), offs.data_ptr())
    ctx.synth_reads_device(GENOMES[group], 0, j * n2, n2, rl, 100_000, bases.data_ptr() + n1 * rl, offs[n1:].data_ptr())
    offs[n1:] += n1 * rl
    t = ctx.count_wide_table(bases.data_ptr(), offs.data_ptr(), args.reads, args.reads * rl, k, 0)
    torch.cuda.synchronize()
    return t


def timed(fn, steps):
    times, out = [], None
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times, out


def profiled(ctx, fn):
    ctx.set_option("profile", 1)
    ctx.reset_timers()
    out = fn()
    torch.cuda.synchronize()
    rep = {name: [n, round(ms, 3)] for name, (n, ms, mx) in sorted(ctx.kernel_report().items()) if n}
    ctx.set_option("profile", 0)
    return rep, out


def shares(km):
    """where the time goes, as shares of the kernels' total: the union's gather, the sorts, the union's reduce, the column gather, the row kernels"""
    total = sum(ms for _, ms in km.values())
    part = lambda *names: sum(km[n][1] for n in names if n in km)
    return dict(kernels_ms=round(total, 3), union_gather=round(part("k_wj_gather") / total, 3), sorts=round(part("k_radix_sort") / total, 3),
                union_reduce=round(part("k_wj_reduce", "k_wj_reduce_groups") / total, 3), column_gather=round(part("k_wstats_gather") / total, 3),
                rows=round(part("k_stats_rows_thread", "k_stats_rows_wave", "k_stats3_rows_thread", "k_stats3_rows_wave") / total, 3))


def measure(ctx, k):
    groups = [[synth_table(ctx, g * args.n + j, g, k) for j in range(args.n)] for g in range(3)]
    every = groups[0] + groups[1] + groups[2]
    base = dict(k=k, samples=3 * args.n, reads_per_sample=args.reads, max_bad=args.max_bad, steps=args.steps, entries=sum(t.stats()[0] for t in every))

    def three():
        *tabs, ctr = ctx.stats_kmers3_wide(*groups, max_bad=args.max_bad)
        for t in tabs:
            t.close()
        return ctr

    def two():
        *tabs, ctr = ctx.stats_kmers_wide(groups[0], groups[1] + groups[2], max_bad=args.max_bad)
        for t in tabs:
            t.close()
        return ctr
    rows = []
    for name, fn in (("mf_stats_kmers3_wide_tables", three), ("mf_stats_kmers_wide_tables", two)):
        fn()                                                   # warm-up (arena, code objects)
        times, ctr = timed(fn, args.steps)
        res = dict(base, call=name, counters=ctr, wall_s=[round(t, 4) for t in times], wall_s_median=round(statistics.median(times), 4))
        res["kernel_ms"], _ = profiled(ctx, fn)
        res["shares"] = shares(res["kernel_ms"])
        print(json.dumps(res), flush=True)
        rows.append(res)
    print("# k = %d: three groups %.4f s, %.2f x the two-group call on the same samples (%.4f s)" %
          (k, rows[0]["wall_s_median"], rows[0]["wall_s_median"] / rows[1]["wall_s_median"], rows[1]["wall_s_median"]), flush=True)
    for t in every:
        t.close()


def main():
    ctx = L.Context(0, stream=torch.cuda.current_stream())
    for k in args.ks:
        measure(ctx, k)


if __name__ == "__main__":
    main()
