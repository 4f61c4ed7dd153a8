"""Time the wide stats-kmers (mf_stats_kmers_wide_tables and the file form mf_stats_kmers_wide, mf_wstats.hip) on a synthetic cohort at k = 33 and
k = 63, next to the k <= 31 call (mf_stats_kmers_tables, the hashed join of mf_stats.hip) at k = 31 on samples of the same reads.

The cohort is tools/wkps_rate.py's, in two groups: --n samples a group of --reads reads each (four fifths from a genome all samples share, one
fifth from the group's own genome), counted by the library.  The table form runs on the tables resident in HBM; for the file form every sample is
written once as a wide .kmers.bin into a temporary directory and the call streams them and writes its four files there.  One warm-up, then --steps
repeats, device-synchronised wall time, the median is reported.  The per-kernel times ([launches, total ms]) are the library's HIP-event timers
(option profile = 1): for the table form over one more repeat, for the file form over its warm-up.  Every row is printed as soon as it is measured.

    python tools/wstats_rate.py --n 8 --reads 1000000 > profiles/wstats_rate.txt
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8, help="samples in each of the two groups")
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--read-len", type=int, default=100)
ap.add_argument("--ks", type=int, nargs="+", default=[31, 33, 63])
ap.add_argument("--max-bad", type=int, default=1)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--no-files", action="store_true", help="the table form alone")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metafast_amd import lib as L  # noqa: E402


def synth_table(ctx, j, group, k):
    n1 = args.reads * 4 // 5
    n2 = args.reads - n1
    rl = args.read_len
    bases = torch.zeros(args.reads * rl + 64, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(args.reads + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads_device(0x5354415453, j, 0, n1, rl, 1_000_000, bases.data_ptr(), offs.data_ptr())
    ctx.synth_reads_device(0x41414141 if group == 0 else 0x42424242, 0, j * n2, n2, rl, 100_000, bases.data_ptr() + n1 * rl, offs[n1:].data_ptr())
    offs[n1:] += n1 * rl
    count = ctx.count_device if k <= 31 else ctx.count_wide_table
    t = count(bases.data_ptr(), offs.data_ptr(), args.reads, args.reads * rl, k, 0)
    torch.cuda.synchronize()
    return t


def entries(t):
    return t.stats()[0] if isinstance(t, L.WideTable) else len(t)


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


def shares(res):
    """where the time of a wide call goes, as shares of the kernels' total: the union's gather, the sorts (the union's two passes and the group
    lists'), the column gather into the matrix, the row kernels"""
    km = res["kernel_ms"]
    total = sum(ms for _, ms in km.values())
    part = lambda *names: sum(km[n][1] for n in names if n in km)
    return dict(kernels_ms=round(total, 3), union_gather=round(part("k_wj_gather") / total, 3), sorts=round(part("k_radix_sort") / total, 3),
                column_gather=round(part("k_wstats_gather") / total, 3), rows=round(part("k_stats_rows_thread", "k_stats_rows_wave") / total, 3))


def emit(res):
    print(json.dumps(res), flush=True)
    return res


def measure(ctx, k):
    ta = [synth_table(ctx, j, 0, k) for j in range(args.n)]
    tb = [synth_table(ctx, args.n + j, 1, k) for j in range(args.n)]
    base = dict(k=k, samples=2 * args.n, reads_per_sample=args.reads, max_bad=args.max_bad, steps=args.steps, entries=sum(entries(t) for t in ta + tb))
    call = ctx.stats_kmers if k <= 31 else ctx.stats_kmers_wide

    def fn():
        chi, ga, gb, ctr = call(ta, tb, max_bad=args.max_bad)
        for t in (chi, ga, gb):
            t.close()
        return ctr
    fn()                                                       # warm-up (arena, code objects)
    times, ctr = timed(fn, args.steps)
    res = dict(base, call="mf_stats_kmers_tables" if k <= 31 else "mf_stats_kmers_wide_tables", counters=ctr, wall_s=[round(t, 4) for t in times],
               wall_s_median=round(statistics.median(times), 4))
    res["kernel_ms"], _ = profiled(ctx, fn)
    if k > 31:
        res["shares"] = shares(res)
    rows = [emit(res)]
    if k > 31 and not args.no_files:
        d = tempfile.mkdtemp(prefix="wstats_rate_")
        try:
            fa, fb = [], []
            for name, tabs, files in (("a", ta, fa), ("b", tb, fb)):
                for j, t in enumerate(tabs):
                    files.append(os.path.join(d, "%s%d.kmers.bin" % (name, j)))
                    t.write_kmers(0, files[-1])
            ffn = lambda: ctx.stats_kmers_wide_files(fa, fb, k, d, max_bad=args.max_bad)
            rep, _ = profiled(ctx, ffn)                        # the warm-up, under the event timers
            times, ctr = timed(ffn, args.steps)
            res = dict(base, call="mf_stats_kmers_wide", counters=ctr, input_bytes=sum(os.path.getsize(f) for f in fa + fb),
                       wall_s=[round(t, 4) for t in times], wall_s_median=round(statistics.median(times), 4), kernel_ms=rep)
            res["shares"] = shares(res)
            rows.append(emit(res))
        finally:
            shutil.rmtree(d, ignore_errors=True)
    for t in ta + tb:
        t.close()
    return rows


def main():
    ctx = L.Context(0, stream=torch.cuda.current_stream())
    rows = [r for k in args.ks for r in measure(ctx, k)]
    narrow = [r for r in rows if r["k"] <= 31]
    if narrow:
        for r in rows:
            if r["call"] == "mf_stats_kmers_wide_tables":
                print("# k = %d: %.4f s, %.2f x the k = %d call (%.4f s)" % (r["k"], r["wall_s_median"], r["wall_s_median"] / narrow[0]["wall_s_median"],
                                                                        narrow[0]["k"], narrow[0]["wall_s_median"]))


if __name__ == "__main__":
    main()
