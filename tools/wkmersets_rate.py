"""Time the wide unique-kmers-multi (mf_unique_kmers_multi_wide_tables, mf_wjoin.hip) on a synthetic cohort at k = 33 and k = 63, next to the
k <= 31 call (mf_unique_kmers_multi_tables, the hashed join of mf_join.hip) at k = 31 on samples of the same reads.

The cohort is tools/kmersets_rate.py's: --n samples of --reads reads each (four fifths from a genome all samples share, one fifth from one
of two group genomes), the first --n minus two as inputs and the last two as filters, counted by the library.  Each call runs on the
tables resident in HBM (b = 1, min-samples 1 .. max-samples = inputs): one warm-up, then --steps repeats, device-synchronised wall time,
the median is reported.  The per-kernel times ([launches, total ms]) are the library's HIP-event timers (option profile = 1) over one more
repeat; the radix sorts inside mf_wide_sort_runs show up under their own names.

    python tools/wkmersets_rate.py --n 8 --reads 1000000 > profiles/wkmersets_rate.txt
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8)
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--read-len", type=int, default=100)
ap.add_argument("--ks", type=int, nargs="+", default=[31, 33, 63])
ap.add_argument("--steps", type=int, default=5)
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


def measure(ctx, k):
    ni = args.n - 2
    ta = [synth_table(ctx, j, 0, k) for j in range(ni)]
    tb = [synth_table(ctx, ni + j, 1, k) for j in range(2)]
    res = dict(k=k, call="mf_unique_kmers_multi_tables" if k <= 31 else "mf_unique_kmers_multi_wide_tables", inputs=ni, filters=2,
               reads_per_sample=args.reads, steps=args.steps, entries_inputs=sum(entries(t) for t in ta), entries_filters=sum(entries(t) for t in tb))
    call = ctx.unique_kmers_multi if k <= 31 else ctx.unique_kmers_multi_wide

    def fn():
        outs, n_union, counts = call(ta, tb, 1, 1, ni)
        for t in outs:
            t.close()
        return dict(n_union=n_union, counts=counts)
    fn()                                                       # warm-up (arena, code objects; a wide table fresh from the count needs no order here)
    times = []
    for _ in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    res.update(out)
    res["wall_s"] = [round(t, 4) for t in times]
    res["wall_s_median"] = round(statistics.median(times), 4)
    ctx.set_option("profile", 1)                               # one more repeat under the event timers (they are off for the wall times)
    ctx.reset_timers()
    fn()
    torch.cuda.synchronize()
    res["kernel_ms"] = {name: [n, round(ms, 3)] for name, (n, ms, mx) in sorted(ctx.kernel_report().items()) if n}
    ctx.set_option("profile", 0)
    for t in ta + tb:
        t.close()
    return res


def main():
    ctx = L.Context(0, stream=torch.cuda.current_stream())
    rows = [measure(ctx, k) for k in args.ks]
    for r in rows:
        print(json.dumps(r))
    narrow = [r for r in rows if r["k"] <= 31]
    if narrow:
        for r in rows:
            if r["k"] > 31:
                print("# k = %d: %.4f s, %.2f x the k = %d call (%.4f s)" % (r["k"], r["wall_s_median"], r["wall_s_median"] / narrow[0]["wall_s_median"],
                                                                        narrow[0]["k"], narrow[0]["wall_s_median"]))


if __name__ == "__main__":
    main()
