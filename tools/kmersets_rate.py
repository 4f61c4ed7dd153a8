"""Time unique-kmers-multi and kmers-multiple-filters (mf_kmersets.hip) on a synthetic cohort, next to kmers-samples-counter on the same
inputs (it does the same union pass).

The cohort is tools/stats_rate.py's: --n inputs (group A) + --n filters (group B) of --reads reads each, counted by the library at k = 31.
Each operation runs on the tables resident in HBM: one warm-up, then --steps repeats, device-synchronised wall time, the median is
reported.  The per-kernel times ([launches, total ms]) are the library's HIP-event timers (option profile = 1) over one more repeat.
  --what unique     mf_unique_kmers_multi_tables(inputs, filters, b = 1, min-samples 1 .. max-samples n)
  --what filters    mf_kmers_multiple_filters_tables(input 0; CD, UC, nonIBD = kmers-samples-counter of A, of B, of half of each)
  --what nsamples   mf_kmers_samples_count_tables(inputs)
--root names another checkout of this project whose built library is measured instead (kmers-samples-counter of an older commit).

    python tools/kmersets_rate.py --what unique --n 16 --reads 2000000
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--what", choices=("unique", "filters", "nsamples"), required=True)
ap.add_argument("--n", type=int, default=16)
ap.add_argument("--reads", type=int, default=2_000_000)
ap.add_argument("--read-len", type=int, default=100)
ap.add_argument("-k", type=int, default=31)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from metafast_amd import lib as L  # noqa: E402


def synth_table(ctx, j, group):
    n1 = args.reads * 4 // 5
    n2 = args.reads - n1
    rl = args.read_len
    bases = torch.zeros(args.reads * rl + 64, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(args.reads + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads_device(0x5354415453, j, 0, n1, rl, 1_000_000, bases.data_ptr(), offs.data_ptr())
    ctx.synth_reads_device(0x41414141 if group == 0 else 0x42424242, 0, j * n2, n2, rl, 100_000, bases.data_ptr() + n1 * rl, offs[n1:].data_ptr())
    offs[n1:] += n1 * rl
    t = ctx.count_device(bases.data_ptr(), offs.data_ptr(), args.reads, args.reads * rl, args.k, 0)
    torch.cuda.synchronize()
    return t


def main():
    ctx = L.Context(0, stream=torch.cuda.current_stream())
    ta = [synth_table(ctx, j, 0) for j in range(args.n)]
    tb = [synth_table(ctx, args.n + j, 1) for j in range(args.n)] if args.what != "nsamples" else []
    res = dict(what=args.what, inputs=args.n, reads_per_sample=args.reads, k=args.k, steps=args.steps, entries_inputs=sum(len(t) for t in ta),
               entries_filters=sum(len(t) for t in tb))
    if args.what == "unique":
        def fn():
            outs, n_union, counts = ctx.unique_kmers_multi(ta, tb, 1, 1, args.n)
            for t in outs:
                t.close()
            return dict(n_union=n_union, counts=counts)
    elif args.what == "filters":
        h = args.n // 2
        sets = [ctx.kmers_samples_count(g, 1) for g in (ta, tb, ta[:h] + tb[:h])]
        res["entries_filters"] = sum(len(t) for t in sets)

        def fn():
            kept, triples, counts, found, nkept = ctx.kmers_multiple_filters(ta[0], *sets, 1)
            kept.close()
            return dict(found=found, kept=nkept, distinct_triples=len(triples))
    else:
        def fn():
            t = ctx.kmers_samples_count(ta, 1)
            n = len(t)
            t.close()
            return dict(n_kmers=n)
    fn()                                                       # warm-up (arena, code objects)
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
    print(json.dumps(res))


if __name__ == "__main__":
    main()
