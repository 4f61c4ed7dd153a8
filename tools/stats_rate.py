"""Time the multi-sample join behind stats-kmers (mf_stats.hip on the join core mf_join.hip) on a synthetic cohort.

The cohort: --a + --b samples of --reads reads each (mf_synth_reads_device: most reads from one shared seed with the sample's own
abundances, a share from its group's seed), counted by the library at k = 31.  Timed with device-synchronised wall time:
  resident   mf_stats_kmers_tables on the tables in HBM;
  files      mf_stats_kmers on the samples' .kmers.bin files (load at b, load at 0, write the three outputs).
The join is priced at the bytes it must move: every sample's entries (10 B: key + count) once per pass (union, gather), plus the union
table (16 B slots: written once, read by the select) and one probe per entry and pass; the share of 8 TB/s that rate is printed.

    python tools/stats_rate.py --a 16 --b 16 --reads 20000000 [--dir /tmp/cohort] [--steps 3]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metafast_amd import lib as L  # noqa: E402

HBM_BYTES_PER_S = 8e12


def synth_table(ctx, j, group, n_reads, k, rl):
    n1 = n_reads * 4 // 5
    n2 = n_reads - n1
    bases = torch.zeros(n_reads * rl + 64, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(n_reads + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads_device(0x5354415453, j, 0, n1, rl, 1_000_000, bases.data_ptr(), offs.data_ptr())
    ctx.synth_reads_device(0x41414141 if group == 0 else 0x42424242, 0, j * n2, n2, rl, 100_000, bases.data_ptr() + n1 * rl, offs[n1:].data_ptr())
    offs[n1:] += n1 * rl
    t = ctx.count_device(bases.data_ptr(), offs.data_ptr(), n_reads, n_reads * rl, k, 0)
    torch.cuda.synchronize()
    return t


def timed(fn, steps):
    best = None
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", type=int, default=16)
    ap.add_argument("--b", type=int, default=16)
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the samples' .kmers.bin files go (default: a temporary directory)")
    ap.add_argument("--no-files", action="store_true")
    args = ap.parse_args()

    ctx = L.Context(0, stream=torch.cuda.current_stream())
    tabs = [synth_table(ctx, j, 0 if j < args.a else 1, args.reads, args.k, args.read_len) for j in range(args.a + args.b)]
    n = [len(t) for t in tabs]
    ta, tb = tabs[:args.a], tabs[args.a:]
    ctx.stats_kmers(ta, tb)                                    # warm-up (arena, code objects)
    t_res, (chi, ga, gb, ctr) = timed(lambda: ctx.stats_kmers(ta, tb), args.steps)
    entries = sum(n)
    cap = 1
    while cap < 2 * entries:
        cap <<= 1
    priced = 2 * entries * 10 + cap * 16 * 2 + 2 * entries * 16
    res = dict(samples=len(tabs), reads_per_sample=args.reads, k=args.k, distinct_total=entries, counters=ctr,
               resident_s=round(t_res, 4), priced_bytes=priced, resident_share_of_8TBps=round(priced / t_res / HBM_BYTES_PER_S, 4))
    if not args.no_files:
        d = args.dir or tempfile.mkdtemp(prefix="stats_rate_")
        files = []
        for j, t in enumerate(tabs):
            f = os.path.join(d, "s%03d.kmers.bin" % j)
            t.write_kmers(-1, f)
            files.append(f)
        out = os.path.join(d, "out")
        os.makedirs(out, exist_ok=True)
        t_files, _ = timed(lambda: ctx.stats_kmers_files(files[:args.a], files[args.a:], out), args.steps)
        res["files_s"] = round(t_files, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
