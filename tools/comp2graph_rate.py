#!/usr/bin/env python3
"""comp2graph on one GPU, on the input of tools/comp2seq_rate.py: the components of 3 M synthetic reads, k = 31,
default cutter bounds.

  * in-process: wall time of mf_comps_graph_device and its kernels under option profile, next to comp2seq's segmented build
    (mf_comps_unitigs_device, split) of the same rows;
  * whole processes: `metafast.sh -t comp2graph`, without and with -i (the two halves of the reads as samples).

    python tools/comp2graph_rate.py --reads 3000000 --out profiles/comp2graph_rate.txt
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from comp2seq_rate import make_components, run      # noqa: E402

KERNELS = ("k_c2s_rows", "k_radix_sort", "k_c2s_index_insert", "k_c2s_flags", "k_c2g_values", "k_c2g_links", "k_c2g_double", "k_c2g_ends", "k_c2g_assign",
           "k_c2g_segments", "k_c2g_links_of", "k_c2g_link_len", "k_c2g_write")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3000000)
    ap.add_argument("--genome-scale", type=int, default=1000000)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x4D45544146415354)
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("--b1", type=int, default=1000)
    ap.add_argument("--b2", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "comp2graph_rate.txt"))
    args = ap.parse_args()
    import torch
    from metafast_amd import lib as L
    here = os.path.join(ROOT, "metafast.sh")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()

    def say(s):
        print(s, flush=True)
        with open(args.out, "a") as f:
            f.write(s + "\n")

    tmp = tempfile.mkdtemp(prefix="c2g_rate_")
    cf = os.path.join(tmp, "components.bin")
    ctx = L.Context(0, stream=torch.cuda.current_stream())
    nc, nk = make_components(ctx, L, args, cf)
    say(f"# comp2graph_rate: {args.reads} synthetic reads x 150 (genome scale {args.genome_scale}), k = {args.k}, -b1 {args.b1} -b2 {args.b2}: {nc} components, "
        f"{nk} k-mers, components.bin {os.path.getsize(cf)} bytes; {torch.cuda.get_device_name(0)}")
    comps = ctx.load_components(cf)
    ctx.comps_unitigs(comps, split=True, k=args.k)                       # warm-up of both
    text, stats = ctx.comps_graph(comps)
    say(f"GFA: {len(text)} bytes, {stats['segments']} segments, {stats['links']} L lines, {stats['cycles']} opened cycles")
    del text
    ctx.set_option("profile", 1)
    for what in ("unitigs", "graph"):
        wall = []
        for _ in range(max(args.repeats, 3)):
            ctx.reset_timers()
            ctx.synchronize()
            t0 = time.perf_counter()
            r = ctx.comps_unitigs(comps, split=True) if what == "unitigs" else ctx.comps_graph(comps)
            ctx.synchronize()
            wall.append(time.perf_counter() - t0)
            del r
        name = "mf_comps_unitigs_device(split=1), the yardstick" if what == "unitigs" else "mf_comps_graph_device + text to the host"
        say(f"{name}: wall per call (ms): " + " ".join(f"{w * 1e3:.2f}" for w in wall) + f"; median {statistics.median(wall) * 1e3:.2f} ms")
        if what == "graph":
            total = 0.0
            for kn in KERNELS:
                n, ms = ctx.kernel_time(kn)
                total += ms
                say(f"  last call, {kn}: {n} timed launches, {ms:.3f} ms")
            say(f"  last call, the kernels above: {total:.3f} ms")
    ctx.set_option("profile", 0)
    # two samples: the halves of the reads
    files = []
    for i in range(2):
        tb = torch.zeros(args.reads // 2 * 150 + 64, dtype=torch.uint8, device="cuda")
        to = torch.zeros(args.reads // 2 + 1, dtype=torch.int64, device="cuda")
        ctx.synth_reads_device(args.seed, 0, i * (args.reads // 2), args.reads // 2, 150, args.genome_scale, tb.data_ptr(), to.data_ptr())
        ctx.synchronize()
        t = ctx.count_device(tb.data_ptr(), to.data_ptr(), args.reads // 2, args.reads // 2 * 150, args.k, 0)
        files.append(os.path.join(tmp, f"half{i}.kmers.bin"))
        t.write_kmers(0, files[-1])
        del t, tb, to
    for label, extra in (("no -i", []), ("-i two samples", ["-i", *files]), ("-i two samples -cov", ["-i", *files, "-cov"])):
        ts = []
        for r in range(args.repeats + 1):
            wd = os.path.join(tmp, "wd")
            t = run([here, "-t", "comp2graph", "-k", args.k, "-cf", cf, *extra, "-w", wd, "--device", 0])
            if r:
                ts.append(t)
            size = os.path.getsize(os.path.join(wd, "components-graph.gfa"))
            shutil.rmtree(wd)
        say(f"comp2graph {label}: {size} bytes of GFA; s per run after one warm-up: " + " ".join(f"{t:.3f}" for t in ts) + f"; median {statistics.median(ts):.3f}")
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
