#!/usr/bin/env python3
"""comp2seq against the three-tool chain it replaces, on one GPU.

Cuts the components of one synthetic sample (the benchmark's generator, default -b1 / -b2), writes components.bin, then times
  * `metafast.sh -t comp2seq [--split]` of this tree, and
  * bin2fasta -> kmer-counter-many -b 0 -> seq-builder-many -b 0 -l k with the driver given by --chain-exe (a build of the parent
    commit; several may be given: the same source built twice shows the chain's own spread),
one warm-up and --repeats timed runs each, whole processes, files compared at the end; then the per-kernel times of one in-process
mf_comps_unitigs_device(split) under option profile and the row rate.  The report goes to --out.

    python tools/comp2seq_rate.py --reads 3000000 --chain-exe /path/to/parent/metafast --out profiles/comp2seq_rate.txt
"""
import argparse
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIRS = ("kmers_fasta", "kmer-counter-many/kmers", "kmer-counter-many/stats", "seq-builder-many/sequences")


def make_components(ctx, L, args, path):
    import torch
    tb = torch.zeros(args.reads * 150 + 64, dtype=torch.uint8, device="cuda")
    to = torch.zeros(args.reads + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads_device(args.seed, 0, 0, args.reads, 150, args.genome_scale, tb.data_ptr(), to.data_ptr())
    ctx.synchronize()
    t = ctx.count_device_above(tb.data_ptr(), to.data_ptr(), args.reads, args.reads * 150, args.k, 1)
    t = t[0] if isinstance(t, tuple) else t
    seqs = ctx.build_unitigs(t, 1, 100)
    v = seqs.device_view()
    cutter = ctx.count_device(v["bases"], v["offsets"], v["n"], v["n_bases"], args.k, 100)
    comps = ctx.cut_components(cutter, args.b1, args.b2)
    comps.write(path)
    return comps.stats()


def run(cmd):
    t0 = time.perf_counter()
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(map(str, cmd[:4]))} ... failed:\n{r.stderr[-2000:]}")
    return time.perf_counter() - t0


def chain(exe, cf, k, split, wd):
    t = run([exe, "-t", "bin2fasta", "-k", k, "-cf", cf, *(["--split"] if split else []), "-o", os.path.join(wd, "kmers_fasta", "component"), "-w", os.path.join(wd, "bin2fasta"), "--device", 0])
    fastas = sorted(glob.glob(os.path.join(wd, "kmers_fasta", "*.fasta")))
    print(f"  (chain: bin2fasta {t:.2f} s, {len(fastas)} files)", flush=True)
    t += run([exe, "-t", "kmer-counter-many", "-k", k, "-b", 0, "-i", *fastas, "-w", os.path.join(wd, "kmer-counter-many"), "--device", 0])
    kbins = sorted(glob.glob(os.path.join(wd, "kmer-counter-many", "kmers", "*.kmers.bin")))
    print(f"  (chain: ... kmer-counter-many done at {t:.2f} s)", flush=True)
    t += run([exe, "-t", "seq-builder-many", "-k", k, "-b", 0, "-l", k, "-i", *kbins, "-w", os.path.join(wd, "seq-builder-many"), "--device", 0])
    return t


def tree(wd):
    out = {}
    for d in DIRS:
        for p in glob.glob(os.path.join(wd, d, "*")):
            out[os.path.relpath(p, wd)] = open(p, "rb").read()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3000000)
    ap.add_argument("--genome-scale", type=int, default=1000000)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x4D45544146415354)
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("--b1", type=int, default=1000)
    ap.add_argument("--b2", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chain-exe", action="append", default=[], help="driver that runs the chain (default: this tree's)")
    ap.add_argument("--no-split-chain", action="store_true", help="skip the chain with --split (minutes for thousands of components)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "comp2seq_rate.txt"))
    args = ap.parse_args()
    import torch
    from metafast_amd import lib as L
    here = os.path.join(ROOT, "metafast.sh")
    exes = args.chain_exe or [here]

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()

    def say(s):                                             # (the report grows line by line: a run that is cut short leaves what it had)
        print(s, flush=True)
        with open(args.out, "a") as f:
            f.write(s + "\n")

    tmp = tempfile.mkdtemp(prefix="c2s_rate_")
    cf = os.path.join(tmp, "components.bin")
    ctx = L.Context(0, stream=torch.cuda.current_stream())
    nc, nk = make_components(ctx, L, args, cf)
    say(f"# comp2seq_rate: {args.reads} synthetic reads x 150 (genome scale {args.genome_scale}), k = {args.k}, -b1 {args.b1} -b2 {args.b2}: {nc} components, {nk} k-mers, "
        f"components.bin {os.path.getsize(cf)} bytes; {torch.cuda.get_device_name(0)}")
    # in-process: the kernels of one segmented build
    comps = ctx.load_components(cf)
    ctx.comps_unitigs(comps, split=True, k=args.k)                       # warm-up
    ctx.set_option("profile", 1)
    wall = []
    for _ in range(max(args.repeats, 3)):
        ctx.reset_timers()
        ctx.synchronize()
        t0 = time.perf_counter()
        seqs, ids = ctx.comps_unitigs(comps, split=True)
        ctx.synchronize()
        wall.append(time.perf_counter() - t0)
    say(f"mf_comps_unitigs_device(split=1): {len(seqs)} sequences; wall per call (ms): " + " ".join(f"{w * 1e3:.2f}" for w in wall)
        + f"; median {statistics.median(wall) * 1e3:.2f} ms = {nk / statistics.median(wall) / 1e6:.1f} M rows/s")
    for name in ("k_c2s_rows", "k_radix_sort", "k_c2s_index_insert", "k_c2s_flags", "k_ut_links", "k_ut_contract", "k_ut_walk1", "k_ut_ends", "k_ut_segments", "k_ut_walk2"):
        n, ms = ctx.kernel_time(name)
        say(f"  last call, {name}: {n} timed launches, {ms:.3f} ms")
    ctx.set_option("profile", 0)
    # whole processes
    for split in (True, False):
        mode = "--split" if split else "unsplit"
        ts = []
        for r in range(args.repeats + 1):
            wd = os.path.join(tmp, f"new_{mode}_{r}")
            t = run([here, "-t", "comp2seq", "-k", args.k, "-cf", cf, *(["--split"] if split else []), "-w", wd, "--device", 0])
            if r:
                ts.append(t)
            if r < args.repeats:
                shutil.rmtree(wd)
        new_tree = tree(wd)
        say(f"comp2seq {mode}: {len(new_tree)} files; s per run after one warm-up: " + " ".join(f"{t:.3f}" for t in ts) + f"; median {statistics.median(ts):.3f}")
        if split and args.no_split_chain:
            say("chain --split: skipped (--no-split-chain)")
            continue
        for i, exe in enumerate(exes):
            cs = []
            # (with --split a chain run takes minutes: one run per build, no warm-up -- process start-up is a thousandth of it)
            for r in range(1 if split else args.repeats + 1):
                wd = os.path.join(tmp, f"chain{i}_{mode}_{r}")
                t = chain(exe, cf, args.k, split, wd)
                if r or split:
                    cs.append(t)
                same = tree(wd) == new_tree
                shutil.rmtree(wd)
            say(f"chain {mode} with {'this tree' if exe == here else 'parent build ' + str(i + 1)}: s per run" + ("" if split else " after one warm-up") + ": " + " ".join(f"{t:.3f}" for t in cs)
                + f"; median {statistics.median(cs):.3f}; files identical to comp2seq's: {same}")
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
