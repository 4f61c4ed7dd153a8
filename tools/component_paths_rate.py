#!/usr/bin/env python3
"""component-paths on one GPU: the marking pass (k_cp_mark, mf_comppaths.hip: one index lookup per k-mer position,
in two launches -- count, then emit) next to k_presence of mf_presence_core (the reads route of features_reads, unchanged since the
parent commit: the same one-lookup-per-position work) on the SAME sequences and components, made on the device: --genes random
sequences of --gene-len bases as components (seq2comp), --seqs query sequences of --seq-len bases, half of them windows of the genes'
text (windows that cross from one gene into the next leave the component and enter another), half random.

Wall time of mf_paths_add (a fresh mf_paths each time, the index built before) and of mf_features_reads_device, synchronised on both
sides, after one warm-up call each, best of three; then one more call of each under option profile for the kernels' own times.

    python tools/component_paths_rate.py --out profiles/component_paths_rate.txt

--wide (32 <= k <= 63): the same workload through wcomps_from_sequences and paths_wide (mf_wcomppaths.hip); there is no reads route at
that width, so only mf_paths_add and k_cp_mark are timed.  --append adds to --out instead of starting it again.

    python tools/component_paths_rate.py --repeats 5 --out profiles/wcomponent_paths_rate.txt
    python tools/component_paths_rate.py --repeats 5 --wide -k 33 --append --out profiles/wcomponent_paths_rate.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--gene-len", type=int, default=3000)
    ap.add_argument("--seqs", type=int, default=1000000)
    ap.add_argument("--seq-len", type=int, default=300)
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("--min-len", type=int, default=50)
    ap.add_argument("--seed", type=int, default=20200203)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "component_paths_rate.txt"))
    args = ap.parse_args()
    import torch
    from metafast_amd import lib as L
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if not args.append:
        open(args.out, "w").close()

    def say(s):
        print(s, flush=True)
        with open(args.out, "a") as f:
            f.write(s + "\n")

    g = torch.Generator(device="cuda")
    g.manual_seed(args.seed)
    letters = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device="cuda")
    gb = args.genes * args.gene_len
    genes = torch.zeros(gb + 64, dtype=torch.uint8, device="cuda")
    genes[:gb] = letters[torch.randint(0, 4, (gb,), generator=g, device="cuda")]
    goff = torch.arange(0, gb + 1, args.gene_len, dtype=torch.int64, device="cuda")
    nb = args.seqs * args.seq_len
    bases = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
    off = torch.arange(0, nb + 1, args.seq_len, dtype=torch.int64, device="cuda")
    step = 1 << 20                                         # sequences per piece
    ar = torch.arange(args.seq_len, device="cuda")
    for a in range(0, args.seqs, step):
        b = min(args.seqs, a + step)
        start = torch.randint(0, gb - args.seq_len, (b - a,), generator=g, device="cuda")
        text = genes[(start[:, None] + ar[None, :]).reshape(-1)]
        rnd = letters[torch.randint(0, 4, ((b - a) * args.seq_len,), generator=g, device="cuda")]
        from_gene = (torch.arange(a, b, device="cuda") % 2 == 0).repeat_interleave(args.seq_len)
        bases[a * args.seq_len: b * args.seq_len] = torch.where(from_gene, text, rnd)
    ctx = L.Context(0, stream=torch.cuda.current_stream())
    c = (ctx.wcomps_from_sequences if args.wide else ctx.comps_from_sequences)(genes.data_ptr(), goff.data_ptr(), args.genes, gb, args.k)
    npos = args.seqs * max(0, args.seq_len - args.k + 1)
    say(f"# component_paths_rate: {args.genes} components (random sequences of {args.gene_len} bases, {c.stats()[1]} members), {args.seqs} sequences of "
        f"{args.seq_len} bases ({nb} bases, {npos} k-mer positions; every second one a window of the components' text), k = {args.k}, -l {args.min_len}, all "
        f"components; {torch.cuda.get_device_name(0)}")

    def paths_once():
        p = ctx.paths_wide(c, min_len=args.min_len) if args.wide else ctx.paths(c, min_len=args.min_len)
        ctx.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p.add(bases.data_ptr(), off.data_ptr(), args.seqs, nb)
        ctx.synchronize()
        t = time.perf_counter() - t0
        return t, p

    def features_once():
        ctx.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.features_reads(c, bases.data_ptr(), off.data_ptr(), args.seqs, nb, args.k)
        ctx.synchronize()
        return time.perf_counter() - t0

    ctx.set_option("profile", 0)
    _, p = paths_once()                                    # warm-up: the workspace is there afterwards
    p.finish()
    no, cnt, nbytes, cap = p.slots()
    say(f"paths kept: {int(cnt.sum())} in {int((cnt > 0).sum())} components, {int(nbytes.sum())} bytes of text; most listings of one k-mer: {p.max_listings()}")
    del p
    if not args.wide:
        features_once()
    wall_p = [paths_once()[0] for _ in range(max(args.repeats, 3))]
    wall_f = [] if args.wide else [features_once() for _ in range(max(args.repeats, 3))]
    say("mf_paths_add (marking, two sorts, pairing, cap, store): wall per call (ms): " + " ".join(f"{w * 1e3:.1f}" for w in wall_p) +
        f"; best {min(wall_p) * 1e3:.1f} ms, median {statistics.median(wall_p) * 1e3:.1f} ms, spread {(max(wall_p) - min(wall_p)) * 1e3:.1f} ms, "
        f"{npos / min(wall_p) / 1e9:.2f} G positions / s")
    if args.wide:
        ctx.set_option("profile", 1)
        ctx.reset_timers()
        paths_once()
        ctx.synchronize()
        n_m, ms_m = ctx.kernel_time("k_cp_mark")
        n_s, ms_s = ctx.kernel_time("k_radix_sort")
        ctx.set_option("profile", 0)
        say(f"one more call under option profile: k_cp_mark {n_m} launches (count + emit) {ms_m:.2f} ms = {npos / (ms_m / 1e3) / 1e9:.2f} G positions / s; "
            f"k_radix_sort (starts, ends) {n_s} timed sorts {ms_s:.2f} ms")
        return
    say("mf_features_reads_device (k_presence + the vector): wall per call (ms): " + " ".join(f"{w * 1e3:.1f}" for w in wall_f) +
        f"; best {min(wall_f) * 1e3:.1f} ms, spread {(max(wall_f) - min(wall_f)) * 1e3:.1f} ms")
    ctx.set_option("profile", 1)
    ctx.reset_timers()
    paths_once()
    features_once()
    ctx.synchronize()
    n_m, ms_m = ctx.kernel_time("k_cp_mark")
    n_p, ms_p = ctx.kernel_time("k_presence")
    n_s, ms_s = ctx.kernel_time("k_radix_sort")
    ctx.set_option("profile", 0)
    say(f"one more call of each under option profile: k_cp_mark {n_m} launches (count + emit) {ms_m:.2f} ms = {npos / (ms_m / 1e3) / 1e9:.2f} G positions / s; "
        f"k_presence {n_p} launch {ms_p:.2f} ms = {npos / (ms_p / 1e3) / 1e9:.2f} G positions / s; k_radix_sort (starts, ends) {n_s} timed sorts {ms_s:.2f} ms")
    say(f"ratio: the marking pass takes {ms_m / ms_p:.2f} x the time of k_presence ({ms_m / max(n_m, 1) / ms_p:.2f} x per launch)")


if __name__ == "__main__":
    main()
