#!/usr/bin/env python3
"""comp2seq on wide components on one GPU: the wall time of mf_wcomps_unitigs_device(split = 1) on the wide
cutter output of synthetic reads at k = 63 (the benchmark's generator, a few thousand components), made on the device -- and beside
it the k = 31 mf_comps_unitigs_device on components cut from the SAME reads: existing code, and the only yardstick there is.
Synchronised on both sides, one warm-up and three runs each; then the per-kernel times of one more call under option profile.
This is a record, not a pass/fail time: nothing wide existed before to compare against.

    python tools/wcomp2seq_rate.py --out profiles/wcomp2seq_rate.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDE_KERNELS = ("k_wc2s_rows", "k_radix_sort", "k_wc2s_index_insert", "k_wc2s_flags", "k_ut_links", "k_ut_contract", "k_ut_walk1", "k_ut_ends", "k_ut_segments", "k_ut_walk2")
NARROW_KERNELS = ("k_c2s_rows", "k_radix_sort", "k_c2s_index_insert", "k_c2s_flags", "k_ut_links", "k_ut_contract", "k_ut_walk1", "k_ut_ends", "k_ut_segments", "k_ut_walk2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3000000)
    ap.add_argument("--genome-scale", type=int, default=1000000)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x4D45544146415354)
    ap.add_argument("-k", type=int, default=63)
    ap.add_argument("--narrow-k", type=int, default=31)
    ap.add_argument("--b1", type=int, default=1000)
    ap.add_argument("--b2", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wcomp2seq_rate.txt"))
    args = ap.parse_args()
    import torch
    from metafast_amd import lib as L
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()

    def say(s):                                             # (the report grows line by line: a run that is cut short leaves what it had)
        print(s, flush=True)
        with open(args.out, "a") as f:
            f.write(s + "\n")

    ctx = L.Context(0, stream=torch.cuda.current_stream())
    nb = args.reads * 150
    tb = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
    to = torch.zeros(args.reads + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads_device(args.seed, 0, 0, args.reads, 150, args.genome_scale, tb.data_ptr(), to.data_ptr())
    ctx.synchronize()
    # the wide cutter output: count > 1, unitigs of 100 bases and more, their k-mers, the cutter
    wt = ctx.count_wide_above(tb.data_ptr(), to.data_ptr(), args.reads, nb, args.k, 1)
    wt = wt[0] if isinstance(wt, tuple) else wt
    ws = ctx.build_unitigs_wide(wt, 1, 100)
    v = ws.device_view()
    wcomps = ctx.cut_components_wide(ctx.count_wide_table(v["bases"], v["offsets"], v["n"], v["n_bases"], args.k, 100), args.b1, args.b2)
    # ... and the k <= 31 one of the same reads
    nt = ctx.count_device_above(tb.data_ptr(), to.data_ptr(), args.reads, nb, args.narrow_k, 1)
    nt = nt[0] if isinstance(nt, tuple) else nt
    ns = ctx.build_unitigs(nt, 1, 100)
    v = ns.device_view()
    ncomps = ctx.cut_components(ctx.count_device(v["bases"], v["offsets"], v["n"], v["n_bases"], args.narrow_k, 100), args.b1, args.b2)
    del wt, ws, nt, ns
    wn, wk = wcomps.stats()
    nn, nk = ncomps.stats()
    say(f"# wcomp2seq_rate: {args.reads} synthetic reads x 150 (genome scale {args.genome_scale}), -b1 {args.b1} -b2 {args.b2}; {torch.cuda.get_device_name(0)}")
    say(f"# k = {args.k}: {wn} components, {wk} members; k = {args.narrow_k}: {nn} components, {nk} members")
    say("# pair index: the plain form (eight finds per row); the canonical-interior form (two walks per row) was not built")

    def measure(label, call, members, kernels):
        call()                                              # warm-up: the workspace is there afterwards
        wall = []
        for _ in range(max(args.repeats, 3)):
            ctx.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = call()
            ctx.synchronize()
            wall.append(time.perf_counter() - t0)
            n = len(s)
            del s
        med = statistics.median(wall)
        say(f"{label}: {n} sequences; wall per call (ms): " + " ".join(f"{w * 1e3:.2f}" for w in wall) + f"; median {med * 1e3:.2f} ms = {members / med / 1e6:.1f} M members/s")
        ctx.set_option("profile", 1)
        ctx.reset_timers()
        s = call()
        ctx.synchronize()
        for name in kernels:
            n, ms = ctx.kernel_time(name)
            if n:
                say(f"  one more call under option profile, {name}: {n} timed launches, {ms:.3f} ms")
        ctx.set_option("profile", 0)
        del s

    measure(f"mf_wcomps_unitigs_device(split=1), k = {args.k}", lambda: ctx.wcomps_unitigs(wcomps, split=True), wk, WIDE_KERNELS)
    measure(f"mf_comps_unitigs_device(split=1), k = {args.narrow_k}", lambda: ctx.comps_unitigs(ncomps, split=True)[0], nk, NARROW_KERNELS)


if __name__ == "__main__":
    main()
