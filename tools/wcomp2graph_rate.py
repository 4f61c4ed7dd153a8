#!/usr/bin/env python3
"""comp2graph on wide components on one GPU (the wide paragraph of section 7g): mf_wcomps_graph_device at k = 63 on the
components of 3 M synthetic reads (default cutter bounds), and beside it mf_comps_graph_device at k = 31 on the components of the same
reads.  One visit, device-synchronised, best of 3, then one more call under option profile for the per-kernel split.

    python tools/wcomp2graph_rate.py --out profiles/wcomp2graph_rate.txt

--narrow-only skips the wide half: the narrow tool's k_c2g_* kernel sum is what a change to the shared steps (mf_c2g.h) is held against
(METAFAST_HIP_LIB selects the library; --append adds to the report instead of starting it).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C2G = ("k_c2g_values", "k_c2g_links", "k_c2g_double", "k_c2g_ends", "k_c2g_assign", "k_c2g_segments", "k_c2g_links_of", "k_c2g_link_len", "k_c2g_write")
WIDE_KERNELS = ("k_wc2s_rows", "k_radix_sort", "k_wc2s_index_insert", "k_wc2s_flags") + C2G
NARROW_KERNELS = ("k_c2s_rows", "k_radix_sort", "k_c2s_index_insert", "k_c2s_flags") + C2G


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
    ap.add_argument("--narrow-only", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wcomp2graph_rate.txt"))
    args = ap.parse_args()
    import torch
    from metafast_amd import lib as L
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if not args.append:
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
    say(f"# wcomp2graph_rate{' ' + args.label if args.label else ''}: {args.reads} synthetic reads x 150 (genome scale {args.genome_scale}), -b1 {args.b1} -b2 {args.b2}; "
        f"{torch.cuda.get_device_name(0)}")
    wcomps = None
    if not args.narrow_only:
        # the wide cutter output: count > 1, unitigs of 100 bases and more, their k-mers, the cutter
        wt = ctx.count_wide_above(tb.data_ptr(), to.data_ptr(), args.reads, nb, args.k, 1)
        wt = wt[0] if isinstance(wt, tuple) else wt
        ws = ctx.build_unitigs_wide(wt, 1, 100)
        v = ws.device_view()
        wcomps = ctx.cut_components_wide(ctx.count_wide_table(v["bases"], v["offsets"], v["n"], v["n_bases"], args.k, 100), args.b1, args.b2)
        del wt, ws
    nt = ctx.count_device_above(tb.data_ptr(), to.data_ptr(), args.reads, nb, args.narrow_k, 1)
    nt = nt[0] if isinstance(nt, tuple) else nt
    ns = ctx.build_unitigs(nt, 1, 100)
    v = ns.device_view()
    ncomps = ctx.cut_components(ctx.count_device(v["bases"], v["offsets"], v["n"], v["n_bases"], args.narrow_k, 100), args.b1, args.b2)
    del nt, ns, tb, to

    def measure(label, call, members, kernels):
        text, stats = call()                                # warm-up: the workspace is there afterwards
        say(f"{label}: {members} members -> {len(text)} bytes of GFA, {stats['segments']} segments, {stats['links']} L lines, {stats['cycles']} opened cycles")
        del text
        wall = []
        for _ in range(max(args.repeats, 3)):
            ctx.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = call()
            ctx.synchronize()
            wall.append(time.perf_counter() - t0)
            del r
        best = min(wall)
        say(f"  wall per call, text to the host included (ms): " + " ".join(f"{w * 1e3:.2f}" for w in wall) + f"; best {best * 1e3:.2f} ms = {members / best / 1e6:.1f} M members/s")
        ctx.set_option("profile", 1)
        ctx.reset_timers()
        r = call()
        ctx.synchronize()
        total = 0.0
        for name in kernels:
            n, ms = ctx.kernel_time(name)
            if n:
                say(f"  one more call under option profile, {name}: {n} timed launches, {ms:.3f} ms")
            if name.startswith("k_c2g_"):
                total += ms
        say(f"  the k_c2g_* timers of that call: {total:.3f} ms")
        ctx.set_option("profile", 0)
        del r

    if wcomps is not None:
        wn, wk = wcomps.stats()
        say(f"# k = {args.k}: {wn} components")
        measure(f"mf_wcomps_graph_device, k = {args.k}", lambda: ctx.wcomps_graph(wcomps), wk, WIDE_KERNELS)
    nn, nk = ncomps.stats()
    say(f"# k = {args.narrow_k}: {nn} components")
    measure(f"mf_comps_graph_device, k = {args.narrow_k}", lambda: ctx.comps_graph(ncomps, k=args.narrow_k), nk, NARROW_KERNELS)


if __name__ == "__main__":
    main()
