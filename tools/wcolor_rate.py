"""Time the wide kmers-color (mf_kmers_color_wide_tables and the file form mf_kmers_color_wide, mf_wcolor.hip) on a synthetic cohort at k = 33 and
k = 63, next to the k <= 31 call (mf_kmers_color_tables, the hashed join of mf_color.hip) at k = 31 on samples of the same reads, and the wide
component-colored (mf_colored_components_wide_device) next to one threshold level of the wide cutter (mf_cut_components_wide_device) on the same
k-mers.

The cohort is tools/wstats_rate.py's with three classes: --n samples of --reads reads each (four fifths from a genome all samples share, one fifth
from the class's own genome), class j % 3, counted by the library.  The table form runs on the tables resident in HBM; for the file form every
sample is written once as a wide .kmers.bin into a temporary directory and the call streams them and writes its two files there.  The components
run on the coloured table of the cohort (default mode, perc = 0.9, three groups); the cutter runs on the first sample's table at b1 = 1,
b2 = 2^31 - 1, where no component is oversize and the first threshold level is the only one.  One warm-up, then --steps repeats,
device-synchronised wall time, the median is reported.  The per-kernel times ([launches, total ms]) are the library's HIP-event timers (option
profile = 1): for the table form over one more repeat, for the file form over its warm-up.  Every row is printed as soon as it is measured.

    python tools/wcolor_rate.py --n 16 --reads 1000000 > profiles/wcolor_rate.txt
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
ap.add_argument("--n", type=int, default=16, help="samples in the cohort")
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--read-len", type=int, default=100)
ap.add_argument("--ks", type=int, nargs="+", default=[31, 33, 63])
ap.add_argument("--max-bad", type=int, default=1)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--no-files", action="store_true", help="the table form alone")
ap.add_argument("--no-components", action="store_true", help="kmers-color alone")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metafast_amd import lib as L  # noqa: E402

OWN = (0x41414141, 0x42424242, 0x43434343)


def synth_table(ctx, j, k):
    n1 = args.reads * 4 // 5
    n2 = args.reads - n1
    rl = args.read_len
    bases = torch.zeros(args.reads * rl + 64, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(args.reads + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads_device(0x5354415453, j, 0, n1, rl, 1_000_000, bases.data_ptr(), offs.data_ptr())
    ctx.synth_reads_device(OWN[j % 3], 0, j * n2, n2, rl, 100_000, bases.data_ptr() + n1 * rl, offs[n1:].data_ptr())
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
    """where the time of a wide kmers-color call goes, as shares of the kernels' total: the union's gather, its sorts, and the add pass -- the second
    read of the samples"""
    km = res["kernel_ms"]
    total = sum(ms for _, ms in km.values())
    part = lambda *names: sum(km[n][1] for n in names if n in km)
    return dict(kernels_ms=round(total, 3), union_gather=round(part("k_wj_gather") / total, 3), sorts=round(part("k_radix_sort") / total, 3),
                add_pass=round(part("k_wcolor_add") / total, 3))


def emit(res):
    print(json.dumps(res), flush=True)
    return res


def measure(ctx, k):
    tabs = [synth_table(ctx, j, k) for j in range(args.n)]
    classes = [j % 3 for j in range(args.n)]
    base = dict(k=k, samples=args.n, reads_per_sample=args.reads, max_bad=args.max_bad, steps=args.steps, entries=sum(entries(t) for t in tabs))
    call = ctx.kmers_color if k <= 31 else ctx.kmers_color_wide

    def fn():
        ct = call(tabs, classes, b=args.max_bad)
        n = len(ct)
        ct.close()
        return n
    fn()                                                       # warm-up (arena, code objects)
    times, n = timed(fn, args.steps)
    res = dict(base, call="mf_kmers_color_tables" if k <= 31 else "mf_kmers_color_wide_tables", kmers=n, wall_s=[round(t, 4) for t in times],
               wall_s_median=round(statistics.median(times), 4))
    res["kernel_ms"], _ = profiled(ctx, fn)
    if k > 31:
        res["shares"] = shares(res)
    rows = [emit(res)]
    if k > 31 and not args.no_files:
        d = tempfile.mkdtemp(prefix="wcolor_rate_")
        try:
            files = []
            for j, t in enumerate(tabs):
                files.append(os.path.join(d, "s%d.kmers.bin" % j))
                t.write_kmers(0, files[-1])
            out, st = os.path.join(d, "colored_kmers.kmers.bin"), os.path.join(d, "colored_kmers.stat.txt")
            ffn = lambda: ctx.kmers_color_wide_files(files, classes, k, out, st, b=args.max_bad)
            rep, _ = profiled(ctx, ffn)                        # the warm-up, under the event timers
            times, n = timed(ffn, args.steps)
            res = dict(base, call="mf_kmers_color_wide", kmers=n, input_bytes=sum(os.path.getsize(f) for f in files), output_bytes=os.path.getsize(out),
                       wall_s=[round(t, 4) for t in times], wall_s_median=round(statistics.median(times), 4), kernel_ms=rep)
            res["shares"] = shares(res)
            rows.append(emit(res))
        finally:
            shutil.rmtree(d, ignore_errors=True)
    if k > 31 and not args.no_components:
        ct = ctx.kmers_color_wide(tabs, classes, b=args.max_bad)

        def cfn():
            cs = ctx.colored_components_wide(ct)
            n = [len(c) for c in cs]
            for c in cs:
                c.close()
            return n

        def cut():
            c = ctx.cut_components_wide(tabs[0], 1, 2 ** 31 - 1)
            n = len(c)
            c.close()
            return n
        for name, f, vertices in (("mf_colored_components_wide_device", cfn, len(ct)), ("mf_cut_components_wide_device", cut, entries(tabs[0]))):
            f()
            times, n = timed(f, args.steps)
            res = dict(k=k, call=name, vertices=vertices, components=n, steps=args.steps, wall_s=[round(t, 4) for t in times],
                       wall_s_median=round(statistics.median(times), 4))
            res["kernel_ms"], _ = profiled(ctx, f)
            res["ns_per_vertex"] = round(1e9 * res["wall_s_median"] / max(vertices, 1), 2)
            rows.append(emit(res))
        ct.close()
    for t in tabs:
        t.close()
    return rows


def main():
    ctx = L.Context(0, stream=torch.cuda.current_stream())
    rows = [r for k in args.ks for r in measure(ctx, k)]
    narrow = [r for r in rows if r["k"] <= 31]
    for r in rows:
        if narrow and r["call"] == "mf_kmers_color_wide_tables":
            print("# kmers-color, k = %d: %.4f s, %.2f x the k = %d call (%.4f s); the add pass is %.0f %% of the kernels' time"
                  % (r["k"], r["wall_s_median"], r["wall_s_median"] / narrow[0]["wall_s_median"], narrow[0]["k"], narrow[0]["wall_s_median"],
                     100 * r["shares"]["add_pass"]))
        if r["call"] == "mf_colored_components_wide_device":
            cut = [c for c in rows if c["call"] == "mf_cut_components_wide_device" and c["k"] == r["k"]]
            if cut:
                print("# component-colored, k = %d: %.2f ns per vertex, %.2f x one level of the cutter (%.2f ns per vertex)"
                      % (r["k"], r["ns_per_vertex"], r["ns_per_vertex"] / cut[0]["ns_per_vertex"], cut[0]["ns_per_vertex"]))


if __name__ == "__main__":
    main()
