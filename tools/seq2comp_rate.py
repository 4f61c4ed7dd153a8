#!/usr/bin/env python3
"""seq2comp on one GPU: the two ways to the distinct k-mers of a sequence on ONE input -- a synthetic catalogue
of --seqs random sequences of 300 .. 3000 bases plus --long sequences of 10^6 .. 10^7 bases, made on the device --

  * option s2c_lds = 1 (default): sequences of up to 4096 k-mers build their sets in LDS, the rest is sorted;
  * option s2c_lds = 0: every sequence through the sort path.

Wall time of mf_comps_from_sequences_device, synchronised on both sides, after one warm-up call each; best of --repeats and the
spread.  The LDS path stays only if it beats the sort path by more than the spread of the sort path's own runs.

    python tools/seq2comp_rate.py --out profiles/seq2comp_rate.txt
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("k_s2c_lds", "k_s2c_pairs", "k_radix_sort")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=1000000)
    ap.add_argument("--long", type=int, default=4)
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("--seed", type=int, default=20200203)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq2comp_rate.txt"))
    args = ap.parse_args()
    import torch
    from metafast_amd import lib as L
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()

    def say(s):
        print(s, flush=True)
        with open(args.out, "a") as f:
            f.write(s + "\n")

    g = torch.Generator(device="cuda")
    g.manual_seed(args.seed)
    lens = torch.randint(300, 3001, (args.seqs,), generator=g, device="cuda", dtype=torch.int64)
    if args.long:
        longs = torch.randint(10 ** 6, 10 ** 7 + 1, (args.long,), generator=g, device="cuda", dtype=torch.int64)
        at = torch.linspace(0, args.seqs - 1, args.long, device="cuda").long()
        lens[at] = longs
    off = torch.zeros(args.seqs + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(lens, 0)
    nb = int(off[-1])
    letters = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device="cuda")
    bases = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for a in range(0, nb, step):
        b = min(nb, a + step)
        bases[a:b] = letters[torch.randint(0, 4, (b - a,), generator=g, device="cuda")]
    occ = int(torch.clamp(lens - args.k + 1, min=0).sum())
    ctx = L.Context(0, stream=torch.cuda.current_stream())
    T = ctx.stat("s2c_lds_max")
    n_long = int((lens - args.k + 1 > T).sum())
    say(f"# seq2comp_rate: {args.seqs} random sequences of 300 .. 3000 bases, {args.long} of them replaced by sequences of 10^6 .. 10^7 bases "
        f"({nb} bases, {occ} k-mer occurrences, {n_long} sequences above {T} k-mers), k = {args.k}; {torch.cuda.get_device_name(0)}")
    best, spread, members = {}, {}, {}
    for lds in (0, 1):
        ctx.set_option("s2c_lds", lds)
        ctx.set_option("profile", 0)
        c = ctx.comps_from_sequences(bases.data_ptr(), off.data_ptr(), args.seqs, nb, args.k)         # warm-up: the workspace is there afterwards
        members[lds] = c.stats()
        del c
        wall = []
        for _ in range(max(args.repeats, 3)):
            ctx.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c = ctx.comps_from_sequences(bases.data_ptr(), off.data_ptr(), args.seqs, nb, args.k)
            ctx.synchronize()
            wall.append(time.perf_counter() - t0)
            del c
        best[lds], spread[lds] = min(wall), max(wall) - min(wall)
        name = "s2c_lds = 1 (sets in LDS up to %d k-mers, the rest sorted)" % T if lds else "s2c_lds = 0 (every sequence through the sort path)"
        say(f"{name}: wall per call (ms): " + " ".join(f"{w * 1e3:.1f}" for w in wall) + f"; best {best[lds] * 1e3:.1f} ms, spread {spread[lds] * 1e3:.1f} ms, "
            f"{occ / best[lds] / 1e9:.2f} G k-mer occurrences / s; {members[lds][0]} components, {members[lds][1]} members")
        ctx.set_option("profile", 1)
        ctx.reset_timers()
        c = ctx.comps_from_sequences(bases.data_ptr(), off.data_ptr(), args.seqs, nb, args.k)
        ctx.synchronize()
        for kn in KERNELS:
            n, ms = ctx.kernel_time(kn)
            if n:
                say(f"  one more call under option profile, {kn}: {n} timed launches, {ms:.2f} ms")
        del c
    ctx.set_option("profile", 0)
    ctx.set_option("s2c_lds", 1)
    assert members[0] == members[1], "the two paths disagree"
    gain = best[0] - best[1]
    say(f"decision: the LDS path is {'KEPT' if gain > spread[0] else 'NOT kept'}: it is {gain * 1e3:.1f} ms ({best[0] / best[1]:.2f} x) faster than the sort path alone, "
        f"whose own runs spread over {spread[0] * 1e3:.1f} ms")


if __name__ == "__main__":
    main()
