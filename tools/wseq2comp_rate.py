"""wseq2comp rate: a catalogue-like input, the device call with s2c_lds = 1 against 0 at k = 33 and 63, the narrow tool at k = 31 for orientation"""
import os, statistics, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metafast_amd import lib as L

out = open(sys.argv[1] if len(sys.argv) > 1 else "wseq2comp_rate.txt", "w")
def say(s):
    print(s, flush=True); out.write(s + "\n"); out.flush()

rng = np.random.default_rng(2026)
NSEQ = 200000
lens = rng.integers(300, 3001, NSEQ).astype(np.int64)
for at in (1000, 100000, 199000):
    lens[at] = 5_000_000
off = np.zeros(NSEQ + 1, dtype=np.uint64); off[1:] = np.cumsum(lens).astype(np.uint64)
nb = int(off[-1])
g = torch.Generator(device="cuda"); g.manual_seed(7)
lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
tb = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
tb[:nb] = lut[torch.randint(0, 4, (nb,), generator=g, device="cuda")]
to = torch.from_numpy(off.view(np.int64).copy()).cuda()
ctx = L.Context(0, stream=torch.cuda.current_stream())
T = ctx.stat("ws2c_lds_max")
say(f"# wseq2comp_rate: {NSEQ} random sequences of 300 .. 3000 bases, 3 of them replaced by sequences of 5 x 10^6 bases ({nb} bases); {torch.cuda.get_device_name(0)}; ws2c_lds_max = {T}, s2c_lds_max = {ctx.stat('s2c_lds_max')}")
REP = 5
res = {}
for k, call, names in ((33, ctx.wcomps_from_sequences, ("k_ws2c_lds", "k_ws2c_pairs", "k_ws2c_sort")), (63, ctx.wcomps_from_sequences, ("k_ws2c_lds", "k_ws2c_pairs", "k_ws2c_sort")),
                       (31, ctx.comps_from_sequences, ("k_s2c_lds", "k_s2c_pairs", "k_radix_sort"))):
    occ = int(np.maximum(lens - k + 1, 0).sum())
    lim = T if k > 31 else ctx.stat("s2c_lds_max")
    say(f"k = {k}: {occ} k-mer occurrences, {int((lens - k + 1 > lim).sum())} sequences above {lim} k-mers, {int((lens - k + 1 <= lim // 4).sum())} of at most {lim // 4}")
    times = {0: [], 1: []}
    stats = None
    for rep in range(REP + 1):                       # the first round warms up; the two settings alternate
        for lds in (0, 1):
            ctx.set_option("s2c_lds", lds)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            c = call(tb.data_ptr(), to.data_ptr(), NSEQ, nb, k)
            torch.cuda.synchronize(); dt = (time.perf_counter() - t0) * 1e3
            if rep: times[lds].append(dt)
            st = c.stats()
            assert stats is None or st == stats
            stats = st
            c.close(); del c
    for lds in (0, 1):
        t = times[lds]; med = statistics.median(t)
        say(f"  s2c_lds = {lds}: wall per call (ms): {' '.join('%.1f' % x for x in t)}; median {med:.1f} ms, spread {max(t) - min(t):.1f} ms, {occ / med / 1e6:.2f} G k-mer occurrences / s; {stats[0]} components, {stats[1]} members")
        res[(k, lds)] = (med, max(t) - min(t))
        ctx.set_option("s2c_lds", lds); ctx.set_option("profile", 1); ctx.reset_timers() if hasattr(ctx, "reset_timers") else L.lib().mf_ctx_reset_timers(ctx.h)
        c = call(tb.data_ptr(), to.data_ptr(), NSEQ, nb, k); torch.cuda.synchronize(); c.close(); del c
        rep_ = ctx.kernel_report()
        ctx.set_option("profile", 0)
        for nm in names:
            if nm in rep_: say(f"    one more call under option profile, {nm}: {rep_[nm][0]} timed launches, {rep_[nm][1]:.2f} ms")
    ctx.set_option("s2c_lds", 1)
for k in (33, 63):
    (m0, s0), (m1, s1) = res[(k, 0)], res[(k, 1)]
    say(f"k = {k}: LDS class on {m1:.1f} ms, off {m0:.1f} ms: {'ON is faster' if m1 < m0 else 'OFF is faster'} by {abs(m0 - m1):.1f} ms ({max(m0, m1) / min(m0, m1):.2f} x); spreads {s1:.1f} / {s0:.1f} ms")
out.close()
