"""wide features from reads, rate: mf_features_reads_wide_device against the route that existed before it (mf_count_wide_device +
mf_features_wide_device on the same reads and components) at k = 33 and 63, the two alternating; per-kernel split from the context's timers.

    python tools/wfeatures_reads_rate.py OUT.txt [R=LIBRARY ...]

With R=LIBRARY arguments (builds of the library with another WF_RUN: make BUILD=... OUTDIR=... EXTRA=-DWF_RUN=64 in metafast_amd/csrc) the
measurement runs once per library, each in a child process of its own, after the one of the default build; everything lands in OUT.txt."""
import os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[1] if len(sys.argv) > 1 else "wfeatures_reads_rate.txt"
VARIANTS = [a.split("=", 1) for a in sys.argv[2:]]

if VARIANTS or os.environ.get("WFR_CHILD") is None:
    # the parent opens no GPU: one child per library, one after the other
    open(OUT, "w").close()
    for name, path in [("default", "")] + VARIANTS:
        env = dict(os.environ, WFR_CHILD=name)
        if path:
            env["METAFAST_HIP_LIB"] = os.path.abspath(path)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), OUT], env=env)
        if r.returncode != 0:
            sys.exit(r.returncode)
    sys.exit(0)

import numpy as np, torch
sys.path.insert(0, ROOT)
from metafast_amd import lib as L

out = open(OUT, "a")
def say(s):
    print(s, flush=True); out.write(s + "\n"); out.flush()

NCONTIG, CLEN, NREADS, RLEN = 2000, 1000, 1_000_000, 150
g = torch.Generator(device="cuda"); g.manual_seed(11)
lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
comp = torch.zeros(256, dtype=torch.uint8, device="cuda")
for a, b in zip(b"ACGT", b"TGCA"):
    comp[a] = b
genome = lut[torch.randint(0, 4, (NCONTIG * CLEN,), generator=g, device="cuda")]
starts = torch.randint(0, NCONTIG, (NREADS,), generator=g, device="cuda") * CLEN + torch.randint(0, CLEN - RLEN + 1, (NREADS,), generator=g, device="cuda")
reads = genome[starts[:, None] + torch.arange(RLEN, device="cuda")[None, :]]
flip = torch.randint(0, 2, (NREADS,), generator=g, device="cuda").bool()
reads[flip] = comp[reads[flip].long()].flip(1)
nb = NREADS * RLEN
tb = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
tb[:nb] = reads.reshape(-1)
to = (torch.arange(NREADS + 1, dtype=torch.int64, device="cuda") * RLEN)
del reads, genome
ctx = L.Context(0, stream=torch.cuda.current_stream())
say(f"# wfeatures_reads_rate [{os.environ['WFR_CHILD']}]: WF_RUN = {ctx.stat('wf_run')}; {NREADS} reads of {RLEN} bases ({nb} bases) from {NCONTIG} random contigs of {CLEN} bases, "
    f"either strand, no errors; components: cut_components_wide(count_wide_above(reads, 1), 1, 10^9); {torch.cuda.get_device_name(0)}")
REP = 5
for k in (33, 63):
    cutter, _ = ctx.count_wide_above(tb.data_ptr(), to.data_ptr(), NREADS, nb, k, 1)
    comps = ctx.cut_components_wide(cutter, 1, 10 ** 9)
    cutter.close(); del cutter
    ncomp, nmem = comps.stats()
    occ = NREADS * (RLEN - k + 1)
    say(f"k = {k}: {occ} k-mer positions, {ncomp} components, {nmem} members")
    def new():
        return ctx.features_reads_wide(comps, tb.data_ptr(), to.data_ptr(), NREADS, nb, 0)
    def old():
        t = ctx.count_wide_table(tb.data_ptr(), to.data_ptr(), NREADS, nb, k)
        try:
            return ctx.features_wide(comps, t, 0)
        finally:
            t.close()
    times = {"new": [], "old": []}
    res = {}
    for rep in range(REP + 1):                       # the first round warms up; the two routes alternate
        for name, fn in (("old", old), ("new", new)):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            res[name] = fn()
            torch.cuda.synchronize(); dt = (time.perf_counter() - t0) * 1e3
            if rep: times[name].append(dt)
    assert np.array_equal(res["new"][0], res["old"][0]) and np.array_equal(res["new"][1], res["old"][1])     # (no count reaches 32767 here)
    med = {}
    for name, what in (("new", "mf_features_reads_wide_device"), ("old", "mf_count_wide_device + mf_features_wide_device")):
        t = times[name]; med[name] = statistics.median(t)
        say(f"  {what}: wall per call (ms): {' '.join('%.1f' % x for x in t)}; median {med[name]:.1f} ms, spread {max(t) - min(t):.1f} ms, {occ / med[name] / 1e6:.2f} G positions / s")
    ctx.set_option("profile", 1); ctx.reset_timers()
    new(); torch.cuda.synchronize()
    rep_ = ctx.kernel_report()
    ctx.set_option("profile", 0)
    for nm in ("k_wf_index", "k_wf_presence", "k_wf_occ"):
        if nm in rep_: say(f"    one more call under option profile, {nm}: {rep_[nm][0]} timed launches, {rep_[nm][1]:.2f} ms")
    say(f"  k = {k}: {'the reads route is faster' if med['new'] < med['old'] else 'count + features is faster'} ({max(med.values()) / min(med.values()):.2f} x); sum of vec {int(res['new'][0].sum())}")
    comps.close(); del comps
ctx.close()
out.close()
