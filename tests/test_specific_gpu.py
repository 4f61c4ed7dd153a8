"""specific-kmers (src/tools/SpecificKmersFinder.java:65-245), specific-kmers-3 (src/tools/SpecificKmers3GroupsFinder.java:70-313) and
unique-kmers (src/tools/UniqueKmersFinder.java:73-144) on the GPU (mf_specific.hip, mf_stats.hip, mf_kmersets.hip on the join core),
through the C-ABI and the driver, against the independent restatement tests/specific_ref.py: record sets byte-identical, counters
equal.  The (nA, nB[, nC], pchi2, pmw) used here are GPU_SHAPES2 / GPU_SHAPES3 of tests/test_specific_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

import specific_ref as S
import stats3_ref as R3
import stats_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

SEED_SHARED, SEEDS = 0x5350454349, (0x41414141, 0x42424242, 0x43434343)


def _same(got, want, what):
    gk, gv = got
    wk, wv = want
    assert len(gk) == len(wk), (what, len(gk), len(wk))
    assert R.records_to_bytes(gk, gv) == R.records_to_bytes(wk, np.asarray(wv)), what


def _records(t):
    k, c = t.export(-1)
    return k, c.astype(np.int16)


def _margins(want, pmw):
    q = want["q"]
    kk = want["kk"][np.isfinite(want["kk"])]
    assert not np.any(np.abs(kk - q) <= 1e-9 * q)
    if want["p"] is not None:
        p = np.asarray(want["p"], dtype=np.float64)
        assert not np.any(np.abs(p[~np.isnan(p)] - pmw) <= 1e-12)


def _check2(ctx, groups, pchi2, pmw, recs=None):
    ga, gb, ctr = ctx.specific_kmers(*groups, p_chi2=pchi2, p_mw=pmw)
    recs = recs or [[_records(t) for t in g] for g in groups]
    want = S.specific_kmers(*recs, p_chi2=pchi2, p_mw=pmw)
    _same(ga.export(-1), want["A"], "A")
    _same(gb.export(-1), want["B"], "B")
    assert ctr == want["counters"], (ctr, want["counters"])
    assert ctr["n"] == ctr["scarce"] + ctr["chi2_rejected"] + ctr["mw_rejected"] + ctr["group_a"] + ctr["group_b"], ctr
    _margins(want, pmw)
    return ctr


def _check3(ctx, groups, pchi2, pmw, recs=None):
    ga, gb, gc, ctr = ctx.specific_kmers3(*groups, p_chi2=pchi2, p_mw=pmw)
    recs = recs or [[_records(t) for t in g] for g in groups]
    want = S.specific_kmers3(*recs, p_chi2=pchi2, p_mw=pmw)
    for t, name in ((ga, "A"), (gb, "B"), (gc, "C")):
        _same(t.export(-1), want[name], name)
    assert ctr == want["counters"], (ctr, want["counters"])
    assert ctr["group_a"] + ctr["group_b"] + ctr["group_c"] == ctr["n"] - ctr["in_all"] - ctr["scarce"] - ctr["chi2_rejected"] - ctr["mw_rejected"], ctr
    _margins(want, pmw)
    return ctr


def _synth_sample(ctx, j, group, n_reads, k, rl=100):
    """most reads from the shared seed, a share from the group's own; the generator's `sample` varies the abundances"""
    import torch
    n1 = n_reads * 4 // 5
    n2 = n_reads - n1
    bases = torch.zeros(n_reads * rl + 64, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(n_reads + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads_device(SEED_SHARED, j, 0, n1, rl, 20_000, bases.data_ptr(), offs.data_ptr())
    ctx.synth_reads_device(SEEDS[group], 0, j * n2, n2, rl, 2_000, bases.data_ptr() + n1 * rl, offs[n1:].data_ptr())
    offs[n1:] += n1 * rl
    t = ctx.count_device(bases.data_ptr(), offs.data_ptr(), n_reads, n_reads * rl, k, 0)
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("k", [21, 31])
def test_synthetic_cohorts(gpu_ctx, k):
    """4 + 4 and 4 + 4 + 4 samples; on the same tables stats-kmers and stats-kmers-3 still give what their own restatements say"""
    groups = [[_synth_sample(gpu_ctx, 4 * g + j, g, 10_000, k) for j in range(4)] for g in range(3)]
    recs = [[_records(t) for t in g] for g in groups]
    c = _check2(gpu_ctx, groups[:2], 0.05, 0.05, recs[:2])
    assert min(c["group_a"], c["group_b"], c["mw_rejected"], c["scarce"], c["unique"], c["unique_left"]) > 0, c
    _check2(gpu_ctx, groups[:2], 0.05, 0.0, recs[:2])
    _check2(gpu_ctx, groups[:2], 0.2, 0.1, recs[:2])
    c = _check3(gpu_ctx, groups, 0.05, 0.05, recs)
    assert min(c["group_a"], c["group_b"], c["group_c"], c["mw_rejected"], c["unique"]) > 0, c
    _check3(gpu_ctx, groups, 0.05, 0.0, recs)
    _check3(gpu_ctx, groups, 0.2, 0.1, recs)
    # the older tools on the same data
    chi, ga, gb, ctr = gpu_ctx.stats_kmers(*groups[:2], p_chi2=0.05, p_mw=0.05)
    want = R.stats_kmers(*recs[:2], p_chi2=0.05, p_mw=0.05)
    for t, name in ((chi, "chi"), (ga, "A"), (gb, "B")):
        _same(t.export(-1), want[name], "stats-kmers " + name)
    assert ctr == want["counters"]
    chi, ga, gb, gc, ctr = gpu_ctx.stats_kmers3(*groups, p_chi2=0.05, p_mw=0.05)
    want = R3.stats_kmers3(*recs, p_chi2=0.05, p_mw=0.05)
    for t, name in ((chi, "chi"), (ga, "A"), (gb, "B"), (gc, "C")):
        _same(t.export(-1), want[name], "stats-kmers-3 " + name)
    assert ctr == want["counters"]


def _tab(ctx, keys, counts, k=31):
    return ctx.table_from_host(np.asarray(keys, np.uint64), np.asarray(counts, np.uint16), k)


EMPTY = (np.zeros(0, np.uint64), np.zeros(0))


def _edge_cases():
    rng = np.random.default_rng(45)
    base = np.arange(0, 3000, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7) % np.uint64(1 << 62)
    base[0] = 0                                                     # the poly-A k-mer
    def sample(frac, lo, hi, sel=None):
        m = rng.random(len(base)) < frac
        if sel is not None:
            m &= sel
        return base[m], rng.integers(lo, hi, size=int(m.sum()))
    big = (base, np.full(len(base), 32767))                        # every k-mer at 32767: a k-mer of all samples where the others hold it
    part = np.arange(len(base)) % 3
    everywhere = (base[:40], np.arange(1, 41))                      # k-mers that every sample of "in all" holds, first counts 1 .. 40
    def with_all(s):
        m = ~np.isin(s[0], everywhere[0])
        return np.concatenate([everywhere[0], s[0][m]]), np.concatenate([everywhere[1], s[1][m]])
    return {
        "big": ([sample(0.7, 1, 40), big], [sample(0.5, 1, 5), sample(0.9, 1, 3)], [sample(0.4, 1, 9), big]),
        "empty in A": ([sample(0.7, 1, 40), EMPTY], [sample(0.6, 1, 40), sample(0.5, 1, 40)], [sample(0.3, 1, 40), sample(0.4, 1, 9)]),
        "empty in B": ([sample(0.7, 1, 40), sample(0.5, 1, 9)], [EMPTY, sample(0.6, 1, 40)], [sample(0.3, 1, 40), sample(0.4, 1, 9)]),
        "empty in C": ([sample(0.7, 1, 40), sample(0.5, 1, 9)], [sample(0.3, 1, 40), sample(0.4, 1, 9)], [EMPTY, sample(0.6, 1, 40)]),
        "1 1": ([sample(0.7, 1, 40)], [sample(0.6, 1, 40)], [sample(0.5, 1, 40)]),
        "1 3": ([sample(0.7, 1, 40)], [sample(0.6, 1, 40), big, sample(0.2, 1, 3)], [sample(0.5, 1, 40), sample(0.5, 1, 4)]),
        "3 1 1": ([sample(0.7, 1, 40), big, sample(0.2, 1, 3)], [sample(0.6, 1, 40)], [sample(0.5, 1, 40)]),
        "one group only": tuple([sample(0.8, 1, 40, part == g) for _ in range(3)] for g in range(3)),
        "in all": tuple([with_all(sample(0.5, 1, 40)) for _ in range(2)] for g in range(3)),
    }


@pytest.mark.parametrize("name", list(_edge_cases()))
def test_edge_tables(gpu_ctx, name):
    groups = [[_tab(gpu_ctx, *s) for s in g] for g in _edge_cases()[name]]
    for pmw in (0.05, 0.0):
        c2 = _check2(gpu_ctx, groups[:2], 0.3, pmw)
        c3 = _check3(gpu_ctx, groups, 0.3, pmw)
    if name == "one group only":
        assert c2["unique"] == c2["n"] > 0 and c2["unique_left"] == c2["group_a"] + c2["group_b"] > 0, c2
        assert c3["unique_left"] == c3["group_a"] + c3["group_b"] + c3["group_c"] > 0, c3
    if name == "in all":                                            # kept by the two-group tool (first counts 1 .. 40: one is scarce), dropped by the other
        assert c3["in_all"] >= 40 and c2["group_a"] + c2["group_b"] >= 39 and c2["scarce"] >= 1, (c2, c3)


def _many(ctx, sizes, seed):
    rng = np.random.default_rng(seed)
    keys = np.arange(1, 801, dtype=np.uint64) * np.uint64(1000003)
    groups = []
    for g, n in enumerate(sizes):
        p = np.where(np.arange(len(keys)) % 3 == g, 0.8, 0.4)
        tabs = []
        for _ in range(n):
            m = rng.random(len(keys)) < p
            tabs.append(_tab(ctx, keys[m], rng.integers(1, (12, 20, 16)[g] * (40 if n > 50 else 1), size=int(m.sum()))))
        groups.append(tabs)
    return groups


@pytest.mark.parametrize("sizes", [(16, 16), (16, 17), (150, 150), (11, 11, 10), (11, 11, 11), (100, 100, 100)])
def test_kernel_switch_and_wave_kernels(gpu_ctx, sizes):
    """N = 32: the last shape of the thread-per-row kernels; N = 33: the first of the wave-per-row kernels; N = 300: several 64-lane
    strides in every group (and a scarce bound of 15: the counts there run up to 40 times higher, so that both sides of it are met)"""
    groups = _many(gpu_ctx, sizes, 46)
    if len(sizes) == 2:
        c = _check2(gpu_ctx, groups, 0.05, 0.05)
        assert min(c["group_a"], c["group_b"], c["scarce"]) > 0, c
    else:
        c = _check3(gpu_ctx, groups, 0.05, 0.05)
        assert min(c["group_a"], c["group_b"], c["group_c"]) > 0, c


def _write_samples(tmp_path, samples, prefix):
    files = []
    for i, (k, c) in enumerate(samples):
        f = tmp_path / ("%s%d.kmers.bin" % (prefix, i))
        f.write_bytes(R.records_to_bytes(k, c))
        files.append(str(f))
    return files


def _file_cohort(seed, n, pool_size=20000):
    """n samples over one pool, a twentieth of each sample's k-mers listed twice, some counts at 32767"""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 1 << 62, size=pool_size, dtype=np.uint64)
    pool[0] = 0
    samples = []
    for j in range(n):
        m = rng.random(len(pool)) < (0.5, 0.35, 0.42)[j % 3]
        k = pool[m]
        c = rng.integers(1, 60, size=len(k)).astype(np.int16)
        dup = rng.choice(len(k), size=len(k) // 20, replace=False)           # k-mers listed twice in one file
        k = np.concatenate([k, k[dup]])
        c = np.concatenate([c, rng.integers(0, 3, size=len(dup)).astype(np.int16)])
        c[:3] = 32767
        samples.append((k, c))
    return pool, samples


def test_slices_give_identical_files_and_duplicates(gpu_ctx, tmp_path):
    _, samples = _file_cohort(47, 8)
    samples = sorted(samples, key=lambda s: len(s[0]))              # (the groups differ in how much of the pool they hold)
    g2, g3 = [samples[:4], samples[4:]], [samples[:3], samples[3:6], samples[6:]]
    f2 = [_write_samples(tmp_path, g, "ab"[i]) for i, g in enumerate(g2)]
    f3 = [_write_samples(tmp_path, g, "xyz"[i]) for i, g in enumerate(g3)]
    w2, w3 = S.specific_kmers(*g2, p_chi2=0.3, p_mw=0.2), S.specific_kmers3(*g3, p_chi2=0.3, p_mw=0.2)
    assert len(w2["A"][0]) and len(w2["B"][0]) and len(w3["A"][0]) + len(w3["B"][0]) + len(w3["C"][0])
    try:
        for n_slices in (1, 3, 7):
            gpu_ctx.set_option("stats_slices", n_slices)
            o2, o3 = tmp_path / ("o2_%d" % n_slices), tmp_path / ("o3_%d" % n_slices)
            os.makedirs(o2), os.makedirs(o3)
            assert gpu_ctx.specific_kmers_files(*f2, str(o2), p_chi2=0.3, p_mw=0.2) == w2["counters"]
            assert sorted(os.listdir(o2)) == ["filtered_groupA.kmers.bin", "filtered_groupB.kmers.bin"]
            for g in "AB":
                assert (o2 / ("filtered_group%s.kmers.bin" % g)).read_bytes() == R.records_to_bytes(*w2[g]), g
            assert gpu_ctx.specific_kmers3_files(*f3, str(o3), p_chi2=0.3, p_mw=0.2) == w3["counters"]
            assert len(os.listdir(o3)) == 3                         # (no filtered_chisquared file)
            for g in "ABC":
                assert (o3 / ("filtered_group%s.kmers.bin" % g)).read_bytes() == R.records_to_bytes(*w3[g]), g
    finally:
        gpu_ctx.set_option("stats_slices", 0)


def test_unique_kmers(gpu_ctx, tmp_path):
    """pooled sums that cross b where no single record does (not there), a k-mer whose records above b add past 32767, a filter file that
    holds everything, no filter at all; files and resident tables, one slice and several"""
    pool, samples = _file_cohort(48, 6, pool_size=8000)
    ones = (pool[:500], np.ones(500, np.int16))                    # count 1 in two inputs: 1 + 1 crosses b = 1, no record does
    inputs = [(np.concatenate([s[0], ones[0]]), np.concatenate([s[1], ones[1]])) for s in samples[:3]]
    inputs[0][1][:3] = 32767
    filters = samples[3:5]
    everything = (pool, np.full(len(pool), 9, np.int16))
    fin, ff, fall = _write_samples(tmp_path, inputs, "in"), _write_samples(tmp_path, filters, "f"), _write_samples(tmp_path, [everything], "all")
    k = 31
    try:
        for n_slices in (1, 3):
            gpu_ctx.set_option("stats_slices", n_slices)
            for b in (1, 0, 4):
                for fl, ffl, tag in ((filters, ff, "f"), ([everything], fall, "all"), ([], [], "none")):
                    want = S.unique_kmers(inputs, fl, b=b)
                    out, st = tmp_path / ("u_%d_%d_%s.kmers.bin" % (n_slices, b, tag)), tmp_path / ("u_%d_%d_%s.stat.txt" % (n_slices, b, tag))
                    assert gpu_ctx.unique_kmers_files(fin, ffl, k, str(out), str(st), max_bad=b) == (want["n"], want["c"])
                    assert out.read_bytes() == R.records_to_bytes(*want["out"]) and st.read_text() == R.stat_txt(want["hm"][1])
                    if tag == "all":
                        assert want["c"] == 0 and want["n"] > 0
                    if tag == "none":
                        assert want["out"][1].max() == 32767
                    # resident tables hold a file's records summed: loaded at b they are what the tool pools
                    tin = [gpu_ctx.load_kmers([f], b, k) for f in fin]
                    tf = [gpu_ctx.load_kmers([f], b, k) for f in ffl]
                    t, n = gpu_ctx.unique_kmers(tin, tf, max_bad=b)
                    assert n == want["n"]
                    _same(t.export(-1), want["out"], "tables")
    finally:
        gpu_ctx.set_option("stats_slices", 0)
    want = S.unique_kmers(inputs, [], b=1)
    assert not np.isin(ones[0][~np.isin(ones[0], np.concatenate([s[0][s[1] > 1] for s in inputs]))], want["hm"][0]).any()


def test_limits(gpu_ctx, tmp_path):
    one = _tab(gpu_ctx, [5, 6, 7, 8, 9], np.ones(5))
    big = _tab(gpu_ctx, [5, 1 << 62], [3, 3])
    with pytest.raises(Exception, match="at most 1024"):
        gpu_ctx.specific_kmers([one] * 600, [one] * 425)
    with pytest.raises(Exception, match="at most 1024"):
        gpu_ctx.specific_kmers3([one] * 400, [one] * 400, [one] * 225)
    for groups in (([], [one]), ([one], [])):
        with pytest.raises(Exception, match="both groups need at least one sample"):
            gpu_ctx.specific_kmers(*groups)
    for groups in (([], [one], [one]), ([one], [], [one]), ([one], [one], [])):
        with pytest.raises(Exception, match="every group needs at least one sample"):
            gpu_ctx.specific_kmers3(*groups)
    with pytest.raises(Exception, match=r"not in \[0, 1\]"):
        gpu_ctx.specific_kmers([one], [one], p_chi2=2.0)
    with pytest.raises(Exception, match=r"not in \[0, 1\]"):
        gpu_ctx.specific_kmers3([one], [one], [one], p_chi2=-0.5)
    for bad in (lambda: gpu_ctx.specific_kmers([big], [one]), lambda: gpu_ctx.specific_kmers([one], [big]),
                lambda: gpu_ctx.specific_kmers3([one], [one], [big]), lambda: gpu_ctx.unique_kmers([big], [one]),
                lambda: gpu_ctx.unique_kmers([one], [big])):
        with pytest.raises(Exception, match=r"2\^62"):
            bad()
    with pytest.raises(Exception, match="is negative"):
        gpu_ctx.unique_kmers([one], [one], max_bad=-1)
    f = _write_samples(tmp_path, [(np.array([5, 6], np.uint64), np.array([3, 3]))], "k")
    for k in (0, 32):
        with pytest.raises(Exception, match=r"k must be in \[1,31\]"):
            gpu_ctx.unique_kmers_files(f, f, k, str(tmp_path / "x.kmers.bin"))
    # the errors leave nothing behind on the context
    c = _check2(gpu_ctx, [[one, _tab(gpu_ctx, [5, 6], [4, 9])], [one]], 0.3, 0.05)
    assert c["n"] == 5


def test_cli_round_trips(gpu_ctx, ref_files, tmp_path):
    exe = os.path.join(ROOT, "metafast.sh")
    wd = tmp_path / "w"
    r = subprocess.run([exe, "-t", "kmer-counter-many", "-k", "31", "-i", *ref_files[:3], "-w", str(wd)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    f = sorted(str(p) for p in (wd / "kmers").iterdir())
    assert len(f) == 3
    recs = {p: R.records_from_bytes(open(p, "rb").read()) for p in f}
    for i, pmw in enumerate((0.0, 0.3)):
        # specific-kmers: two samples against one
        want = S.specific_kmers([recs[f[0]], recs[f[1]]], [recs[f[2]]], p_mw=pmw)
        c = want["counters"]
        assert c["group_a"] > 0 and c["group_b"] > 0, c        # (no scarce k-mer here: kmer-counter-many keeps counts > 1, the bound is 1)
        w2 = tmp_path / ("w2_%d" % i)
        cmd = [exe, "-t", "specific-kmers", "-A", f[0], f[1], "-B", f[2], "-pmw", str(pmw), "-w", str(w2), "-v"]
        r = subprocess.run(cmd + ["--force"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        log = (w2 / "log").read_text()
        r = subprocess.run(cmd + ["-c"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "SUCCESS file found" in r.stderr, r.stderr
        for g in "AB":
            assert (w2 / "kmers" / ("filtered_group%s.kmers.bin" % g)).read_bytes() == R.records_to_bytes(*want[g]), g
        assert sorted(os.listdir(w2 / "kmers")) == ["filtered_groupA.kmers.bin", "filtered_groupB.kmers.bin"] and (w2 / "SUCCESS").exists()
        for line in ("Total specific k-mers in Group A = %d" % c["group_a"], "Total specific k-mers in Group B = %d" % c["group_b"],
                     "Total unique k-mers = %d" % c["unique"], "Total scarce k-mers = = %d" % c["scarce"],
                     "Total skipped by chi-squared test = %d" % c["chi2_rejected"], "Total skipped by Mann-Whitney test = %d" % c["mw_rejected"],
                     "Total unique left = %d" % c["unique_left"], "Total kmers left = %d" % (c["group_a"] + c["group_b"]), "Processed %d k-mers" % c["n"]):
            assert line in log, line
        # specific-kmers-3: the grouping of the stats-kmers-3 round trip
        A, B, C = [f[0], f[1]], [f[1], f[2]], [f[2], f[0]]
        want = S.specific_kmers3([recs[p] for p in A], [recs[p] for p in B], [recs[p] for p in C], p_mw=pmw)
        c = want["counters"]
        assert c["group_a"] + c["group_b"] + c["group_c"] > 0, c
        w3 = tmp_path / ("w3_%d" % i)
        r = subprocess.run([exe, "-t", "specific-kmers-3", "-A", *A, "-B", *B, "-C", *C, "-pmw", str(pmw), "-w", str(w3), "-v"], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        log = (w3 / "log").read_text()
        for g in "ABC":
            assert (w3 / "kmers" / ("filtered_group%s.kmers.bin" % g)).read_bytes() == R.records_to_bytes(*want[g]), g
        assert len(os.listdir(w3 / "kmers")) == 3 and (w3 / "SUCCESS").exists()
        for line in ("Total k-mers count = %d" % c["n"], "Total unique k-mers = %d" % c["unique"], "Total k-mers present in all files = %d" % c["in_all"],
                     "Total k-mers left = %d" % (c["group_a"] + c["group_b"] + c["group_c"]), "Total unique left = %d" % c["unique_left"],
                     "Total group C k-mers = %d" % c["group_c"], "Total scarce k-mers = %d" % c["scarce"],
                     "Total skipped by Chi-squared test = %d" % c["chi2_rejected"], "Total skipped by Mann-Whitney test = %d" % c["mw_rejected"]):
            assert line in log, line
    # unique-kmers: two inputs pooled, one filter
    want = S.unique_kmers([recs[f[0]], recs[f[1]]], [recs[f[2]]], b=2)
    assert 0 < want["c"] < want["n"]
    w4 = tmp_path / "w4"
    r = subprocess.run([exe, "-t", "unique-kmers", "-k", "31", "-i", f[0], f[1], "--filter-kmers", f[2], "-b", "2", "-w", str(w4)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (w4 / "kmers" / "filtered.kmers.bin").read_bytes() == R.records_to_bytes(*want["out"])
    assert (w4 / "stats" / "filtered.stat.txt").read_text() == R.stat_txt(want["hm"][1])
    assert "of them is good (present in one dataset and missing in other)" in (w4 / "log").read_text() and (w4 / "SUCCESS").exists()
    r = subprocess.run([exe, "-t", "unique-kmers", "-k", "32", "-i", f[0], "--filter-kmers", f[2], "-w", str(tmp_path / "w5")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 1 and "no more than 31" in r.stderr
    r = subprocess.run([exe, "-t", "specific-kmers", "-A", f[0], "-w", str(tmp_path / "w6")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "Mandatory argument --b-kmers" in r.stderr
