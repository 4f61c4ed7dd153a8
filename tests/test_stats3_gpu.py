"""stats-kmers-3 (src/tools/StatsKmers3GroupsFinder.java:92-377) and kmers-grouped-counter (src/tools/KmersGroupedSamplesCounter.java:82-190)
on the GPU (mf_stats.hip on the join core mf_join.hip), through the C-ABI, against the independent restatement tests/stats3_ref.py: record
sets byte-identical, counters equal.  The (nA, nB, nC, pchi2, pmw) used here are the GPU_SHAPES of tests/test_stats3_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

import stats3_ref as R3
import stats_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

SEED_SHARED, SEEDS = 0x5354415453, (0x41414141, 0x42424242, 0x43434343)


def _export(t):
    return t.export(-1)


def _same(got, want, what):
    gk, gv = got
    wk, wv = want
    assert len(gk) == len(wk), (what, len(gk), len(wk))
    assert R.records_to_bytes(gk, gv) == R.records_to_bytes(wk, np.asarray(wv)), what


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


def _records(t):
    k, c = t.export(-1)
    return k, c.astype(np.int16)


def _check_stats(ctx, groups, b, pchi2, pmw, recs=None):
    """recs: the groups' records, where a caller checks one cohort several times"""
    chi, ga, gb, gc, ctr = ctx.stats_kmers3(*groups, p_chi2=pchi2, p_mw=pmw, max_bad=b)
    recs = recs or [[_records(t) for t in g] for g in groups]
    want = R3.stats_kmers3(*recs, b=b, p_chi2=pchi2, p_mw=pmw)
    _same(_export(chi), want["chi"], "chi")
    _same(_export(ga), want["A"], "A")
    _same(_export(gb), want["B"], "B")
    _same(_export(gc), want["C"], "C")
    assert ctr == want["counters"], (ctr, want["counters"])
    R3.check_identities(ctr, len(chi))
    q = want["q"]
    kk = want["kk"][np.isfinite(want["kk"])]
    assert not np.any(np.abs(kk - q) <= 1e-9 * q)
    if want["p"] is not None:
        assert not np.any(np.abs(want["p"][~np.isnan(want["p"])] - pmw) <= 1e-12)
    return ctr


@pytest.mark.parametrize("k", [21, 31])
def test_synthetic_cohort(gpu_ctx, k):
    groups = [[_synth_sample(gpu_ctx, 4 * g + j, g, 120_000, k) for j in range(4)] for g in range(3)]
    recs = [[_records(t) for t in g] for g in groups]
    c = _check_stats(gpu_ctx, groups, 0, 0.05, 0.05, recs)
    assert min(c["group_a"], c["group_b"], c["group_c"], c["mw_rejected"], c["chi2_rejected"], c["unique"]) > 0, c
    _check_stats(gpu_ctx, groups, 0, 0.05, 0.0, recs)
    _check_stats(gpu_ctx, groups, 2, 0.2, 0.1, recs)


def _tab(ctx, keys, counts, k=31):
    return ctx.table_from_host(np.asarray(keys, np.uint64), np.asarray(counts, np.uint16), k)


EMPTY = (np.zeros(0, np.uint64), np.zeros(0))


def _edge_cases():
    rng = np.random.default_rng(35)
    base = np.arange(0, 3000, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7) % np.uint64(1 << 62)
    base[0] = 0                                                     # the poly-A k-mer
    def sample(frac, lo, hi, sel=None):
        m = rng.random(len(base)) < frac
        if sel is not None:
            m &= sel
        return base[m], rng.integers(lo, hi, size=int(m.sum()))
    big = (base, np.full(len(base), 32767))                        # counts at 32767: F large, M large
    tiny = (base[:1], np.array([32767]))                            # F = 32767: v = c * M / F >= 32768 -> values wrap
    third = np.arange(len(base)) % 3
    same = sample(0.8, 1, 30)
    return {
        "wrap": ([sample(0.7, 1, 40), sample(0.6, 1, 40), big], [sample(0.5, 1, 5), tiny, sample(0.9, 1, 3)], [sample(0.4, 1, 9), big, tiny]),
        "empty in A": ([sample(0.7, 1, 40), EMPTY], [sample(0.6, 1, 40), sample(0.5, 1, 40)], [sample(0.3, 1, 40), sample(0.4, 1, 9)]),
        "empty in B": ([sample(0.7, 1, 40), sample(0.5, 1, 9)], [sample(0.6, 1, 40), EMPTY], [sample(0.3, 1, 40), sample(0.4, 1, 9)]),
        "empty in C": ([sample(0.7, 1, 40), sample(0.5, 1, 9)], [sample(0.3, 1, 40), sample(0.4, 1, 9)], [EMPTY, sample(0.6, 1, 40)]),
        "1 1 1": ([sample(0.7, 1, 40)], [sample(0.6, 1, 40)], [sample(0.5, 1, 40)]),
        "1 3 2": ([sample(0.7, 1, 40)], [sample(0.6, 1, 40), big, tiny], [sample(0.5, 1, 40), sample(0.5, 1, 4)]),
        "3 1 1": ([sample(0.7, 1, 40), big, tiny], [sample(0.6, 1, 40)], [sample(0.5, 1, 40)]),
        "ties": ([same, same, same], [same, sample(0.8, 1, 30), same], [same, same, sample(0.8, 1, 30)]),
        # every k-mer in one group only: unique, and two of the three means are 0
        "one group only": tuple([sample(0.8, 1, 40, third == g) for _ in range(3)] for g in range(3)),
    }


@pytest.mark.parametrize("name", list(_edge_cases()))
def test_edge_tables(gpu_ctx, name):
    groups = [[_tab(gpu_ctx, *s) for s in g] for g in _edge_cases()[name]]
    for pmw in (0.05, 0.0):
        for b in (0, 1):
            c = _check_stats(gpu_ctx, groups, b, 0.3, pmw)
    if name == "one group only":
        assert c["unique"] > 0 and c["unique_left"] == c["group_a"] + c["group_b"] + c["group_c"] > 0, c


@pytest.mark.parametrize("sizes", [(11, 11, 10), (11, 11, 11), (100, 100, 100)])
def test_kernel_switch_and_wave_kernel(gpu_ctx, sizes):
    """N = 32: the last shape of the thread-per-row kernel; N = 33: the first of the wave-per-row kernel; N = 300: several 64-lane
    strides in every group"""
    rng = np.random.default_rng(36)
    keys = np.arange(1, 801, dtype=np.uint64) * np.uint64(1000003)
    groups = []
    for g, n in enumerate(sizes):
        p = np.where(np.arange(len(keys)) % 3 == g, 0.8, 0.4)
        tabs = []
        for _ in range(n):
            m = rng.random(len(keys)) < p
            tabs.append(_tab(gpu_ctx, keys[m], rng.integers(1, (12, 20, 16)[g], size=int(m.sum()))))
        groups.append(tabs)
    c = _check_stats(gpu_ctx, groups, 0, 0.05, 0.05)
    assert c["group_a"] > 0 and c["group_b"] > 0 and c["group_c"] > 0, c


def test_limits(gpu_ctx):
    one = _tab(gpu_ctx, [5, 6, 7, 8, 9], np.ones(5))
    with pytest.raises(Exception, match="at most 1024"):
        gpu_ctx.stats_kmers3([one] * 400, [one] * 400, [one] * 225)
    for groups in (([], [one], [one]), ([one], [], [one]), ([one], [one], [])):
        with pytest.raises(Exception, match="at least one sample"):
            gpu_ctx.stats_kmers3(*groups)
    with pytest.raises(Exception, match=r"not in \[0, 1\]"):
        gpu_ctx.stats_kmers3([one], [one], [one], p_chi2=2.0)
    with pytest.raises(Exception, match="at most 1022"):
        gpu_ctx.kmers_grouped_count(one, [one] * 1023, [one], [one])


def test_key_limit_through_the_presence_word(gpu_ctx):
    """a key >= 2^62 in any group is an error of the union pass, and the error leaves nothing behind on the context"""
    rng = np.random.default_rng(39)
    pool = rng.integers(0, 1 << 62, size=400, dtype=np.uint64)
    tabs = []
    for j in range(6):
        m = rng.random(len(pool)) < 0.6
        tabs.append(_tab(gpu_ctx, pool[m], rng.integers(1, 30, size=int(m.sum()))))
    one = _tab(gpu_ctx, [5, 6], [3, 3])
    big = _tab(gpu_ctx, [5, 1 << 62], [3, 3])
    for bad in (lambda: gpu_ctx.stats_kmers3([big], [one], [one]), lambda: gpu_ctx.stats_kmers3([one], [big], [one]),
                lambda: gpu_ctx.stats_kmers3([one], [one], [big]), lambda: gpu_ctx.kmers_grouped_count(one, [one], [big], []),
                lambda: gpu_ctx.kmers_grouped_count(big, [one], [one], [one])):
        with pytest.raises(Exception, match=r"2\^62"):
            bad()
        _check_stats(gpu_ctx, [tabs[:2], tabs[2:4], tabs[4:]], 0, 0.3, 0.05)


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
    _, samples = _file_cohort(37, 8)
    samples = sorted(samples, key=lambda s: len(s[0]))              # (the groups differ in how much of the pool they hold)
    groups = [samples[:3], samples[3:6], samples[6:]]
    files = [_write_samples(tmp_path, g, "abc"[i]) for i, g in enumerate(groups)]
    want = R3.stats_kmers3(*groups, b=1, p_chi2=0.3, p_mw=0.2)
    names = ("filtered_chisquared.kmers.bin", "filtered_groupA.kmers.bin", "filtered_groupB.kmers.bin", "filtered_groupC.kmers.bin",
             "filtered_chisquared.stat.txt")
    blobs = None
    try:
        for S in (1, 3, 7):
            gpu_ctx.set_option("stats_slices", S)
            out = tmp_path / ("o%d" % S)
            os.makedirs(out)
            ctr = gpu_ctx.stats_kmers3_files(*files, str(out), p_chi2=0.3, p_mw=0.2, max_bad=1)
            assert ctr == want["counters"]
            got = [(out / n).read_bytes() for n in names]
            assert got[:4] == [R.records_to_bytes(*want[x]) for x in ("chi", "A", "B", "C")]
            assert got[4] == R.stat_txt(want["chi"][1]).encode()
            blobs = blobs or got
            assert got == blobs
    finally:
        gpu_ctx.set_option("stats_slices", 0)
    assert len(want["chi"][0]) > 0


def test_kmers_grouped_counter(gpu_ctx, tmp_path):
    pool, samples = _file_cohort(38, 9, pool_size=5000)
    rng = np.random.default_rng(40)
    outside = rng.integers(0, 1 << 40, size=300, dtype=np.uint64)           # keys of -kf that no group holds
    kf = [(np.concatenate([pool[:1500], outside[:200]]), np.concatenate([rng.integers(0, 3, size=1500), np.ones(200)]).astype(np.int16)),
          (np.concatenate([pool[1000:2500], outside[100:]]), np.ones(1700, np.int16))]                                    # (k-mers listed in both files)
    groups = [samples[:4], samples[4:6], samples[6:]]
    fkf = _write_samples(tmp_path, kf, "kf")
    files = [_write_samples(tmp_path, g, ("cd", "uc", "ni")[i]) for i, g in enumerate(groups)]
    k = 31
    try:
        for S in (1, 3):
            gpu_ctx.set_option("stats_slices", S)
            for b in (0, 1):
                wk, wc = R3.kmers_grouped_count(kf, *groups, b=b)
                assert (wc.sum(axis=1) == 0).sum() >= 300 and (wc > 0).all(axis=1).any()
                out = tmp_path / ("g_%d_%d.txt" % (S, b))
                assert gpu_ctx.kmers_grouped_count_files(fkf, *files, k, str(out), max_bad=b) == len(wk)
                assert out.read_text() == R3.groups_txt(wk, wc, k)
                tkf = gpu_ctx.load_kmers(fkf, 0, k)
                tabs = [[gpu_ctx.load_kmers([f], b, k) for f in g] for g in files]
                gk, gc = gpu_ctx.kmers_grouped_count(tkf, *tabs, max_bad=b)
                assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    finally:
        gpu_ctx.set_option("stats_slices", 0)
    # an empty group and an empty -kf
    gk, gc = gpu_ctx.kmers_grouped_count(gpu_ctx.load_kmers(fkf, 0, k), [gpu_ctx.load_kmers([files[0][0]], 1, k)], [], [], max_bad=1)
    wk, wc = R3.kmers_grouped_count(kf, groups[0][:1], [], [], b=1)
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    gk, gc = gpu_ctx.kmers_grouped_count(_tab(gpu_ctx, [], []), [gpu_ctx.load_kmers([files[0][0]], 1, k)], [], [])
    assert len(gk) == 0 and gc.shape == (0, 3)


def test_cli_round_trip(gpu_ctx, ref_files, tmp_path):
    exe = os.path.join(ROOT, "metafast.sh")
    wd = tmp_path / "w"
    r = subprocess.run([exe, "-t", "kmer-counter-many", "-k", "31", "-i", *ref_files[:3], "-w", str(wd)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    f = sorted(str(p) for p in (wd / "kmers").iterdir())
    assert len(f) == 3
    A, B, C = [f[0], f[1]], [f[1], f[2]], [f[2], f[0]]
    recs = {p: R.records_from_bytes(open(p, "rb").read()) for p in f}
    # (2 against 2 with a shared file: p >= 0.245, so the default -pmw 0.05 would reject every row; tests/test_stats3_cpu.py checks on
    # the oracle's counts that both runs leave a chi-squared list and groups, and that -pmw 0.3 rejects some rows and keeps others)
    for i, pmw in enumerate((0.0, 0.3)):
        want = R3.stats_kmers3([recs[p] for p in A], [recs[p] for p in B], [recs[p] for p in C], p_mw=pmw)
        c = want["counters"]
        assert len(want["chi"][0]) > 0 and c["group_a"] + c["group_b"] + c["group_c"] > 0 and (c["mw_rejected"] > 0) == (pmw > 0), c
        w3 = tmp_path / ("w3_%d" % i)
        cmd = [exe, "-t", "stats-kmers-3", "-A", *A, "-B", *B, "-C", *C, "-pmw", str(pmw), "-w", str(w3), "-v"]
        r = subprocess.run(cmd + ["--force"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        log = (w3 / "log").read_text()
        r = subprocess.run(cmd + ["-c"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "SUCCESS file found" in r.stderr, r.stderr
        kd = w3 / "kmers"
        for name, key in (("filtered_chisquared", "chi"), ("filtered_groupA", "A"), ("filtered_groupB", "B"), ("filtered_groupC", "C")):
            assert (kd / (name + ".kmers.bin")).read_bytes() == R.records_to_bytes(*want[key]), name
        assert (kd / "filtered_chisquared.stat.txt").read_text() == R.stat_txt(want["chi"][1])
        assert (w3 / "SUCCESS").exists()
        for line in ("Total k-mers count = %d" % c["n"], "Total unique k-mers = %d" % c["unique"], "Total k-mers present in all files = %d" % c["in_all"],
                     "Total k-mers left = %d" % (c["group_a"] + c["group_b"] + c["group_c"]), "Total unique left = %d" % c["unique_left"],
                     "Total group A k-mers = %d" % c["group_a"], "Total group B k-mers = %d" % c["group_b"], "Total group C k-mers = %d" % c["group_c"],
                     "Total scarce k-mers = %d" % c["scarce"], "Total skipped by Chi-squared test = %d" % c["chi2_rejected"],
                     "Total skipped by Mann-Whitney test = %d" % c["mw_rejected"]):
            assert line in log, line
    w4 = tmp_path / "w4"
    r = subprocess.run([exe, "-t", "kmers-grouped-counter", "-k", "31", "-kf", f[0], f[1], "-cd", *A, "-uc", *B, "-nonibd", *C, "-w", str(w4)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    wk, wc = R3.kmers_grouped_count([recs[f[0]], recs[f[1]]], [recs[p] for p in A], [recs[p] for p in B], [recs[p] for p in C], b=1)
    assert (w4 / "kmers" / "kmers.groups.txt").read_text() == R3.groups_txt(wk, wc, 31)
    assert (w4 / "SUCCESS").exists()
