"""stats-kmers (src/tools/StatsKmersFinder.java:89-297) and kmers-samples-counter (src/tools/KmersSamplesCounter.java:69-140) on the GPU
(mf_stats.hip on the join core mf_join.hip), through the C-ABI, against the independent restatement tests/stats_ref.py: record sets byte-identical, counters equal."""
import os
import subprocess

import numpy as np
import pytest

import stats_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

SEED_SHARED, SEED_A, SEED_B = 0x5354415453, 0x41414141, 0x42424242


def _export(t):
    k, c = t.export(-1)
    return k, c


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
    # (the group's share: one small genome set per group, read at several-fold coverage, so that most of its k-mers are in every sample of the group)
    ctx.synth_reads_device(SEED_A if group == 0 else SEED_B, 0, j * n2, n2, rl, 2_000, bases.data_ptr() + n1 * rl, offs[n1:].data_ptr())
    offs[n1:] += n1 * rl
    t = ctx.count_device(bases.data_ptr(), offs.data_ptr(), n_reads, n_reads * rl, k, 0)
    torch.cuda.synchronize()
    return t


def _records(t):
    k, c = t.export(-1)
    return k, c.astype(np.int16)


def _check_stats(ctx, ta, tb, b, pchi2, pmw):
    chi, ga, gb, ctr = ctx.stats_kmers(ta, tb, p_chi2=pchi2, p_mw=pmw, max_bad=b)
    want = R.stats_kmers([_records(t) for t in ta], [_records(t) for t in tb], b=b, p_chi2=pchi2, p_mw=pmw)
    _same(_export(chi), want["chi"], "chi")
    _same(_export(ga), want["A"], "A")
    _same(_export(gb), want["B"], "B")
    assert ctr == want["counters"], (ctr, want["counters"])
    q = want["q"]
    assert not np.any(np.abs(want["kk"] - q) <= 1e-9 * q)
    if want["p"] is not None:
        assert not np.any(np.abs(want["p"][~np.isnan(want["p"])] - pmw) <= 1e-12)
    return ctr


@pytest.mark.parametrize("k", [21, 31])
def test_synthetic_cohort(gpu_ctx, k):
    ta = [_synth_sample(gpu_ctx, j, 0, 120_000, k) for j in range(6)]
    tb = [_synth_sample(gpu_ctx, 6 + j, 1, 120_000, k) for j in range(6)]
    c = _check_stats(gpu_ctx, ta, tb, 0, 0.05, 0.05)
    assert c["group_a"] > 0 and c["group_b"] > 0 and c["mw_rejected"] > 0 and c["chi2_rejected"] > 0 and c["unique"] > 0, c
    _check_stats(gpu_ctx, ta, tb, 0, 0.05, 0.0)
    _check_stats(gpu_ctx, ta, tb, 2, 0.2, 0.1)


def _tab(ctx, keys, counts, k=31):
    return ctx.table_from_host(np.asarray(keys, np.uint64), np.asarray(counts, np.uint16), k)


def test_edge_tables(gpu_ctx):
    rng = np.random.default_rng(5)
    base = np.arange(0, 3000, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7) % np.uint64(1 << 62)
    base[0] = 0                                                     # the poly-A k-mer
    def sample(frac, lo, hi):
        m = rng.random(len(base)) < frac
        c = rng.integers(lo, hi, size=int(m.sum()))
        return base[m], c
    big = (base, np.full(len(base), 32767))                        # counts at 32767: F large, M large
    tiny = (base[:1], np.array([32767]))                            # F = 32767: v = c * M / F >= 32768 -> values wrap
    cases = [
        ([sample(0.7, 1, 40), sample(0.6, 1, 40), big], [sample(0.5, 1, 5), tiny, sample(0.9, 1, 3)]),
        ([sample(0.7, 1, 40), (np.zeros(0, np.uint64), np.zeros(0))], [sample(0.6, 1, 40), sample(0.5, 1, 40)]),   # empty sample in A
        ([sample(0.7, 1, 40), sample(0.5, 1, 9)], [sample(0.6, 1, 40), (np.zeros(0, np.uint64), np.zeros(0))]),     # empty sample in B
        ([sample(0.7, 1, 40)], [sample(0.6, 1, 40), big, tiny]),                                                       # nA = 1
        ([sample(0.7, 1, 40), big, tiny], [sample(0.6, 1, 40)]),                                                       # nB = 1
    ]
    same = sample(0.8, 1, 30)
    cases.append(([same, same, same], [same, sample(0.8, 1, 30), same]))                                              # identical samples: ties
    for pmw in (0.05, 0.0):
        for ca, cb in cases:
            ta = [_tab(gpu_ctx, *s) for s in ca]
            tb = [_tab(gpu_ctx, *s) for s in cb]
            _check_stats(gpu_ctx, ta, tb, 0, 0.3, pmw)
            _check_stats(gpu_ctx, ta, tb, 1, 0.3, pmw)


def test_large_n_and_the_limit(gpu_ctx):
    rng = np.random.default_rng(6)
    keys = np.arange(1, 801, dtype=np.uint64) * np.uint64(1000003)
    tabs = []
    for j in range(300):
        grp = j >= 150
        p = np.where(np.arange(len(keys)) % 3 == (1 if grp else 2), 0.8, 0.4)
        m = rng.random(len(keys)) < p
        tabs.append(_tab(gpu_ctx, keys[m], rng.integers(1, 20 if grp else 12, size=int(m.sum()))))
    c = _check_stats(gpu_ctx, tabs[:150], tabs[150:], 0, 0.05, 0.05)       # (N = 300: the wave-per-row kernel)
    assert c["group_a"] + c["group_b"] > 0
    one = _tab(gpu_ctx, keys[:5], np.ones(5))
    with pytest.raises(Exception, match="at most 1024"):
        gpu_ctx.stats_kmers([one] * 600, [one] * 425)
    with pytest.raises(Exception, match="at least one sample"):
        gpu_ctx.stats_kmers([one], [])


def _write_samples(tmp_path, samples, prefix):
    files = []
    for i, (k, c) in enumerate(samples):
        f = tmp_path / ("%s%d.kmers.bin" % (prefix, i))
        f.write_bytes(R.records_to_bytes(k, c))
        files.append(str(f))
    return files


def test_slices_give_identical_files_and_duplicates(gpu_ctx, tmp_path):
    rng = np.random.default_rng(7)
    pool = rng.integers(0, 1 << 62, size=20000, dtype=np.uint64)
    pool[0] = 0
    samples = []
    for j in range(8):
        m = rng.random(len(pool)) < (0.5 if j < 4 else 0.35)
        k = pool[m]
        c = rng.integers(1, 60, size=len(k)).astype(np.int16)
        dup = rng.choice(len(k), size=len(k) // 20, replace=False)           # k-mers listed twice in one file
        k = np.concatenate([k, k[dup]])
        c = np.concatenate([c, rng.integers(0, 3, size=len(dup)).astype(np.int16)])
        c[:3] = 32767
        samples.append((k, c))
    fa = _write_samples(tmp_path, samples[:4], "a")
    fb = _write_samples(tmp_path, samples[4:], "b")
    want = R.stats_kmers(samples[:4], samples[4:], b=1, p_chi2=0.3, p_mw=0.2)
    blobs = None
    try:
        for S in (1, 3, 16):
            gpu_ctx.set_option("stats_slices", S)
            out = tmp_path / ("o%d" % S)
            os.makedirs(out)
            ctr = gpu_ctx.stats_kmers_files(fa, fb, str(out), p_chi2=0.3, p_mw=0.2, max_bad=1)
            assert ctr == want["counters"]
            got = [(out / n).read_bytes() for n in ("filtered_chisquared.kmers.bin", "filtered_groupA.kmers.bin", "filtered_groupB.kmers.bin",
                                                     "filtered_chisquared.stat.txt")]
            assert got[0] == R.records_to_bytes(*want["chi"]) and got[1] == R.records_to_bytes(*want["A"]) and got[2] == R.records_to_bytes(*want["B"])
            assert got[3] == R.stat_txt(want["chi"][1]).encode()
            blobs = blobs or got
            assert got == blobs
    finally:
        gpu_ctx.set_option("stats_slices", 0)


def _counter_cohort():
    """7 samples over a pool of 5 000 keys, a tenth of each sample's k-mers listed twice"""
    rng = np.random.default_rng(8)
    pool = rng.integers(0, 1 << 40, size=5000, dtype=np.uint64)
    samples = []
    for j in range(7):
        m = rng.random(len(pool)) < 0.4
        k = pool[m]
        c = rng.integers(0, 6, size=len(k)).astype(np.int16)
        dup = rng.choice(len(k), size=len(k) // 10, replace=False)
        samples.append((np.concatenate([k, k[dup]]), np.concatenate([c, rng.integers(0, 6, size=len(dup)).astype(np.int16)])))
    return samples


def test_kmers_samples_counter(gpu_ctx, tmp_path):
    samples = _counter_cohort()
    files = _write_samples(tmp_path, samples, "s")
    for b in (0, 1, 3):
        wk, wn = R.kmers_samples_count(samples, b)
        out, st = tmp_path / ("n%d.kmers.bin" % b), tmp_path / ("n%d.stat.txt" % b)
        n = gpu_ctx.kmers_samples_count_files(files, 31, str(out), str(st), max_bad=b)
        assert n == len(wk)
        assert out.read_bytes() == R.records_to_bytes(wk, wn)
        assert st.read_text() == R.stat_txt(wn)
        tabs = [gpu_ctx.load_kmers([f], b, 31) for f in files]
        _same(_export(gpu_ctx.kmers_samples_count(tabs, b)), (wk, wn), "tables b=%d" % b)


def test_kmers_samples_counter_over_slices(gpu_ctx, tmp_path):
    """the per-slice pieces of the read-out: every number of slices gives the restatement's bytes, from files and from tables"""
    samples = _counter_cohort()
    files = _write_samples(tmp_path, samples, "s")
    b = 1
    wk, wn = R.kmers_samples_count(samples, b)
    want = [R.records_to_bytes(wk, wn), R.stat_txt(wn).encode()]
    tabs = [gpu_ctx.load_kmers([f], b, 31) for f in files]
    blobs = None
    try:
        for S in (1, 3, 16):
            gpu_ctx.set_option("stats_slices", S)
            out, st = tmp_path / ("n_S%d.kmers.bin" % S), tmp_path / ("n_S%d.stat.txt" % S)
            assert gpu_ctx.kmers_samples_count_files(files, 31, str(out), str(st), max_bad=b) == len(wk)
            got = [out.read_bytes(), st.read_bytes()]
            assert got == want, S
            tk, tv = _export(gpu_ctx.kmers_samples_count(tabs, b))
            assert [R.records_to_bytes(tk, tv), R.stat_txt(tv).encode()] == want, S
            blobs = blobs or got
            assert got == blobs
    finally:
        gpu_ctx.set_option("stats_slices", 0)


def test_key_limit_through_the_presence_mode(gpu_ctx):
    """a key >= 2^62 in any sample is an error of the union pass, and the error leaves nothing behind on the context"""
    rng = np.random.default_rng(9)
    pool = rng.integers(0, 1 << 62, size=400, dtype=np.uint64)
    tabs = []
    for j in range(6):
        m = rng.random(len(pool)) < 0.6
        tabs.append(_tab(gpu_ctx, pool[m], rng.integers(1, 30, size=int(m.sum()))))
    recs = [_records(t) for t in tabs]
    one = _tab(gpu_ctx, [5, 6], [3, 3])
    big = _tab(gpu_ctx, [5, 1 << 62], [3, 3])

    def still_right():
        _check_stats(gpu_ctx, tabs[:3], tabs[3:], 0, 0.3, 0.05)
        _same(_export(gpu_ctx.kmers_samples_count(tabs, 0)), R.kmers_samples_count(recs, 0), "n_samples")

    for bad in (lambda: gpu_ctx.stats_kmers([big], [one]), lambda: gpu_ctx.stats_kmers([one], [big]),
                lambda: gpu_ctx.kmers_samples_count([one, big], 0)):
        with pytest.raises(Exception, match=r"2\^62"):
            bad()
        still_right()


def test_cli_end_to_end(gpu_ctx, ref_files, tmp_path):
    exe = os.path.join(ROOT, "metafast.sh")
    wd = tmp_path / "w"
    r = subprocess.run([exe, "-t", "kmer-counter-posneg", "-k", "31", "-pos", ref_files[0], "-neg", ref_files[1], ref_files[2], "-w", str(wd)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    A = sorted(str(p) for p in (wd / "pos" / "kmers").iterdir())
    B = sorted(str(p) for p in (wd / "neg" / "kmers").iterdir())
    for extra in ([], ["-c"]):
        r = subprocess.run([exe, "-t", "stats-kmers", "-A", *A, "-B", *B, "-w", str(wd), "--force" if not extra else "-c"], capture_output=True, text=True,
                           timeout=300, input="y\n")
        assert r.returncode == 0, r.stderr
        if extra:
            assert "SUCCESS file found" in r.stderr
    samples = [R.records_from_bytes(open(f, "rb").read()) for f in A + B]
    want = R.stats_kmers(samples[:len(A)], samples[len(A):])
    kd = wd / "kmers"
    assert (kd / "filtered_chisquared.kmers.bin").read_bytes() == R.records_to_bytes(*want["chi"])
    assert (kd / "filtered_groupA.kmers.bin").read_bytes() == R.records_to_bytes(*want["A"])
    assert (kd / "filtered_groupB.kmers.bin").read_bytes() == R.records_to_bytes(*want["B"])
    assert (wd / "SUCCESS").exists()
    assert (wd / "out.properties").read_text().splitlines()[0] == "resulting-kmers-file = %s" % (kd / "filtered_groupA.kmers.bin")
    r = subprocess.run([exe, "-t", "kmers-samples-counter", "-k", "31", "-i", *A, *B, "-w", str(tmp_path / "w2")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    wk, wn = R.kmers_samples_count(samples, 1)
    assert (tmp_path / "w2" / "kmers" / "n_samples.kmers.bin").read_bytes() == R.records_to_bytes(wk, wn)
    assert (tmp_path / "w2" / "stats" / "n_samples.stat.txt").read_text() == R.stat_txt(wn)


def test_size_cohort_counters_add_up(gpu_ctx):
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < (20 << 30):
        pytest.skip("needs 20 GB of free HBM")
    n_reads = 1_000_000
    ta = [_synth_sample(gpu_ctx, j, 0, n_reads, 31) for j in range(16)]
    tb = [_synth_sample(gpu_ctx, 16 + j, 1, n_reads, 31) for j in range(16)]
    chi, ga, gb, c = gpu_ctx.stats_kmers(ta, tb)
    assert c["n"] == c["scarce"] + c["in_all"] + c["chi2_rejected"] + c["mw_rejected"] + c["group_a"] + c["group_b"]
    assert len(chi) == c["mw_rejected"] + c["group_a"] + c["group_b"] and len(ga) == c["group_a"] and len(gb) == c["group_b"]
    # the restatement on a fixed sample of the union's keys (1 / 64 of the key space by hash), with the whole samples' F_j
    recs = [_records(t) for t in ta + tb]
    F = [int(r[1].astype(np.int64).sum()) for r in recs]
    sub = [(k[sel], cnt[sel]) for k, cnt in recs for sel in [((k * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(58)) == 0]]
    want = R.stats_kmers(sub[:16], sub[16:], F_override=F)
    def pick(kv):
        k, v = kv
        sel = ((k * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(58)) == 0
        return k[sel], v[sel]
    _same(pick(_export(chi)), want["chi"], "chi")
    _same(pick(_export(ga)), want["A"], "A")
    _same(pick(_export(gb)), want["B"], "B")
