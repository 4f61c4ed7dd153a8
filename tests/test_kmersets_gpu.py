"""unique-kmers-multi (src/tools/UniqueKmersMultipleSamplesFinder.java:84-185) and kmers-multiple-filters
(src/tools/KmersMultipleFilters.java:77-133) on the GPU join (mf_kmersets.hip), through the C-ABI, against the independent restatement
tests/kmersets_ref.py: record sets byte-identical, counters equal."""
import os
import subprocess

import numpy as np
import pytest

import kmersets_ref as K
import stats_ref as R
from conftest import ROOT
from test_stats_gpu import _synth_sample, _write_samples

pytestmark = pytest.mark.gpu

EMPTY = (np.zeros(0, np.uint64), np.zeros(0, np.int16))


def _tab(ctx, sample, k=31):
    return ctx.table_from_host(np.asarray(sample[0], np.uint64), np.asarray(sample[1]).astype(np.uint16), k)


def _bytes(t):
    k, c = t.export(-1)
    return R.records_to_bytes(k, c)


def _pool(n, seed):
    """n distinct keys below 2^62, key 0 (the poly-A k-mer) among them"""
    keys = np.unique(np.random.default_rng(seed).integers(1, 1 << 62, size=n + 64, dtype=np.uint64))[:n]
    keys[0] = 0
    return keys


def _sample(rng, pool, frac, lo, hi):
    m = rng.random(len(pool)) < frac
    return pool[m], rng.integers(lo, hi, size=int(m.sum())).astype(np.int16)


def _check_unique(ctx, ins, filts, b, mn, mx, tabs=None):
    want = K.unique_kmers_multi(ins, filts, b, mn, mx)
    ti, tf = tabs or ([_tab(ctx, s) for s in ins], [_tab(ctx, s) for s in filts])
    outs, n_union, counts = ctx.unique_kmers_multi(ti, tf, b, mn, mx)
    assert n_union == want["n_union"] and counts == want["counts"], (n_union, counts, want["n_union"], want["counts"])
    assert len(outs) == len(want["files"])
    for t, (i, wk, wv) in zip(outs, want["files"]):
        assert _bytes(t) == R.records_to_bytes(wk, wv), i
    return want, [_bytes(t) for t in outs]


def _check_filters(ctx, sample, cd, uc, nonibd, b, tabs=None):
    """cd, uc, nonibd: one sample each (the table form takes one table per set)"""
    want = K.kmers_multiple_filters(sample, [cd], [uc], [nonibd], b)
    t, tc, tu, tn = tabs or [_tab(ctx, s) for s in (sample, cd, uc, nonibd)]
    kept, triples, counts, found, nkept = ctx.kmers_multiple_filters(t, tc, tu, tn, b)
    assert (found, nkept) == (want["found"], len(want["kept"][0]))
    assert _bytes(kept) == R.records_to_bytes(*want["kept"])
    assert np.array_equal(triples, want["triples"]) and np.array_equal(counts.astype(np.int64), want["counts"])
    return want, (_bytes(kept), triples.tobytes(), counts.tobytes())


@pytest.mark.parametrize("n_in,n_f", [(5, 3), (40, 7)])
def test_unique_random_presence(gpu_ctx, n_in, n_f):
    rng = np.random.default_rng(n_in)
    pool = _pool(3000, 11)
    ins = [_sample(rng, pool, rng.uniform(0.05, 0.6), 0, 6) for _ in range(n_in)]          # counts that straddle b = 0, 1, 3
    filts = [_sample(rng, pool, 0.03, 0, 6) for _ in range(n_f)]
    ti, tf = [_tab(gpu_ctx, s) for s in ins], [_tab(gpu_ctx, s) for s in filts]
    for b in (0, 1, 3):
        want, _ = _check_unique(gpu_ctx, ins, filts, b, 1, n_in + 2, (ti, tf))              # a range that runs past the first empty i
        assert want["counts"][-1] == 0 and len(want["counts"]) >= 3 and len(want["counts"]) < n_in + 2
        assert want["n_union"] > want["counts"][0] > 0                                      # some knocked out, some left
        _check_unique(gpu_ctx, ins, filts, b, 2, 2, (ti, tf))                               # min-samples = max-samples
    assert 0 in K.unique_kmers_multi(ins, [], 0)["files"][0][1]                             # key 0 is a key like any other
    _check_unique(gpu_ctx, ins, [], 0, 1, 1, (ti, []))


def test_unique_wraps_and_empty_samples(gpu_ctx):
    rng = np.random.default_rng(3)
    pool = _pool(3000, 12)
    full = (pool, np.full(len(pool), 32767, np.int16))
    half = (pool, np.full(len(pool), 16384, np.int16))
    for n in (3, 4, 5, 9):                                                                   # n x 32767 -> -n + 65536 * ...: 4 -> -4, 5 -> 32763
        _check_unique(gpu_ctx, [full] * n, [EMPTY], 1, 1, n)
    _check_unique(gpu_ctx, [half] * 2, [], 0, 1, 2)                                          # a sum of exactly 32768
    _check_unique(gpu_ctx, [half] * 4, [], 0, 1, 4)                                          # exactly 65536 -> 0
    want, _ = _check_unique(gpu_ctx, [half] * 4 + [_sample(rng, pool, 0.5, 1, 9)], [_sample(rng, pool, 0.2, 1, 9)], 0, 5, 5)
    assert want["counts"][0] > 0
    twenty = (pool[:100], np.full(100, 20000, np.int16))
    want, _ = _check_unique(gpu_ctx, [twenty] * 3 + [_sample(rng, pool, 0.3, 1, 50)], [], 1, 1, 4)      # 3 x 20000 -> -5536 (+ a few)
    assert want["counts"][0] > 0
    # empty samples among the inputs and the filters, nothing but empty samples, no inputs at all
    s = _sample(rng, pool, 0.4, 1, 9)
    _check_unique(gpu_ctx, [EMPTY, s, EMPTY], [EMPTY, _sample(rng, pool, 0.1, 1, 9)], 1, 1, 3)
    _check_unique(gpu_ctx, [EMPTY, EMPTY], [s], 1, 1, 2)
    _check_unique(gpu_ctx, [], [s], 1, 1, 2)


def test_filters_overlaps_and_values(gpu_ctx):
    rng = np.random.default_rng(4)
    pool = _pool(3000, 13)
    sample = _sample(rng, pool, 0.8, 0, 6)
    r = rng.integers(0, 8, size=len(pool))                          # which of the three sets hold a key: every combination, none included
    def sub(bit):
        m = (r >> bit) & 1 == 1
        v = rng.integers(0, 40, size=int(m.sum())).astype(np.int16)
        v[:5] = 32767
        return pool[m], v
    cd, uc, ni = sub(0), sub(1), sub(2)
    for b in (0, 1, 3):
        want, _ = _check_filters(gpu_ctx, sample, cd, uc, ni, b)
        assert 0 < len(want["kept"][0]) < want["found"] and want["triples"].max() == 32767
        assert (want["triples"] > 0).all(axis=1).any() and ((want["triples"] > 0).sum(axis=1) == 2).any()
    # disjoint sets
    third = len(pool) // 3
    parts = [(pool[i * third:(i + 1) * third], rng.integers(1, 9, size=third).astype(np.int16)) for i in range(3)]
    want, _ = _check_filters(gpu_ctx, sample, *parts, 1)
    assert ((want["triples"] > 0).sum(axis=1) <= 1).all()
    # none of the input's keys is in a filter: empty output, one (0, 0, 0) line; empty filters; an empty input
    other = (_pool(500, 99)[1:] | np.uint64(1 << 61), np.ones(499, np.int16))
    nz = (sample[0][1:], sample[1][1:]) if sample[0][0] == 0 else sample
    want, _ = _check_filters(gpu_ctx, nz, other, other, EMPTY, 1)
    assert len(want["kept"][0]) == 0 and want["triples"].tolist() == [[0, 0, 0]]
    _check_filters(gpu_ctx, sample, EMPTY, EMPTY, EMPTY, 1)
    _check_filters(gpu_ctx, EMPTY, cd, uc, ni, 1)


def test_filters_many_distinct_triples(gpu_ctx):
    n = 12000
    pool = _pool(n, 14)
    i = np.arange(n)
    cd = (pool, (i // 100 + 1).astype(np.int16))
    uc = (pool, (i % 100 + 1).astype(np.int16))
    ni = (pool[::2], (i[::2] % 7 + 1).astype(np.int16))
    want, _ = _check_filters(gpu_ctx, (pool, np.full(n, 2, np.int16)), cd, uc, ni, 1)
    assert len(want["triples"]) == n > 10_000


def test_slices_give_identical_bytes(gpu_ctx, tmp_path):
    rng = np.random.default_rng(5)
    pool = _pool(3000, 15)
    ins = [_sample(rng, pool, 0.4, 0, 6) for _ in range(6)]
    filts = [_sample(rng, pool, 0.05, 0, 6) for _ in range(3)]
    cd, uc, ni = (_sample(rng, pool, 0.3, 0, 30) for _ in range(3))
    ti, tf = [_tab(gpu_ctx, s) for s in ins], [_tab(gpu_ctx, s) for s in filts]
    tabs = [_tab(gpu_ctx, s) for s in (ins[0], cd, uc, ni)]
    # the file forms too: two input files per tool, duplicate records inside a file
    dup = lambda s: (np.concatenate([s[0], s[0][:200]]), np.concatenate([s[1], s[1][:200]]))
    fins = [dup(s) for s in ins]
    fi = _write_samples(tmp_path, fins, "in")
    ff = _write_samples(tmp_path, filts, "f")
    fc = [_write_samples(tmp_path, [s, dup(s)], p) for s, p in ((cd, "cd"), (uc, "uc"), (ni, "ni"))]
    want_u = K.unique_kmers_multi(fins, filts, 1, 1, 8)
    want_f = [K.kmers_multiple_filters(s, *[[x, dup(x)] for x in (cd, uc, ni)], 1) for s in fins[:2]]
    seen = None
    try:
        for S in (1, 3, 7):
            gpu_ctx.set_option("stats_slices", S)
            _, bu = _check_unique(gpu_ctx, ins, filts, 1, 1, 8, (ti, tf))
            _, bf = _check_filters(gpu_ctx, ins[0], cd, uc, ni, 1, tabs)
            out = tmp_path / ("o%d" % S)
            os.makedirs(out)
            n_union, counts = gpu_ctx.unique_kmers_multi_files(fi, ff, 31, str(out), 1, 1, 8)
            assert (n_union, counts) == (want_u["n_union"], want_u["counts"])
            assert sorted(os.listdir(out)) == ["filtered_%d.kmers.bin" % i for i, _, _ in want_u["files"]]
            for i, wk, wv in want_u["files"]:
                assert (out / ("filtered_%d.kmers.bin" % i)).read_bytes() == R.records_to_bytes(wk, wv)
            ok = [str(out / ("k%d.bin" % j)) for j in range(2)]
            os_ = [str(out / ("s%d.txt" % j)) for j in range(2)]
            fk = gpu_ctx.kmers_multiple_filters_files(fi[:2], *fc, 31, ok, os_, 1)
            for j, w in enumerate(want_f):
                assert fk[j] == (w["found"], len(w["kept"][0]))
                assert open(ok[j], "rb").read() == R.records_to_bytes(*w["kept"]) and open(os_[j]).read() == w["stat_txt"]
            seen = seen or (bu, bf)
            assert (bu, bf) == seen
    finally:
        gpu_ctx.set_option("stats_slices", 0)


@pytest.mark.parametrize("k", [21, 31])
def test_synthetic_cohort(gpu_ctx, k):
    ta = [_synth_sample(gpu_ctx, j, 0, 120_000, k) for j in range(6)]
    tb = [_synth_sample(gpu_ctx, 6 + j, 1, 120_000, k) for j in range(6)]
    recs = lambda ts: [(lambda kc: (kc[0], kc[1].astype(np.int16)))(t.export(-1)) for t in ts]
    ra, rb = recs(ta), recs(tb)
    # the case is not trivial: some keys are knocked out, some survive, c_i strictly decreasing over at least three i
    want = K.unique_kmers_multi(ra, rb, 1, 1, 6)
    with_no_filter = K.unique_kmers_multi(ra, [], 1, 1, 1)
    c = want["counts"]
    print("unique-kmers-multi k=%d: n_union %d, c_i %s, without filters %s" % (k, want["n_union"], c, with_no_filter["counts"]))
    assert 0 < c[0] < with_no_filter["counts"][0]
    assert sum(1 for x, y in zip(c, c[1:]) if x > y > 0) >= 2, c
    _check_unique(gpu_ctx, ra, rb, 1, 1, 6, (ta, tb))
    # pipeline 3 on the same cohort: the three sets are kmers-samples-counter outputs
    sets = [gpu_ctx.kmers_samples_count(g, 1) for g in (ta, tb, ta[:3] + tb[:3])]
    rs = recs(sets)
    for t, r in ((ta[0], ra[0]), (tb[5], rb[5])):
        w, _ = _check_filters(gpu_ctx, r, *rs, 1, [t] + sets)
        assert len(w["triples"]) > 10 and w["triples"].max() == 6


def test_cli_round_trips(gpu_ctx, ref_files, tmp_path):
    exe = os.path.join(ROOT, "metafast.sh")
    run = lambda *args: subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    r = run("-t", "kmer-counter-many", "-k", "31", "-i", *ref_files, "-w", str(tmp_path / "count"))
    assert r.returncode == 0, r.stderr
    files = sorted(str(p) for p in (tmp_path / "count" / "kmers").iterdir())
    assert len(files) == 3
    samples = [R.records_from_bytes(open(f, "rb").read()) for f in files]
    # pipeline 3: kmers-samples-counter for three groups, then kmers-multiple-filters
    groups = [files[:2], files[1:], [files[0], files[2]]]
    sets = []
    for g, name in zip(groups, ("cd", "uc", "nonibd")):
        r = run("-t", "kmers-samples-counter", "-k", "31", "-i", *g, "-w", str(tmp_path / name))
        assert r.returncode == 0, r.stderr
        sets.append(str(tmp_path / name / "kmers" / "n_samples.kmers.bin"))
    set_recs = [R.records_from_bytes(open(f, "rb").read()) for f in sets]
    wd = tmp_path / "p3"
    args = ["-t", "kmers-multiple-filters", "-k", "31", "-i", *files, "-cd", sets[0], "-uc", sets[1], "-nonibd", sets[2], "-w", str(wd)]
    r = run(*args)
    assert r.returncode == 0, r.stderr
    for f, s in zip(files, samples):
        w = K.kmers_multiple_filters(s, [set_recs[0]], [set_recs[1]], [set_recs[2]], 1)
        name = K.output_name(f)
        assert (wd / "kmers" / (name + ".kmers.bin")).read_bytes() == R.records_to_bytes(*w["kept"])
        assert (wd / "stats" / (name + ".stat.txt")).read_text() == w["stat_txt"]
        assert "%s k-mers found" % "{:,}".format(w["found"]).replace(",", "'") in r.stderr
    assert (wd / "SUCCESS").exists()
    r = run(*args, "-c")
    assert r.returncode == 0 and "SUCCESS file found" in r.stderr, r.stderr
    r = run("-t", "kmers-multiple-filters", "-k", "31", "-i", *files, "-cd", sets[0], "-nonibd", sets[2], "-w", str(tmp_path / "e1"))
    assert r.returncode == 1 and "Mandatory argument --uc-filter-kmers (-uc) not set" in r.stderr, r.stderr
    # pipeline 2: unique-kmers-multi
    wd = tmp_path / "p2"
    args = ["-t", "unique-kmers-multi", "-k", "31", "-i", *files[:2], "--filter-kmers", files[2], "--min-samples", "1", "--max-samples", "4",
            "-w", str(wd)]
    r = run(*args)
    assert r.returncode == 0, r.stderr
    w = K.unique_kmers_multi(samples[:2], samples[2:], 1, 1, 4)
    assert sorted(os.listdir(wd / "kmers")) == ["filtered_%d.kmers.bin" % i for i, _, _ in w["files"]]
    for i, wk, wv in w["files"]:
        assert (wd / "kmers" / ("filtered_%d.kmers.bin" % i)).read_bytes() == R.records_to_bytes(wk, wv)
    assert w["counts"][-1] == 0 and "No good k-mers found. Stop at maxSamples=%d" % w["files"][-1][0] in r.stderr
    assert "(%.1f%%) of them is good (present in one dataset and missing in other)" % (w["counts"][0] * 100.0 / w["n_union"]) in r.stderr
    assert (wd / "stats").is_dir() and not os.listdir(wd / "stats")
    assert (wd / "out.properties").read_text().splitlines()[0] == "resulting-kmers-file = %s" % (wd / "kmers" / "filtered_1.kmers.bin")
    r = run(*args, "-c")
    assert r.returncode == 0 and "SUCCESS file found" in r.stderr, r.stderr
    r = run("-t", "unique-kmers-multi", "-k", "31", "-i", *files[:2], "--filter-kmers", files[2], "--min-samples", "3", "--max-samples", "2",
            "-w", str(tmp_path / "e2"))
    assert r.returncode == 1 and "--min-samples parameter cannot be greater than --max-samples parameter." in r.stderr, r.stderr
    r = run("-t", "unique-kmers-multi", "-k", "31", "-i", *files[:2], "-w", str(tmp_path / "e3"))
    assert r.returncode == 1 and "Mandatory argument --filter-kmers not set" in r.stderr, r.stderr
    r = run("-ts")
    assert "unique-kmers-multi" in r.stdout and "kmers-multiple-filters" in r.stdout


def test_limits(gpu_ctx):
    one = _tab(gpu_ctx, (np.array([5, 6], np.uint64), np.array([3, 3], np.int16)))
    with pytest.raises(Exception, match="at most 32767"):
        gpu_ctx.unique_kmers_multi([one] * 32768, [], 1, 1, 1)
    outs, n_union, counts = gpu_ctx.unique_kmers_multi([one] * 300, [], 1, 300, 301)          # many inputs are fine
    assert (n_union, counts) == (2, [2, 0]) and outs[0].export(-1)[1].tolist() == [900, 900]
    with pytest.raises(Exception, match="cannot be greater than --max-samples"):
        gpu_ctx.unique_kmers_multi([one], [], 1, 2, 1)
    with pytest.raises(Exception, match="negative"):
        gpu_ctx.unique_kmers_multi([one], [], -1, 1, 1)
    with pytest.raises(Exception, match="negative"):
        gpu_ctx.kmers_multiple_filters(one, one, one, one, -1)
    big = _tab(gpu_ctx, (np.array([5, 1 << 62], np.uint64), np.array([3, 3], np.int16)))
    with pytest.raises(Exception, match=r"2\^62"):
        gpu_ctx.unique_kmers_multi([one, big], [], 1, 1, 1)
    with pytest.raises(Exception, match=r"2\^62"):
        gpu_ctx.unique_kmers_multi([one], [big], 1, 1, 1)
    with pytest.raises(Exception, match=r"2\^62"):
        gpu_ctx.kmers_multiple_filters(big, one, one, one, 1)
    with pytest.raises(Exception, match=r"2\^62"):
        gpu_ctx.kmers_multiple_filters(one, one, big, one, 1)
