"""stats-kmers-3 / kmers-grouped-counter without a GPU: the restatement (tests/stats3_ref.py) on hand-worked cases, the margin guard of
the decisions for the shapes the GPU tests use, and the driver's option handling in the sanitizer build (tests/host/mf_stub.cpp has no GPU)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import stats3_ref as R3
import stats_ref as R
from conftest import ROOT

F32 = np.float32
# (nA, nB, nC, pchi2, pmw) of tests/test_stats3_gpu.py and tools/stats3_rate.py
GPU_SHAPES = [(4, 4, 4, 0.05, 0.05), (4, 4, 4, 0.05, 0.0), (4, 4, 4, 0.2, 0.1),
              (3, 3, 3, 0.3, 0.05), (2, 2, 2, 0.3, 0.05), (1, 1, 1, 0.3, 0.05), (1, 3, 2, 0.3, 0.05), (3, 1, 1, 0.3, 0.05),
              (11, 11, 10, 0.05, 0.05), (11, 11, 11, 0.05, 0.05), (100, 100, 100, 0.05, 0.05),
              (3, 3, 2, 0.3, 0.2), (2, 2, 2, 0.05, 0.0), (2, 2, 2, 0.05, 0.3)]
CLI_RUNS = ((0.05, 0.0), (0.05, 0.3))                 # (pchi2, pmw) of the CLI round trip, groups {1, 2}, {2, 3}, {3, 1} of the reference's test files


def test_chisq3_hand_worked():
    # A = (n0 0, n1 4), B = (4, 0), C = (4, 0): percentages c = (0, 100), p = q = (100, 0); gr = 100 each, all = 300;
    # ones = 100, zeros = 200; x1 = x3 = x5 = 100/3, x2 = x4 = x6 = 200/3
    third = F32(100) / F32(300)
    x_one, x_zero = float(third * F32(100)), float(third * F32(200))
    t = lambda a, x: (abs(float(F32(a) - F32(x))) - 0.5) ** 2 / x
    want = t(0, x_one) + t(100, x_zero) + t(100, x_one) + t(0, x_zero) + t(0, x_one) + t(100, x_zero)
    got = float(R3.chisq3_stat(0, 4, 4, 0, 4, 0))
    assert got == pytest.approx(want, rel=1e-12)
    f = lambda a, x: (abs(a - x) - 0.5) ** 2 / x
    assert got == pytest.approx(2 * f(0, 100 / 3) + 2 * f(100, 200 / 3) + f(100, 100 / 3) + f(0, 200 / 3), rel=1e-6)
    # identical groups: every |observed - expected| is (about) 0, six terms of 0.25 / x with x = 100/300 * 150 in float
    x = float(third * F32(150))
    assert float(R3.chisq3_stat(3, 3, 3, 3, 3, 3)) == pytest.approx(6 * (abs(float(F32(50) - F32(x))) - 0.5) ** 2 / x, rel=1e-12)
    assert float(R3.chisq3_stat(3, 3, 3, 3, 3, 3)) == pytest.approx(6 * 0.25 / x, rel=1e-5)
    # an asymmetric case, in float32 step by step and by the formula
    n = (1, 2, 3, 1, 0, 5)
    c0, c1 = F32(100) * F32(1) / F32(3), F32(100) * F32(2) / F32(3)
    p0, p1 = F32(100) * F32(3) / F32(4), F32(100) * F32(1) / F32(4)
    q0, q1 = F32(100) * F32(0) / F32(5), F32(100) * F32(5) / F32(5)
    g1, g2, g3 = c0 + c1, p0 + p1, q0 + q1
    al = g1 + g2 + g3
    ones, zeros = p1 + c1 + q1, p0 + c0 + q0
    xs = [g1 / al * ones, g1 / al * zeros, g2 / al * ones, g2 / al * zeros, g3 / al * ones, g3 / al * zeros]
    obs = [p1, p0, c1, c0, q1, q0]
    want = 0.0
    for o, x in zip(obs, xs):
        assert o.dtype == np.float32 and x.dtype == np.float32
        want = want + (float(abs(o - x)) - 0.5) ** 2 / float(x)
    assert float(R3.chisq3_stat(*n)) == want
    O = [25.0, 75.0, 200 / 3, 100 / 3, 100.0, 0.0]
    E = [x * y / 300 for x in (100.0,) * 3 for y in (25 + 200 / 3 + 100, 75 + 100 / 3 + 0)]
    assert float(R3.chisq3_stat(*n)) == pytest.approx(sum((abs(o - e) - 0.5) ** 2 / e for o, e in zip(O, E)), rel=1e-5)
    # an empty group gives NaN, which no threshold lets through
    assert math.isnan(float(R3.chisq3_stat(0, 0, 1, 1, 1, 1)))


def test_chi2_two_degrees_quantile():
    assert R3.chi2_2_quantile(0.05) == pytest.approx(5.991464547107979, rel=1e-15)
    assert R3.chi2_2_quantile(0.01) == pytest.approx(9.210340371976182, rel=1e-15)
    assert R3.chi2_2_quantile(0.0) == math.inf and R3.chi2_2_quantile(1.0) == 0.0
    for p in (0.3, 0.2, 0.05):
        assert math.exp(-R3.chi2_2_quantile(p) / 2) == pytest.approx(p, rel=1e-14)


def _rows(*rows):
    return np.array(rows, dtype=np.float64)


def test_group_choice_and_ties():
    # (A, B, C) of one sample each: the mean is the value
    V = _rows([3, 1, 2], [1, 3, 2], [1, 2, 3], [3, 3, 1], [3, 1, 3], [1, 3, 3], [2, 2, 2], [np.nan, 5, 1], [5, np.nan, 1], [5, 1, np.nan])
    keep, grp, val, ul, ps = R3.decide_rows(V, 1, 1, 1, 0.0)
    assert keep.all() and ps is None
    #                      A  B  C  A==B>C -> C, A==C>B -> C, B==C>A -> C, all equal -> C, NaN anywhere -> C
    assert grp.tolist() == [0, 1, 2, 2, 2, 2, 2, 2, 2, 2]
    assert val.tolist() == [3, 3, 3, 1, 3, 3, 2, 1, 1, 0]          # (the NaN mean of C is written as 0)
    # unique left: some pairwise sum of the means is 0
    V = _rows([0, 0, 4], [0, 4, 0], [4, 0, 0], [0, 4, 4], [0, 0, 0], [np.nan, 0, 0])
    assert R3.decide_rows(V, 1, 1, 1, 0.0)[3].tolist() == [True, True, True, False, True, True]


def test_nan_rule_on_each_side_of_each_pair():
    nan = np.nan
    # groups of 4: a clean split 1 1 1 1 | 9 9 9 9 gives Umin = 0, p = 0.0209 < 0.05; equal groups give p = 1
    lo, hi = [1.0] * 4, [9.0] * 4
    p_split = R.mw_pvalue_from_umin(0.0, 4, 4)
    assert p_split < 0.05
    def ps(a, b, c):
        return R3.decide_rows(_rows(a + b + c), 4, 4, 4, 0.05)[4][0]
    assert ps(lo, hi, hi).tolist() == [p_split, 1.0, p_split]
    # a NaN in the first group of a pair: that pair's p is NaN (never < pmw)
    a_nan = [nan, 1.0, 1.0, 1.0]
    p = ps(a_nan, hi, hi)
    assert math.isnan(p[0]) and p[1] == 1.0 and math.isnan(p[2])
    assert not R3.decide_rows(_rows(a_nan + hi + hi), 4, 4, 4, 0.05)[0][0]          # (A, B) and (A, C) are out, (B, C) is no difference
    assert R3.decide_rows(_rows(a_nan + hi + lo), 4, 4, 4, 0.05)[0][0]              # (B, C) alone passes the row
    # a NaN in B: second group of (A, B) -> it adds 0 there; first group of (B, C) -> NaN
    b_nan = [nan, 9.0, 9.0, 9.0]
    p = ps(lo, b_nan, hi)
    assert p[0] == R.mw_pvalue_from_umin(0.0, 4, 4) and math.isnan(p[1]) and p[2] == p_split
    b_nan_lo = [nan, 1.0, 1.0, 1.0]                                                     # A > B nowhere, ties in 12 pairs: 2 U1 = 12
    assert ps(lo, b_nan_lo, hi)[0] == R.mw_pvalue_from_umin(6.0, 4, 4)
    # a NaN in C: second group of (B, C) and of (A, C)
    c_nan = [nan, 9.0, 9.0, 9.0]
    p = ps(lo, lo, c_nan)
    assert p.tolist() == [1.0, p_split, p_split]
    c_nan_hi = [nan, 1.0, 1.0, 1.0]
    p = ps(hi, hi, c_nan_hi)                                                            # 2 U1 = 2 * 12 = 24 of 32: Umin = 4
    assert p[1] == R.mw_pvalue_from_umin(4.0, 4, 4) and p[2] == p[1]
    # pmw <= 0 passes every row, NaN or not
    for pmw in (0.0, -1.0):
        assert R3.decide_rows(_rows(a_nan + hi + hi, lo + lo + lo), 4, 4, 4, pmw)[0].all()
    # a NaN mean (an empty sample) sends the row to C with C's value
    keep, grp, val, _, _ = R3.decide_rows(_rows(a_nan + hi + lo), 4, 4, 4, 0.05)
    assert keep[0] and grp[0] == 2 and val[0] == 1


def _s(keys, counts):
    return np.asarray(keys, np.uint64), np.asarray(counts, np.int16)


NONE = _s([], [])


@pytest.mark.parametrize("N,cut", [(3, 1), (12, 1), (21, 2)])
def test_scarce_cut(N, cut):
    """ceil(N * 0.05) = 1, 1, 2: a k-mer in that many samples is scarce, in one more it is not"""
    assert math.ceil(N * 0.05) == cut
    g = N // 3
    keys = [1, 2, 3]                                   # key 1 in `cut` samples, key 2 in cut + 1, key 3 in none but the last
    samples = []
    for j in range(N):
        ks = [x for x, n in ((1, cut), (2, cut + 1)) if j < n] + ([3] if j == N - 1 else [])
        samples.append(_s(ks, [5] * len(ks)))
    r = R3.stats_kmers3(samples[:g], samples[g:2 * g], samples[2 * g:], p_chi2=1.0, p_mw=0.0)
    c = r["counters"]
    assert c["n"] == len(keys) and c["scarce"] == 2 and r["chi"][0].tolist() == [2], c
    R3.check_identities(c, len(r["chi"][0]))


def test_counters_satisfy_the_reference_identities():
    rng = np.random.default_rng(31)
    pool = np.arange(1, 601, dtype=np.uint64) * np.uint64(7919)
    def sample(g):
        p = np.where(np.arange(len(pool)) % 3 == g, 0.85, 0.35)
        m = rng.random(len(pool)) < p
        return _s(pool[m], rng.integers(1, 30, size=int(m.sum())))
    groups = [[sample(g) for _ in range(n)] for g, n in enumerate((4, 5, 4))]
    for pchi2, pmw, b in ((0.05, 0.05, 0), (0.3, 0.0, 1), (0.0, 0.05, 0), (1.0, 0.5, 0)):
        r = R3.stats_kmers3(*groups, b=b, p_chi2=pchi2, p_mw=pmw)
        c = r["counters"]
        R3.check_identities(c, len(r["chi"][0]))
        assert len(r["A"][0]) == c["group_a"] and len(r["B"][0]) == c["group_b"] and len(r["C"][0]) == c["group_c"]
        if pchi2 == 0.0:
            assert len(r["chi"][0]) == 0                # q = inf rejects everything
        if pchi2 == 0.05:
            assert min(c["group_a"], c["group_b"], c["group_c"], c["mw_rejected"], c["chi2_rejected"]) > 0, c


def test_margin_guard_for_the_gpu_shapes():
    """no reachable statistic within 1e-9 q of q and no reachable p within 1e-12 of pmw: the decisions depend neither on the last bit
    of the quantile (closed form here, a solver in the reference) nor on that of an erfc"""
    for na, nb, nc, pchi2, pmw in GPU_SHAPES:
        q = R3.chi2_2_quantile(pchi2)
        n1a, n1b, n1c = np.meshgrid(np.arange(na + 1), np.arange(nb + 1), np.arange(nc + 1), indexing="ij")
        kk = R3.chisq3_stat(na - n1a, n1a, nb - n1b, n1b, nc - n1c, n1c).ravel()
        kk = kk[np.isfinite(kk)]
        assert not np.any(np.abs(kk - q) <= 1e-9 * q), (na, nb, nc, pchi2)
        if pmw > 0:
            for nx, ny in ((na, nb), (nb, nc), (na, nc)):
                ps = np.array([R.mw_pvalue_from_umin(u / 2.0, nx, ny) for u in range(nx * ny + 1)])
                assert not np.any(np.abs(ps - pmw) <= 1e-12), (nx, ny, pmw)


def test_kmers_grouped_counter_restatement():
    kf = [_s([7, 7, 3, 9, 11], [1, 2, 2, 5, 0]), _s([3, 20], [1, 1])]       # 7 and 3 listed twice; 11 has no record > 0; 20 is in no group
    cd = [_s([7, 3], [2, 1]), _s([7, 7], [1, 1])]                          # at b = 1: 7 once (two records of 1 are no presence)
    uc = [_s([9], [9])]
    keys, cnt = R3.kmers_grouped_count(kf, cd, uc, [], b=1)
    assert keys.tolist() == [3, 7, 9, 20]
    assert cnt.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0]]
    keys, cnt = R3.kmers_grouped_count(kf, cd, uc, [NONE], b=0)
    assert cnt.tolist() == [[1, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 0]]
    assert R3.kmer_text(0b00011011, 4) == "AGCT" and R3.kmer_text(0, 3) == "AAA"
    assert R3.groups_txt(keys[:2], cnt[:2], 2) == "Kmer\tcd_count\tuc_count\tnonibd_count\nAT\t1\t0\t0\nGT\t2\t0\t0\n"


# ---- the driver in the sanitizer build (same recipe as tests/test_stats_cpu.py) ----
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
ENV = dict(os.environ, ASAN_OPTIONS="exitcode=99:detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="exitcode=99:halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def san_cli(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("san") / "metafast_san")
    r = subprocess.run(["g++", *SAN, os.path.join(ROOT, "metafast_amd", "cli", "metafast_main.cpp"), os.path.join(ROOT, "tests", "host", "mf_stub.cpp"),
                        "-o", out, "-lpthread"], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("g++ has no sanitizer runtime here")
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _run(cli, args, cwd):
    r = subprocess.run([cli, *args], capture_output=True, text=True, errors="replace", env=ENV, timeout=120, input="y\n", cwd=cwd)
    assert r.returncode in (0, 1), (args, r.returncode, (r.stdout + r.stderr)[-2000:])
    return r


def test_driver_accepts_the_three_group_tools(san_cli, tmp_path):
    r = _run(san_cli, ["-ts"], str(tmp_path))
    assert r.returncode == 0 and "stats-kmers-3" in r.stdout and "kmers-grouped-counter" in r.stdout
    f = tmp_path / "a.kmers.bin"
    f.write_bytes(R.records_to_bytes(np.array([1, 2], np.uint64), np.array([3, 4])))
    w = lambda n: str(tmp_path / n)
    r = _run(san_cli, ["-t", "stats-kmers-3", "-A", str(f), str(f), "-B", str(f), "-C", str(f), "-pchi2", "0.01", "-pmw", "0.1", "-b", "2", "-w", w("w1")], str(tmp_path))
    assert r.returncode == 1 and "mf_stats_kmers3" in r.stderr, r.stderr
    props = (tmp_path / "w1" / "in.properties").read_text()
    assert "p-value-chi2 = 0.01" in props and "maximal-bad-frequence = 2" in props and "c-kmers" in props
    # a missing group, an empty one, a p-value outside [0, 1]
    for miss, opts in (("a-kmers", ["-B", str(f), "-C", str(f)]), ("b-kmers", ["-A", str(f), "-C", str(f)]), ("c-kmers", ["-A", str(f), "-B", str(f)])):
        r = _run(san_cli, ["-t", "stats-kmers-3", *opts, "-w", w("m_" + miss)], str(tmp_path))
        assert r.returncode == 1 and "Mandatory argument --%s" % miss in r.stderr, r.stderr
    r = _run(san_cli, ["-t", "stats-kmers-3", "-A", str(f), "-B", "-C", str(f), "-w", w("w2")], str(tmp_path))
    assert r.returncode == 1 and "every group needs at least one sample (|A| = 1, |B| = 0, |C| = 1)" in r.stderr, r.stderr
    r = _run(san_cli, ["-t", "stats-kmers-3", "-A", str(f), "-B", str(f), "-C", str(f), "-pchi2", "2", "-w", w("w3")], str(tmp_path))
    assert r.returncode == 1 and "Error calculating chi-squared value!" in r.stderr, r.stderr
    # kmers-grouped-counter: its own -cd / -uc / -nonibd, a list after -kf, the default b = 1
    r = _run(san_cli, ["-t", "kmers-grouped-counter", "-k", "5", "-kf", str(f), str(f), "-cd", str(f), "-uc", str(f), str(f), "-nonibd", str(f), "-w", w("w4")],
             str(tmp_path))
    assert r.returncode == 1 and "mf_kmers_grouped_count" in r.stderr, r.stderr
    props = (tmp_path / "w4" / "in.properties").read_text()
    assert "cd-kmers" in props and "uc-kmers" in props and "nonibd-kmers" in props and "maximal-bad-frequence = 1" in props and "filter-kmers" not in props
    assert "Mandatory argument --uc-kmers" in _run(san_cli, ["-t", "kmers-grouped-counter", "-k", "5", "-cd", str(f), "-nonibd", str(f), "-w", w("w5")], str(tmp_path)).stderr
    assert "no more than 31" in _run(san_cli, ["-t", "kmers-grouped-counter", "-k", "32", "-kf", str(f), "-cd", str(f), "-uc", str(f), "-nonibd", str(f), "-w", w("w6")],
                                     str(tmp_path)).stderr
    # the older tool keeps its meaning of -cd
    r = _run(san_cli, ["-t", "kmers-multiple-filters", "-k", "5", "-i", str(f), "-cd", str(f), "-uc", str(f), "-nonibd", str(f), "-w", w("w7")], str(tmp_path))
    assert "cd-filter-kmers" in (tmp_path / "w7" / "in.properties").read_text()


def test_cli_grouping_reaches_both_decisions(oracle, ref_files):
    """the grouping and p-values of the GPU suite's CLI round trip (tests/test_stats3_gpu.py), on the oracle's counts of the reference's
    three test files as kmer-counter-many writes them (k = 31, count > 1): the chi-squared list is not empty, and -pmw 0.3 rejects some
    rows and keeps others.  Two samples against two that share a file: the shared sample ties with itself, so 2 Umin >= 1 and the
    reachable p are 0.245 (2 Umin = 1), 0.439, 0.699, 1: 0.3 lies between the first two, 0.05 would reject every row."""
    assert [round(R.mw_pvalue_from_umin(u / 2.0, 2, 2), 3) for u in range(5)] == [0.121, 0.245, 0.439, 0.699, 1.0]
    recs = []
    for f in ref_files:
        k, c = oracle.Table().count_files([f], 31).export(1)
        recs.append((k, c.astype(np.int16)))
    A, B, C = [recs[0], recs[1]], [recs[1], recs[2]], [recs[2], recs[0]]
    for pchi2, pmw in CLI_RUNS:
        assert (2, 2, 2, pchi2, pmw) in GPU_SHAPES
        r = R3.stats_kmers3(A, B, C, p_chi2=pchi2, p_mw=pmw)
        c = r["counters"]
        R3.check_identities(c, len(r["chi"][0]))
        assert len(r["chi"][0]) > 0 and c["group_a"] + c["group_b"] + c["group_c"] > 0, c
        assert (c["mw_rejected"] > 0) == (pmw > 0), c
