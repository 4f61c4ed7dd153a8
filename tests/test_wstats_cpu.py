"""The wide (k = 32 ... 63) stats-kmers without a GPU: the reference (tests/wstats_ref.py: tests/stats_ref.py on ranked k-mers) on hand-worked
literals, the crafted cohort of tests/wstats_cases.py against every rule it is made for, the margin guard of the decisions for the shapes the GPU
tests use, and the driver's stats-kmers with --wide-kmers on the host-only stub build."""
import subprocess

import numpy as np
import pytest

import stats_ref as SR
import wide_files_ref as WF
import wkmersets_ref as WR
import wstats_cases as CASES
import wstats_ref as R
from test_driver_tools_cpu import ENV, stub_driver

KS = (32, 33, 63)


def test_reference_by_hand():
    # three k-mers that differ in the high word, in the low word, and in both; their order is that of the 128-bit value
    X, Y, Z, W = (5 << 64) | 7, (5 << 64) | 8, (6 << 64) | 1, 9
    # 2 x 2: N = 4, scarce <= ceil(0.2) = 1 holder.  F = 100 for every sample, so M = 100 and v = c
    a0, a1 = {X: 10, Y: 90}, {X: 20, W: 80}
    b0, b1 = {Z: 60, Y: 40}, {Z: 70, W: 1, X: 29}
    # at max_bad = 1: X is held 2 : 1, Y 1 : 1, Z 0 : 2, W 1 : 0 (b1's count of 1 is no presence)
    r = R.stats_kmers([a0, a1], [b0, b1], b=1, p_chi2=0.3, p_mw=0.0)
    q = SR.chi2_quantile(0.3)
    kk = lambda n1a, n1b: float(SR.chisq_kk(2 - n1a, n1a, 2 - n1b, n1b))
    assert kk(2, 1) > q and kk(0, 2) > q and not kk(1, 1) > q
    assert r["counters"] == dict(n=4, scarce=1, in_all=0, unique=1, chi2_rejected=1, mw_rejected=0, group_a=1, group_b=1, unique_left=1)
    assert r["chi"][0] == [X, Z] and r["chi"][1].tolist() == [1, 1]
    # X: mean A = 15, mean B = 14.5 -> A with 15; Z: mean B = 65 -> B
    assert r["A"][0] == [X] and r["A"][1].tolist() == [15] and r["B"][0] == [Z] and r["B"][1].tolist() == [65]
    # the same k-mers under other values give the same lists: only equality and order matter
    keys, recs = R.ranked([a0, a1, b0, b1])
    assert keys == [W, X, Y, Z] and recs[0][0].tolist() == [1, 2] and recs[0][1].tolist() == [10, 90]


def test_sample_counter_by_hand():
    X, Y, Z = (5 << 64) | 7, (5 << 64) | 8, 3
    keys, n = R.kmers_samples_count([{X: 2, Y: 1}, {X: 5, Z: 2}, {}], b=1)
    assert keys == [Z, X] and n.tolist() == [1, 2]
    keys, n = R.kmers_samples_count([{X: 2, Y: 1}, {X: 5, Z: 2}, {}], b=0)
    assert keys == [Z, X, Y] and n.tolist() == [1, 2, 1]
    assert R.kmers_samples_count([], b=1)[0] == []
    with pytest.raises(ValueError):
        R.kmers_samples_count([{}] * 32768)
    assert R.records([X], np.array([0x8001], np.uint16)) == WF.encode_kmers([5], [7], [-32767])


def _where(r):
    return set(r["chi"][0]), dict(zip(r["A"][0], r["A"][1].tolist())), dict(zip(r["B"][0], r["B"][1].tolist()))


@pytest.mark.parametrize("k", KS)
def test_crafted_cohort_meets_every_rule(k):
    A, B, nm = CASES.crafted(k)
    b = CASES.MAX_BAD
    S = A + B
    assert all(x == WR.canonical(x, k) and x < 1 << (2 * k) for t in S for x in t) and all(0 < c <= 32767 for t in S for c in t.values())
    assert [sum(t.values()) for t in S] == [4000, 4000, 64000, 64000, 4000, 4000, 4000, 4000]
    # the keys: pairs that differ in one word only, the ends of the key range, both sides of every slice border of S = 3 and 7
    union = set().union(*S)
    lo_x, lo_y, hi_x, hi_y = nm["chi_rejected"], nm["mw_rejected"], nm["group_a"], nm["tie"]
    assert lo_x >> 64 == lo_y >> 64 and lo_x != lo_y and hi_x ^ hi_y == 1 << (64 if k > 32 else 63)      # (k = 32 has no high word: its top bit)
    assert nm["scarce_smallest"] == 0 == min(union) and nm["in_all_largest"] == max(union)
    for n_slices in (3, 7):
        for s in range(1, n_slices):
            below = [x for x in nm["borders"] if CASES.slice_of(x, k, n_slices) == s - 1]
            above = [x for x in nm["borders"] if CASES.slice_of(x, k, n_slices) == s]
            assert below and above and max(below) >> (2 * k - 24) == (min(above) >> (2 * k - 24)) - 1
        assert {CASES.slice_of(x, k, n_slices) for x in union} == set(range(n_slices))
    # the counts: 1, max_bad, max_bad + 1, 32767
    assert {1, b, b + 1, 32767} <= {c for t in S for c in t.values()}
    r = R.stats_kmers(A, B, b=b, p_chi2=CASES.P_CHI2, p_mw=CASES.P_MW)
    r0 = R.stats_kmers(A, B, b=b, p_chi2=CASES.P_CHI2, p_mw=0.0)
    chi, ga, gb = _where(r)
    chi0, ga0, gb0 = _where(r0)
    c = r["counters"]
    assert all(c[name] > 0 for name in R.COUNTERS), c
    held = lambda x: (sum(t.get(x, 0) > b for t in A), sum(t.get(x, 0) > b for t in B))
    # each counter by the k-mer that is there for it: without that k-mer the counter is one lower
    def without(name, p_mw=CASES.P_MW):
        x = nm[name]
        strip = lambda g: [{y: v for y, v in t.items() if y != x} for t in g]
        return R.stats_kmers(strip(A), strip(B), b=b, p_chi2=CASES.P_CHI2, p_mw=p_mw)["counters"]
    assert held(nm["scarce"]) == (1, 0) and without("scarce")["scarce"] == c["scarce"] - 1
    assert held(nm["scarce_smallest"]) == (0, 1) and without("scarce_smallest")["scarce"] == c["scarce"] - 1
    for name in ("in_all", "in_all_largest"):
        assert held(nm[name]) == (4, 4) and without(name)["in_all"] == c["in_all"] - 1 and nm[name] not in chi
    assert held(nm["unique_a"]) == (4, 0) and held(nm["unique_b"]) == (0, 4)
    for name, g in (("unique_a", ga), ("unique_b", gb)):
        w = without(name)
        assert w["unique"] == c["unique"] - 1 and w["unique_left"] == c["unique_left"] - 1 and nm[name] in g
    assert held(nm["chi_rejected"]) == (2, 2) and without("chi_rejected")["chi2_rejected"] == c["chi2_rejected"] - 1 and nm["chi_rejected"] not in chi
    x = nm["mw_rejected"]
    assert held(x) == (4, 1) and x in chi and x not in ga and x not in gb and without("mw_rejected")["mw_rejected"] == c["mw_rejected"] - 1
    x = nm["group_a"]
    assert held(x) == (4, 1) and without("group_a")["group_a"] == c["group_a"] - 1
    assert ga[x] == int((100 * 4.75 + 200 * 4.75 + 300 * 19000 / 64000 + 400 * 19000 / 64000) / 4) == 408
    # tied means go to B (at p_mw = 0: the test of 4 x 4 rejects every row whose means are equal), with the mean they share
    x = nm["tie"]
    assert held(x) == (2, 1) and x in chi and x not in ga and x not in gb and x not in ga0 and gb0[x] == 19
    assert without("tie", 0.0)["group_b"] == r0["counters"]["group_b"] - 1
    # a mean that truncates to 0: a record with value 0 in group A
    x = nm["mean_zero"]
    assert held(x) == (2, 0) and ga0[x] == 0 and 0 < 2 * 3 * 19000 / 64000 / 4 < 1
    x = nm["big_counts"]
    assert A[2][x] == 32767 and ga0[x] == int((32767 * 19000 / 64000 + 20000 * 19000 / 64000) / 4)
    # the gather's threshold is 0: no sample of A holds low_counts, A's counts of 1 and max_bad still make its mean of A positive -- the row is
    # unique by presence and not "unique left"; cut at max_bad it would be
    x = nm["low_counts"]
    assert held(x) == (0, 4) and gb[x] == 1425 and {t[x] for t in A} == {1, b}
    cut = lambda g: [{y: v for y, v in t.items() if y != x or v > b} for t in g]
    rc = R.stats_kmers(cut(A), cut(B), b=b, p_chi2=CASES.P_CHI2, p_mw=CASES.P_MW)["counters"]
    assert rc["unique_left"] == c["unique_left"] + 1 and {n_: v for n_, v in rc.items() if n_ != "unique_left"} == {n_: v for n_, v in c.items() if n_ != "unique_left"}
    # the rows at the slice borders survive, in both groups
    kept = [x for x in nm["borders"] if x in ga or x in gb]
    assert kept == nm["borders"] and any(x in ga for x in kept) and any(x in gb for x in kept)
    # an empty sample in A: F = 0, every value of that sample is NaN and Mann-Whitney rejects every row; without the test the NaN mean of A
    # is not greater than anything and every row goes to B.  An empty sample in B: the mean of B is NaN, no row goes to A
    Ae, Be, _ = CASES.crafted(k, "A")
    assert Ae[-1] == {} and len(Ae) == 5
    re_ = R.stats_kmers(Ae, Be, b=b, p_chi2=CASES.P_CHI2, p_mw=CASES.P_MW)["counters"]
    assert re_["mw_rejected"] == re_["n"] - re_["scarce"] - re_["in_all"] - re_["chi2_rejected"] > 0 and re_["group_a"] == re_["group_b"] == 0
    re0 = R.stats_kmers(Ae, Be, b=b, p_chi2=CASES.P_CHI2, p_mw=0.0)
    assert re0["counters"]["group_a"] == 0 and re0["counters"]["group_b"] > 0 and set(re0["B"][1].tolist()) > {0}
    Ae, Be, _ = CASES.crafted(k, "B")
    assert Be[-1] == {} and len(Be) == 5
    rb = R.stats_kmers(Ae, Be, b=b, p_chi2=CASES.P_CHI2, p_mw=CASES.P_MW)
    assert rb["counters"]["group_a"] == 0 and rb["counters"]["group_b"] > 0 and set(rb["B"][1].tolist()) == {0}


def test_margin_guard_for_the_gpu_shapes():
    """the guard of tests/test_stats_cpu.py over the shapes of tests/test_wstats_gpu.py: no reachable kk within 1e-9 q of q and no reachable p
    within 1e-12 of p_mw, so the last bits of an erfc or of the quantile solver move no decision"""
    for na, nb, pchi2, pmw in CASES.GPU_SHAPES:
        q = SR.chi2_quantile(pchi2)
        n1a, n1b = np.meshgrid(np.arange(na + 1), np.arange(nb + 1), indexing="ij")
        kk = SR.chisq_kk(na - n1a, n1a, nb - n1b, n1b).ravel()
        kk = kk[np.isfinite(kk)]
        if np.isfinite(q):
            assert not np.any(np.abs(kk - q) <= 1e-9 * q), (na, nb, pchi2)
        if pmw > 0:
            ps = np.array([SR.mw_pvalue_from_umin(u / 2.0, na, nb) for u in range(na * nb + 1)])
            assert not np.any(np.abs(ps - pmw) <= 1e-12), (na, nb, pmw)


def test_random_cohorts_reach_both_row_kernels_and_every_list():
    for na, nb in CASES.RANDOM_SHAPES[1:]:
        A, B = CASES.random_cohort(33, na, nb)
        assert len(A) == na and len(B) == nb and 200 < len(set().union(*A, *B)) <= 300
        r = R.stats_kmers(A, B, b=CASES.MAX_BAD, p_chi2=0.05, p_mw=0.05)["counters"]
        assert min(r["chi2_rejected"], r["mw_rejected"], r["group_a"], r["group_b"], r["unique_left"]) > 5, r
        r = R.stats_kmers(A, B, b=CASES.MAX_BAD, p_chi2=0.0, p_mw=0.05)
        assert r["chi"][0] == [] and r["counters"]["chi2_rejected"] == r["counters"]["n"]


# ---- the driver on the stub build ----
@pytest.fixture(scope="module")
def driver():
    return stub_driver()


def _run(driver, cwd, *args):
    return subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, env=ENV, timeout=120, cwd=str(cwd))


def test_driver_takes_wide_stats_kmers(driver, tmp_path):
    for name in ("a.kmers.bin", "b.kmers.bin", "c.kmers.bin"):
        (tmp_path / name).write_bytes(b"")
    args = ["-A", "a.kmers.bin", "-B", "b.kmers.bin"]
    # with the flag and -k in 32 ... 63 the tool asks for the wide entry point: the stub has none, and the run names it
    r = _run(driver, tmp_path, "--wide-kmers", "-t", "stats-kmers", "-k", 41, *args, "-w", "w1")
    out = r.stderr + r.stdout
    assert r.returncode == 1 and "this build of the library has no mf_stats_kmers_wide" in out, out
    props = (tmp_path / "w1" / "in.properties").read_text()
    assert "wide-kmers = true" in props and "\nk = 41\n" in "\n" + props and not (tmp_path / "w1" / "SUCCESS").exists()
    r = _run(driver, tmp_path, "--wide-kmers", "-t", "stats-kmers", "-k", 64, *args, "-w", "w2")
    assert r.returncode == 1 and "The size of k-mer must be no more than 63." in r.stderr + r.stdout
    # without the flag, without -k, and with k <= 31: the narrow tool as ever, which ignores a -k it does not declare
    for i, more in enumerate((["-k", 41], ["--wide-kmers"], ["--wide-kmers", "-k", 31])):
        w = "n%d" % i
        r = _run(driver, tmp_path, *more, "-t", "stats-kmers", *args, "-w", w)
        out = r.stderr + r.stdout
        assert r.returncode == 1 and "this build of the library has no mf_stats_kmers" in out and "mf_stats_kmers_wide" not in out, out
        props = (tmp_path / w / "in.properties").read_text()
        assert "wide-kmers" not in props and "\nk = " not in "\n" + props
    # three groups stay narrow
    r = _run(driver, tmp_path, "--wide-kmers", "-t", "stats-kmers-3", "-k", 41, *args, "-C", "c.kmers.bin", "-w", "w3")
    out = r.stderr + r.stdout
    assert r.returncode == 1 and "this build of the library has no mf_stats_kmers3" in out and "_wide" not in out, out
    assert "wide-kmers" not in (tmp_path / "w3" / "in.properties").read_text()
