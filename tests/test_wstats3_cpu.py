"""The wide (k = 32 ... 63) stats-kmers-3 and kmers-grouped-counter without a GPU: the crafted cohort of tests/wstats3_cases.py against every rule
it is made for on the reference (tests/wstats3_ref.py: tests/stats3_ref.py on ranked k-mers), the margin guard of the decisions for the shapes the
GPU tests use, the grouped counter's restatement on a hand-worked case, and the driver's kmers-grouped-counter with --wide-kmers on the host-only
stub build."""
import subprocess

import numpy as np
import pytest

import stats3_ref as S3
import stats_ref as SR
import wkmersets_ref as WR
import wstats3_cases as CASES
import wstats3_ref as R
from test_driver_tools_cpu import ENV, stub_driver

KS = (32, 33, 63)


def _where(r):
    return set(r["chi"][0]), [dict(zip(r[g][0], r[g][1].tolist())) for g in "ABC"]


@pytest.mark.parametrize("k", KS)
def test_crafted_cohort_meets_every_rule(k):
    A, B, C, nm = CASES.crafted(k)
    b = CASES.MAX_BAD
    S = A + B + C
    assert all(x == WR.canonical(x, k) and x < 1 << (2 * k) for t in S for x in t) and all(0 < c <= 32767 for t in S for c in t.values())
    assert [sum(t.values()) for t in S] == [4000, 64000, 64000] + [4000] * 6
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
    assert {1, b, b + 1, 32767} <= {c for t in S for c in t.values()}
    run = lambda a, b_, c, p_mw: R.stats_kmers3(a, b_, c, b=b, p_chi2=CASES.P_CHI2, p_mw=p_mw)
    r, r0 = run(A, B, C, CASES.P_MW), run(A, B, C, 0.0)
    chi, (ga, gb, gc) = _where(r)
    chi0, (ga0, gb0, gc0) = _where(r0)
    c = r["counters"]
    assert all(c[name] > 0 for name in R.COUNTERS), c
    for res in (r, r0):
        S3.check_identities(res["counters"], len(res["chi"][0]))
    held = lambda x: tuple(sum(t.get(x, 0) > b for t in g) for g in (A, B, C))

    spare = CASES.W2._fresh(np.random.default_rng(k), k, len(S), set(union))

    def without(name, p_mw=CASES.P_MW, keep_sums=True):
        """the counters of the cohort without that k-mer; keep_sums: a sample that held it holds a private (scarce) k-mer with its count instead, so
        that every F_j, and with them every other row's values and ties, stay as they are"""
        x = nm[name]
        out = []
        for j, t in enumerate(S):
            u = {y: v for y, v in t.items() if y != x}
            if keep_sums and x in t:
                u[spare[j]] = t[x]
            out.append(u)
        return run(out[:3], out[3:6], out[6:], p_mw)["counters"]
    # each counter by the k-mer that is there for it: without that k-mer the counter is one lower
    assert held(nm["scarce"]) == (1, 0, 0) and without("scarce", keep_sums=False)["scarce"] == c["scarce"] - 1
    assert held(nm["scarce_smallest"]) == (0, 0, 1) and without("scarce_smallest", keep_sums=False)["scarce"] == c["scarce"] - 1
    for name in ("in_all", "in_all_largest"):
        assert held(nm[name]) == (3, 3, 3) and without(name)["in_all"] == c["in_all"] - 1 and nm[name] not in chi
    for name, h, g in (("only_a", (3, 0, 0), ga), ("only_b", (0, 3, 0), gb), ("only_c", (0, 0, 3), gc)):
        w = without(name)
        assert held(nm[name]) == h and w["unique"] == c["unique"] - 1 and w["unique_left"] == c["unique_left"] - 1 and nm[name] in g
    assert held(nm["chi_rejected"]) == (1, 1, 1) and without("chi_rejected")["chi2_rejected"] == c["chi2_rejected"] - 1 and nm["chi_rejected"] not in chi
    x = nm["mw_rejected"]
    assert held(x) == (3, 3, 1) and x in chi and not (x in ga or x in gb or x in gc) and without("mw_rejected")["mw_rejected"] == c["mw_rejected"] - 1
    assert x in ga0 or x in gb0 or x in gc0
    # one row for each group, by name: M = 156000 / 9
    M = 156000 / 9
    v = lambda cnt, j: cnt * M / (64000 if j in (1, 2) else 4000)
    for name, g, key, cnts in (("group_a", ga, "group_a", (100, 200, 300)), ("group_b", gb, "group_b", (100, 200, 300)), ("group_c", gc, "group_c", (100, 200, 300))):
        x = nm[name]
        j0 = 3 * "abc".index(name[-1])
        assert without(name)[key] == c[key] - 1 and g[x] == int(((v(cnts[0], j0) + v(cnts[1], j0 + 1)) + v(cnts[2], j0 + 2)) / 3), name
    # tied means of B and C, above A's: the row goes to C with the mean they share
    x = nm["tie"]
    assert held(x) == (1, 3, 3) and x in chi and x not in ga and x not in gb and gc[x] == gc0[x] == int(v(8, 6)) == 34
    assert without("tie")["group_c"] == c["group_c"] - 1
    # a mean that truncates to 0: a record with value 0 in group A (at p_mw = 0: the test rejects the row)
    x = nm["mean_zero"]
    assert held(x) == (0, 2, 0) or held(x) == (2, 0, 0)
    assert x not in ga and ga0[x] == 0 and 0 < 2 * v(3, 1) / 3 < 1
    x = nm["big_counts"]
    assert A[1][x] == 32767 and ga0[x] == int((0.0 + v(32767, 1) + v(20000, 2)) / 3)
    # the gather's threshold is 0: no sample of A or B holds low_counts, their counts of 1 and max_bad still make their means positive -- the row is
    # unique by presence and not "unique left"; cut at max_bad it would be
    x = nm["low_counts"]
    assert held(x) == (0, 0, 3) and x in gc and {t[x] for t in A + B} == {1, b}
    cut = [{(spare[j] if y == x and v_ <= b else y): v_ for y, v_ in t.items()} for j, t in enumerate(S)]      # (the low counts moved to private k-mers: every F_j stays)
    rc = run(cut[:3], cut[3:6], cut[6:], CASES.P_MW)["counters"]
    same = lambda d: {n_: v_ for n_, v_ in d.items() if n_ != "unique_left"}          # (a count at max_bad is no presence: the private k-mers are in no union)
    assert rc["unique_left"] == c["unique_left"] + 1 and same(rc) == same(c)
    # the rows at the slice borders survive, in all three groups
    kept = [x for x in nm["borders"] if x in ga or x in gb or x in gc]
    assert kept == nm["borders"] and all(any(x in g for x in kept) for g in (ga, gb, gc))
    # an empty sample (F = 0: every value of that sample is NaN).  In A: (A, B) and (A, C) fail, (B, C) still keeps rows, and the NaN mean of A is
    # greater than nothing -- no row goes to A.  In B: (A, B) adds nothing for the NaN, (B, C) fails; no row goes to B.  In C: no mean is greater
    # than the NaN mean of C, so neither A nor B wins a row -- every kept row goes to C with value 0
    for e, lost in (("A", "group_a"), ("B", "group_b")):
        Ae, Be, Ce, _ = CASES.crafted(k, e)
        assert {"A": Ae, "B": Be}[e][-1] == {} and len(Ae) + len(Be) + len(Ce) == 10
        for p_mw in (CASES.P_MW, 0.0):
            re_ = run(Ae, Be, Ce, p_mw)
            S3.check_identities(re_["counters"], len(re_["chi"][0]))
            assert re_["counters"][lost] == 0 and re_["counters"]["group_c"] > 0, (e, p_mw, re_["counters"])
    Ae, Be, Ce, _ = CASES.crafted(k, "C")
    assert Ce[-1] == {} and len(Ce) == 4
    for p_mw in (CASES.P_MW, 0.0):
        re_ = run(Ae, Be, Ce, p_mw)
        S3.check_identities(re_["counters"], len(re_["chi"][0]))
        assert re_["counters"]["group_c"] > 0 and set(re_["C"][1].tolist()) == {0} and re_["counters"]["group_a"] + re_["counters"]["group_b"] == 0


def test_margin_guard_for_the_gpu_shapes():
    """the guard of tests/test_stats3_cpu.py over every (nA, nB, nC, p_chi2, p_mw) of tests/test_wstats3_gpu.py: no reachable statistic within
    1e-9 q of q and no reachable p within 1e-12 of p_mw, so the last bits of an erfc or of the quantile move no decision"""
    for na, nb, nc, pchi2, pmw in CASES.GPU_SHAPES:
        q = S3.chi2_2_quantile(pchi2)
        n1a, n1b, n1c = np.meshgrid(np.arange(na + 1), np.arange(nb + 1), np.arange(nc + 1), indexing="ij")
        kk = S3.chisq3_stat(na - n1a, n1a, nb - n1b, n1b, nc - n1c, n1c).ravel()
        kk = kk[np.isfinite(kk)]
        if np.isfinite(q):
            assert not np.any(np.abs(kk - q) <= 1e-9 * q), (na, nb, nc, pchi2)
        if pmw > 0:
            for nx, ny in ((na, nb), (nb, nc), (na, nc)):
                ps = np.array([SR.mw_pvalue_from_umin(u / 2.0, nx, ny) for u in range(nx * ny + 1)])
                assert not np.any(np.abs(ps - pmw) <= 1e-12), (nx, ny, pmw)


def test_random_cohorts_reach_both_row_kernels_and_every_list():
    for na, nb, nc in CASES.RANDOM_SHAPES[1:]:
        A, B, C = CASES.random_cohort(33, na, nb, nc)
        assert (len(A), len(B), len(C)) == (na, nb, nc) and 200 < len(set().union(*A, *B, *C)) <= 300
        r = R.stats_kmers3(A, B, C, b=CASES.MAX_BAD, p_chi2=0.05, p_mw=0.05)["counters"]
        assert min(r["chi2_rejected"], r["mw_rejected"], r["group_a"], r["group_b"], r["group_c"], r["unique_left"]) > 2, r
        r = R.stats_kmers3(A, B, C, b=CASES.MAX_BAD, p_chi2=0.0, p_mw=0.05)
        assert r["chi"][0] == [] and r["counters"]["chi2_rejected"] + r["counters"]["scarce"] + r["counters"]["in_all"] == r["counters"]["n"]


def test_grouped_counter_by_hand():
    X, Y, Z, W = (5 << 64) | 7, (5 << 64) | 8, (6 << 64) | 1, 9
    kf = [{X: 1, W: 4}, {Y: 2, X: 3}]                        # X listed twice; Z is not asked for
    cd = [{X: 2, Z: 9}, {X: 1, Y: 2}]
    uc = [{W: 2}]
    keys, n = R.kmers_grouped_count(kf, cd, uc, [], b=1)
    assert keys == [W, X, Y] and n.tolist() == [[0, 1, 0], [1, 0, 0], [1, 0, 0]] and n.dtype == np.int64
    keys, n = R.kmers_grouped_count(kf, cd, uc, [{}, {Y: 1}], b=0)
    assert n.tolist() == [[0, 1, 0], [2, 0, 0], [1, 0, 1]]
    assert R.kmers_grouped_count([], cd, uc, [])[0] == [] and R.kmers_grouped_count([{}], [], [], [])[1].shape == (0, 3)
    assert R.kmers_grouped_count([{X: 1}], [], [], [])[1].tolist() == [[0, 0, 0]]
    with pytest.raises(ValueError):
        R.kmers_grouped_count(kf, [{}] * 1023, [], [])
    # the text: the first base in the highest bits, also across the two words (k = 33: base 0 is bits 65 .. 64)
    assert R.kmer_text((3 << 64) | 0b0110, 33) == "T" + "A" * 30 + "GC"
    assert R.groups_txt([1], [[1022, 0, 3]], 32) == "Kmer\tcd_count\tuc_count\tnonibd_count\n" + "A" * 31 + "G\t1022\t0\t3\n"
    # the cohort of the GPU test asks for every kind of k-mer
    for k in KS:
        kf, cd, uc, ni = CASES.grouped_case(k)
        keys, n1 = R.kmers_grouped_count(kf, cd, uc, ni, b=1)
        _, n0 = R.kmers_grouped_count(kf, cd, uc, ni, b=0)
        assert keys[0] == 0 and keys[-1] == max(x for t in kf for x in t) and len(keys) == len(set().union(*kf))
        rows = n1.tolist()
        assert [0, 0, 0] in rows and any(r[0] and not r[1] and not r[2] for r in rows) and any(r[1] and not r[0] and not r[2] for r in rows)
        assert any(r[2] == 4 and not r[0] and not r[1] for r in rows) and not np.array_equal(n0, n1) and (n0 >= n1).all()
        for n_slices in (3, 7):
            assert {CASES.slice_of(x, k, n_slices) for x in keys} == set(range(n_slices))


# ---- the driver on the stub build ----
@pytest.fixture(scope="module")
def driver():
    return stub_driver()


def _run(driver, cwd, *args):
    return subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, env=ENV, timeout=120, cwd=str(cwd))


def test_driver_takes_wide_grouped_counter(driver, tmp_path):
    for name in ("kf.kmers.bin", "a.kmers.bin", "b.kmers.bin", "c.kmers.bin"):
        (tmp_path / name).write_bytes(b"")
    args = ["-kf", "kf.kmers.bin", "-cd", "a.kmers.bin", "-uc", "b.kmers.bin", "-nonibd", "c.kmers.bin"]
    # with the flag and -k in 32 ... 63 the tool asks for the wide entry point: the stub has none, and the run names it
    r = _run(driver, tmp_path, "--wide-kmers", "-t", "kmers-grouped-counter", "-k", 40, *args, "-w", "w1")
    out = r.stderr + r.stdout
    assert r.returncode == 1 and "this build of the library has no mf_kmers_grouped_count_wide" in out and "no more than 31" not in out, out
    props = (tmp_path / "w1" / "in.properties").read_text()
    assert "wide-kmers = true" in props and "\nk = 40\n" in "\n" + props and "maximal-bad-frequence = 1" in props
    assert not (tmp_path / "w1" / "SUCCESS").exists()
    r = _run(driver, tmp_path, "--wide-kmers", "-t", "kmers-grouped-counter", "-k", 64, *args, "-w", "w2")
    assert r.returncode == 1 and "The size of k-mer must be no more than 63." in r.stderr + r.stdout
    # without the flag: the reference's message; with the flag and k <= 31: the narrow entry point
    r = _run(driver, tmp_path, "-t", "kmers-grouped-counter", "-k", 32, *args, "-w", "w3")
    out = r.stderr + r.stdout
    assert r.returncode == 1 and "no more than 31" in out and "_wide" not in out, out
    r = _run(driver, tmp_path, "--wide-kmers", "-t", "kmers-grouped-counter", "-k", 31, *args, "-w", "w4")
    out = r.stderr + r.stdout
    assert r.returncode == 1 and "this build of the library has no mf_kmers_grouped_count" in out and "_wide" not in out, out
    assert "wide-kmers" not in (tmp_path / "w4" / "in.properties").read_text()
    # the sample counter keeps its refusal
    r = _run(driver, tmp_path, "--wide-kmers", "-t", "kmers-samples-counter", "-k", 40, "-i", "a.kmers.bin", "-w", "w5")
    assert r.returncode == 1 and "no more than 31" in r.stderr + r.stdout
