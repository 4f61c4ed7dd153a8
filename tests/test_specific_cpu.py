"""specific-kmers / specific-kmers-3 / unique-kmers without a GPU: the restatement (tests/specific_ref.py) on hand-worked cases, the margin
guard of the decisions for the shapes the GPU tests use, and the driver's option handling in the sanitizer build of tests/test_stats3_cpu.py
(tests/host/mf_stub.cpp has no GPU and none of the new entry points: the tools stop where they would call the library)."""
import math

import numpy as np
import pytest

import specific_ref as S
import stats3_ref as R3
import stats_ref as R
from test_stats3_cpu import _run, san_cli  # noqa: F401  (the sanitizer build of the driver, as the other *_cpu.py suites use it)

# (nA, nB, pchi2, pmw) of tests/test_specific_gpu.py and tools/specific_rate.py
GPU_SHAPES2 = [(4, 4, 0.05, 0.05), (4, 4, 0.05, 0.0), (4, 4, 0.2, 0.1), (2, 2, 0.3, 0.05), (1, 1, 0.3, 0.05), (1, 3, 0.3, 0.05), (3, 1, 0.3, 0.05),
               (16, 16, 0.05, 0.05), (16, 17, 0.05, 0.05), (150, 150, 0.05, 0.05), (4, 4, 0.3, 0.2), (2, 1, 0.05, 0.0), (2, 1, 0.05, 0.3), (2, 1, 0.3, 0.05)]
# (nA, nB, nC, pchi2, pmw)
GPU_SHAPES3 = [(4, 4, 4, 0.05, 0.05), (4, 4, 4, 0.05, 0.0), (4, 4, 4, 0.2, 0.1), (2, 2, 2, 0.3, 0.05), (1, 1, 1, 0.3, 0.05), (3, 1, 1, 0.3, 0.05), (1, 3, 2, 0.3, 0.05),
               (11, 11, 10, 0.05, 0.05), (11, 11, 11, 0.05, 0.05), (100, 100, 100, 0.05, 0.05), (3, 3, 2, 0.3, 0.2), (2, 2, 2, 0.05, 0.0), (2, 2, 2, 0.05, 0.3)]


def _s(keys, counts):
    return np.asarray(keys, np.uint64), np.asarray(counts, np.int16)


NONE = _s([], [])


def _cohort(n, cells):
    """n samples; cells: {key: {sample: count}}"""
    out = [([], []) for _ in range(n)]
    for key, row in cells.items():
        for j, c in row.items():
            out[j][0].append(key)
            out[j][1].append(c)
    return [_s(k, c) for k, c in out]


@pytest.mark.parametrize("N,bound", [(20, 1), (21, 2)])
def test_first_holder_scarce_rule(N, bound):
    """the scarce cut compares the COUNT of the first sample that holds the k-mer with ceil(N * 0.05): a count against a bound made from
    a number of samples.  Key 1: its first holder has the bound itself and fifteen later holders have 500 -- scarce all the same.  Key 2:
    one more in the first holder -- kept.  Key 3: sample 0 alone, count 1 -- scarce, and counted as unique before the cut."""
    assert S.scarce_bound(N) == bound
    later = {j: 500 for j in range(5, 20)}
    samples = _cohort(N, {1: {3: bound, **later}, 2: {3: bound + 1, **later}, 3: {0: 1}})
    r = S.specific_kmers(samples[:10], samples[10:], p_chi2=1.0, p_mw=0.0)
    # key 2: n1A = 6, n1B = 10 of 10 (N = 21: of 11); mean(A) = (bound + 1 + 5 * 500) / 10 < mean(B) -> B, value (int)mean(B)
    mean_b = 10 * 500 / (N - 10)
    assert r["A"][0].tolist() == [] and r["B"][0].tolist() == [2] and r["B"][1].tolist() == [int(mean_b)]
    assert r["counters"] == dict(n=3, unique=1, scarce=2, chi2_rejected=0, mw_rejected=0, unique_left=0, group_a=0, group_b=1)


def test_in_all_kmer_is_kept_by_two_groups_and_dropped_by_three():
    """:160-162 against SpecificKmers3GroupsFinder :161-164.  The two-group statistic of a k-mer of all samples is +inf (an expected
    count of 0), which passes every finite quantile by itself; at pchi2 = 0 the quantile is +inf too and only the in-all rule keeps it."""
    assert math.isinf(float(R.chisq_kk(0, 2, 0, 2)))
    samples = _cohort(4, {5: {0: 9, 1: 9, 2: 1, 3: 1}, 6: {0: 7, 1: 7}})
    for pchi2 in (0.05, 0.0):
        r = S.specific_kmers(samples[:2], samples[2:], p_chi2=pchi2, p_mw=0.0)
        assert r["A"][0].tolist() == ([5, 6] if pchi2 else [5]) and r["A"][1][0] == 9
        assert r["counters"]["chi2_rejected"] == (0 if pchi2 else 1)
    three = _cohort(3, {5: {0: 9, 1: 9, 2: 1}, 6: {0: 7, 1: 7}})
    r = S.specific_kmers3(three[:1], three[1:2], three[2:], p_chi2=1.0, p_mw=0.0)
    assert r["counters"]["in_all"] == 1 and r["counters"]["n"] == 2
    assert sum(len(r[g][0]) for g in "ABC") == 1 and 5 not in np.concatenate([r[g][0] for g in "ABC"]).tolist()


def test_mean_tie_goes_to_b_and_the_cast_truncates():
    r = S.specific_kmers([_s([8], [3])], [_s([8], [3])], p_mw=0.0)
    assert r["A"][0].tolist() == [] and r["B"][0].tolist() == [8] and r["B"][1].tolist() == [3]
    # mean(A) = (200 + 99 * 1) / 100 = 2.99 -> (int) 2; N = 101: the bound is 6, the first holder's 200 is above it
    a = [_s([7], [200])] + [_s([7], [1])] * 99
    r = S.specific_kmers(a, [_s([7], [1])], p_mw=0.0)
    assert S.scarce_bound(101) == 6
    assert r["A"][0].tolist() == [7] and r["A"][1].tolist() == [2] and r["B"][0].tolist() == []


def test_a_value_above_32767_cannot_arise():
    """the raw counts are Java shorts that addAndBound keeps at 32767 (two records of 20000 in one file are 32767, not 40000 or -25536),
    and a mean of values <= 32767 is <= 32767: writeShort's low 16 bits are the value itself.  (stats-kmers differs: it normalises.)"""
    two = _s([4, 4], [20000, 20000])
    assert S.load_map(two, 0)[1].tolist() == [32767]
    r = S.specific_kmers([two, _s([4], [32767])], [_s([4], [32767])], p_mw=0.0)
    assert r["B"][1].tolist() == [32767]                  # (all means equal: B)
    r = S.specific_kmers([two, _s([4], [32767])], [_s([4], [32766])], p_mw=0.0)
    assert r["A"][1].tolist() == [32767]


def test_mann_whitney_is_skipped_at_pmw_zero_and_below():
    samples = _cohort(8, {9: {j: 5 for j in range(8)}})     # equal counts everywhere: U1 = U2, p = 1
    r = S.specific_kmers(samples[:4], samples[4:], p_mw=0.05)
    assert r["counters"]["mw_rejected"] == 1 and r["p"].tolist() == [1.0]
    for pmw in (0.0, -1.0):
        r = S.specific_kmers(samples[:4], samples[4:], p_mw=pmw)
        assert r["counters"]["mw_rejected"] == 0 and r["counters"]["group_b"] == 1 and r["p"] is None
        r3 = S.specific_kmers3(samples[:3], samples[3:6], [samples[6], NONE], p_chi2=1.0, p_mw=pmw)
        assert r3["counters"]["mw_rejected"] == 0 and r3["p"] is None


def test_the_inequalities_at_p_equal_to_pmw():
    """specific-kmers drops a row when p > pmw (:168), specific-kmers-3 keeps one when some p < pmw (:220).  A p exactly equal to pmw is
    reachable, since pmw is any double the user gives: 4 against 4 cleanly split has Umin = 0 and p = 0.0209...; that double as pmw."""
    p0 = R.mw_pvalue_from_umin(0.0, 4, 4)
    assert p0 == pytest.approx(0.020921335337794, rel=1e-12)
    samples = _cohort(8, {1: {**{j: 2 for j in range(4)}, **{j: 9 for j in range(4, 8)}}})
    assert S.scarce_bound(8) == 1
    r = S.specific_kmers(samples[:4], samples[4:], p_mw=p0)
    assert r["p"].tolist() == [p0] and r["counters"]["mw_rejected"] == 0 and r["B"][1].tolist() == [9]
    r = S.specific_kmers(samples[:4], samples[4:], p_mw=math.nextafter(p0, 0.0))
    assert r["counters"]["mw_rejected"] == 1
    # three groups of 4, every sample with F = 100 so that M = 100 and v = c: key 1 has A = 2 2 2 2, B = 9 9 9 9, C absent
    cells = {1: {**{j: 2 for j in range(4)}, **{j: 9 for j in range(4, 8)}}, 2: {**{j: 98 for j in range(4)}, **{j: 91 for j in range(4, 8)}},
             3: {j: 100 for j in range(8, 12)}}
    s3 = _cohort(12, cells)
    r = S.specific_kmers3(s3[:4], s3[4:8], s3[8:], p_chi2=1.0, p_mw=p0)
    assert r["M"] == 100 and r["counters"]["mw_rejected"] == 3 and r["p"][0].tolist() == [p0, p0, p0]
    r = S.specific_kmers3(s3[:4], s3[4:8], s3[8:], p_chi2=1.0, p_mw=math.nextafter(p0, 1.0))
    assert r["counters"]["mw_rejected"] == 0 and r["B"][0].tolist() == [1] and r["B"][1].tolist() == [9]
    assert r["counters"]["unique"] == 1 and r["counters"]["unique_left"] == 1 and r["C"][0].tolist() == [3]


def test_three_groups_use_the_quantile_of_one_degree_of_freedom():
    """:91.  8 + 8 + 8 samples, a k-mer in (2, 2, 3) of them: its statistic 4.27 lies between the quantile of 1 degree of freedom (3.84)
    and that of 2 (5.99): specific-kmers-3 keeps it, stats-kmers-3 drops it."""
    q1, q2 = R.chi2_quantile(0.05), R3.chi2_2_quantile(0.05)
    assert q1 == pytest.approx(3.841458820694124, rel=1e-12) and q2 == pytest.approx(5.991464547107979, rel=1e-12)
    kk = float(R3.chisq3_stat(6, 2, 6, 2, 5, 3))
    assert kk == pytest.approx(4.2716, abs=1e-4) and q1 < kk < q2
    s = _cohort(24, {1: {0: 4, 1: 4, 8: 4, 9: 4, 16: 4, 17: 4, 18: 4}})
    assert S.scarce_bound(24) == 2
    r = S.specific_kmers3(s[:8], s[8:16], s[16:], p_mw=0.0)
    assert r["q"] == q1 and r["counters"]["chi2_rejected"] == 0 and r["C"][0].tolist() == [1]
    r = R3.stats_kmers3(s[:8], s[8:16], s[16:], p_mw=0.0)
    assert r["q"] == q2 and r["counters"]["chi2_rejected"] == 1


def test_three_groups_normalise_with_a_truncated_mean_and_zero_for_absent():
    # F = 10, 4, 7 -> M = 21 // 3 = 7 (not 7.0 exactly by chance: 10, 4, 9 -> 23 // 3 = 7 as well)
    s = _cohort(3, {1: {0: 6, 1: 4}, 2: {0: 4, 2: 9}})
    r = S.specific_kmers3(s[:1], s[1:2], s[2:], p_chi2=1.0, p_mw=0.0)
    assert r["M"] == 7
    # key 1: v = 6 * 7 / 10 = 4.2, 4 * 7 / 4 = 7, absent 0 -> B with 7; key 2: 4 * 7 / 10 = 2.8, 0, 9 * 7 / 9 = 7 -> C with 7
    assert r["B"][0].tolist() == [1] and r["B"][1].tolist() == [7] and r["C"][0].tolist() == [2] and r["C"][1].tolist() == [7]
    # an empty sample is no NaN here: its value is 0 whatever its F (stats-kmers-3 divides 0 by 0)
    # F = 12, 4, 0, 0 -> M = 4; key 1: 6 * 4 / 12 = 2, 4 * 4 / 4 = 4, C = 0 0 -> B with 4 (a NaN mean of C would send it to C); key 2 is scarce
    s = _cohort(4, {1: {0: 6, 1: 4}, 2: {0: 6}})
    r = S.specific_kmers3(s[:1], s[1:2], s[2:], p_chi2=1.0, p_mw=0.0)
    assert r["M"] == 4 and r["B"][0].tolist() == [1] and r["B"][1].tolist() == [4] and r["counters"]["scarce"] == 1
    assert len(r["A"][0]) == 0 and len(r["C"][0]) == 0


def test_unique_kmers_pools_records_not_sums():
    """IOUtils.loadKmers(files, b): Kmers2HMWorker.processKmer tests every RECORD against b and adds the ones above it with addAndBound"""
    f1 = _s([10, 11, 12, 13], [1, 1, 5, 20000])
    f2 = _s([10, 11, 13, 14], [1, 2, 20000, 3])
    g1 = _s([12, 14], [9, 1])                              # at b = 1 the filter holds 12 alone
    r = S.unique_kmers([f1, f2], [g1], b=1)
    # 10: 1 + 1, no record above 1 -> not there.  11: the record 2 alone.  13: bounded.  12: zeroed, still in the map.
    assert r["hm"][0].tolist() == [11, 12, 13, 14] and r["hm"][1].tolist() == [2, 0, 32767, 3]
    assert r["out"][0].tolist() == [11, 13, 14] and (r["n"], r["c"]) == (4, 3)
    assert R.stat_txt(r["hm"][1]) == "# k-mer frequency\tnumber of such k-mers\n0\t1\n2\t1\n3\t1\n32767\t1\n\n"
    r = S.unique_kmers([f1, f2], [g1, _s([10, 11, 12, 13, 14], [7] * 5)], b=0)
    assert r["hm"][0].tolist() == [10, 11, 12, 13, 14] and r["hm"][1].tolist() == [0] * 5 and r["c"] == 0


def test_margin_guard_for_the_gpu_shapes():
    """no reachable statistic within 1e-9 q of q and no reachable p within 1e-12 of pmw (the project's margins): the decisions depend
    neither on the last bit of the quantile nor on that of an erfc"""
    for na, nb, pchi2, pmw in GPU_SHAPES2:
        q = R.chi2_quantile(pchi2)
        n1a, n1b = np.meshgrid(np.arange(na + 1), np.arange(nb + 1), indexing="ij")
        kk = R.chisq_kk(na - n1a, n1a, nb - n1b, n1b).ravel()
        kk = kk[np.isfinite(kk)]
        assert not np.any(np.abs(kk - q) <= 1e-9 * q), (na, nb, pchi2)
        if pmw > 0:
            ps = np.array([R.mw_pvalue_from_umin(u / 2.0, na, nb) for u in range(na * nb + 1)])
            assert not np.any(np.abs(ps - pmw) <= 1e-12), (na, nb, pmw)
    for na, nb, nc, pchi2, pmw in GPU_SHAPES3:
        q = R.chi2_quantile(pchi2)
        n1a, n1b, n1c = np.meshgrid(np.arange(na + 1), np.arange(nb + 1), np.arange(nc + 1), indexing="ij")
        kk = R3.chisq3_stat(na - n1a, n1a, nb - n1b, n1b, nc - n1c, n1c).ravel()
        kk = kk[np.isfinite(kk)]
        assert not np.any(np.abs(kk - q) <= 1e-9 * q), (na, nb, nc, pchi2)
        if pmw > 0:
            for nx, ny in ((na, nb), (nb, nc), (na, nc)):
                ps = np.array([R.mw_pvalue_from_umin(u / 2.0, nx, ny) for u in range(nx * ny + 1)])
                assert not np.any(np.abs(ps - pmw) <= 1e-12), (nx, ny, pmw)


def test_driver_accepts_the_three_tools(san_cli, tmp_path):
    r = _run(san_cli, ["-ts"], str(tmp_path))
    assert r.returncode == 0
    for tool in ("specific-kmers\t", "specific-kmers-3\t", "unique-kmers\t", "unique-kmers-multi\t"):
        assert tool in r.stdout, tool
    f = tmp_path / "a.kmers.bin"
    f.write_bytes(R.records_to_bytes(np.array([1, 2], np.uint64), np.array([3, 4])))
    f, w = str(f), lambda n: str(tmp_path / n)
    # the reference's option names reach the library call; in.properties lists the tool's own parameters (no maximal-bad-frequence)
    r = _run(san_cli, ["-t", "specific-kmers", "-A", f, f, "-B", f, "-pchi2", "0.01", "-pmw", "0.1", "-w", w("w1")], str(tmp_path))
    assert r.returncode == 1 and "no mf_specific_kmers" in r.stderr, r.stderr
    props = (tmp_path / "w1" / "in.properties").read_text()
    assert "p-value-chi2 = 0.01" in props and "p-value-mw = 0.1" in props and "a-kmers" in props and "maximal-bad-frequence" not in props
    r = _run(san_cli, ["-t", "specific-kmers-3", "-A", f, "-B", f, f, "-C", f, "--output-dir", w("o2"), "-w", w("w2")], str(tmp_path))
    assert r.returncode == 1 and "no mf_specific_kmers3" in r.stderr, r.stderr
    props = (tmp_path / "w2" / "in.properties").read_text()
    assert "c-kmers" in props and "p-value-chi2 = 0.05" in props and "o2" in props
    r = _run(san_cli, ["-t", "unique-kmers", "-k", "5", "-i", f, f, "--filter-kmers", f, "-w", w("w3")], str(tmp_path))
    assert r.returncode == 1 and "no mf_unique_kmers" in r.stderr and "multi" not in r.stderr, r.stderr
    props = (tmp_path / "w3" / "in.properties").read_text()
    assert "filter-kmers" in props and "maximal-bad-frequence = 1" in props and "min-samples" not in props
    assert "maximal-bad-frequence = 3" in (_run(san_cli, ["-t", "unique-kmers", "-k", "5", "-i", f, "--filter-kmers", f, "-b", "3", "-w", w("w4")],
                                                str(tmp_path)), (tmp_path / "w4" / "in.properties").read_text())[1]
    # a missing group, an empty one, a p-value outside [0, 1], k outside 1 .. 31
    for tool, groups in (("specific-kmers", "AB"), ("specific-kmers-3", "ABC")):
        for miss in groups:
            opts = [x for g in groups if g != miss for x in ("-" + g, f)]
            r = _run(san_cli, ["-t", tool, *opts, "-w", w("m_%s_%s" % (tool, miss))], str(tmp_path))
            assert r.returncode == 1 and "Mandatory argument --%s-kmers" % miss.lower() in r.stderr, r.stderr
        opts = [x for g in groups for x in (("-" + g,) if g == "B" else ("-" + g, f))]
        r = _run(san_cli, ["-t", tool, *opts, "-w", w("e_" + tool)], str(tmp_path))
        assert r.returncode == 1 and "at least one sample (|A| = 1, |B| = 0" in r.stderr, r.stderr
        opts = [x for g in groups for x in ("-" + g, f)]
        r = _run(san_cli, ["-t", tool, *opts, "-pchi2", "2", "-w", w("p_" + tool)], str(tmp_path))
        assert r.returncode == 1 and "Error calculating chi-squared value!" in r.stderr, r.stderr
    for k, text in (("32", "no more than 31"), ("0", "at least 1")):
        r = _run(san_cli, ["-t", "unique-kmers", "-k", k, "-i", f, "--filter-kmers", f, "-w", w("k" + k)], str(tmp_path))
        assert r.returncode == 1 and text in r.stderr, r.stderr
    r = _run(san_cli, ["-t", "unique-kmers", "-k", "5", "-i", f, "-w", w("nf")], str(tmp_path))
    assert r.returncode == 1 and "Mandatory argument --filter-kmers" in r.stderr, r.stderr
    assert "Mandatory argument --k-mers" in _run(san_cli, ["-t", "unique-kmers", "-k", "5", "--filter-kmers", f, "-w", w("ni")], str(tmp_path)).stderr
