"""The reference of the wide set tools (tests/wkmersets_ref.py) pinned by hand-worked cases and cross-checked against the k <= 31 numpy reference
(tests/kmersets_ref.py) at k = 32, where every high word is 0; the driver's three tools of pipeline 2 with --wide-kmers on the host-only stub build."""
import os
import subprocess

import numpy as np
import pytest

import kmersets_ref as NR
import wide_files_ref as WF
import wkmersets_cases as CASES
import wkmersets_ref as R
from test_driver_tools_cpu import ENV, stub_driver

A, B, C, D, E = (5 << 64) | 7, (5 << 64) | 8, (6 << 64) | 7, 9, (1 << 70) | 1


def test_java_short():
    assert [R.java_short(x) for x in (0, 32767, 32768, 60000, 65534, 65536 + 5)] == [0, 32767, -32768, -5536, -2, 5]


def test_unique_kmers_multi_by_hand():
    ins = [{A: 3, B: 1, C: 20000, D: 32767}, {A: 2, C: 20000, D: 32767, E: 2}, {A: 5, C: 20000}]
    flt = [{B: 9, E: 1}, {A: 1, 12345: 7}]
    r = R.unique_kmers_multi(ins, flt, b=1, min_samples=1, max_samples=5)
    # b = 1: B (count 1) is in no input; A: 3 samples, sum 10; C: 3 x 20000 wraps to -5536 and is dropped; D: 2 x 32767 = 65534 -> -2, dropped;
    # E: one sample, sum 2.  Filters at b = 1: B 9 (not in the union), E 1 and A 1 (not > b: knock nothing), 12345 (outside)
    assert r["n_union"] == 4
    assert r["tables"] == [{A: 10, E: 2}, {A: 10}, {A: 10}, {}] and r["counts"] == [2, 1, 1, 0]
    # b = 0: everything counts; B: sum 1 but knocked out by the first filter; E knocked out too; A by the second
    r = R.unique_kmers_multi(ins, flt, b=0, min_samples=1, max_samples=1)
    assert r["n_union"] == 5 and r["tables"] == [{}] and r["counts"] == [0]
    r = R.unique_kmers_multi(ins, [], b=0, min_samples=2, max_samples=3)
    assert r["tables"] == [{A: 10}, {A: 10}] and r["n_union"] == 5
    # sums of exactly b and b + 1
    r = R.unique_kmers_multi([{A: 3, B: 2}, {A: 2, B: 2}], [], b=4, min_samples=1, max_samples=1)
    assert r["tables"] == [{}] and r["n_union"] == 0           # every count <= b: nothing goes in
    r = R.unique_kmers_multi([{A: 5, B: 5}, {B: 6}], [], b=4, min_samples=1, max_samples=1)
    assert r["tables"] == [{A: 5, B: 11}]
    for bad in (dict(b=-1), dict(min_samples=3, max_samples=2)):
        with pytest.raises(ValueError):
            R.unique_kmers_multi(ins, flt, **bad)


def test_filter_and_load_by_hand():
    t = {A: 1, B: 2, C: 3, D: 4}
    f = {A: 9, B: 3, C: 2}
    assert R.filter_kmers(t, 1, f, 2) == {B: 2}                # A: count 1 <= 1; C: filter value 2 <= 2; D: absent = 0
    assert R.filter_kmers(t, 0, f, -1) == t                   # absent = 0 > -1
    assert R.filter_kmers(t, 0, {}, 0) == {} and R.filter_kmers({}, 0, f, 0) == {}
    assert R.load([{A: 1, B: 30000}, {A: 4, B: 30000}], 1) == {A: 4, B: 32767}
    assert R.kmers_bin({C: 3, A: 1}) == bytes([0] * 7 + [5] + [0] * 7 + [7, 0, 1] + [0] * 7 + [6] + [0] * 7 + [7, 0, 3])
    assert R.canonical(0, 33) == 0 and R.canonical((1 << 66) - 1, 33) == 0


def test_against_the_narrow_reference_at_k32():
    """k = 32: a k-mer is its low word, so the numpy reference of the k <= 31 tools applies to the low words as they are"""
    rng = np.random.default_rng(32)
    pool = np.unique(rng.integers(0, 1 << 63, 400, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 400, dtype=np.uint64))
    samples = []
    for _ in range(6):
        keys = np.sort(rng.choice(pool, 150, replace=False))
        cnt = rng.choice(np.array([1, 2, 3, 20000, 32767]), len(keys), p=[0.3, 0.3, 0.2, 0.15, 0.05])
        samples.append((keys, cnt))
    ins, flt = samples[:4], samples[4:]
    as_dict = lambda s: {int(x): int(c) for x, c in zip(*s)}
    for b in (0, 1, 2):
        want = NR.unique_kmers_multi(ins, flt, b, 1, 6)
        got = R.unique_kmers_multi([as_dict(s) for s in ins], [as_dict(s) for s in flt], b, 1, 6)
        assert got["n_union"] == want["n_union"] and got["counts"] == want["counts"] and any(got["counts"])
        for t, (_, wk, wv) in zip(got["tables"], want["files"]):
            assert sorted(t) == [int(x) for x in wk] and [t[x] for x in sorted(t)] == [int(v) for v in wv]
    assert any(v < 0 for v in NR.java_short(np.array([3 * 20000])))


@pytest.mark.parametrize("k", (32, 33, 47, 63))
def test_crafted_cohort_meets_the_rules(k):
    """what tests/wkmersets_cases.py is for, checked on the reference alone"""
    ins, flt, nm = CASES.crafted(k)
    assert ins[3] == {} and all(x == R.canonical(x, k) and x < 4 ** k for t in ins + flt for x in t)
    with_f, no_f = R.unique_kmers_multi(ins, flt, 1, 1, 9), R.unique_kmers_multi(ins, [], 1, 1, 9)
    t, n = with_f["tables"][0], no_f["tables"][0]
    assert t[0] == 7 and t[nm["top"]] == 11 and t[nm["above_b"]] == 2 and nm["at_b"] not in n                     # key 0, the largest key, sums of b + 1 and b
    assert nm["wrap"] not in n and nm["sat"] not in n and with_f["n_union"] == no_f["n_union"] == len(n) + 2      # 3 x 20000 and 2 x 32767 are in the union alone
    assert set(n) - set(t) == {nm["everywhere"], nm["f_hit"]}                  # f_small (count <= b) knocks nothing, f_only is outside the union
    assert nm["f_small"] in t and nm["f_only"] not in n and nm["hi_pair"][1] in t
    (lx, ly), (hx, hy) = nm["lo_pair"], nm["hi_pair"]
    assert lx >> 64 == ly >> 64 and lx != ly and t[lx] == 4 and t[ly] == 3
    assert (hx & R.MASK64 == hy & R.MASK64 and hx >> 64 != hy >> 64) or k == 32
    assert t[hx] == 2 and t[hy] == 6                                           # (the 1 of the third input is not > b)
    # min ... max runs past the inputs: the list ends with its first empty table
    assert [c > 0 for c in with_f["counts"]] == [True, True, False] and [c > 0 for c in no_f["counts"]] == [True, True, True, False]
    assert R.unique_kmers_multi(ins[:1], flt, 1, 1, 9)["counts"][1:] == [0]
    # b = 0: the filters' counts of 1 knock out as well
    r0, n0 = R.unique_kmers_multi(ins, flt, 0, 1, 1)["tables"][0], R.unique_kmers_multi(ins, [], 0, 1, 1)["tables"][0]
    assert set(n0) - set(r0) == {nm["everywhere"], nm["f_hit"], nm["f_small"], hy} and n0[hx] == 3


def test_largest_canonical_kmer():
    for k in (4, 5, 6, 7):
        assert CASES.largest_canonical(k) == max(x for x in range(4 ** k) if x <= WF.revcomp(x, k)), k
    for k in (32, 33, 47, 63):
        x = CASES.largest_canonical(k)
        assert x == R.canonical(x, k) and x >> (2 * k - 2) == 3


# ---- the driver on the stub build ----
@pytest.fixture(scope="module")
def driver():
    return stub_driver()


def _run(driver, cwd, *args):
    return subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, env=ENV, timeout=120, cwd=str(cwd))


TOOLS = {
    "kmer-counter-posneg": (["--positiveReads", "a.fa", "--negativeReads", "b.fa"], "mf_count_reads_wide"),
    "unique-kmers-multi": (["-i", "a.kmers.bin", "--filter-kmers", "b.kmers.bin"], "this build of the library has no mf_unique_kmers_multi_wide"),
    "kmers-filter": (["-i", "a.kmers.bin", "--filter-kmers", "b.kmers.bin"], "this build of the library has no mf_wtable_write_kmers_filtered"),
}


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_driver_takes_the_wide_set_tools(driver, tmp_path, tool):
    for name in ("a.fa", "b.fa"):
        (tmp_path / name).write_text(">a\n" + "ACGT" * 20 + "\n")
    for name in ("a.kmers.bin", "b.kmers.bin"):
        (tmp_path / name).write_bytes(b"")
    args, missing = TOOLS[tool]
    # with the flag and k > 31 the run gets past check_k to the library: the stub has no such entry, and the run names it
    r = _run(driver, tmp_path, "-t", tool, "--wide-kmers", "-k", 40, *args, "-w", "w1")
    out = r.stderr + r.stdout
    assert r.returncode == 1 and missing in out and "no more than 31" not in out, out
    assert "wide-kmers" in (tmp_path / "w1" / "in.properties").read_text() and not (tmp_path / "w1" / "SUCCESS").exists()
    # without the flag the reference's message, as ever
    r = _run(driver, tmp_path, "-t", tool, "-k", 40, *args, "-w", "w2")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr + r.stdout
    r = _run(driver, tmp_path, "-t", tool, "--wide-kmers", "-k", 64, *args, "-w", "w3")
    assert r.returncode == 1 and "The size of k-mer must be no more than 63." in r.stderr + r.stdout
    # k <= 31: the flag changes nothing
    r = _run(driver, tmp_path, "-t", tool, "--wide-kmers", "-k", 21, *args, "-w", "w4")
    out = r.stderr + r.stdout
    assert "_wide" not in out and "no more than" not in out, out
    assert "wide-kmers" not in (tmp_path / "w4" / "in.properties").read_text()


def test_the_pinned_refusal_stays(driver, tmp_path):
    (tmp_path / "a.kmers.bin").write_bytes(b"")
    r = _run(driver, tmp_path, "--wide-kmers", "-t", "kmers-samples-counter", "-k", 40, "-i", "a.kmers.bin", "-w", "w")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr + r.stdout
