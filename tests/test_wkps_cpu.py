"""The reference of the wide kmers-per-sample (tests/wkps_ref.py) cross-checked against the k <= 31 restatement (tests/kps_ref.py) through an
order-preserving map of the k-mers to their ranks, and pinned by hand; the crafted cohort (tests/wkps_cases.py) checked to meet every rule of
the definition; the driver's kmers-per-sample with --wide-kmers on the host-only stub build."""
import subprocess

import numpy as np
import pytest

import kps_ref as NR
import wkmersets_ref as WR
import wkps_cases as CASES
import wkps_ref as R
from test_driver_tools_cpu import ENV, stub_driver

KS = (32, 33, 47, 63)


def test_thresh_is_java_int_arithmetic():
    assert [R.thresh(6, p) for p in (-50, 0, 20, 50, 100, 150)] == [-3, 0, 1, 3, 6, 9]
    assert R.thresh(3, 34) == 1 and R.thresh(1, 20) == 0 and R.thresh(1, 100) == 1 and R.thresh(7, -20) == -1       # toward zero
    assert R.thresh(32767, 2 ** 31 - 1) == NR.thresh_of(32767, 2 ** 31 - 1) and R.thresh(3, -2 ** 31) == NR.thresh_of(3, -2 ** 31)   # the product wraps
    assert R.thresh(2, 2 ** 30) == -21474836


def test_select_by_hand():
    A, B, C, D = (5 << 64) | 7, (5 << 64) | 8, (6 << 64) | 7, 9
    s = [{A: 3, D: 1}, {A: 2, B: 40000 // 4, C: 1}, {B: 7, C: 2}]
    keys, n, mat = R.select(s, 34)                          # thresh 1: D is in sample 0 alone
    assert keys == [A, B, C] and n.tolist() == [1, 2, 2] and mat.tolist() == [[3, 0, 0], [2, 10000, 1], [0, 7, 2]]
    keys, n, mat = R.select(s, 0)
    assert keys == [D, A, B, C] and n.tolist() == [0, 1, 2, 2] and mat[0].tolist() == [1, 3, 0, 0]
    keys, n, mat = R.select(s, 67, count_first=True)       # thresh 2
    assert keys == [A, B, C] and n.tolist() == [2, 2, 2]
    keys, n, mat = R.select(s, 34, max_bad=1)              # C's 1 and D's 1 are not there
    assert keys == [A, B, C] and n.tolist() == [1, 2, 1] and mat.tolist() == [[3, 0, 0], [2, 10000, 0], [0, 7, 2]]
    assert R.select(s, 101)[0] == [] and R.select(s, 101)[2].shape == (3, 0)
    assert R.header_text([A, D], 34) == b"\tGG" + b"A" * 30 + b"GT" + b"\t" + b"A" * 32 + b"CG"          # k = 34: two bases in the high word
    assert R.row_text([0, 7, 32767]) == b"\t0\t7\t32767" and R.row_name("/x/a.kmers.bin.kmers.bin") == "a"
    assert R.file_text(s, ["p/s0.kmers.bin", "s1", "s2.kmers.bin"], 33, 101) == ([], b"\ns0\ns1\ns2\n")


def _ranked(samples):
    """the cohort with every k-mer replaced by its rank among the cohort's k-mers: order kept, values far below 2^62"""
    rank = {x: i for i, x in enumerate(sorted(set().union(*samples)))}
    narrow = [(np.array([rank[x] for x in t], dtype=np.uint64), np.array(list(t.values()), dtype=np.int64)) for t in samples]
    return rank, narrow


def _random_cohort(k, seed):
    rng = np.random.default_rng(seed)
    mask = (1 << (2 * k)) - 1
    pool = sorted({WR.canonical(int.from_bytes(rng.bytes(16), "big") & mask, k) for _ in range(600)})
    samples = []
    for j in range(5):
        pick = rng.choice(len(pool), (300, 200, 350, 0, 250)[j], replace=False)
        samples.append({pool[int(i)]: int(c) for i, c in zip(pick, rng.choice(np.array([1, 2, 3, 50, 700, 9000, 32767]), len(pick)))})
    return samples


@pytest.mark.parametrize("k", (33, 63))
def test_against_the_narrow_restatement(k):
    for samples in (_random_cohort(k, 77 + k), CASES.cohort(k)[0]):
        rank, narrow = _ranked(samples)
        some = set()
        for percent, count_first, max_bad in ((20, False, 0), (50, False, 0), (50, True, 0), (0, False, 1), (60, True, 2), (100, False, 0), (-50, True, 0), (150, True, 0)):
            keys, n, mat = R.select(samples, percent, count_first, max_bad)
            wk, wn, wm = NR.select(narrow, percent, count_first, max_bad)
            assert [rank[x] for x in keys] == wk.tolist() and np.array_equal(n, wn) and np.array_equal(mat, wm), (percent, count_first, max_bad)
            some.add(len(keys))
        assert 0 in some and len(some) >= 4


@pytest.mark.parametrize("k", KS)
def test_crafted_cohort_meets_the_rules(k):
    samples, nm = CASES.cohort(k)
    assert len(samples) == 6 and samples[3] == {} and all(x == WR.canonical(x, k) and x < 4 ** k for t in samples for x in t)
    all_keys, all_n, all_mat = R.select(samples, 0)
    k20 = R.select(samples, 20)[0]
    k50, n50, _ = R.select(samples, 50)
    assert R.thresh(6, 50) == 3
    # a k-mer of sample 0 alone: a candidate with n = 0, counted only with count_first
    assert all(nm["only0"] not in t for t in samples[1:]) and all_n[all_keys.index(nm["only0"])] == 0 and nm["only0"] not in k20
    assert nm["only0"] in R.select(samples, 20, count_first=True)[0]
    # n = thresh - 1 and n = thresh
    assert nm["below"] not in k50 and all_n[all_keys.index(nm["below"])] == 2 and n50[k50.index(nm["at"])] == 3 and n50.min() == 3
    # key 0 and the largest canonical k-mer are the ends of the selection
    assert all_keys[0] == 0 and all_keys[-1] == nm["top"] == max(set().union(*samples))
    # neighbours that differ in one word alone
    (lx, ly), (hx, hy) = nm["lo_pair"], nm["hi_pair"]
    assert {lx, ly, hx, hy} <= set(all_keys) and lx >> 64 == ly >> 64 and lx != ly
    assert (hx & WR.MASK64 == hy & WR.MASK64 and hx >> 64 != hy >> 64) or k == 32
    # counts of max_bad and max_bad + 1, for max_bad = 1 (and 1 = max_bad + 1 for max_bad = 0)
    assert samples[0][nm["at_b"]] == 1 and samples[0][nm["above_b"]] == 2
    k1 = R.select(samples, 0, max_bad=1)[0]
    assert nm["at_b"] in all_keys and nm["at_b"] not in k1 and nm["above_b"] in k1
    # every decimal width, and every percent of the GPU test selects something else
    assert {len(str(int(v))) for v in np.unique(all_mat)} == {1, 2, 3, 4, 5}
    sizes = [len(R.select(samples, p)[0]) for p in (-50, 0, 20, 50, 100, 150)]
    assert sizes[0] == sizes[1] == len(all_keys) > sizes[2] > sizes[3] > sizes[4] == sizes[5] == 0
    assert len(R.select(samples, 100, count_first=True)[0]) == 0 and len(R.select(samples, 50, count_first=True)[0]) > sizes[3]


# ---- the driver on the stub build ----
@pytest.fixture(scope="module")
def driver():
    return stub_driver()


def _run(driver, cwd, *args):
    return subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, env=ENV, timeout=120, cwd=str(cwd))


def test_driver_takes_wide_kmers_per_sample(driver, tmp_path):
    for name in ("a.kmers.bin", "b.kmers.bin"):
        (tmp_path / name).write_bytes(b"")
    args = ["-i", "a.kmers.bin", "b.kmers.bin", "-perc", 40]
    # with the flag and k > 31 the run gets past check_k to the library: the stub has no such entry, and the run names it
    r = _run(driver, tmp_path, "--wide-kmers", "-t", "kmers-per-sample", "-k", 40, *args, "-w", "w1")
    out = r.stderr + r.stdout
    assert r.returncode == 1 and "this build of the library has no mf_kmers_per_sample_wide" in out and "no more than 31" not in out, out
    assert "wide-kmers" in (tmp_path / "w1" / "in.properties").read_text() and not (tmp_path / "w1" / "SUCCESS").exists()
    # without the flag the reference's message, as ever
    r = _run(driver, tmp_path, "-t", "kmers-per-sample", "-k", 40, *args, "-w", "w2")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr + r.stdout
    r = _run(driver, tmp_path, "-t", "kmers-per-sample", "-k", 32, *args, "-w", "w2b")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr + r.stdout
    r = _run(driver, tmp_path, "--wide-kmers", "-t", "kmers-per-sample", "-k", 64, *args, "-w", "w3")
    assert r.returncode == 1 and "The size of k-mer must be no more than 63." in r.stderr + r.stdout
    # k <= 31: the flag changes nothing
    r = _run(driver, tmp_path, "--wide-kmers", "-t", "kmers-per-sample", "-k", 21, *args, "-w", "w4")
    out = r.stderr + r.stdout
    assert "_wide" not in out and "no more than" not in out, out
    assert "wide-kmers" not in (tmp_path / "w4" / "in.properties").read_text()
