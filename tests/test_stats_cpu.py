"""stats-kmers / kmers-samples-counter without a GPU: the restatement (tests/stats_ref.py) on hand-worked cases, the margin guard of the
decisions for the shapes the GPU tests use, and the driver's option handling in the sanitizer build (tests/host/mf_stub.cpp has no GPU)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import stats_ref as R
from conftest import ROOT

# (nA, nB, pchi2, pmw) of tests/test_stats_gpu.py
GPU_SHAPES = [(6, 6, 0.05, 0.05), (6, 6, 0.01, 0.0), (6, 6, 0.2, 0.1), (1, 5, 0.05, 0.05), (5, 1, 0.05, 0.05), (3, 3, 0.05, 0.05),
              (150, 150, 0.05, 0.05), (16, 16, 0.05, 0.05), (1, 2, 0.05, 0.05), (2, 2, 0.05, 0.05), (1, 1, 0.05, 0.05),
              (3, 3, 0.3, 0.05), (2, 2, 0.3, 0.05), (1, 3, 0.3, 0.05), (3, 1, 0.3, 0.05), (4, 4, 0.3, 0.2)]


def test_chisq_hand_worked():
    # n0A = 1, n1A = 5, n0B = 5, n1B = 1: c0 = 100/6, c1 = 500/6, p0 = 500/6, p1 = 100/6 (float); gr_1 = gr_2 = 100, all = 200;
    # x1 = x2 = x3 = x4 = 50; kk = 4 * (|100/6 - 50| - 0.5)^2 / 50
    kk = float(R.chisq_kk(1, 5, 5, 1))
    c = float(np.float32(100) * np.float32(1) / np.float32(6))
    d = abs(np.float32(c) - np.float32(50))
    want = 4 * ((float(d) - 0.5) ** 2) / 50.0
    assert kk == pytest.approx(want, rel=1e-12) and kk == pytest.approx(4 * (100 / 3 - 0.5) ** 2 / 50, rel=1e-6)
    # identical groups: no difference
    assert float(R.chisq_kk(3, 3, 3, 3)) == pytest.approx(4 * 0.25 / 50)
    # chi2(1) quantiles
    assert R.chi2_quantile(0.05) == pytest.approx(3.841458820694124, rel=1e-12)
    assert R.chi2_quantile(0.01) == pytest.approx(6.634896601021214, rel=1e-12)
    assert R.chi2_quantile(0.0) == math.inf and R.chi2_quantile(1.0) == 0.0


def test_mann_whitney_small_examples_with_ties():
    # x = [1, 2, 3], y = [4, 5, 6]: U1 = 0, Umin = 0, z = (0 - 4.5) / sqrt(9 * 7 / 12)
    z = -4.5 / math.sqrt(63 / 12)
    assert R.mw_test([1, 2, 3], [4, 5, 6]) == pytest.approx(math.erfc(-z / math.sqrt(2)), rel=1e-14)
    # ties: x = [1, 2, 2], y = [2, 3, 3]: ranks 1, 3, 3 | 3, 5.5, 5.5 -> R1 = 7, U1 = 1; pairs: 2 [a>b] + [a==b] = 0 + 1 + 1 = 2
    assert R.ranks_fixed_average([1, 2, 2, 2, 3, 3]).tolist() == [1, 3, 3, 3, 5.5, 5.5]
    assert R.mw_twice_u1(np.array([[1., 2, 2]]), np.array([[2., 3, 3]]))[0] == 2
    assert R.mw_test([1, 2, 2], [2, 3, 3]) == pytest.approx(R.mw_pvalue_from_umin(1.0, 3, 3), rel=1e-15)
    # all equal: U1 = nA nB / 2, z = 0, p = 1
    assert R.mw_test([5, 5], [5, 5, 5]) == 1.0
    # the pairwise form equals the rank form on random rows with ties
    rng = np.random.default_rng(3)
    for _ in range(300):
        na, nb = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        x, y = rng.integers(0, 4, na).astype(float), rng.integers(0, 4, nb).astype(float)
        u2 = int(R.mw_twice_u1(x[None], y[None])[0])
        p = R.mw_pvalue_from_umin(min(u2, 2 * na * nb - u2) / 2.0, na, nb)
        assert p == R.mw_test(x, y)


def test_nan_rule_on_each_side():
    # NaN in A: the rank sum is NaN -> p NaN -> rejected
    assert math.isnan(R.mw_test([np.nan, 1.0, 2.0], [3.0, 4.0]))
    # NaN in B: it drops out of the pairwise count, U2 = nA nB - U1 with the full nB
    x, y = np.array([1.0, 5.0]), np.array([np.nan, 2.0, 7.0])
    u2 = int(R.mw_twice_u1(x[None], y[None])[0])
    assert u2 == 2                                   # (5 > 2)
    assert R.mw_test(x, y) == R.mw_pvalue_from_umin(min(u2, 12 - u2) / 2.0, 2, 3)
    # through the whole restatement: an empty sample in A -> every survivor rejected by MW; in B -> rows still decided
    k = np.arange(1, 200, dtype=np.uint64)
    full = (k, np.full(len(k), 5, np.int16))
    empty = (np.zeros(0, np.uint64), np.zeros(0, np.int16))
    part = (k[:100], np.full(100, 9, np.int16))
    r = R.stats_kmers([empty, part, full], [full, full, part], b=0, p_chi2=0.9, p_mw=0.9)
    assert r["counters"]["group_a"] + r["counters"]["group_b"] == 0 and r["counters"]["mw_rejected"] == len(r["chi"][0])
    r0 = R.stats_kmers([empty, part, full], [full, full, part], b=0, p_chi2=0.9, p_mw=0.0)
    # pmw <= 0: the mean of A is NaN, the record goes to B with value 0 ... unless B's mean is NaN too (never here)
    assert r0["counters"]["group_a"] == 0 and r0["counters"]["group_b"] == len(r0["chi"][0])


def test_scarce_cut():
    for N in range(1, 2000):
        assert math.ceil(N * 0.05) == -(-N // 20)
    # N = 12: ceil(0.6) = 1 -> a k-mer in one sample is scarce, in two it is not
    k = np.array([1, 2], dtype=np.uint64)
    s1 = (k, np.array([3, 3], np.int16))
    s2 = (k[:1], np.array([3], np.int16))
    none = (np.zeros(0, np.uint64), np.zeros(0, np.int16))
    r = R.stats_kmers([s1, s2] + [none] * 4, [none] * 6, p_chi2=0.99, p_mw=0.0)
    assert r["counters"]["scarce"] == 1 and r["counters"]["n"] == 2


def test_java_cast():
    v = R.java_short_of_int([np.nan, 0.9, -0.9, 32767.9, 32768.0, 65536.5, 70000.0, 3e9, -3e9, -1.5, np.inf, -np.inf])
    want = [0, 0, 0, 32767, 32768, 0, 70000 - 65536, 0xFFFF, 0x0000, 0xFFFF, 0xFFFF, 0x0000]
    assert v.tolist() == want


def test_margin_guard_for_the_gpu_shapes():
    """no reachable kk within 1e-9 q of q and no reachable p within 1e-12 of pmw: the decisions do not depend on the last bits of an
    erfc or of the quantile solver"""
    for na, nb, pchi2, pmw in GPU_SHAPES:
        q = R.chi2_quantile(pchi2)
        n1a, n1b = np.meshgrid(np.arange(na + 1), np.arange(nb + 1), indexing="ij")
        kk = R.chisq_kk(na - n1a, n1a, nb - n1b, n1b).ravel()
        kk = kk[np.isfinite(kk)]
        assert not np.any(np.abs(kk - q) <= 1e-9 * q), (na, nb, pchi2)
        if pmw > 0:
            ps = np.array([R.mw_pvalue_from_umin(u / 2.0, na, nb) for u in range(na * nb + 1)])
            assert not np.any(np.abs(ps - pmw) <= 1e-12), (na, nb, pmw)


def test_kmers_samples_counter_restatement():
    k = np.array([7, 7, 3, 9], dtype=np.uint64)
    f1 = (k, np.array([1, 1, 2, 5], np.int16))        # 7 listed twice, each record <= 1: absent at b = 1 (a sum would say present)
    f2 = (np.array([3, 8], np.uint64), np.array([1, 4], np.int16))
    keys, n = R.kmers_samples_count([f1, f2], b=1)
    assert keys.tolist() == [3, 8, 9] and n.tolist() == [1, 1, 1]
    keys, n = R.kmers_samples_count([f1, f2], b=0)
    assert keys.tolist() == [3, 7, 8, 9] and n.tolist() == [2, 1, 1, 1]
    assert R.stat_txt(n) == "# k-mer frequency\tnumber of such k-mers\n1\t3\n2\t1\n\n"


# ---- the driver in the sanitizer build (same recipe as tests/test_host_sanitized_cpu.py) ----
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


def test_driver_accepts_the_new_tools(san_cli, tmp_path):
    r = _run(san_cli, ["-ts"], str(tmp_path))
    assert r.returncode == 0 and "stats-kmers" in r.stdout and "kmers-samples-counter" in r.stdout
    f = tmp_path / "a.kmers.bin"
    f.write_bytes(R.records_to_bytes(np.array([1, 2], np.uint64), np.array([3, 4])))
    r = _run(san_cli, ["-t", "stats-kmers", "-A", str(f), str(f), "-B", str(f), "-pchi2", "0.01", "-pmw", "0.1", "-b", "2", "-w", str(tmp_path / "w1")], str(tmp_path))
    assert r.returncode == 1 and "mf_stats_kmers" in r.stderr, r.stderr
    props = (tmp_path / "w1" / "in.properties").read_text()
    assert "p-value-chi2 = 0.01" in props and "maximal-bad-frequence = 2" in props and "a-kmers" in props
    r = _run(san_cli, ["-t", "kmers-samples-counter", "-k", "31", "-i", str(f), str(f), "-b", "3", "-w", str(tmp_path / "w2")], str(tmp_path))
    assert r.returncode == 1 and "mf_kmers_samples_count" in r.stderr, r.stderr
    assert "maximal-bad-frequence = 3" in (tmp_path / "w2" / "in.properties").read_text()
    # mandatory options and k
    assert "Mandatory argument --b-kmers" in _run(san_cli, ["-t", "stats-kmers", "-A", str(f), "-w", str(tmp_path / "w3")], str(tmp_path)).stderr
    assert "at least 1" in _run(san_cli, ["-t", "kmers-samples-counter", "-k", "0", "-i", str(f), "-w", str(tmp_path / "w4")], str(tmp_path)).stderr
    assert "no more than 31" in _run(san_cli, ["-t", "kmers-samples-counter", "-k", "32", "-i", str(f), "-w", str(tmp_path / "w5")], str(tmp_path)).stderr
    assert "Can't parse double" in _run(san_cli, ["-t", "stats-kmers", "-A", str(f), "-B", str(f), "-pchi2", "x", "-w", str(tmp_path / "w6")], str(tmp_path)).stderr
