"""kmers-per-sample without a GPU: the restatement (tests/kps_ref.py) on hand-worked cases, the declarations (header, Python mirror,
driver text) and the driver's option handling in the sanitizer build (tests/host/mf_stub.cpp has no GPU)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import kps_ref as K
from conftest import ROOT
from metafast_amd import lib as L


def _s(keys, counts):
    return np.asarray(keys, np.uint64), np.asarray(counts, np.int64)


# k = 2: AA = 0, AG = 1, GA = 4, TT = 15
X0, X01, X12 = 1, 4, 15                        # only in sample 0; in samples 0 and 1; in samples 1 and 2
THREE = [_s([X0, X01], [7, 3]), _s([X01, X12], [10, 100]), _s([X12], [32767])]
NAMES3 = ["/d/s0.kmers.bin", "s1.kmers.bin", "x/y/s2"]


def test_three_samples_hand_worked():
    # N = 3, perc 20: thresh = 60 / 100 = 0 -> the whole union; the first file is not counted: n = 0, 1, 2
    keys, n, mat, text = K.kmers_per_sample(THREE, NAMES3, 2, 20)
    assert keys.tolist() == [X0, X01, X12] and n.tolist() == [0, 1, 2]
    assert mat.tolist() == [[7, 3, 0], [0, 10, 100], [0, 0, 32767]]
    assert text == b"\tAG\tGA\tTT\ns0\t7\t3\t0\ns1\t0\t10\t100\ns2\t0\t0\t32767\n"
    # perc 34: thresh = 102 / 100 = 1 -> the k-mer of sample 0 alone is gone
    keys, n, mat, text = K.kmers_per_sample(THREE, NAMES3, 2, 34)
    assert keys.tolist() == [X01, X12] and n.tolist() == [1, 2]
    assert text == b"\tGA\tTT\ns0\t3\t0\ns1\t10\t100\ns2\t0\t32767\n"
    # perc 67: thresh = 201 / 100 = 2: a k-mer of files 0 and 1 has n = 1 and is gone as well
    keys, n, mat, _ = K.kmers_per_sample(THREE, NAMES3, 2, 67)
    assert keys.tolist() == [X12] and n.tolist() == [2] and mat.tolist() == [[0], [100], [32767]]
    # count_first: file 0 counts like the others: n = 1, 2, 2, and exactly these cases change
    keys, n, _, _ = K.kmers_per_sample(THREE, NAMES3, 2, 34, count_first=True)
    assert keys.tolist() == [X0, X01, X12] and n.tolist() == [1, 2, 2]
    keys, n, _, _ = K.kmers_per_sample(THREE, NAMES3, 2, 67, count_first=True)
    assert keys.tolist() == [X01, X12] and n.tolist() == [2, 2]
    assert K.kmers_per_sample(THREE, NAMES3, 2, 20, count_first=True)[3] == K.kmers_per_sample(THREE, NAMES3, 2, 20)[3]


def test_threshold_is_java_int_arithmetic():
    assert [K.thresh_of(4, 20), K.thresh_of(5, 20), K.thresh_of(3, 101), K.thresh_of(99, 101), K.thresh_of(100, 101)] == [0, 1, 3, 99, 101]
    assert [K.thresh_of(3, -5), K.thresh_of(30, -5), K.thresh_of(1, 100), K.thresh_of(2, 50), K.thresh_of(6, 50)] == [0, -1, 1, 1, 3]
    assert K.thresh_of(3, 2 ** 30) == -10737418          # 3 * 2^30 wraps to -2^30 as a Java int; / 100 truncates toward zero
    only0 = _s([9], [2])
    # N = 4, perc 20: thresh 0 -- the k-mer that only file 0 holds is a column, with n = 0
    keys, n, mat, _ = K.kmers_per_sample([_s([5, 9], [4, 2]), only0, only0, only0], list("abcd"), 3, 20)
    assert keys.tolist() == [5, 9] and n.tolist() == [0, 3] and mat[:, 0].tolist() == [4, 0, 0, 0]
    # N = 5, perc 20: thresh 1 -- it is gone
    keys, n, mat, _ = K.kmers_per_sample([_s([5, 9], [4, 2]), only0, only0, only0, only0], list("abcde"), 3, 20)
    assert keys.tolist() == [9] and n.tolist() == [4]
    # perc 101 with fewer than 100 files keeps nothing; a negative perc keeps everything
    keys, n, mat, text = K.kmers_per_sample(THREE, NAMES3, 2, 101, count_first=True)
    assert len(keys) == 0 and mat.shape == (3, 0)
    assert text == b"\ns0\ns1\ns2\n"                   # the empty selection: a lone newline, then the bare names
    assert K.kmers_per_sample(THREE, NAMES3, 2, -5)[0].tolist() == [X0, X01, X12]
    assert K.kmers_per_sample(THREE, NAMES3, 2, -50)[0].tolist() == [X0, X01, X12]        # thresh = -1


def test_records_duplicates_and_saturation():
    # a k-mer listed more than once: the values > 0 are added, saturating; 0 and negative values are no records at all
    s = _s([8, 8, 8, 3, 3, 6, 2, 2], [20000, 20000, 5, 0, 4, -7, 0, -1])
    k, c = K.load_kmers(s)
    assert k.tolist() == [3, 8] and c.tolist() == [4, 32767]
    k, c = K.load_kmers(_s([1, 1], [40000, 3]))          # 40000 as an unsigned field is the short -25536
    assert k.tolist() == [1] and c.tolist() == [3]
    keys, n, mat, text = K.kmers_per_sample([_s([], []), s], ["e", "f"], 2, 50)
    assert keys.tolist() == [3, 8] and n.tolist() == [1, 1] and mat.tolist() == [[0, 0], [4, 32767]]
    assert text == b"\tAT\tCA\ne\t0\t0\nf\t4\t32767\n"
    # a resident table read at max_bad = 4: the entry with the sum 4 is no presence and no count
    keys, n, mat = K.select([_s([], []), s], 50, max_bad=4)
    assert keys.tolist() == [8] and mat.tolist() == [[0], [32767]]
    assert K.records_to_bytes([1, 258], [3, -1]) == bytes([0] * 7 + [1, 0, 3] + [0] * 6 + [1, 2, 255, 255])


def test_name_rule_and_text():
    assert K.row_name("/a/b/a.kmers.bin.kmers.bin") == "a"
    assert K.row_name("x.kmers.bin") == "x" and K.row_name("plain.txt") == "plain.txt" and K.row_name("q/.kmers.bin") == ""
    assert K.row_name("a.kmers.kmers.bin.bin") == "a.kmers.bin"          # String.replace: one pass, left to right
    assert K.kmer_text(0b00011011, 4) == "AGCT" and K.kmer_text(0, 3) == "AAA" and K.kmer_text(4 ** 31 - 1, 31) == "T" * 31
    assert K.row_text(np.array([0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 32767, 65535], np.uint16)) == \
        "\t0\t9\t10\t99\t100\t999\t1000\t9999\t10000\t32767\t65535"
    assert K.header_text([0, 15], 2) == "\tAA\tTT" and K.header_text([], 5) == ""


# ---- the declarations ----
EXPORTS = ("mf_kmers_per_sample_tables", "mf_kmers_per_sample", "mf_kps_destroy", "mf_kps_stats", "mf_kps_device_view", "mf_kps_export",
           "mf_kps_header_text", "mf_kps_row_text")


def test_declared_everywhere():
    hdr = open(L.HEADER_PATH).read()
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", hdr))
    for name in EXPORTS:
        assert name in declared and name in L.exported_symbols(), name
    assert "typedef struct mf_kps mf_kps;" in hdr
    assert callable(L.Context.kmers_per_sample) and callable(L.Context.kmers_per_sample_files)
    for m in ("export", "shape", "device_view", "header_text", "row_text", "close"):
        assert callable(getattr(L.KmersPerSample, m)), m
    # (the driver's declaration: test_driver_options below reads the tool's line from the -ts listing of the stub build)
    # no JNI declaration, as for the other file tools
    assert "mf_kmers_per_sample" not in open(os.path.join(ROOT, "jni", "metafast_jni.cpp")).read()
    so = __import__("ctypes").CDLL(L.LIB_PATH)
    for name in EXPORTS:
        assert hasattr(so, name), name


# ---- the driver in the sanitizer build (same recipe as tests/test_stats3_cpu.py) ----
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


def test_driver_options(san_cli, tmp_path):
    r = _run(san_cli, ["-ts"], str(tmp_path))
    assert r.returncode == 0 and "kmers-per-sample\tCounts the abundance of frequent k-mers from dataset in each sample" in r.stdout
    f = tmp_path / "a.kmers.bin"
    f.write_bytes(K.records_to_bytes([1, 2], [3, 4]))
    w = lambda n: str(tmp_path / n)
    # the defaults reach in.properties, then the (absent) library call
    r = _run(san_cli, ["-t", "kmers-per-sample", "-k", "5", "-i", str(f), str(f), "-w", w("w1")], str(tmp_path))
    assert r.returncode == 1 and "mf_kmers_per_sample" in r.stderr, r.stderr
    props = (tmp_path / "w1" / "in.properties").read_text()
    assert "percent-present = 20" in props and "kmers_per_samples" in props and "k-mers" in props and "maximal-bad" not in props, props
    assert (tmp_path / "w1" / "kmers_per_samples").is_dir()
    # -perc takes a negative number; --percent-present and --output-dir are the long names
    r = _run(san_cli, ["-t", "kmers-per-sample", "-k", "5", "-i", str(f), "-perc", "-5", "-w", w("w2")], str(tmp_path))
    assert r.returncode == 1 and "mf_kmers_per_sample" in r.stderr and "percent-present = -5" in (tmp_path / "w2" / "in.properties").read_text(), r.stderr
    r = _run(san_cli, ["-t", "kmers-per-sample", "-k", "5", "--k-mers", str(f), "--percent-present", "50", "--output-dir", w("o3"), "-w", w("w3")], str(tmp_path))
    assert r.returncode == 1 and "mf_kmers_per_sample" in r.stderr and os.path.isdir(w("o3")), r.stderr
    # the two error texts of KmersPerSampleCounter.java:58-65, and the mandatory arguments
    assert "must be at least 1" in _run(san_cli, ["-t", "kmers-per-sample", "-k", "0", "-i", str(f), "-w", w("w4")], str(tmp_path)).stderr
    assert "no more than 31" in _run(san_cli, ["-t", "kmers-per-sample", "-k", "32", "-i", str(f), "-w", w("w5")], str(tmp_path)).stderr
    assert "Mandatory argument --k-mers" in _run(san_cli, ["-t", "kmers-per-sample", "-k", "5", "-w", w("w6")], str(tmp_path)).stderr
    assert "Mandatory argument --k " in _run(san_cli, ["-t", "kmers-per-sample", "-i", str(f), "-w", w("w7")], str(tmp_path)).stderr
    r = _run(san_cli, ["-t", "kmers-per-sample", "-k", "5", "-i", str(f), "-perc", "x", "-w", w("w8")], str(tmp_path))
    assert r.returncode == 1 and "Can't parse integer value 'x'" in r.stderr, r.stderr
    # there is no -b here, and -perc stays unknown to the tools that have none
    r = _run(san_cli, ["-t", "kmers-samples-counter", "-k", "5", "-i", str(f), "-perc", "3", "-w", w("w9")], str(tmp_path))
    assert r.returncode == 1 and "Unrecognized option: -perc" in r.stderr, r.stderr
    # the tool is known by name
    assert "not found" not in _run(san_cli, ["-t", "kmers-per-sample", "-k", "5", "-i", str(f), "-w", w("w10")], str(tmp_path)).stderr
