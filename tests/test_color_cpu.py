"""kmers-color / component-colored without a GPU: the restatement (tests/color_ref.py) on hand-worked cases, the driver's option handling
in the sanitizer build (tests/host/mf_stub.cpp has no GPU and none of the new entry points), header and exported symbols."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import color_ref as CR
import stats_ref as R
from conftest import ROOT
from metafast_amd import lib as L

NEW_ENTRIES = ["mf_ctable_from_host", "mf_ctable_load", "mf_ctable_stats", "mf_ctable_export", "mf_ctable_write", "mf_ctable_destroy",
               "mf_kmers_color_tables", "mf_kmers_color", "mf_colored_components_device", "mf_colored_components"]


# ---- the packed value ----
def test_fields_and_saturation():
    assert CR.pack(1, 2, 3) == 1 + (2 << 20) + (3 << 40)
    v = CR.add_value(CR.add_value(0, 1), 1)
    assert v == 2 << 20 and CR.get_value(v, 1) == 2 and CR.get_value(v, 0) == 0
    # exactly 2^20 - 1 and no further, and the neighbours untouched
    top = (1 << 20) - 1
    v = CR.pack(7, top - 1, 9)
    assert CR.add_value(v, 1) == CR.pack(7, top, 9) and CR.add_value(CR.add_value(v, 1), 1) == CR.pack(7, top, 9)
    assert CR.add_value(CR.pack(0, 0, top - 5), 2, 32767) == CR.pack(0, 0, top)
    # counts: a key in 5 samples of class 2; -val: 32 x 32767 = 1048544 < 2^20 - 1 = 1048575 <= 33 x 32767
    one = (np.array([5], np.uint64), np.array([32767], np.int16))
    assert CR.kmers_color([one] * 5, [2] * 5)[1].tolist() == [5 << 40]
    assert CR.kmers_color([one] * 32, [0] * 32, val=True)[1].tolist() == [1048544]
    assert CR.kmers_color([one] * 33, [0] * 33, val=True)[1].tolist() == [top]
    assert CR.kmers_color([one] * 40, [1] * 40, val=True)[1].tolist() == [top << 20]


def test_kmers_color_loading_rules():
    # key 7 twice in one file: the records > b are summed first (1 + 1 -> absent at b = 1, 2 + 3 = 5 at b = 1), one add per sample
    f1 = (np.array([7, 7, 3], np.uint64), np.array([1, 1, 2], np.int16))
    f2 = (np.array([7, 7, 9], np.uint64), np.array([2, 3, 1], np.int16))
    k, v = CR.kmers_color([f1, f2], [0, 2], b=1)
    assert k.tolist() == [3, 7] and v.tolist() == [1, 1 << 40]
    k, v = CR.kmers_color([f1, f2], [0, 2], b=1, val=True)
    assert v.tolist() == [2, 5 << 40]
    k, v = CR.kmers_color([f1, f2], [0, 2], b=0, val=True)
    assert k.tolist() == [3, 7, 9] and v.tolist() == [2, 2 + (5 << 40), 1 << 40]
    assert CR.stat_txt(v) == "# k-mer frequency\tnumber of such k-mers\n2\t1\n%d\t1\n%d\t1\n\n" % (1 << 40, 2 + (5 << 40))
    assert CR.ctable_to_bytes(k[:1], v[:1]) == bytes(7) + b"\x03" + bytes(7) + b"\x02"
    for bad in ([3], [-1]):
        with pytest.raises(ValueError):
            CR.kmers_color([f1], bad)
    with pytest.raises(ValueError):
        CR.kmers_color([f1] * 1025, [0] * 1025)
    with pytest.raises(ValueError):
        CR.kmers_color([(np.array([1 << 62], np.uint64), np.array([5], np.int16))], [0])


def test_get_color_boundaries():
    assert CR.get_color(CR.pack(9, 1, 0), 0.9) == 0                 # 9 of 10 at 0.9: 0.9 >= 0.9
    assert CR.get_color(CR.pack(8, 2, 0), 0.9) == -1
    assert CR.get_color(CR.pack(1, 9, 0), 0.9) == 1 and CR.get_color(CR.pack(0, 1, 9), 0.9) == 2
    assert CR.get_color(CR.pack(1, 1, 0), 0.5) == 0                 # a tie goes to the first colour
    assert CR.get_color(CR.pack(0, 1, 1), 0.5) == 1
    assert CR.get_color(CR.pack(1, 1, 1), 0.9) == -1
    assert CR.get_color(CR.pack(0, 0, 5), 0.0) == 0                 # perc = 0: 0 / 5 >= 0
    assert CR.get_color(1 << 60, 0.9) == -1 and CR.get_color(1 << 60, 0.0) == -1      # no field set: 0 / 0 = NaN, neutral


def test_threshold_is_k():
    keys = np.array([10, 11, 12, 13], np.uint64)
    vals = np.array([31, 32, 1 << 20, -5], np.int64)
    hm = CR.load_long([(keys, vals)], 31)
    assert sorted(hm) == [11, 12] and hm[12] == 1 << 20             # 31 is dropped at k = 31, 32 and 2^20 (one sample of class 1) are kept
    assert sorted(CR.load_long([(keys, vals)], 0)) == [10, 11, 12]  # the sign bit never passes
    # duplicates across files: added as integers, saturating at 2^63 - 1; the cut is made per record
    hm = CR.load_long([(keys[:2], vals[:2]), (keys[:2], np.array([40, CR.LONG_MAX], np.int64))], 31)
    assert hm == {10: 40, 11: CR.LONG_MAX}


# a path of six 5-mers: consecutive windows of a sequence whose k-mers are all different, also from their reverse complements
PATH_SEQ = "AAGACTCGTA"
PATH_K = 5


def path_table():
    """c0 - n - c1 - n - c0 - n along PATH_SEQ -> (kmers in path order, dict key -> packed value)"""
    km = [CR.canon(CR.encode(PATH_SEQ[i:i + PATH_K]), PATH_K) for i in range(6)]
    assert len(set(km)) == 6
    vals = [CR.pack(10, 0, 0), CR.pack(5, 5, 0), CR.pack(0, 10, 0), CR.pack(3, 3, 3), CR.pack(10, 0, 0), CR.pack(0, 5, 5)]
    # the path and nothing else: neighbours inside the set are exactly the path's edges
    s = set(km)
    for i, x in enumerate(km):
        nb = {u for u in CR.neighbours(x, PATH_K) if u in s and u != x}
        assert nb == {km[j] for j in (i - 1, i + 1) if 0 <= j < 6}, i
    return km, dict(zip(km, vals))


def test_six_vertex_path_both_modes():
    km, hm = path_table()
    assert [CR.get_color(hm[x], 0.9) for x in km] == [0, -1, 1, -1, 0, -1]
    d = CR.colored_components(hm, PATH_K, 3, False, 0.9)
    # colour 0 without the colour-1 vertex: {c0, n} and {n, c0, n}; colour 1: {n, c1, n}; colour 2: nothing; no neutral-only component
    assert d[0] == [sorted(km[3:6]), sorted(km[0:2])] and d[1] == [sorted(km[1:4])] and d[2] == []
    assert km[1] in d[0][1] and km[1] in d[1][0] and km[3] in d[0][0] and km[3] in d[1][0]        # neutral k-mers shared between colours
    s = CR.colored_components(hm, PATH_K, 3, True, 0.9)
    assert s[0] == sorted([[km[0]], [km[4]]]) and s[1] == [[km[2]]] and s[2] == []
    assert CR.components_bytes(s[1]) == b"\x00\x00\x00\x01" + b"\x00\x00\x00\x01" + bytes(7) + b"\x01" + int(km[2]).to_bytes(8, "big")
    assert CR.components_stat(s) == CR.STAT_HEADER + "1\t1\t1\t0\n2\t1\t1\t0\n3\t1\t1\t1\n"
    with pytest.raises(ValueError):
        CR.colored_components(hm, PATH_K, 1, True, 0.9)             # a colour-1 k-mer with n_groups = 1


# ---- header and exported symbols ----
def test_header_and_library_agree_on_the_new_entry_points():
    hdr = open(L.HEADER_PATH).read()
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", hdr))
    so = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert hasattr(so, name), name
        assert name in L.exported_symbols(), name
    assert "typedef struct mf_ctable mf_ctable;" in hdr


# ---- the driver in the sanitizer build (the recipe of tests/test_stats_cpu.py) ----
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


def test_driver_lists_and_parses_the_colour_tools(san_cli, tmp_path):
    r = _run(san_cli, ["-ts"], str(tmp_path))
    assert r.returncode == 0 and "kmers-color" in r.stdout and "component-colored" in r.stdout
    f = tmp_path / "a.kmers.bin"
    g = tmp_path / "b.kmers.bin"
    for p in (f, g):
        p.write_bytes(R.records_to_bytes(np.array([1, 2], np.uint64), np.array([3, 4])))
    cls = tmp_path / "classes.txt"
    cls.write_text("a\t0\nb\t2\n")
    r = _run(san_cli, ["-t", "kmers-color", "-k", "31", "-kf", str(f), str(g), "--class", str(cls), "-b", "2", "-val", "-w", str(tmp_path / "w1")], str(tmp_path))
    assert r.returncode == 1 and "mf_kmers_color" in r.stderr, r.stderr
    props = (tmp_path / "w1" / "in.properties").read_text()
    assert "maximal-bad-frequency = 2" in props and "val = true" in props and "a.kmers.bin" in props and "classes.txt" in props
    assert "colored-kmers" in props                                  # the default output directory
    # bad class files: a class outside 0 .. 2, a sample without a line, a line without a class
    for i, (text, want) in enumerate([("a\t0\nb\t3\n", "class 3"), ("a\t0\n", "'b'"), ("a\t0\nb\n", "line 2")]):
        cls.write_text(text)
        r = _run(san_cli, ["-t", "kmers-color", "-k", "31", "-kf", str(f), str(g), "--class", str(cls), "-w", str(tmp_path / ("wb%d" % i))], str(tmp_path))
        assert r.returncode == 1 and want in r.stderr and "classes.txt" in r.stderr and "mf_kmers_color" not in r.stderr, (want, r.stderr)
    assert "Mandatory argument --class" in _run(san_cli, ["-t", "kmers-color", "-k", "31", "-kf", str(f), "-w", str(tmp_path / "w2")], str(tmp_path)).stderr

    c = tmp_path / "colored_kmers.kmers.bin"
    c.write_bytes(CR.ctable_to_bytes(np.array([1, 2], np.uint64), np.array([40, 50], np.uint64)))
    r = _run(san_cli, ["-t", "component-colored", "-k", "21", "-i", str(c), "-group", "2", "--separate", "--perc", "0.75", "-w", str(tmp_path / "w3")], str(tmp_path))
    assert r.returncode == 1 and "mf_colored_components" in r.stderr, r.stderr
    props = (tmp_path / "w3" / "in.properties").read_text()
    assert "n_groups = 2" in props and "separate = true" in props and "perc = 0.75" in props and "n_comps = -1" in props and "linear = false" in props
    assert "colored-components" in props
    r = _run(san_cli, ["-t", "component-colored", "-k", "21", "-i", str(c), "--linear", "-w", str(tmp_path / "w4")], str(tmp_path))
    assert r.returncode == 1 and "--linear" in r.stderr and "iteration order" in r.stderr and "mf_colored_components" not in r.stderr
    r = _run(san_cli, ["-t", "component-colored", "-k", "21", "-i", str(c), "--n_comps", "5", "-w", str(tmp_path / "w5")], str(tmp_path))
    assert r.returncode == 1 and "--n_comps" in r.stderr and "iteration order" in r.stderr and "mf_colored_components" not in r.stderr
    r = _run(san_cli, ["-t", "component-colored", "-k", "21", "-i", str(c), "-comp", "-1", "-w", str(tmp_path / "w6")], str(tmp_path))
    assert r.returncode == 1 and "mf_colored_components" in r.stderr          # -1 = all components: accepted
    assert "Mandatory argument --k-mers" in _run(san_cli, ["-t", "component-colored", "-k", "21", "-w", str(tmp_path / "w7")], str(tmp_path)).stderr
