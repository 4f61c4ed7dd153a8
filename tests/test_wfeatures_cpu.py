"""features-calculator for k = 32 ... 63 without a GPU: the Python-int reference (tests/wfeatures_ref.py) pinned by hand-worked literals and
compared with the oracle compiled for 128-bit keys (orw_features_reads_selected, orw_features_selected) on components the oracle cuts
itself; the driver's argument checks on the host-only stub build (the recipe of tests/test_driver_tools_cpu.py)."""
import math
import subprocess

import numpy as np
import pytest

import wfeatures_ref as R
from test_driver_tools_cpu import ENV, stub_driver
from util import genome_reads

K = 33
# A0 G1 C2 T3: A^33 = 0; A^32 C = 2 (its reverse complement G T^32 starts with G: larger); A^32 G = 1; A^31 CC = 10
X0, X1, X2, X3 = 0, 2, 1, 10
COMPS = [[X0, X1], [X2, X1], [X2], [X3]]                        # X1 is listed by two components
READS = ["A" * 34,                                                # X0 at both positions
         "A" * 32 + "C",                                          # X1
         "G" + "T" * 32,                                          # the reverse complement of A^32 C: credits X1
         "A" * 32,                                                # k - 1 bases: nothing
         "a" * 32 + "g"]                                          # lower case: X2


def test_the_k_mers_of_the_literals():
    assert [R.encode("A" * 33), R.encode("A" * 32 + "C"), R.encode("A" * 32 + "G"), R.encode("A" * 31 + "CC")] == [X0, X1, X2, X3]
    assert R.canonical_kmers(READS[0], K) == [X0, X0] and R.canonical_kmers(READS[1], K) == [X1] == R.canonical_kmers(READS[2], K)
    assert R.canonical_kmers(READS[3], K) == [] and R.canonical_kmers(READS[4], K) == [X2]
    assert R.encode("G" + "T" * 32) == (1 << 64) | (R.MASK64) and R.revcomp_str("A" * 32 + "C") == "G" + "T" * 32
    assert R.presence(COMPS, READS, K) == {X0: 2, X1: 2, X2: 1, X3: 0}


def _is(got, vec, br):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64
    assert got[0].tolist() == vec
    assert [("nan" if math.isnan(b) else b) for b in got[1].tolist()] == br


def test_reads_branch_by_hand():
    # threshold 0: the shared X1 counts in both components; X3 never occurs
    _is(R.from_reads(COMPS, READS, K, 0), [4, 3, 1, 0], [1.0, 1.0, 1.0, 0.0])
    # threshold 1: X2 (value 1) is no longer above it
    _is(R.from_reads(COMPS, READS, K, 1), [4, 2, 0, 0], [1.0, 0.5, 0.0, 0.0])
    # threshold -1: the absent X3 (value 0) counts as found and adds nothing
    _is(R.from_reads(COMPS, READS, K, -1), [4, 3, 1, 0], [1.0, 1.0, 1.0, 1.0])
    # no reads: all zero, breadth 0 / size
    _is(R.from_reads(COMPS, [], K, 0), [0, 0, 0, 0], [0.0, 0.0, 0.0, 0.0])
    # an empty component: NaN
    _is(R.from_reads(COMPS + [[]], READS, K, 0), [4, 3, 1, 0, 0], [1.0, 1.0, 1.0, 0.0, "nan"])


def test_selected_by_hand():
    sel = {X1: 5, X3: 0, 999: 1}                                # X3 with value 0 is NOT selected; 999 is in no component
    # only the X1 listings take part; components 2 and 3 list nothing selected: 0.0 / 0.0
    _is(R.from_reads(COMPS, READS, K, 0, sel), [2, 2, 0, 0], [1.0, 1.0, "nan", "nan"])
    _is(R.from_reads(COMPS, READS, K, 2, sel), [0, 0, 0, 0], [0.0, 0.0, "nan", "nan"])
    _is(R.from_reads(COMPS, READS, K, -1, {X3: 1}), [0, 0, 0, 0], ["nan", "nan", "nan", 1.0])
    _is(R.from_reads(COMPS, READS, K, 0, {}), [0, 0, 0, 0], ["nan"] * 4)


def test_kmers_branch_by_hand():
    sample = {X0: 7, X1: 32767, X2: 1, 12345: 9}
    _is(R.from_kmers(COMPS, sample, 0), [32774, 32768, 1, 0], [1.0, 1.0, 1.0, 0.0])
    _is(R.from_kmers(COMPS, sample, 1), [32774, 32767, 0, 0], [1.0, 0.5, 0.0, 0.0])
    _is(R.from_kmers(COMPS, sample, 7, {X0: 1, X2: 3}), [0, 0, 0, 0], [0.0, 0.0, 0.0, "nan"])
    _is(R.from_kmers(COMPS, sample, 6, {X0: 1, X2: 3}), [7, 0, 0, 0], [1.0, 0.0, 0.0, "nan"])


def test_counts_do_not_saturate_in_the_reads_branch():
    reads = ["A" * 34] * 20000                                   # X0 40 000 times
    assert R.from_reads([[X0]], reads, K)[0].tolist() == [40000]
    assert R.count(reads, K) == {X0: 32767} and R.from_kmers([[X0]], R.count(reads, K))[0].tolist() == [32767]


def test_the_files_text():
    assert R.vec_text([4, 0, 40000]) == "4\n0\n40000\n"
    assert R.breadth_text([1.0, 0.5, 0.0, math.nan, 1 / 3, 2 / 300, 1 / 1024, 1 / 3000]) == \
        "1.0\n0.5\n0.0\nNaN\n0.3333333333333333\n0.006666666666666667\n9.765625E-4\n3.333333333333333E-4\n"


# ---- against the oracle on components it cuts itself ----
def _oracle_case(oracle, k, seed):
    rng = np.random.default_rng(seed)
    bases, off = genome_reads(rng, 1200, 120, 90, err=0.004)
    lower = bases.copy()
    lower[: int(off[40])] |= 0x20                               # the first 40 reads in lower case
    table = oracle.WTable().count_buffer(bases, off, k, 0)
    comps = oracle.wide_cut_components(table.good(1), k, 5, 300)
    assert len(comps) >= 2
    members = [oracle.w128_to_ints(km) for _, _, _, km in comps.all()]
    reads = [bytes(lower[int(off[i]):int(off[i + 1])]).decode() for i in range(len(off) - 1)]
    return bases, lower, off, table, comps, members, reads


def _orw_reads(oracle, comps, bases, off, k, thr, selected):
    n = len(comps)
    vec = np.zeros(n, dtype=np.int64); br = np.zeros(n, dtype=np.float64)
    b = np.ascontiguousarray(bases, dtype=np.uint8); o = np.ascontiguousarray(off, dtype=np.uint64)
    rc = oracle.lib().orw_features_reads_selected(comps.h, b.ctypes.data, o.ctypes.data, len(o) - 1, k, thr, selected.h if selected is not None else None,
                                                  vec.ctypes.data, br.ctypes.data)
    assert rc == 0, oracle.lib().orw_last_error()
    return vec, br


def _same(got, exp):
    assert np.array_equal(got[0], exp[0])
    assert np.array_equal(np.isnan(got[1]), np.isnan(exp[1]))
    assert got[1][~np.isnan(got[1])].tobytes() == exp[1][~np.isnan(exp[1])].tobytes()


@pytest.mark.parametrize("k", [33, 63])
def test_against_the_oracle(oracle, k):
    bases, lower, off, table, comps, members, reads = _oracle_case(oracle, k, 100 + k)
    flat = [x for m in members for x in m]
    sel_py = {x: 1 + i % 3 for i, x in enumerate(flat[::3])}
    sel_py.update({x: 0 for x in flat[1::9] if x not in sel_py})              # present with value 0: not selected
    sel_py[(1 << (2 * k)) - 5] = 4                                              # outside every component
    sel = oracle.WTable()
    for x, v in sel_py.items():
        if v:
            sel.add(x, v)
    keys, vals = table.export()
    sample = dict(zip(oracle.w128_to_ints(keys), vals.tolist()))
    for thr in (-1, 0, 1, 3):
        for s_or, s_py in ((None, None), (sel, sel_py)):
            exp = _orw_reads(oracle, comps, bases, off, k, thr, s_or)           # (the oracle takes upper case only)
            _same(R.from_reads(members, reads, k, thr, s_py), exp)
            _same(R.from_kmers(members, sample, thr, s_py), comps.features(table, thr, s_or))
        assert exp[0].sum() > 0 or thr == 3
    # a selection that leaves a whole component out gives NaN there, in both
    only = oracle.WTable(); only.add(members[0][0], 1)
    exp = _orw_reads(oracle, comps, bases, off, k, 0, only)
    _same(R.from_reads(members, reads, k, 0, {members[0][0]: 1}), exp)
    assert np.isnan(exp[1][1:]).all() and not np.isnan(exp[1][0])


# ---- the driver on the stub build ----
@pytest.fixture(scope="module")
def driver():
    return stub_driver()


def _run(driver, cwd, *args):
    return subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, env=ENV, timeout=120, cwd=str(cwd))


def test_driver_argument_checks(driver, tmp_path):
    (tmp_path / "a.fa").write_text(">a\n" + "ACGT" * 20 + "\n")
    (tmp_path / "c.bin").write_bytes(b"\0\0\0\0")
    common = ["-t", "features-calculator", "-cm", "c.bin", "-i", "a.fa", "--selected", "c.bin"]
    # without the flag k = 40 is the reference's error, before any library call
    r = _run(driver, tmp_path, *common, "-k", 40, "-w", "w1")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr + r.stdout
    assert not (tmp_path / "w1" / "vectors").exists()
    r = _run(driver, tmp_path, "--wide-kmers", *common, "-k", 64, "-w", "w2")
    assert r.returncode == 1 and "The size of k-mer must be no more than 63." in r.stderr + r.stdout
    # with the flag the options are no longer refused: the run goes on to the library, which the stub build does not have
    r = _run(driver, tmp_path, "--wide-kmers", *common, "-k", 40, "-w", "w3")
    out = r.stderr + r.stdout
    assert r.returncode == 1 and "is not supported with --wide-kmers" not in out and "this build of the library has no" in out, out
