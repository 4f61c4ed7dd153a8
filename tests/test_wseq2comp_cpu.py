"""seq2comp for k = 32 ... 63 without a GPU: the Python-integer reference (tests/wseq2comp_ref.py) against a literal and against the
k <= 31 yardstick (tests/seq2comp_ref.py), the conditions the GPU cases of tests/test_wseq2comp_gpu.py rely on -- asserted on the
reference alone --, and the driver on the host-only stub build (the recipe of tests/test_driver_tools_cpu.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import seq2comp_ref as N
import wide_files_ref as WF
import wseq2comp_cases as CASES
import wseq2comp_ref as R
from test_driver_tools_cpu import ENV, stub_driver


def test_literal_k33():
    """a 35-base sequence: window 0 is canonical as its reverse complement, windows 1 and 2 as they stand; A < G < C < T"""
    seq = "TCGATTGCAAGGCTTACCGATAGGCTAACGTTCAG"
    want = ["GAACGTTAGCCTATCGGTAAGCCTTGCAATCGA", "GATTGCAAGGCTTACCGATAGGCTAACGTTCAG", "CGATTGCAAGGCTTACCGATAGGCTAACGTTCA"]
    members, size, weight = R.component(seq, 33)
    assert [R.decode(x, 33) for x in members] == want and (size, weight) == (3, 3)
    assert members == sorted(members) and all(x >> 66 == 0 for x in members)
    assert members[0] >> 64 == 0b01 and members[2] >> 64 == 0b10                  # the first base is the high word's two bits at k = 33
    assert R.component(seq[:32], 33) == ([], 0, 0) and R.component(seq.lower(), 33)[0] == members
    data = R.components_bin([R.component(seq, 33), R.component("ACGT", 33)])
    assert data[:16] == struct.pack(">iiq", 2, 3, 3) and len(data) == 4 + 12 + 3 * 16 + 12 and data[-12:] == struct.pack(">iq", 0, 0)
    assert data[16:32] == struct.pack(">QQ", members[0] >> 64, members[0] & R.MASK64)
    sizes, weights, hi, lo = WF.decode_components(data)
    assert sizes.tolist() == [3, 0] and weights.tolist() == [3, 0] and [(int(h) << 64) | int(l) for h, l in zip(hi, lo)] == members
    assert R.stat_txt([R.component(seq, 33), R.component("ACGT", 33)]) == "# component.no\tcomponent.size\tcomponent.weight\n1\t3\t3\n2\t0\t0\n"


@pytest.mark.parametrize("k", [21, 31])
def test_equals_the_narrow_reference(k):
    """the restatement pinned to the yardstick that already stands, on the edge list"""
    seqs = [s for s in CASES.edges(32)[0]] + CASES.edges(63)[0][:4]
    wide, narrow = R.components(seqs, k), N.components(seqs, k)
    for w, n in zip(wide, narrow):
        assert w[0] == n[0].tolist() and w[1:] == n[1:]
    assert R.stat_txt(wide) == N.stat_txt(narrow)
    sample = {int(x): 1 + i % 9 for i, x in enumerate(np.unique(np.concatenate([c[0] for c in narrow]))[::3].tolist())}
    (v, b), (nv, nb) = R.features(wide, sample, 2), N.features(narrow, sample, 2)
    assert np.array_equal(v, nv) and np.array_equal(np.isnan(b), np.isnan(nb)) and np.array_equal(b[~np.isnan(b)], nb[~np.isnan(nb)])


@pytest.mark.parametrize("k", CASES.KS)
def test_what_the_edge_cases_hold(k):
    seqs, comps = CASES.edges(k)
    assert [c[1:] for c in comps[:6]] == [(0, 0), (0, 0), (1, 1), (2, 2), (1, 6), (1, 21)]      # empty components stay; the homopolymers
    assert comps[6][1] <= 6 and comps[6][2] == 500 - k + 1                                       # 3-periodic: three k-mers and their reverse complements
    assert comps[7][1] < comps[7][2] and comps[8] == comps[9] and comps[8][1] > 0                # s + rc(s) repeats; the same sequence twice
    assert comps[12][1] == 300 - k + 1 and comps[12] == R.component(seqs[12].upper(), k)
    pal = seqs[11]
    if k % 2 == 0:
        assert len(pal) == k and comps[11][1] == 1 and WF.revcomp(comps[11][0][0], k) == comps[11][0][0]
    else:
        assert len(pal) == k + 1 and comps[11][1] == 1 and comps[11][2] == 2                     # the two windows are each other's reverse complement
    top = max(x for c in comps for x in c[0])
    assert top >> (2 * k) == 0
    if k == 32:
        assert all(x >> 64 == 0 for c in comps for x in c[0])
    if k == 63:
        assert (top >> 64).bit_length() >= 61                                                    # the high word's 62 bits are in use


@pytest.mark.parametrize("k", CASES.KS)
def test_both_words_decide(k):
    seqs, comps, (a, g, pa, pg) = CASES.both_words(k)
    for c in comps:
        assert c[0] == sorted(c[0])
    assert {a, g} <= set(comps[0][0]) and {pa, pg} <= set(comps[1][0]) and {a, g, pa, pg} <= set(comps[2][0])
    assert a & R.MASK64 == g & R.MASK64 or k == 32
    assert pa >> 64 == pg >> 64 and pa & R.MASK64 != pg & R.MASK64 and pa ^ pg == 1                 # the last base: A 0, G 1
    if k >= 33:
        assert a >> 64 != g >> 64 and a & R.MASK64 == g & R.MASK64                                 # the first base lies in the high word


def test_what_the_class_borders_hold():
    T = CASES.lds_max_in_source()
    assert T >= 256 and T & (T - 1) == 0
    k, seqs, comps = CASES.borders(T)
    occ = [T // 4 - 1, T // 4, T // 4 + 1, T - 1, T, T + 1, 2 * T]
    assert [c[2] for c in comps[0:14:2]] == occ and [c[2] for c in comps[1:14:2]] == occ
    assert [c[1] for c in comps[0:14:2]] == occ                                 # random bases: every occurrence is a k-mer of its own
    assert all(c[1] == 50 for c in comps[1:14:2])                               # few distinct k-mers, many occurrences
    assert comps[14][2] == 20000 - k + 1 == comps[14][1]
    assert 10000 < sum(len(s) for s in seqs) < 100000


def test_what_many_short_holds():
    k, seqs, comps = CASES.many()
    T = CASES.lds_max_in_source()
    occ = [c[2] for c in comps]
    assert sum(1 for o in occ if o == 0) > 100 and sum(1 for o in occ if 0 < o <= T // 4) > 2000 and sum(1 for o in occ if o > T) == 3
    assert len(seqs) > 4 * 256 * 2                                              # more sequences than one round of teams on a small grid


def test_roundtrip_sequences_repeat_no_shorter_kmer():
    """comp2seq gives back ONE contig per sequence when no canonical (k - 1)-mer occurs twice in it (the seed is fixed)"""
    k, seqs, comps = CASES.roundtrip()
    for s, c in zip(seqs, comps):
        assert c[1] == c[2] == 200 - k + 1
        inner = R.occurrences(s, k - 1)
        assert len(set(inner)) == len(inner)


def test_sample_recipe():
    k, seqs, comps = CASES.roundtrip()
    sample = CASES.sample_of(comps, k, np.random.default_rng(5))
    members = {x for c in comps for x in c[0]}
    assert 0 < len(members & set(sample)) < len(members) and len(set(sample) - members) == 40
    hi, lo = R.words(sorted(sample))
    assert WF.first_bad_record(hi, lo, k) is None and len(R.kmers_bin(sample)) == 18 * len(sample)


# ---- the driver on the stub build ----
@pytest.fixture(scope="module")
def driver():
    return stub_driver()


def _run(driver, cwd, *args):
    return subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, env=ENV, timeout=120, cwd=str(cwd))


def test_driver_takes_wide_seq2comp(driver, tmp_path):
    (tmp_path / "s.fa").write_text(">a\n" + "ACGT" * 20 + "\n")
    # with the flag and k > 31 the run gets past check_k to the library: the stub has no such entry, and the run names it
    r = _run(driver, tmp_path, "-t", "seq2comp", "--wide-kmers", "-k", 33, "-i", "s.fa", "-w", "w1")
    assert r.returncode == 1 and "this build of the library has no mf_seq2comp_wide" in r.stderr + r.stdout, r.stderr
    assert not (tmp_path / "w1" / "SUCCESS").exists() and not (tmp_path / "w1" / "components.bin").exists()
    assert "wide-kmers" in (tmp_path / "w1" / "in.properties").read_text()
    # without the flag the reference's message, as ever
    r = _run(driver, tmp_path, "-t", "seq2comp", "-k", 32, "-i", "s.fa", "-w", "w2")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr + r.stdout
    r = _run(driver, tmp_path, "-t", "seq2comp", "--wide-kmers", "-k", 64, "-i", "s.fa", "-w", "w3")
    assert r.returncode == 1 and "The size of k-mer must be no more than 63." in r.stderr + r.stdout
    # k <= 31: the flag changes nothing, the narrow entry point is the one called
    r = _run(driver, tmp_path, "-t", "seq2comp", "--wide-kmers", "-k", 21, "-i", "s.fa", "-w", "w4")
    out = r.stderr + r.stdout
    assert r.returncode == 1 and "mf_seq2comp_wide" not in out and "no more than" not in out, out
    assert "wide-kmers" not in (tmp_path / "w4" / "in.properties").read_text()
    r = _run(driver, tmp_path, "-t", "seq2comp", "--wide-kmers", "-k", 33, "-i", "none.fa", "-w", "w5")
    assert r.returncode == 1 and "none.fa" in r.stderr + r.stdout
