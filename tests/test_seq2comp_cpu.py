"""tests/seq2comp_ref.py, the restatement of SequencesToComponents.java / ComponentFromSequence.java that the GPU tests compare with:
hand-written answers, the committed fixture (tests/golden/seq2comp: a FASTA and the components.bin / components-stat.txt the
restatement gave for it at k = 21 -- the bytes and the restatement pin each other), and the two declarations in the header."""
import math
import os
import re
import struct

import numpy as np

import seq2comp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "seq2comp")


def test_k3_on_ACGTACGT_collapses_reverse_complements():
    # ACG CGT GTA TAC ACG CGT: rc(ACG) = CGT, rc(GTA) = TAC -> two canonical k-mers, ACG (A0 C2 G1 = 9) and GTA (G1 T3 A0 = 28)
    members, size, weight = R.component("ACGTACGT", 3)
    assert members.tolist() == [R.encode("ACG"), R.encode("GTA")] == [9, 28]
    assert (size, weight) == (2, 6)
    assert R.occurrences("ACGTACGT", 3).tolist() == [9, 9, 28, 28, 9, 9]


def test_homopolymers():
    for k in (1, 5, 21, 31):
        members, size, weight = R.component("A" * (k + 5), k)
        assert members.tolist() == [0] and (size, weight) == (1, 6)
        members, size, weight = R.component("T" * (k + 5), k)          # rc(T..T) = A..A
        assert members.tolist() == [0] and (size, weight) == (1, 6)


def test_shorter_than_k_is_an_empty_component():
    for k in (2, 5, 31):
        members, size, weight = R.component("ACGTACGTACGTACGTACGTACGTACGTACGT"[:k - 1], k)
        assert len(members) == 0 and (size, weight) == (0, 0)
    assert R.component("", 5)[1:] == (0, 0)
    assert R.component("ACGTA", 5)[1:] == (1, 1)


def test_even_k_palindrome():
    # ACGT is its own reverse complement: one member, A0 C2 G1 T3 = 0b00100111
    assert R.rc_str("ACGT") == "ACGT"
    members, size, weight = R.component("ACGT", 4)
    assert members.tolist() == [0b00100111] and (size, weight) == (1, 1)
    # AACGTT (k = 6) inside a longer sequence: the palindrome counts once, its neighbours AAACGT / ACGTTT are each other's reverse complement
    members, size, weight = R.component("AAACGTTT", 6)
    assert (size, weight) == (2, 3)
    assert members.tolist() == sorted([R.encode("AAACGT"), R.encode("AACGTT")])


def test_first_base_is_most_significant_and_lower_case_reads_the_same():
    assert R.occurrences("GATTACA", 7).tolist() == [min(R.encode("GATTACA"), R.encode(R.rc_str("GATTACA")))]
    assert R.encode("GATTACA") == int("01" "00" "11" "11" "00" "10" "00", 2)
    assert R.occurrences("gattaca", 4).tolist() == R.occurrences("GATTACA", 4).tolist()


def test_k31_uses_62_bits():
    s = "T" * 15 + "G" + "T" * 15
    (x,) = R.occurrences(s, 31).tolist()
    assert x == min(R.encode(s), R.encode(R.rc_str(s))) and x < 1 << 62


def test_fixture():
    seqs = R.read_fasta(os.path.join(GOLD, "catalogue.fa"))
    names = [ln[1:].strip() for ln in open(os.path.join(GOLD, "catalogue.fa")) if ln.startswith(">")]
    assert len(names) == 13 and len(seqs) == 12 and "with_N" in names          # the record with an N is not there
    assert all(set(s) <= set("ACGT") for s in seqs)
    comps = R.components(seqs, 21)
    blob = open(os.path.join(GOLD, "catalogue.k21.components.bin"), "rb").read()
    assert R.components_bin(comps) == blob
    assert R.stat_txt(comps) == open(os.path.join(GOLD, "catalogue.k21.components-stat.txt")).read()
    # the bytes, read back by hand: count, then (size, weight, members) with ascending members below 2^42
    (n,) = struct.unpack(">I", blob[:4])
    assert n == 12
    at, sizes, weights = 4, [], []
    for _ in range(n):
        size, weight = struct.unpack(">Iq", blob[at:at + 12])
        km = np.frombuffer(blob, dtype=">u8", count=size, offset=at + 12)
        assert (np.diff(km.astype(np.uint64).astype(np.int64)) > 0).all() and (km < 1 << 42).all()
        at += 12 + 8 * size
        sizes.append(size)
        weights.append(weight)
    assert at == len(blob)
    assert weights == [max(0, len(s) - 20) for s in seqs]
    assert sizes[1] == 0 and weights[1] == 0 and len(seqs[1]) == 10            # shorter than k: kept, empty
    assert sizes[3] == 1 and weights[3] == 20                                  # poly-A
    assert sizes[5] == 3 and weights[5] == 70                                  # (ACG)30: three k-mers
    assert sizes[6] == sizes[7] and (comps[6][0] == comps[7][0]).all()         # the same record twice: two equal components
    assert sizes[8] * 2 == weights[8]                                          # a sequence + its reverse complement: every k-mer twice
    # a shared stretch of 70 bases, 71 as the base in front of it happens to agree: 71 - 20 shared k-mers
    assert seqs[4][29:100] == seqs[0][39:110] and seqs[4][100] != seqs[0][110] and seqs[4][28] != seqs[0][38]
    assert len(set(comps[0][0].tolist()) & set(comps[4][0].tolist())) == 51


def test_features_count_a_shared_kmer_in_every_component_that_lists_it():
    comps = R.components(["ACGTTGCAAC", "TTGCAACGGA", "ACG", "ACGTTGCAAC"], 5)
    shared = set(comps[0][0].tolist()) & set(comps[1][0].tolist())
    assert shared
    sample = {x: 3 for x in shared}
    sample[min(set(comps[1][0].tolist()) - shared)] = 1
    vec, br = R.features(comps, sample)
    assert vec[0] == vec[3] == 3 * len(shared) and vec[1] == vec[0] + 1 and vec[2] == 0
    assert br[0] == len(shared) / comps[0][1] and math.isnan(br[2])
    assert R.vec_txt(vec).splitlines()[2] == "0"


def test_header_declares_the_two_calls():
    from metafast_amd import lib as L
    text = open(L.HEADER_PATH).read()
    assert re.search(r"\bint\s+mf_comps_from_sequences_device\(mf_ctx \*ctx, const void \*d_bases, const void \*d_offsets, uint64_t n_seqs, uint64_t n_bases, int k,\s*mf_comps \*\*out\);", text)
    assert re.search(r"\bint\s+mf_seq2comp\(mf_ctx \*ctx, const char \*const \*files, int nfiles, int k, const char \*components_bin, const char \*stat_txt,\s*uint64_t \*n_components, uint64_t \*per_file\);", text)
    assert {"mf_comps_from_sequences_device", "mf_seq2comp"} <= set(L.exported_symbols())
