"""The checker of the wide comp2seq (tests/wcomp2seq_ref.py) against the pinned one, and hand-worked literals at k = 33.

At k <= 31 the 128-bit oracle must give exactly what the 64-bit oracle gives through tests/comp2seq_ref.py: that ties the new checker to the
pinned text.  The literals at k = 33 are worked out by hand from the definitions (A0 G1 C2 T3; a path is printed from the end whose canonical
k-mer is the smaller one; a k-mer's weight is its multiplicity in the member list after canonicalisation)."""
import pytest

import comp2seq_ref as R
import wcomp2seq_ref as W

NARROW_CASES = {
    "adjacent_k21": lambda: R.case_adjacent(21),
    "adjacent_k31": lambda: R.case_adjacent(31),
    "shared_k21": lambda: R.case_shared(21),
    "shared_k31": lambda: R.case_shared(31),
    "shapes_k21": lambda: R.case_shapes(21),
    "shapes_k31": lambda: R.case_shapes(31),
    "palindromes_k20": R.case_palindromes,
}


@pytest.mark.parametrize("name", list(NARROW_CASES))
def test_the_wide_reference_is_the_narrow_one_where_both_exist(oracle, name):
    k, comps = NARROW_CASES[name]()
    narrow, wide = R.expected_split(oracle, comps, k), W.expected_split(oracle, comps, k)
    assert wide == narrow and sum(len(p) for p in narrow) > 0
    assert W.expected_union(oracle, comps, k) == R.expected_union(oracle, comps, k)


# a path of three 33-mers: the forward first k-mer starts with five A, nothing else in sight starts with more than three, and every reverse
# complement starts with G or C or T: the canonical k-mers are the forward ones, the first is the smallest, and the path is printed as written
PATH35 = "AAAAAC" + "GTCAGGCTATTCGACCTGAATGCCTTAGC"
assert len(PATH35) == 35


def test_one_path_of_three_kmers_as_one_component_and_as_three(oracle):
    k = 33
    km = R.kmers_of(PATH35, k)
    assert km == [R.encode(PATH35[i:i + k]) for i in range(3)] and km == sorted(km)        # forward = canonical, ascending
    assert W.expected_split(oracle, [km], k) == [[(PATH35, 1, 1, 1)]]
    three = W.expected_split(oracle, [[x] for x in km], k)
    assert three == [[(PATH35[i:i + k], 1, 1, 1)] for i in range(3)]
    assert all(len(s[0][0]) == 33 and s[0][1] == 1 for s in three)
    # all together the three components are the one path again
    assert W.expected_union(oracle, [[x] for x in km], k) == [(PATH35, 1, 1, 1)]
    files = W.expected_files(oracle, [km], k, split=True)
    assert files["seq-builder-many/sequences/component_1.seq.fasta"] == (
        b">1 length=35 av_weight=1 min_weight=1 max_weight=1\nAAAAACGTCAGGCTATTCGACCTGAATGCCTTAGC\n")
    assert files["kmers_fasta/component_1.fasta"] == "".join(f">{j + 1}\n{PATH35[j:j + k]}\n" for j in range(3)).encode()
    assert files["kmer-counter-many/stats/component_1.stat.txt"] == b"# k-mer frequency\tnumber of such k-mers\n1\t3\n\n"


def test_a_component_that_lists_a_kmer_and_its_reverse_complement(oracle):
    k = 33
    x = R.encode("A" * 32 + "C")                     # = 2: high word 0, low word 2
    rx = R.encode("G" + "T" * 32)                    # its reverse complement: G = 1 in bits 64-65, 32 x T = a low word of ones
    assert x == 2 and rx == (1 << 64) | ((1 << 64) - 1) and R.canon(rx, k) == x
    comps = [[x, rx]]                                # ascending, as the loader asks; not canonical, which it does not ask
    assert R.component_tables(comps, k) == [{2: 2}]
    files = W.expected_files(oracle, comps, k, split=True)
    assert files["kmer-counter-many/kmers/component_1.kmers.bin"] == bytes(8) + bytes(7) + b"\x02" + b"\x00\x02"
    assert files["kmer-counter-many/stats/component_1.stat.txt"] == b"# k-mer frequency\tnumber of such k-mers\n2\t1\n\n"
    assert files["seq-builder-many/sequences/component_1.seq.fasta"] == (
        b">1 length=33 av_weight=2 min_weight=2 max_weight=2\n" + b"A" * 32 + b"C\n")
    assert files["kmers_fasta/component_1.fasta"] == b">1\n" + b"A" * 32 + b"C\n>2\nG" + b"T" * 32 + b"\n"
    # the file itself: 1 component of 2 members, weight 2, four big-endian words
    assert W.components_bytes(comps) == (b"\x00\x00\x00\x01" + b"\x00\x00\x00\x02" + bytes(7) + b"\x02" + bytes(8) + bytes(7) + b"\x02"
                                         + bytes(7) + b"\x01" + b"\xff" * 8)
