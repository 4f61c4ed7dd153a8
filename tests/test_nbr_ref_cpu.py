"""Pins tests/nbr_ref.py -- the numpy reference that tests/test_nbr_gpu.py holds the neighbour lookup of mf_nbr.h against -- without a GPU:
hand-worked neighbour lists, the strand symmetry of the partition hash, the minimizers low_mmers promises, and a brute-force lookup
through strings and a dict."""
import numpy as np
import pytest

import nbr_ref as R

N = R.NONE


def _table(words):
    k = len(words[0])
    keys = np.array([R.encode(w) for w in words], dtype=np.uint64)
    assert np.array_equal(keys, R.canonical(keys, k)), "the hand-made tables hold canonical k-mers"
    return keys, k


def test_hand_worked_neighbours_k5():
    """worked on paper.  Slot 2 nuc: nuc appended on the right, slot 2 nuc + 1: nuc prepended on the left (nuc A C G T = 0 1 2 3);
    table positions, not ranks: the table is not in ascending order.
    AAAAA: right AAAAA (itself), AAAAC, AAAAG, AAAAT (absent); left AAAAA (itself), CAAAA, GAAAA / TAAAA (absent).
    AAACG: left A = AAAAC; left T = TAAAC, whose canonical form is GTTTA: held as the reverse complement.
    GTTTA: left C = CGTTT = rc(AAACG): held as the reverse complement."""
    keys, k = _table(["AAAAC", "AAAAA", "AAACG", "AAAAG", "CAAAA", "GTTTA"])
    want = np.array([[N, 1, N, 4, 2, N, N, N],
                     [1, 1, 0, 4, 3, N, N, N],
                     [N, 0, N, N, N, N, N, 5],
                     [N, 1, N, 4, N, N, N, N],
                     [1, N, 0, N, 3, N, N, N],
                     [N, N, N, 2, N, N, N, N]], dtype=np.uint32)
    got, rc = R.neighbours(keys, k, with_strand=True)
    assert np.array_equal(got, want)
    assert got[1, 0] == 1 and got[1, 1] == 1                  # the self loop of poly-A, on both sides
    assert rc[2, 7] and rc[5, 3] and not rc[2, 1] and not rc[0, 4] and not rc[1, 0]
    assert np.array_equal(R.neighbours(keys, k), want)


def test_hand_worked_neighbours_k6_palindromes():
    """ACGCGT, ATATAT and TATATA are their own reverse complements.  AACGCG: right T = ACGCGT, a palindrome: it counts as itself (forward).
    ACGCGT: left A = AACGCG (forward), right T = CGCGTT = rc(AACGCG) (reverse): one vertex in two slots; left C = CACGCG (forward), right G =
    CGCGTG = rc(CACGCG) (reverse).  ATATAT: right A = TATATA and left T = TATATA; TATATA: left A = ATATAT and right T = ATATAT."""
    keys, k = _table(["AACGCG", "ACGCGT", "CACGCG", "AAAAAA", "ATATAT", "TATATA"])
    want = np.array([[N, N, N, N, N, N, 1, N],
                     [N, 0, N, 2, 2, N, 0, N],
                     [N, N, N, N, N, N, 1, N],
                     [3, 3, N, N, N, N, N, N],
                     [5, N, N, N, N, N, N, 5],
                     [N, 4, N, N, N, N, 4, N]], dtype=np.uint32)
    got, rc = R.neighbours(keys, k, with_strand=True)
    assert np.array_equal(got, want)
    assert not rc[0, 6] and not rc[2, 6] and not rc[4, 0] and not rc[4, 7] and not rc[5, 1]      # palindromic neighbours: themselves
    assert rc[1, 6] and rc[1, 4] and not rc[1, 1] and not rc[1, 3]


def test_revcomp_and_codes():
    assert R.encode("ACGT") == 0b00011011 and R.decode(0b00011011, 4) == "ACGT"
    assert R.decode(R.revcomp(R.encode("AACGCG"), 6), 6) == "CGCGTT"
    assert int(R.revcomp(R.encode("ACGCGT"), 6)) == R.encode("ACGCGT")
    assert int(R.canonical(R.encode("TAAAC"), 5)) == R.encode("GTTTA")
    rng = np.random.default_rng(1)
    for k in range(1, 32):                                    # the word-wide form against the base-by-base one
        x = rng.integers(0, 1 << (2 * k), size=300, dtype=np.uint64)
        assert np.array_equal(R.revcomp(x, k), R.revcomp_plain(x, k)) and np.array_equal(R.revcomp(R.revcomp(x, k), k), x)
        assert int(R.revcomp(np.uint64(x[0]), k)) == int(R.revcomp_plain(x[0], k))
    assert R.decode(R.revcomp_plain(R.encode("AACGCG"), 6), 6) == "CGCGTT"


def test_mmer_hash_literals():
    """(canon ^ seed) * 0x9E3779B1 mod 2^32, by hand: the seed itself hashes to 0, seed ^ 1 to the multiplier"""
    for M, seed in ((13, 0x00B9107F), (15, 0x051E6720)):
        assert int(R.mmer_hash(seed, M)) == 0 and int(R.mmer_hash(seed ^ 1, M)) == 0x9E3779B1
        assert int(R.mmer_hash(seed ^ 3, M)) == (3 * 0x9E3779B1) % (1 << 32) == 0xDAA66D13
    assert R.mmer_len(25) == 13 and R.mmer_len(26) == 15
    assert int(R.remix32(0)) == 0 and int(R.remix32(1)) == 0x514E28B7          # (the 32-bit finaliser of MurmurHash3: its known value at 1)


@pytest.mark.parametrize("k", [21, 25, 26, 31])
def test_part_hash_is_strand_symmetric(k):
    rng = np.random.default_rng(k)
    x = rng.integers(0, 1 << (2 * k), size=3000, dtype=np.uint64)
    h = R.part_hash(x, k)
    assert np.array_equal(h, R.part_hash(R.revcomp(x, k), k))
    assert h.max() < (1 << 32) and len(np.unique(h >> np.uint64(23))) > 400      # (and it spreads: 3000 k-mers reach most of 512 partitions)


@pytest.mark.parametrize("k", [21, 25, 26, 31])
def test_low_mmers_are_the_minimizers_of_the_kmers_around_them(k):
    M = R.mmer_len(k)
    low = R.low_mmers(M, 12)
    hs = [h for _, h in low]
    assert hs == sorted(hs) and len(set(hs)) == 12
    rng = np.random.default_rng(100 + k)
    # nothing among a million random canonical M-mers hashes below the twelfth that is not one of the twelve
    f = rng.integers(0, 1 << (2 * M), size=1_000_000, dtype=np.uint64)
    c = np.minimum(f, R.revcomp(f, M))
    below = c[R.mmer_hash(c, M) <= np.uint64(hs[-1])]
    assert set(below.tolist()) <= {m for m, _ in low}
    for m, h in low:
        assert m < (1 << (2 * M)) and m <= int(R.revcomp(m, M)) and int(R.mmer_hash(m, M)) == h
        # the M-mer (or its reverse complement) at every offset of a k-mer with random bases around it
        for j in range(k - M + 1):
            for mer in (m, int(R.revcomp(m, M))):
                left = int(rng.integers(0, 1 << (2 * j))) if j else 0
                right = int(rng.integers(0, 1 << (2 * (k - M - j)))) if k - M - j else 0
                x = (left << (2 * (k - j))) | (mer << (2 * (k - M - j))) | right
                ph = int(R.part_hash(np.uint64(x), k))
                # (a random flank may hold one of the few M-mers below this one: then that one decides)
                assert ph == int(R.remix32(h)) or ph in {int(R.remix32(h2)) for h2 in hs if h2 < h}
    # and the first one decides whatever surrounds it
    m, h = low[0]
    x = rng.integers(0, 1 << (2 * k), size=200, dtype=np.uint64)
    j = (k - M) // 2
    keep = ~(np.uint64(((1 << (2 * M)) - 1) << (2 * j)))
    x = (x & keep) | np.uint64(m << (2 * j))
    assert np.all(R.part_hash(x, k) == R.remix32(h))


def test_neighbours_against_a_dict_of_strings():
    """2000 of the 8192 canonical 7-mers (a quarter of all neighbours present), looked up base by base"""
    k = 7
    rng = np.random.default_rng(7)
    tr = str.maketrans("ACGT", "TGCA")
    allk = np.arange(1 << (2 * k), dtype=np.uint64)
    canon = allk[allk <= R.revcomp(allk, k)]
    keys = rng.permutation(canon)[:2000]                      # table order: shuffled
    where = {R.decode(x, k): i for i, x in enumerate(keys)}
    want = np.full((2000, 8), N, dtype=np.uint32)
    want_rc = np.zeros((2000, 8), dtype=bool)
    for i, x in enumerate(keys):
        s = R.decode(x, k)
        for nuc, ch in enumerate("ACGT"):
            for slot, y in ((2 * nuc, s[1:] + ch), (2 * nuc + 1, ch + s[:-1])):
                r = y[::-1].translate(tr)
                want[i, slot] = where.get(min(y, r), N)
                want_rc[i, slot] = r < y
    got, rc = R.neighbours(keys, k, with_strand=True)
    assert np.array_equal(got, want) and np.array_equal(rc, want_rc)
    present = got != N
    assert 3000 < present.sum() < 5000 and (got == np.arange(2000)[:, None]).any()      # (AAAAAAA or another self loop among them)
