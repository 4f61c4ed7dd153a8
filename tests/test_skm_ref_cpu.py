"""tests/skm_ref.py (the reference of tests/test_skm_records_gpu.py) pinned without a GPU: its records fold to the oracle's table, their
partition hash is nbr_ref.part_hash of every k-mer they hold, and a record survives encoding and decoding."""
import numpy as np
import pytest

import nbr_ref as R
import skm_ref as S
from test_skm_records_gpu import genome_and_ragged, low_complexity
from util import pack_reads, random_reads

KS = [20, 25, 26, 31]


def _inputs(k):
    rng = np.random.default_rng(500 + k)
    yield "random", random_reads(rng, 300, 0, 200), 0
    yield "genome + ragged", genome_and_ragged(k, n_genome=300, n_ragged=200), 0
    yield "low complexity", low_complexity(k), 0
    yield "low complexity, min_len 100", low_complexity(k), 100


def _records(sc, form, bits1):
    start, n = sc.exact() if form == "exact" else sc.one_pass(700)
    return start, n, S.encode_records(sc.code, start, n, sc.mh[start], sc.k, bits1)


@pytest.mark.parametrize("form", ["exact", "one-pass"])
@pytest.mark.parametrize("k", KS)
def test_records_fold_to_the_oracles_table(oracle, k, form):
    for name, (b, o), min_len in _inputs(k):
        sc = S.Scan(b, o, k, min_len)
        start, n, (x, y) = _records(sc, form, 5)
        assert len(start) >= sc.ideal_count() > 0, name
        assert n.min() >= 1 and n.max() <= S.rmax(k), name
        km, _ = S.record_kmers(x, y, k)
        assert np.array_equal(np.sort(km), sc.occurrences()), name          # every forward occurrence, once
        keys, counts = np.unique(R.canonical(km, k), return_counts=True)
        ok, ov = oracle.Table().count_buffer(b, o, k, min_len).export()
        assert counts.max() < 32767, name
        assert np.array_equal(keys, ok) and np.array_equal(counts.astype(np.int32), ov), (name, k, form)
    if form == "one-pass":                                                   # (the reads of 150 bases: runs go on across words)
        sc = S.Scan(*genome_and_ragged(k, n_genome=300, n_ragged=200), k)
        assert len(sc.one_pass(700)[0]) < len(sc.exact()[0])


@pytest.mark.parametrize("k", KS)
def test_partition_hash_of_every_kmer(k):
    for name, (b, o), min_len in _inputs(k):
        sc = S.Scan(b, o, k, min_len)
        for form in ("exact", "one-pass"):
            start, n, (x, y) = _records(sc, form, 7)
            km, rec = S.record_kmers(x, y, k)
            ph = R.part_hash(R.canonical(km, k), k)
            assert np.array_equal(ph, R.remix32(sc.mh[start])[rec]), (name, form)
            # ... and the digit field and the partition are slices of it: 7 bits of level 1, then 22 that travel
            assert np.array_equal(S.rec_digits(y)[rec], ((ph << np.uint64(7)) & np.uint64(0xFFFFFFFF)) >> np.uint64(10)), (name, form)
            assert np.array_equal(S.partition_of(sc.mh[start], 7, 12)[rec], (ph >> np.uint64(20)).astype(np.int64)), (name, form)
            assert np.array_equal(S.partition_of(sc.mh[start], 7, 12, dlo=3)[rec], (ph >> np.uint64(20)).astype(np.int64) - 3 * 32), (name, form)


@pytest.mark.parametrize("k,nbases", [(20, 39), (25, 44), (26, 45), (31, 50)])
def test_record_round_trip(k, nbases):
    rng = np.random.default_rng(k)
    assert S.rmax(k) + k - 1 == nbases and S.rmax(k) == 20
    for n in (1, 2, S.rmax(k) - 1, S.rmax(k)):
        s = "".join("ACGT"[i] for i in rng.integers(0, 4, size=n + k - 1 + 7))       # (seven more bases follow in the read: they stay out)
        code = S.base_codes(np.frombuffer(s.encode(), dtype=np.uint8))
        mh = np.array([0x12345678], dtype=np.uint64)
        x, y = S.encode_records(code, [0], [n], mh, k, 4)
        got_n, digits, kmers = S.decode_record(x[0], y[0], k)
        assert got_n == n and kmers == [s[i:i + k] for i in range(n)]
        ph = int(R.remix32(mh)[0])
        assert digits == ((ph << 4) & 0xFFFFFFFF) >> 10
        jx, jy = S.junk_bits(x, y, k)
        assert jx[0] == 0 and jy[0] == 0
        # the layout, bit by bit: base i < 32 at x bits 63 - 2 i, 62 - 2 i; base 32 + j at y bits 63 - 2 j, 62 - 2 j; nothing else
        want = 0
        for i, ch in enumerate(s[:n + k - 1]):
            want |= "AGCT".index(ch) << (126 - 2 * i)
        want |= (digits << 6) | n
        assert (int(x[0]) << 64) | int(y[0]) == want
        # a set bit behind the last base is junk, wherever it sits
        for bit in {b for b in (126 - 2 * (n + k - 1), 127 - 2 * (n + k - 1), 28) if b >= 28 and n + k - 1 < S.BASES}:   # (50 bases leave none)
            bx, by = np.uint64((1 << bit) >> 64), np.uint64((1 << bit) & 0xFFFFFFFFFFFFFFFF)
            jx, jy = S.junk_bits(x | bx, y | by, k)
            assert (int(jx[0]) << 64) | int(jy[0]) == 1 << bit, (n, bit)
    assert S.is_sentinel(np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0xFFFFFFFFFFFFFFFF)) and S.rec_n(np.uint64(0xFFFFFFFFFFFFFFFF)) == S.SENTINEL_N


def test_cut_rule_by_hand():
    """one read whose k-mers all share a minimizer (the smallest 13-mer of the order, in the middle of the read): a single run of 9 k-mers
    from position 30 is two pieces in the exact form (2 + 7: position 32 cuts) and one where the one-pass form may extend"""
    k, M = 21, 13
    m, _ = R.low_mmers(M, 1)[0]
    rng = np.random.default_rng(7)
    while True:
        left, right = (S.decode(int(v), 8) for v in rng.integers(0, 1 << 16, size=2))
        read = left + S.decode(m, M) + right                                       # 29 bases, 9 k-mers, all of them hold the M-mer
        b, o = pack_reads(["A" * 10, "C" * 20, read])                             # two reads below k in front: the run starts at position 30
        sc = S.Scan(b, o, k)
        ps, pl = sc.pieces(False)
        if len(ps) == 1:
            break
    assert ps.tolist() == [30] and pl.tolist() == [9] and sc.ideal_count() == 1
    assert [a.tolist() for a in sc.exact()] == [[30, 32], [2, 7]]
    assert [a.tolist() for a in sc.one_pass(1000)] == [[30], [9]]                  # word 1 is lane 1 of its batch
    sc = S.Scan(*pack_reads(["A" * 10, "C" * 20] + ["G" * 20] * 99 + ["T" * 4, read]), k)      # the same run from 32 * 63 - 2
    assert sc.pieces(False)[0].tolist() == [32 * 63 - 2]
    assert [a.tolist() for a in sc.one_pass(1000)] == [[32 * 63 - 2, 32 * 63], [2, 7]]          # word 63 is the first of a wave's batch
    assert [a.tolist() for a in sc.one_pass(63)] == [[32 * 63 - 2, 32 * 63], [2, 7]]            # ... of a workgroup
    assert [a.tolist() for a in sc.one_pass(62)] == [[32 * 63 - 2], [9]]                        # ... the second word of a workgroup
