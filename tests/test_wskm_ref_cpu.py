"""tests/wskm_ref.py (the reference of tests/test_wskm_stages_gpu.py) pinned without a GPU: its records fold to the oracle's table, a k-mer's
occurrences lie in one partition, two hand-worked reads give the records written here as literals -- and every crafted input of the GPU tests
has, by the reference alone, the property it is there for, so that no GPU test passes vacuously."""
import numpy as np
import pytest

import nbr_ref as R
import skm_ref as S
import wskm_ref as W
import test_wskm_stages_gpu as G
from test_wide_gpu import _reads
from util import pack_reads


def _ragged(k):
    return _reads(np.random.default_rng(40 + k), 400, 20, 220)


@pytest.mark.parametrize("k", [32, 35, 47, 63])
def test_records_fold_to_the_oracles_table(oracle, k):
    b, o = _ragged(k)
    st = W.Stages(W.Scan(b, o, k))
    assert st.n.min() >= 1 and st.n.max() <= W.RMAX and int(st.n.sum()) == st.sc.n_occ
    rows = st.words()
    hi, lo, rec, wgt = W.record_kmers(rows, k)
    assert len(hi) == st.sc.n_occ and (wgt == 1).all()
    ohi, olo, ocnt, n_occ = oracle.count_wide(b, o, k, 0)
    assert n_occ == st.sc.n_occ and ocnt.max() < W.MAX_COUNT
    for thr in (0, 2):
        keep = ocnt > thr
        ghi, glo, gc, n_all = W.count(hi, lo, wgt, thr)
        assert n_all == len(ocnt) and np.array_equal(ghi, ohi[keep]) and np.array_equal(glo, olo[keep]) and np.array_equal(gc, ocnt[keep])
        thi, tlo, tc, t_all = st.table(thr)                                      # ... and the same from the positions (canonical_at)
        assert t_all == n_all and np.array_equal(thi, ghi) and np.array_equal(tlo, glo) and np.array_equal(tc, gc)
    # packed: the weights stand for the records that went
    packed = W.pack(rows[st.order])
    phi, plo, _, pw = W.record_kmers(packed, k)
    ghi, glo, gc, _ = W.count(phi, plo, pw, 0)
    assert len(phi) < len(hi) and np.array_equal(ghi, ohi) and np.array_equal(glo, olo) and np.array_equal(gc, ocnt)
    # a min_len above k
    st2 = W.Stages(W.Scan(b, o, k, 150))
    ohi, olo, ocnt, n_occ = oracle.count_wide(b, o, k, 150)
    thi, tlo, tc, _ = st2.table(0)
    assert n_occ == st2.sc.n_occ > 0 and np.array_equal(thi, ohi) and np.array_equal(tlo, olo) and np.array_equal(tc, ocnt)


@pytest.mark.parametrize("k", [32, 35, 47, 63])
def test_a_kmers_occurrences_lie_in_one_partition(k):
    b, o = _ragged(k)
    st = W.Stages(W.Scan(b, o, k), unit=64)
    assert st.pbits >= 8
    hi, lo, rec, _ = W.record_kmers(st.words(), k)
    part = st.part[rec].astype(np.int64)
    assert np.array_equal(W.distinct_per_group(hi, lo, part, 1 << st.pbits).sum(), W.count(hi, lo)[3])      # no k-mer in two partitions
    # all k-mers of a record share the record's minimizer hash: the partition is the k-mer's own
    pos = np.flatnonzero(st.sc.valid)
    rec_of_pos = np.repeat(np.arange(st.n_rec), st.n)
    assert np.array_equal(np.repeat(st.start, st.n) + (np.arange(len(pos)) - np.repeat(np.cumsum(st.n) - st.n, st.n)), pos)
    assert np.array_equal(st.sc.mh[pos], st.sc.mh[st.start][rec_of_pos])


def test_canonical_kmers_in_python_ints():
    rng = np.random.default_rng(7)
    for k in (32, 33, 48, 63):
        code = rng.integers(0, 4, size=200).astype(np.uint8)
        code[50:50 + k] = np.where(np.arange(k) % 2 == 0, 0, 3)               # (AT)n: its own reverse complement at even k
        pos = np.arange(0, 200 - k + 1)
        hi, lo = W.canonical_at(code, pos, k)
        for p in pos:
            fw = rc = 0
            for c in code[p:p + k]:
                fw = (fw << 2) | int(c)
            for c in code[p:p + k][::-1]:
                rc = (rc << 2) | (3 - int(c))
            assert (int(hi[p]) << 64) | int(lo[p]) == min(fw, rc), (k, p)


def test_two_hand_worked_reads_at_k33():
    """LOW = the 15-mer with the smallest hash.  Read 1: 10 bases, LOW, 30 bases = 55 bases, 23 k-mers; the k-mers at 0 .. 10 hold LOW whole (10 + 15 <= p + 33
    for every p, and p <= 10), the ones behind do not.  Read 2: poly-A of 150 bases from position 55: 118 k-mers of one hash = 48 + 48 + 22"""
    k = 33
    low = S.decode(R.low_mmers(15, 1)[0][0], 15)
    r1 = "CAGTTGACCA" + low + "GTCAGGTTACCTGAACGGATCTTGCAAGTC"
    b, o = pack_reads([r1, "A" * 150])
    sc = W.Scan(b, o, k)
    start, n = sc.records()
    assert sc.n_occ == 23 + 118
    assert start[0] == 0 and n[0] == 11 and sc.mh[0] == R.low_mmers(15, 1)[0][1]
    assert start[1] == 11 and int(n[start < 55].sum()) == 23
    assert start[start >= 55].tolist() == [55, 103, 151] and n[start >= 55].tolist() == [48, 48, 22]
    w = W.record_words(sc.code, start, n)
    assert w[0, 7] == 11 and S.decode(int(w[0, 0]), 16) == r1[:16] and S.decode(int(w[0, 3]) >> 18, 7) == r1[48:] and int(w[0, 3]) & 0x3FFFF == 0      # runs on into the poly-A
    last = w[-1]
    assert last[7] == 22 and (last[:7] == 0).all()                           # A = 0, and code 0 behind the buffer's end
    assert W.pbits_of(141) == 0 and W.pbits_of(301) == 1 and W.pbits_of(2400 * 8, merge=0) == 3 and W.pbits_of(1 << 20) == 12


def test_units_and_pack_by_hand():
    poff = np.array([0, 3, 3, 20, 21, 40], dtype=np.uint64)                    # 5 partitions of 3, 0, 17, 1, 19 records
    u = W.units(poff, 40, 400, 3, unit=100, merge=1)                           # G = 10: borders at or behind 0, 10, 20, 30
    assert u.tolist() == [0, 20, 20, 40, 40]
    assert W.units(poff, 40, 400, 3, unit=100, merge=0).tolist() == poff.tolist()
    rows = np.zeros((1030, 8), dtype=np.uint32)
    rows[:, 7] = 5
    rows[3, 0] = 9
    p = W.pack(rows)
    assert p[:1023, 7].tolist() == [0] * 1022 + [5 | (1023 << 8)] and p[1023].tolist() == [9, 0, 0, 0, 0, 0, 0, 5 | (1 << 8)]
    assert p[1024:, 7].tolist() == [0] * 5 + [5 | (6 << 8)]
    assert W.lead_runs(np.array([0, 0, 1], dtype=np.uint64), np.array([5 << 32, 5 << 32 | 1, 0], dtype=np.uint64), 33) == [2, 1] and W.aside([0] * 65, list(range(65)), 32) == 65


# ---------------------------------------------------------------------------------------------------------------------------------
# the crafted inputs of tests/test_wskm_stages_gpu.py have the properties they are there for
# ---------------------------------------------------------------------------------------------------------------------------------
def _lens(o):
    return np.diff(o.astype(np.int64))


@pytest.mark.parametrize("k", [32, 35, 63])
def test_crafted_scan_inputs(k):
    b, o = G.long_read(k)
    assert _lens(o).max() == 10000 > W.TILE + W.HALO
    s, e = int(o[np.argmax(_lens(o))]), int(o[np.argmax(_lens(o)) + 1])
    assert (e - k) // W.TILE - s // W.TILE >= 2                                # k-mer starts in three tiles: one tile wholly inside the read
    b, o = G.tile_borders(k)
    ln, st = _lens(o), o[:-1].astype(np.int64)
    long_enough = ln >= k
    assert {4095, 0, 1} <= set((st[long_enough] % W.TILE).tolist())
    assert {4095, 0} <= set(((st[long_enough] + ln[long_enough] - k) % W.TILE).tolist())
    sc = W.Scan(b, o, k)
    assert all(sc.valid[p] for p in G.BORDER_STARTS + G.BORDER_LAST) and not any(sc.valid[p + 1] for p in G.BORDER_LAST)
    assert not sc.valid[G.BORDER_STARTS[0] - 1] and not sc.valid[G.BORDER_STARTS[2] - 1]
    b, o = G.long_runs(k)
    sc = W.Scan(b, o, k)
    rs, rl = sc.runs()
    assert rs[0] == 0 and rl[0] == 301 - k >= 3 * W.RMAX and rs[1] == 300 and rl[1] == 301 - k          # poly-A, (AT)n: one run each
    start, n = sc.records()
    full, rest = divmod(301 - k, W.RMAX)
    assert n[start < 300].tolist() == [W.RMAX] * full + ([rest] if rest else []) and start[start < 300].tolist() == list(range(0, 301 - k, W.RMAX))
    b, o = G.short_and_empty(k)
    ln = _lens(o)
    assert (ln == 0).sum() >= 12 and (ln == k - 1).sum() >= 12 and (ln == k).sum() >= 12 and ((ln >= k) & (ln < 100)).sum() >= 12
    assert 0 < W.Scan(b, o, k, 100).n_occ < W.Scan(b, o, k).n_occ


@pytest.mark.parametrize("k", [32, 63])
def test_crafted_record_room_input(k):
    b, o = G.one_kmer_reads(k)
    sc = W.Scan(b, o, k)
    n_tiles = (((len(b) + 31) // 32) * 32 + W.TILE - 1) // W.TILE
    assert len(sc.records()[0]) == sc.n_occ == 6000 > sc.n_occ // 10 + 4 * n_tiles + 4096


def test_crafted_pack_input():
    k = 32
    b, o = G.many_copies(k)
    st = W.Stages(W.Scan(b, o, k))
    rows = st.words()[st.order]
    p = W.pack(rows)
    assert (p[:, 7] >> 8).max() > 255
    assert any((rows[a - 1] == rows[a]).all() for a in range(W.WINDOW, len(rows), W.WINDOW))        # a class spans a window border
    assert len(np.unique(rows, axis=0)) < len(rows) // 100 and len(rows) > 20 * W.WINDOW


def test_crafted_count_inputs():
    k = 47
    b, o = G.heavy_partition(k)
    st = W.Stages(W.Scan(b, o, k))
    hi, lo, rec, _ = W.record_kmers(st.words(), k)
    per_part = W.distinct_per_group(hi, lo, st.part[rec].astype(np.int64), 1 << st.pbits)
    assert per_part.max() > 4 * W.FILL and per_part.max() >= 400 * 33 - 5 and st.overflowing_units() == 1
    b, o = G.unique_reads(k)
    st = W.Stages(W.Scan(b, o, k), unit=20000)
    assert st.overflowing_units() >= 2
    for kk in (32, 47, 63):                                                    # the default plan on the ragged reads: no unit overflows
        b, o = G.ragged(kk)
        assert W.Stages(W.Scan(b, o, kk)).overflowing_units() == 0
    for unit in (64, 300, 4000):                                               # ... nor do the smaller and larger units of test_sort_and_units
        b, o = G.ragged(47)
        assert W.Stages(W.Scan(b, o, 47), unit=unit).overflowing_units() == 0
    k = 63
    b, o = G.saturating_copies(k)
    st = W.Stages(W.Scan(b, o, k))
    hi, lo, cnt, n_all = st.table(0)
    assert n_all == 2 and cnt.tolist() == [W.MAX_COUNT, W.MAX_COUNT] and st.sc.n_occ == 140000
    assert W.pbits_of(W.Scan(*G.tiny(33), 33).n_occ) == 0


@pytest.mark.parametrize("k", [32, 33, 48, 63])
def test_crafted_order_inputs(k):
    hi, lo, cnt = G.order_case(k, "runs")
    runs = W.lead_runs(hi, lo, k)
    assert {1, 2, 63, 64, 65, 66, 128, 129, 1000} <= set(runs) and runs[0] == 70 and runs[-1] == 70
    v = sorted((int(h) << 64 | int(x)) >> (2 * k - 32) for h, x in zip(hi, lo))
    assert v.count(20000) == 100 and v.count(20001) == 90                     # two long runs side by side
    assert 0 < W.aside(hi, lo, k) == 70 + 65 + 66 + 128 + 129 + 1000 + 100 + 90 + 70 <= len(hi) // 8 + 1024
    assert len(set(zip(hi.tolist(), lo.tolist()))) == len(hi) and (hi < (1 << max(2 * k - 64, 0)) if k > 32 else hi == 0).all()
    hi, lo, cnt = G.order_case(k, "short runs")
    assert W.aside(hi, lo, k) == 0 and max(W.lead_runs(hi, lo, k)) == 64
    hi, lo, cnt = G.order_case(k, "too many aside")
    assert W.aside(hi, lo, k) == 2130 > len(hi) // 8 + 1024
    oh, ol, oc = W.order(hi, lo, cnt)
    back = {(int(h), int(x)): int(c) for h, x, c in zip(hi, lo, cnt)}
    assert [back[(int(h), int(x))] for h, x in zip(oh, ol)] == oc.tolist() and len(set(cnt.tolist())) > 1000
