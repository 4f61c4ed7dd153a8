"""tests/skm_count_ref.py (the reference of tests/test_skm_count_units_gpu.py) pinned without a GPU: the records of skm_ref's exact form, grouped
by partition and fed through it as units, add up to the oracle's table and to the oracle's histogram of dropped counts; and every crafted input
of test_skm_count_units_gpu.py is built here, which asserts what the input is meant to reach (the builders carry their own assertions, with
the kernel's hashes as skm_count_ref.py restates them)."""
import numpy as np
import pytest

import nbr_ref as R
import skm_count_ref as CR
import skm_ref as S
import test_skm_count_units_gpu as G
from test_skm_records_gpu import genome_and_ragged


@pytest.mark.parametrize("k", [20, 25, 31])
def test_units_add_up_to_the_oracles_table(oracle, k):
    b, o = genome_and_ragged(k)
    sc = S.Scan(b, o, k)
    start, n = sc.exact()
    bits1, B = 4, 7
    x, y = S.encode_records(sc.code, start, n, sc.mh[start], k, bits1)
    part = S.partition_of(sc.mh[start], bits1, B)
    order = np.argsort(part, kind="stable")
    x, y = x[order], y[order]
    plen = np.bincount(part, minlength=1 << B)
    pstart = np.cumsum(plen) - plen
    assert plen.min() > 0 and len(plen) == 1 << B
    units = CR.count_units(x, y, pstart, plen, k)
    ok, ov = oracle.Table().count_buffer(b, o, k).export()
    # a partition holds all occurrences of its k-mers: the units' key sets are disjoint, their union is the table
    keys = np.concatenate([u.keys for u in units])
    counts = np.concatenate([u.counts for u in units])
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(keys[order], ok) and np.array_equal(counts[order].astype(np.int32), ov)
    assert ov.max() > 2
    for thr in (-1, 1, 3):
        dcount, n_all, hist, redo = CR.totals(units, thr)
        assert n_all == len(ok) and dcount.sum() == int((ov > thr).sum()) and redo == 0
        assert np.array_equal(hist[:thr + 1], np.bincount(ov[ov <= thr], minlength=thr + 1)[:thr + 1]) and not hist[thr + 1:].any()
        kept = CR.pairs(np.concatenate([u.kept(thr)[0] for u in units]), np.concatenate([u.kept(thr)[1] for u in units]))
        assert np.array_equal(kept, CR.pairs(ok[ov > thr], ov[ov > thr]))
        # the gather: the bin of a key comes from the next bits of its partition hash, i.e. units cut by B + s bits are the table cut by them
        for s_bits in (0, 1, 3):
            dfine, parts = CR.gather(units, thr, k, s_bits, 32 - B - s_bits)
            want = np.bincount((R.part_hash(ok[ov > thr], k) >> np.uint64(32 - B - s_bits)).astype(np.int64), minlength=1 << (B + s_bits))
            assert np.array_equal(np.diff(dfine.astype(np.int64)), want) and [len(p) for p in parts] == want.tolist()


def test_saturation_and_sentinels():
    x, y = G.cat(G.times(G.text_record("A" * 50, 31), 2000), G.sentinels(3), G.text_record("ACGGTCATTGCAAGCTTAGGCATCGATCCGTAAGT"[:33], 31))
    u = CR.count_unit(x, y, 31)
    assert u.keys[0] == 0 and u.counts[0] == CR.MAX_COUNT and u.n_all == 4 and set(u.counts[1:].tolist()) == {1}
    assert u.dropped_hist(1).tolist()[:3] == [0, 3, 0] and len(u.kept(1)[0]) == 1 and len(u.kept(-1)[0]) == 4
    assert CR.count_unit(*G.sentinels(8), 31).n_all == 0


def test_restated_hashes_by_hand():
    """one value each, worked through the kernel's expressions with Python integers"""
    key = 0x0123456789ABCDEF
    hi, lo = key >> 32, key & 0xFFFFFFFF
    rot = lambda v, r: ((v >> r) | (v << (32 - r))) & 0xFFFFFFFF
    x = lo ^ rot(hi, 19)
    x ^= x >> 15
    assert CR.c2_slot(np.array([key], dtype=np.uint64))[0] == ((((x & 0xFFFFFF) * 0x9E3779) & 0xFFFFFFFF) >> 11) & 4095
    g = ((hi * 0xC2B2AE35) ^ (lo * 0x27D4EB2F)) & 0xFFFFFFFF
    g ^= g >> 15
    g = (g * 0x165667B1) & 0xFFFFFFFF
    assert CR.pass_of(np.array([key], dtype=np.uint64))[0] == g >> 24
    rx, ry = 0xFEDCBA9876543210, (0x123456789 << 28) | (0x2AAAAA << 6) | 20
    ym = ry & ~(((1 << 22) - 1) << 6)
    h = (rx >> 32) ^ rot(rx & 0xFFFFFFFF, 11) ^ rot(ym >> 32, 21) ^ rot(ym & 0xFFFFFFFF, 5)
    h ^= h >> 16
    h = (h * 0x9E3779B1) & 0xFFFFFFFF
    h ^= h >> 15
    assert CR.rec_fingerprint(np.uint64(rx), np.uint64(ry)) == h
    assert CR.rec_fingerprint(np.uint64(rx), np.uint64(ry ^ (0x155555 << 6))) == h          # the digit field is left out


@pytest.mark.parametrize("i", range(len(G.ALL_BUILDERS)))
def test_every_crafted_input_has_its_property(i):
    inp = G.ALL_BUILDERS[i]()
    # ... and is well formed, as the hook demands it
    ps, pl = inp.pstart.astype(np.int64), inp.plen.astype(np.int64)
    assert np.all(pl % 4 == 0) and np.all(ps[1:] >= (ps + pl)[:-1]) and ps[-1] + pl[-1] <= len(inp.x)
    v = ~S.is_sentinel(inp.x, inp.y)
    n = S.rec_n(inp.y[v])
    assert np.all((n >= 1) & (n <= S.rmax(inp.k)))
    jx, jy = S.junk_bits(inp.x[v], inp.y[v], inp.k)
    assert not jx.any() and not jy.any()
    assert len(inp.ref) == inp.np and int(inp.occ.sum()) == int(n.sum())
