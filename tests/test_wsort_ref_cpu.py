"""tests/wsort_ref.py on its own (no GPU): lead() against hand-worked literals, the model against Python's sorted() on whole numbers, and every crafted
case of tests/test_wsort_gpu.py against the property it exists for -- asserted from the model alone, so that a case cannot silently stop covering
its border."""
from collections import Counter

import numpy as np
import pytest

import wsort_ref as R

KS = R.KS


def _at(b, start):
    """(entries, distinct) of the bucket that starts at ordered entry `start`, None if none does"""
    s, n, d = b
    i = np.flatnonzero(s == start)
    return (int(n[i[0]]), int(d[i[0]])) if len(i) else None


def _b(name, k):
    hi, lo, opts = R.case(name, k)
    return hi, lo, opts, R.buckets(hi, lo, k), R.reference(name, k)[1]


def test_lead_bits_by_hand():
    # k: (tb, bits of the high word, bits from the top of the low word); hb = 2k - 64 = 0, 2, 22, 24, 30, 32, 60, 62
    want = {32: (32, 0, 32), 33: (32, 2, 30), 43: (32, 22, 10), 44: (24, 24, 0), 47: (30, 30, 0), 48: (32, 32, 0), 62: (32, 32, 0), 63: (32, 32, 0)}
    assert set(want) == set(KS)
    for k, w in want.items():
        assert R.lead(k) == w, k
    assert [R.lead(k)[0] for k in range(32, 64)] == [32] * 12 + [24, 26, 28, 30] + [32] * 16
    # worked ids: the k-mer of all ones has all leading bits set; 1 << (2k - tb) is bucket 1; one less is the last k-mer of bucket 0
    for k in KS:
        tb = R.lead(k)[0]
        v = [(1 << (2 * k)) - 1, 1 << (2 * k - tb), (1 << (2 * k - tb)) - 1, (5 << (2 * k - tb)) | 3]
        ids = R.bucket_ids([x >> 64 for x in v], [x & R.M64 for x in v], k)
        assert ids.tolist() == [(1 << tb) - 1, 1, 0, 5], k


@pytest.mark.parametrize("k", KS)
def test_model_against_whole_numbers(k):
    hi, lo, _ = R.case("tails", k)
    v = sorted((int(h) << 64) | int(x) for h, x in zip(hi, lo))
    oh, ol, dh, dl, c = R.expected(hi, lo, k)
    assert [(int(h) << 64) | int(x) for h, x in zip(oh, ol)] == v
    cnt = Counter(v)
    assert [(int(h) << 64) | int(x) for h, x in zip(dh, dl)] == sorted(cnt) and c.tolist() == [cnt[x] for x in sorted(cnt)]
    tb = R.lead(k)[0]
    assert R.bucket_ids(oh, ol, k).tolist() == [x >> (2 * k - tb) for x in v]
    s, n, d = R.buckets(hi, lo, k)
    runs = Counter(x >> (2 * k - tb) for x in v)
    assert n.tolist() == [runs[i] for i in sorted(runs)] and s.tolist() == np.cumsum([0] + n.tolist())[:-1].tolist()
    assert d.tolist() == [len({x for x in cnt if x >> (2 * k - tb) == i}) for i in sorted(runs)]
    # saturation
    one = R.expected(np.zeros(40000, dtype=np.uint64), np.full(40000, 7, dtype=np.uint64), k)
    assert one[4].tolist() == [32767]
    # the orders are permutations of the case
    for how in R.ORDERS:
        a, b = R.ordered(hi, lo, how)
        assert sorted(zip(a.tolist(), b.tolist())) == sorted(zip(hi.tolist(), lo.tolist()))
    a, b = R.ordered(hi, lo, "descending")
    assert a.tolist() == oh[::-1].tolist() and b.tolist() == ol[::-1].tolist()


def test_route_rules_on_a_worked_example():
    # k = 32: the id is the top half of lo.  Buckets: 0 -> 3 entries, 2 distinct; 1 -> 2 entries, 2 distinct; 2 -> 1 entry; 3 -> 4 entries, 3 distinct
    lo = np.array([(0 << 32) | 5, 5, 6, (1 << 32) | 1, (1 << 32) | 2, 2 << 32, (3 << 32) | 1, (3 << 32) | 2, (3 << 32) | 3, (3 << 32) | 3], dtype=np.uint64)
    hi = np.zeros(10, dtype=np.uint64)
    r = R.route(hi, lo, 32, big=1, dlimit=2)               # listed: 0, 1, 3; more than 2 distinct: 3 -> lists 2 and 3; 4 entries > 10 // 4: the full sort
    assert R.info_vector(r) == [3, 1, 1, 5, 2, 3, 4, 4, 0, 32]
    r = R.route(hi, lo, 32, big=2, dlimit=1)               # listed: 0, 3; both have more than one distinct k-mer: 7 entries aside
    assert R.info_vector(r) == [2, 2, 2, 0, 0, 0, 0, 7, 0, 32]
    r = R.route(hi, lo, 32, big=3, dlimit=3)               # listed: 3, finished by the first kernel
    assert R.info_vector(r) == [1, 0, 0, 4, 1, 4, 3, 0, 1, 32]
    assert R.info_vector(R.route(hi, lo, 32, finish=0)) == [0] * 9 + [32]
    assert R.tile_lists(hi, lo, 32, 1).tolist() == [3]
    # a quarter exactly is still sorted aside: n = 8, 2 entries aside
    lo = np.array([1, 2, 1 << 32, 2 << 32, 3 << 32, 4 << 32, 5 << 32, 6 << 32], dtype=np.uint64)
    assert R.route(np.zeros(8, dtype=np.uint64), lo, 32, big=1, dlimit=1)["kept"] == 1


@pytest.mark.parametrize("k", KS)
def test_every_case_is_well_formed(k):
    hb = 2 * k - 64
    for name in R.CASES:
        hi, lo, opts = R.case(name, k)
        assert hi.dtype == lo.dtype == np.uint64 and len(hi) == len(lo) < 150000
        assert not len(hi) or int(hi.max()) >> hb == 0, name
        assert set(opts) <= {n for n, _ in R.OPTION_DEFAULTS}
        # built order: the buckets one after the other, ascending
        ids = R.bucket_ids(hi, lo, k)
        assert np.all(ids[1:] >= ids[:-1]), name
        # no tile lists more than the 256 buckets it has room for
        assert R.tile_lists(hi, lo, k, opts.get("wide_big_bucket", R.BIG)).max(initial=0) <= 256, name


@pytest.mark.parametrize("k", KS)
def test_seam_cases(k):
    hi, lo, _, b, r = _b("seam511x256", k)
    n, d = _at(b, 511)
    # the last start tile 0 owns and the longest bucket a tile orders itself: entries 511 .. 766, the tile's 768th entry is the next bucket's head
    assert n == 256 and d == 7 and 511 + n == R.TILE + R.SEEN - 1 and _at(b, 767) is not None and r["listed"] == 0
    hi, lo, _, b, r = _b("seam511x257", k)
    n, d = _at(b, 511)
    assert n == 257 and d == 7 and 511 + n == R.TILE + R.SEEN and r["listed"] == 1 and r["hashed_entries"] == 257       # to the tile's last entry: listed
    hi, lo, _, b, r = _b("seam512x256", k)
    assert _at(b, 512) == (256, 7) and r["listed"] == 0                                     # the next tile's; tile 0 sees all of it
    hi, lo, _, b, r = _b("seam512x257", k)
    assert _at(b, 512) == (257, 7) and r["listed"] == 1 and R.tile_lists(hi, lo, k, R.BIG).tolist()[:2] == [0, 1]
    for name in ("seam511x256", "seam511x257", "seam512x256", "seam512x257"):
        hi, lo, _ = R.case(name, k)
        assert len(set(zip(hi.tolist(), lo.tolist()))) < len(hi)                            # repeats


@pytest.mark.parametrize("k", KS)
def test_cont_case(k):
    hi, lo, _, b, r = _b("cont", k)
    assert _at(b, 400) == (200, 5)                                                          # owned by tile 0, seen again by tile 1 as its first bucket
    n, d = _at(b, 700)
    assert (n, d) == (900, 9) and 700 // R.TILE == 1 and 700 + n > 3 * R.TILE               # tile 2 = [1024, 1536) owns nothing of it
    assert not np.any((b[0] >= 2 * R.TILE) & (b[0] < 3 * R.TILE))
    assert _at(b, 1600) is not None and r["listed"] == 1 and r["hashed_entries"] == 900


@pytest.mark.parametrize("k", KS)
def test_big_border_cases(k):
    hi, lo, _, b, r = _b("big256", k)
    s, n, d = b
    i = np.flatnonzero(n >= 256)
    assert n[i].tolist() == [256, 257, 257, 256] and i[1] == i[0] + 1 and i[3] == i[2] + 1 and r["listed"] == 2 and r["hashed_entries"] == 514
    ids = np.unique(R.bucket_ids(hi, lo, k))
    assert ids[i[1]] == ids[i[0]] + 1 and ids[i[3]] == ids[i[2]] + 1                        # neighbouring leading bits
    for big in (1, 2):
        hi, lo, opts, b, r = _b(f"big{big}", k)
        s, n, d = b
        assert opts == {"wide_big_bucket": big} and set(n.tolist()) == {1, big, big + 1}
        assert r["listed"] == int((n == big + 1).sum()) > 50 and int((n == big).sum()) > 50
        pairs = set(zip(n[:-1].tolist(), n[1:].tolist()))
        assert (big, big + 1) in pairs and (big + 1, big) in pairs
        assert set(d[n == big + 1].tolist()) == set(range(1, big + 2))                      # all equal ... all distinct
        assert np.all(np.diff(np.unique(R.bucket_ids(hi, lo, k))) == 1)


@pytest.mark.parametrize("k", KS)
def test_full_list_case(k):
    hi, lo, opts, b, r = _b("full_list", k)
    s, n, d = b
    assert opts == {"wide_big_bucket": 1} and len(hi) == 1 + 2 * 256 * 3 and n[0] == 1 and np.all(n[1:] == 2)
    assert R.tile_lists(hi, lo, k, 1).tolist() == [256, 256, 256, 0]                        # the bound of mybig[] and of tile_cap
    assert _at(b, 511) is not None and r["listed"] == 768 == r["hashed_buckets"] and set(d[1:].tolist()) == {1, 2}


@pytest.mark.parametrize("k", KS)
def test_one_kmer_case(k):
    hi, lo, _, b, r = _b("one_kmer", k)
    s, n, d = b
    big = np.flatnonzero(n > 256)
    assert n[big].tolist() == list(R.ONE_KMER) + [800, 900] and d[big].tolist() == [1, 1, 1, 1, 2, 3]
    assert 40000 > 78 * R.TILE                                                              # streams over about 80 tiles
    c = R.reference("one_kmer", k)[0][4]
    assert sorted(c[c > 256].tolist()) == [300, 300, 300, 400, 400, 32766, 32767, 32767, 32767]
    # built order: a b a b ..., a b c a b c ...
    a = s[big[4]]
    assert (hi[a], lo[a]) == (hi[a + 2], lo[a + 2]) != (hi[a + 1], lo[a + 1])
    a = s[big[5]]
    assert len({(int(hi[a + j]), int(lo[a + j])) for j in range(3)}) == 3 and (hi[a], lo[a]) == (hi[a + 3], lo[a + 3])
    assert r["listed"] == 6 and r["list2"] == 0 and r["hashed_largest"] == 40000


def _distinct_prefix(hi, lo, a, n):
    return len(set(zip(hi[a:a + n].tolist(), lo[a:a + n].tolist())))


@pytest.mark.parametrize("k", KS)
def test_distinct_limit_cases(k):
    hi, lo, _, b, r = _b("dl320", k)
    s, n, d = b
    i = np.flatnonzero(n > 256)
    assert list(zip(n[i].tolist(), d[i].tolist())) == [(320, 320), (700, 320), (321, 321), (700, 321), (562, 448)]
    assert (r["listed"], r["list2"], r["list3"], r["kept"]) == (5, 3, 0, 1)
    a = int(s[i[4]])                                                                        # the wave looks every 128 entries: 320 after three looks, 448 = DCAP at the fourth
    assert _distinct_prefix(hi, lo, a, 384) == 320 and _distinct_prefix(hi, lo, a, 512) == 448 == 512 * 7 // 8
    hi, lo, _, b, r = _b("dl1280", k)
    s, n, d = b
    i = np.flatnonzero(n > 256)
    assert list(zip(n[i].tolist(), d[i].tolist())) == [(30000, 1), (1280, 1280), (3000, 1280), (1281, 1281), (3000, 1281), (2148, 1792)]
    assert (r["listed"], r["list2"], r["list3"], r["kept"]) == (6, 5, 3, 1) and r["big_total"] == 1281 + 3000 + 2148
    a = int(s[i[5]])                                                                        # the workgroup looks every 512 entries: 1280, then 1792 = DCAP
    assert _distinct_prefix(hi, lo, a, 1536) == 1280 and _distinct_prefix(hi, lo, a, 2048) == 1792 == 2048 * 7 // 8
    for dl in (4, 1):
        hi, lo, opts, b, r = _b(f"dl{dl}", k)
        s, n, d = b
        i = np.flatnonzero(n > 256)
        assert opts == {"wide_distinct": dl}
        assert list(zip(n[i].tolist(), d[i].tolist())) == [(5000, 1), (300, dl), (300, dl + 1), (257, dl), (257, dl + 1), (700, dl + 1)]
        assert (r["listed"], r["list2"], r["list3"], r["kept"]) == (6, 3, 3, 1) and r["big_total"] == 1257


@pytest.mark.parametrize("k", KS)
def test_quarter_cases(k):
    hi, lo, opts, b, r = _b("quarter", k)
    assert opts == {"wide_distinct": 1} and len(hi) == 4800
    assert r["list3"] == 3 and r["big_total"] == 1200 and r["big_total"] * 4 == len(hi) and r["kept"] == 1        # a quarter exactly: sorted aside
    s, n, d = b
    i = np.flatnonzero(n > 256)
    assert n[i].tolist() == [300, 400, 260, 640] and d[i].tolist() == [2, 1, 3, 5]
    assert i[1] - i[0] > 100 and i[2] == i[1] + 1 and i[3] - i[2] > 100                                           # the third-list buckets lie apart
    hi, lo, opts, b, r = _b("quarter_over", k)
    assert len(hi) == 4800 and r["big_total"] == 1201 and r["big_total"] * 4 > len(hi) and r["kept"] == 0         # one more: the whole pass
    assert r["hashed_entries"] == 400


@pytest.mark.parametrize("k", KS)
def test_tails_case(k):
    hi, lo, _, b, r = _b("tails", k)
    s, n, d = b
    tb = R.lead(k)[0]
    tail_bits = 2 * k - tb
    ids = np.unique(R.bucket_ids(hi, lo, k))
    assert ids[0] == 0 and ids[-1] == (1 << tb) - 1
    assert r["listed"] == 1 and n[0] <= 256 and n[-1] <= 256
    v = {(int(h) << 64) | int(x) for h, x in zip(hi, lo)}
    for first, size in ((0, int(n[0])), (int(s[n > 256][0]), int(n[n > 256][0])), (int(s[-1]), int(n[-1]))):
        oh, ol = R.expected(hi, lo, k)[:2]
        w = {(int(h) << 64) | int(x) for h, x in zip(oh[first:first + size], ol[first:first + size])}
        assert any(x ^ 1 in w for x in w)                                                   # the last bit of lo
        assert any(x ^ (1 << (tail_bits - 1)) in w for x in w)                              # the bit just below the leading bits
        if tail_bits > 64:                                                                  # (k >= 49: part of hi lies below the leading bits)
            assert any(x ^ (1 << 64) in w for x in w)                                       # bit 0 of hi
            assert any(x >> 64 < y >> 64 and x & R.M64 > y & R.M64 for x in w for y in w)   # hi ascending, lo descending
        assert any(x >> 64 == y >> 64 and x != y for x in w for y in w)                     # hi equal
    assert (2 * k - tb > 64) == (k >= 49)
    assert len(v) < len(hi)


@pytest.mark.parametrize("k", KS)
def test_tiny_cases(k):
    for n in R.TINY:
        hi, lo, _ = R.case(f"tiny{n}", k)
        assert len(hi) == n
        if n > 2:
            assert len(R.buckets(hi, lo, k)[0]) > n // 4
    assert R.TINY == (0, 1, 2, 511, 512, 513, 767, 768, 769)
    assert R.info_vector(R.reference("tiny0", k)[1]) == [0] * 9 + [R.lead(k)[0]]     # (an empty pass is not run)
