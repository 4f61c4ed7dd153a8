"""One pass of the wide sort path (metafast_amd/csrc/mf_wide.hip: the radix passes over the leading bits, k_wide_finish, k_wide_big<64> / <256>,
k_wide_big_extent / _move, the run lengths) restated in numpy and Python ints for tests/test_wsort_gpu.py, and the crafted entries that aim at
its borders.  The rules are stated on the ordered array; nothing here is shared with the kernels' way of getting there (tiles in LDS, tables of
representatives, bitmaps, wave leaders, streamed hash tables).  tests/test_wsort_ref_cpu.py pins lead() and asserts, from this file alone, that
every case has the property it is there for.

    k-mer         a 2k-bit number as (hi, lo): lo = its low 64 bits, hi = the hb = 2k - 64 bits above them
    leading bits  the top tb bits of the 2k-bit number; tb = hb where hb is 24 .. 31 (k = 44 .. 47), otherwise 32.  For hb < tb they are the hb bits
                  of hi followed by the top tb - hb bits of lo, for hb >= tb the top tb of hi's hb bits
    bucket        a run of equal leading bits in the ascending array
    tile          tile t owns the ordered entries [512 t, 512 t + 512) and sees the 256 that follow; a bucket belongs to the tile its first entry lies in
    listed        a bucket of more than `big` entries (option wide_big_bucket, 1 .. 256)
    second list   a listed bucket of more than min(dlimit, 320) distinct k-mers (option wide_distinct, 1 .. 1280)
    third list    ... of more than dlimit distinct k-mers: sorted aside -- or, where the third list's buckets hold more than n / 4 entries, all 2k bits
                  of the whole pass are sorted
    counts        run lengths of the ascending array, saturated at 32767"""
import numpy as np

import wskm_ref as W

_U = np.uint64
M64 = (1 << 64) - 1
TILE, SEEN = 512, 256
BIG, DLIMIT, DLIMIT_WAVE = 256, 1280, 320
KS = (32, 33, 43, 44, 47, 48, 62, 63)
ORDERS = ("built", "ascending", "descending", "shuffled")
INFO = ("listed", "list2", "list3", "hashed_entries", "hashed_buckets", "hashed_largest", "hashed_distinct", "big_total", "kept", "tb")


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
def lead(k):
    """-> (tb, bits taken from the high word, bits taken from the top of the low word)"""
    hb = 2 * k - 64
    tb = hb if 24 <= hb <= 31 else 32
    return tb, min(hb, tb), tb - min(hb, tb)


def bucket_ids(hi, lo, k):
    hi, lo = np.asarray(hi, dtype=np.uint64), np.asarray(lo, dtype=np.uint64)
    hb = 2 * k - 64
    _, nh, nl = lead(k)
    top = hi >> _U(hb - nh) if nh else np.zeros(len(hi), dtype=np.uint64)
    return ((top << _U(nl)) | (lo >> _U(64 - nl))) if nl else top


def expected(hi, lo, k):
    """-> (hi, lo) of the occurrences ascending, (hi, lo, cnt uint16) of the distinct k-mers ascending"""
    hi, lo = np.asarray(hi, dtype=np.uint64), np.asarray(lo, dtype=np.uint64)
    assert not len(hi) or int(hi.max()) >> (2 * k - 64) == 0
    o = np.lexsort((lo, hi))
    dh, dl, c, _ = W.count(hi, lo)
    return hi[o], lo[o], dh, dl, c.astype(np.uint16)


def buckets(hi, lo, k):
    """-> (first ordered entry, entries, distinct k-mers) of every bucket, in ascending order"""
    if not len(hi):
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    oh, ol = expected(hi, lo, k)[:2]
    ids = bucket_ids(oh, ol, k)
    assert np.all(ids[1:] >= ids[:-1])
    first = np.ones(len(ids), dtype=bool)
    first[1:] = ids[1:] != ids[:-1]
    start = np.flatnonzero(first).astype(np.int64)
    size = np.diff(np.append(start, len(ids)))
    group = np.cumsum(first) - 1
    return start, size, W.distinct_per_group(oh, ol, group, len(start))


def route(hi, lo, k, big=BIG, dlimit=DLIMIT, finish=1):
    """-> dict of INFO: what the pass must report"""
    out = dict.fromkeys(INFO, 0)
    out["tb"] = lead(k)[0]
    n = len(hi)
    if not finish or not n:
        return out
    _, size, dist = buckets(hi, lo, k)
    listed = size > big
    second = listed & (dist > min(dlimit, DLIMIT_WAVE))
    third = second & (dist > dlimit)
    done = listed & ~third
    out.update(listed=int(listed.sum()), list2=int(second.sum()), list3=int(third.sum()), hashed_entries=int(size[done].sum()), hashed_buckets=int(done.sum()),
               hashed_largest=int(size[done].max()) if done.any() else 0, hashed_distinct=int(dist[done].sum()), big_total=int(size[third].sum()))
    out["kept"] = 0 if out["big_total"] > n // 4 else 1
    return out


def info_vector(r):
    return [r[name] for name in INFO]


def tile_lists(hi, lo, k, big):
    """-> the number of listed buckets that start in every tile"""
    start, size, _ = buckets(hi, lo, k)
    n_tiles = (len(hi) + TILE - 1) // TILE
    return np.bincount(start[size > big] // TILE, minlength=n_tiles)


# ---------------------------------------------------------------------------------------------------------------------------------
# crafted entries
# ---------------------------------------------------------------------------------------------------------------------------------
class Build:
    """buckets one after the other in ascending order of their leading bits: the place a bucket takes in the ordered array is the number of entries in front"""

    def __init__(self, k, seed):
        self.k, self.rng = k, np.random.default_rng(seed * 100 + k)
        self.tb = lead(k)[0]
        self.tail_bits = 2 * k - self.tb
        self.vals, self.next_id = [], 0

    def at(self):
        return len(self.vals)

    def tail(self):
        r = self.rng
        return ((int(r.integers(0, 1 << 62)) << 62) | int(r.integers(0, 1 << 62))) & ((1 << self.tail_bits) - 1)

    def tails(self, d):
        got = set()
        while len(got) < d:
            got.add(self.tail())
        got = sorted(got)
        return [got[i] for i in self.rng.permutation(d)]

    def mix(self, d, n):
        """n tails, d distinct ones, every one at least once, in shuffled order"""
        t = self.tails(d)
        t = t + [t[i] for i in self.rng.integers(0, d, size=n - d)]
        return [t[i] for i in self.rng.permutation(n)]

    def bucket(self, tails, bid=None):
        """-> (first ordered entry, entries)"""
        if bid is None:
            bid = self.next_id + (int(self.rng.integers(1, 300)) if self.vals else 0)       # (the first bucket: leading bits 0)
        assert self.next_id <= bid < (1 << self.tb) and (bid > self.next_id or not self.vals)
        self.next_id = bid
        s = self.at()
        self.vals += [(bid << self.tail_bits) | t for t in tails]
        return s, len(tails)

    def filler(self, n):
        """n entries in buckets of 1 .. 4, k-mers repeated here and there"""
        while n > 0:
            m = min(n, int(self.rng.integers(1, 5)))
            self.bucket(self.mix(int(self.rng.integers(1, m + 1)), m))
            n -= m

    def arrays(self):
        v = self.vals
        return np.array([x >> 64 for x in v], dtype=np.uint64), np.array([x & M64 for x in v], dtype=np.uint64)


def seam(k, start, size):
    b = Build(k, 11)
    b.filler(start)
    b.bucket(b.mix(7, size))
    b.filler(300)
    return b


def cont(k):
    """[400, 600): a small bucket across a tile border; [700, 1600): starts in tile 1, covers tile 2, ends in tile 3, whose first bucket starts at 1600"""
    b = Build(k, 12)
    b.filler(400); b.bucket(b.mix(5, 200)); b.filler(100); b.bucket(b.mix(9, 900)); b.filler(600)
    return b


def big256(k):
    b = Build(k, 13)
    b.filler(100)
    for n in (256, 257):
        b.bucket(b.mix(6, n), b.next_id + 1)
    b.filler(200)
    for n in (257, 256):
        b.bucket(b.mix(3, n), b.next_id + 1)
    b.filler(100)
    return b


def small_big(k, big):
    """buckets of big and big + 1 entries side by side (neighbouring leading bits), equal and distinct k-mers inside"""
    b = Build(k, 14 + big)
    for i in range(260):
        n = big + int(b.rng.integers(0, 2)) if i % 5 else 1
        b.bucket(b.mix(int(b.rng.integers(1, n + 1)), n), b.next_id + 1 if i else 0)
    return b


def full_list(k):
    """1 + 2 x 256 x 3 entries: a bucket of one entry, then buckets of two -- with wide_big_bucket = 1 every tile lists 256 buckets"""
    b = Build(k, 17)
    b.bucket(b.tails(1))
    for i in range(256 * 3):
        b.bucket(b.mix(1 + i % 2, 2))
    return b


ONE_KMER = (32766, 32767, 32768, 40000)


def one_kmer(k):
    b = Build(k, 18)
    b.filler(50)
    for n in ONE_KMER:
        b.bucket(b.tails(1) * n)
        b.filler(3)
    t = b.tails(2)
    b.bucket(t * 400)                                       # a b a b ...: the two leader rounds of every wave
    t = b.tails(3)
    b.bucket(t * 300)                                       # a b c a b c ...: a third value for the probing loop
    b.filler(50)
    return b


def packed_border(b, d_first, n_first, n_new, n_more):
    """a bucket whose first n_first entries (in built order) hold d_first distinct k-mers, the next n_new only new ones, then n_more repeats"""
    t = b.tails(d_first + n_new)
    head = t[:d_first] + [t[i] for i in b.rng.integers(0, d_first, size=n_first - d_first)]
    head = [head[i] for i in b.rng.permutation(n_first)]
    return head + t[d_first:] + [t[i] for i in b.rng.integers(0, len(t), size=n_more)]


def dl320(k):
    b = Build(k, 19)
    b.filler(30)
    for d, n in ((320, 320), (320, 700), (321, 321), (321, 700)):
        b.bucket(b.mix(d, n)); b.filler(5)
    b.bucket(packed_border(b, 320, 3 * 128, 128, 50))        # 448 k-mers in the table of 512 when the wave gives up
    b.filler(30)
    return b


def dl1280(k):
    b = Build(k, 20)
    b.filler(30)
    b.bucket(b.tails(1) * 30000)                             # (bulk: the third list stays under a quarter)
    for d, n in ((1280, 1280), (1280, 3000), (1281, 1281), (1281, 3000)):
        b.bucket(b.mix(d, n)); b.filler(5)
    b.bucket(packed_border(b, 1280, 3 * 512, 512, 100))      # 1792 k-mers in the table of 2048 when the workgroup gives up
    b.filler(30)
    return b


def dl_small(k, dlimit):
    b = Build(k, 21 + dlimit)
    b.filler(20)
    b.bucket(b.tails(1) * 5000)
    for d, n in ((dlimit, 300), (dlimit + 1, 300), (dlimit, 257), (dlimit + 1, 257), (dlimit + 1, 700)):
        t = b.tails(d)
        body = t[:1] * (n - d + 1) + t[1:]                   # (one abundant k-mer and d - 1 single ones)
        b.bucket([body[i] for i in b.rng.permutation(n)])
        b.filler(4)
    return b


def quarter(k, over):
    """wide_distinct = 1: three third-list buckets apart, a listed bucket of one k-mer and small buckets between; n = 4800, big_total = 1200 + over"""
    b = Build(k, 30)
    b.filler(700); b.bucket(b.mix(2, 300)); b.filler(900); b.bucket(b.tails(1) * 400); b.bucket(b.mix(3, 260), b.next_id + 1)
    b.filler(800); b.bucket(b.mix(5, 640 + over)); b.filler(800 - over)
    return b


def tails_case(k):
    """entries of one bucket that differ in one bit only: the last bit of lo, bit 0 of hi (where it lies below the leading bits: k >= 49), the bit just
    below the leading bits; hi ascending with lo descending (k >= 49); and random tails, whose order goes with and against any hash of theirs.  Once
    in a bucket k_wide_finish orders (leading bits 0), once in a listed one, once in a small one with all leading bits set"""
    b = Build(k, 31)
    tb_ = b.tail_bits

    def special():
        t = b.tail() & ~1 & ~(1 << (tb_ - 1))
        s = [t, t | 1, t | (1 << (tb_ - 1)), t | 1 | (1 << (tb_ - 1))]
        if tb_ > 64:
            t &= ~(1 << 64)
            s += [t ^ (1 << 64), (t & ~M64) | (M64 - 5), ((t & ~M64) | (1 << 64)) + 5, t & ~M64, (t & ~M64) | (1 << 64)]
        return s
    sp = special()
    r = b.tails(60)
    b.bucket([x for x in sp + r + sp[:3] + r[:20]], 0)
    b.filler(200)
    sp, r = special(), b.tails(90)
    body = sp * 3 + r * 4
    b.bucket([body[i] for i in b.rng.permutation(len(body))])
    b.filler(200)
    sp, r = special(), b.tails(30)
    b.bucket(sp + r + sp, (1 << b.tb) - 1)
    return b


def tiny(k, n):
    b = Build(k, 40 + n)
    b.filler(n)
    return b


TINY = (0, 1, 2, 511, 512, 513, 767, 768, 769)
# name -> (builder, options)
CASES = {
    "seam511x256": (lambda k: seam(k, 511, 256), {}),
    "seam511x257": (lambda k: seam(k, 511, 257), {}),
    "seam512x256": (lambda k: seam(k, 512, 256), {}),
    "seam512x257": (lambda k: seam(k, 512, 257), {}),          # (listed by tile 1 alone: tile 0 sees its first 256 entries)
    "cont": (cont, {}),
    "big256": (big256, {}),
    "big1": (lambda k: small_big(k, 1), {"wide_big_bucket": 1}),
    "big2": (lambda k: small_big(k, 2), {"wide_big_bucket": 2}),
    "full_list": (full_list, {"wide_big_bucket": 1}),
    "one_kmer": (one_kmer, {}),
    "dl320": (dl320, {}),
    "dl1280": (dl1280, {}),
    "dl4": (lambda k: dl_small(k, 4), {"wide_distinct": 4}),
    "dl1": (lambda k: dl_small(k, 1), {"wide_distinct": 1}),
    "quarter": (lambda k: quarter(k, 0), {"wide_distinct": 1}),
    "quarter_over": (lambda k: quarter(k, 1), {"wide_distinct": 1}),
    "tails": (tails_case, {}),
}
CASES.update({f"tiny{n}": ((lambda k, n=n: tiny(k, n)), {}) for n in TINY})
OPTION_DEFAULTS = (("wide_big_bucket", BIG), ("wide_distinct", DLIMIT), ("wide_finish", 1))

_made = {}


def case(name, k):
    """-> (hi, lo) in built order, options; made once and left unchanged"""
    if (name, k) not in _made:
        hi, lo = CASES[name][0](k).arrays()
        hi.setflags(write=False); lo.setflags(write=False)
        _made[(name, k)] = hi, lo
    return _made[(name, k)] + (CASES[name][1],)


def ordered(hi, lo, how):
    if how == "built":
        return hi, lo
    if how == "shuffled":
        o = np.random.default_rng(4242).permutation(len(hi))
    else:
        o = np.lexsort((lo, hi))
        if how == "descending":
            o = o[::-1]
    return np.ascontiguousarray(hi[o]), np.ascontiguousarray(lo[o])


_refs = {}


def reference(name, k):
    """-> (expected(...), route(...)) of a case with its options; computed once"""
    if (name, k) not in _refs:
        hi, lo, opts = case(name, k)
        _refs[(name, k)] = expected(hi, lo, k), route(hi, lo, k, opts.get("wide_big_bucket", BIG), opts.get("wide_distinct", DLIMIT))
    return _refs[(name, k)]
