"""The count stage of the super-k-mer path (metafast_amd/csrc/mf_skm_count.h: k_skm_count, k_gather_split, k_gather_split_n) unit by unit on crafted
records against tests/skm_count_ref.py.

mf_debug_skm_count (mf_skm.hip; bound here with ctypes, not part of the C-ABI) takes a record buffer and a directory from the host and launches
the stage as skm_count_batches does (dyn = 1: a unit counter and drop_hist) or as skm_pilot does (dyn = 0: neither), with the grid, the number
of batches, the threshold, the raw value of option skm_dedupe and, where wanted, a room per unit of the caller's choosing; it hands back dcount,
every unit's slice of the (key, count) lists with what lies behind it (filled with 0xA5 before the launch), overflow, n_all, n_redo, drop_hist
and the gathered table (dk, dc, dfine).  Every comparison is bit-exact.  Every case checks

    a  dcount[p] = the unit's k-mers with count > thr
    b  the unit's slice holds exactly those (key, count) pairs, as a multiset (no order is specified); behind them, up to the unit's room and
       behind the last unit, nothing was written
    c  n_all = the distinct k-mers of all units before the cut; drop_hist[c] = the entries with count c <= thr (dyn = 1), each k-mer once
       however many attempts its unit took
    d  n_redo = the units with more than C2_FILL = 3400 distinct k-mers
    e  overflow = 0, or the code the case is about
    f  after the gather: dfine as exact numbers, every table partition the multiset the reference puts there (for two partitions per unit:
       bin 0 at the front of the unit's range, bin 1 at its back)

at dedupe 0, 1 and 5 x dyn 0 and 1 unless the case says otherwise: the results must not depend on either.  The inputs are built by the
functions below; tests/test_skm_count_ref_cpu.py runs every one of them without a GPU and asserts what it is meant to reach (3400 distinct
k-mers, one home slot, one fingerprint for two records, ...), with the kernel's hashes as tests/skm_count_ref.py restates them.

Left out: WHICH path a unit took is inferred from the rules, not observed -- that dedupe = 1 skipped the search for the 15 units after a unit
without repeats (dd_skip), how often a wave's queue was drained, how many passes a unit needed beyond "more than one" (n_redo); the result is
what is pinned.  The content of a unit's slice after overflow code 2 (only: nothing behind its room, what is there belongs to the unit) and the
units a workgroup leaves uncounted after code 1 (the host throws the run away).  The streamed level 1 and the pilot's own launch geometry."""
import ctypes as C
import functools

import numpy as np
import pytest

import nbr_ref as R
import skm_count_ref as CR
import skm_ref as S

gpu = pytest.mark.gpu

K = 31                             # the cases that are not about k
CANARY_KEY, CANARY_CNT = 0xA5A5A5A5A5A5A5A5, 0xA5A5
MODES = [(d, y) for d in (0, 1, 5) for y in (0, 1)]       # (dedupe, dyn)


# ---------------------------------------------------------------------------------------------------------------------------------
# records and inputs (no GPU needed)
# ---------------------------------------------------------------------------------------------------------------------------------
def pack(codes, n, k, mh=0):
    """records of n[i] k-mers from the base codes codes[i, :n[i] + k - 1] (A G C T = 0 .. 3) -> (x, y); mh: what the digit field is made of"""
    codes, n = np.asarray(codes, dtype=np.uint8).reshape(-1, S.BASES), np.asarray(n, dtype=np.int64)
    assert len(codes) == len(n) and n.min(initial=1) >= 1 and n.max(initial=1) <= S.rmax(k)
    mh = np.broadcast_to(np.asarray(mh, dtype=np.uint64), n.shape)
    return S.encode_records(codes.reshape(-1), np.arange(len(n)) * S.BASES, n, mh, k, 0)


def random_records(rng, count, k, n=None):
    n = rng.integers(1, S.rmax(k) + 1, size=count) if n is None else np.full(count, n)
    return pack(rng.integers(0, 4, size=(count, S.BASES)), n, k, rng.integers(0, 1 << 32, size=count))


def kmer_records(v, k):
    """one record of one k-mer per value"""
    v = np.asarray(v, dtype=np.uint64)
    codes = np.zeros((len(v), S.BASES), dtype=np.uint8)
    for i in range(k):
        codes[:, i] = (v >> np.uint64(2 * (k - 1 - i))) & np.uint64(3)
    return pack(codes, np.ones(len(v), dtype=np.int64), k)


def text_record(s, k, mh=0):
    codes = np.zeros((1, S.BASES), dtype=np.uint8)
    codes[0, :len(s)] = S.base_codes(np.frombuffer(s.encode(), dtype=np.uint8))
    return pack(codes, [len(s) - k + 1], k, mh)


def revcomp_text(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def cat(*recs):
    return np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs])


def times(rec, m):
    return np.repeat(rec[0], m), np.repeat(rec[1], m)


def shuffled(rng, rec):
    o = rng.permutation(len(rec[0]))
    return rec[0][o], rec[1][o]


ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def sentinels(m):
    return np.full(m, ONES), np.full(m, ONES)


class Input:
    """units (each the (x, y) of its records, sentinels where the case wants them) -> one record buffer and its directory; every region is
    padded with sentinels to a multiple of 4, `gap` records lie between two regions"""

    def __init__(self, k, units, gap=0):
        self.k = k
        xs, ys, self.pstart, self.plen = [], [], [], []
        at = 0
        for x, y in units:
            pad = -len(x) % 4
            x, y = np.concatenate([x, sentinels(pad)[0]]), np.concatenate([y, sentinels(pad)[1]])
            self.pstart.append(at)
            self.plen.append(len(x))
            xs += [x, sentinels(gap)[0]]
            ys += [y, sentinels(gap)[1]]
            at += len(x) + gap
        self.x, self.y = np.concatenate(xs).astype(np.uint64), np.concatenate(ys).astype(np.uint64)
        self.pstart, self.plen = np.array(self.pstart, dtype=np.uint64), np.array(self.plen, dtype=np.uint32)
        self.np = len(units)

    @functools.cached_property
    def ref(self):
        return CR.count_units(self.x, self.y, self.pstart, self.plen, self.k)

    @functools.cached_property
    def occ(self):
        n = S.rec_n(self.y) * ~S.is_sentinel(self.x, self.y)
        return np.array([n[int(s):int(s) + int(ln)].sum() for s, ln in zip(self.pstart, self.plen)], dtype=np.int64)

    def records(self, p):
        s, n = int(self.pstart[p]), int(self.plen[p])
        v = ~S.is_sentinel(self.x[s:s + n], self.y[s:s + n])
        return self.x[s:s + n][v], self.y[s:s + n][v]


@functools.lru_cache(maxsize=None)
def record_shapes(k):
    """one unit: records of every n from 1 to RMAX (one item, an odd last item, the item that crosses from the record's first word into its
    second, all 50 bases at k = 31) of random bases, poly-A (key 0) and poly-T (key 0 again), for even k a palindromic k-mer, a record and its
    reverse complement"""
    rng = np.random.default_rng(9000 + k)
    r = S.rmax(k)
    al = "ACGT"
    parts = [random_records(rng, 1, k, n) for n in range(1, r + 1) for _ in range(3)]
    parts += [text_record("A" * (n + k - 1), k) for n in (1, 2, r)] + [text_record("T" * (n + k - 1), k, 77) for n in (1, 3, r)]
    s = "".join(al[i] for i in rng.integers(0, 4, size=k + 11))
    parts += [text_record(s, k, 5), text_record(revcomp_text(s), k, 6)]
    if k % 2 == 0:
        h = "".join(al[i] for i in rng.integers(0, 4, size=k // 2))
        pal = h + revcomp_text(h)
        parts += [text_record("G" + pal + "C", k), text_record(pal, k)]
    inp = Input(k, [shuffled(rng, cat(*parts))])
    u = inp.ref[0]
    assert set(S.rec_n(inp.records(0)[1]).tolist()) == set(range(1, r + 1)) and r + k - 1 <= S.BASES and (k < 31 or r + k - 1 == S.BASES)
    assert u.keys[0] == 0 and u.counts[0] == 2 * (1 + r) + 2 + 3                       # poly-A and poly-T fold to key 0
    f = S.record_kmers(*text_record(s, k), k)[0]
    assert np.all(u.counts[np.searchsorted(u.keys, R.canonical(f, k))] == 2)          # a record and its reverse complement: counts add
    if k % 2 == 0:
        p = np.uint64(S.encode(pal))
        assert R.revcomp(p, k) == p and u.counts[np.searchsorted(u.keys, p)] == 2
    return inp


@functools.lru_cache(maxsize=None)
def fingerprint_pair(kind="sorted"):
    """two different records of 20 k-mers (k = 31) with the same 32-bit fingerprint: the same slot and the same tag in the search for identical
    records.  "sorted": sorted out of 2^19 seeded random records (about 32 such pairs are expected; they differ all over).  "y only" / "x only":
    made from one record by flipping two base bits that meet in the fingerprint's first fold (y bits 28 and 44; x bits 20 and 41) -- the two
    records differ in that word alone, so each word's comparison with the claimant is what keeps them apart"""
    rng = np.random.default_rng(77)
    if kind != "sorted":
        x, y = random_records(rng, 1, K, 20)
        x2, y2 = (x, y ^ np.uint64((1 << 28) | (1 << 44))) if kind == "y only" else (x ^ np.uint64((1 << 20) | (1 << 41)), y)
        assert CR.rec_fingerprint(x, y) == CR.rec_fingerprint(x2, y2) and ((x2 == x) == (kind == "y only")) and ((y2 == y) == (kind == "x only"))
        assert S.rec_n(y2) == 20 and S.rec_digits(y2) == S.rec_digits(y)
        return (x, y), (x2, y2)
    m = 1 << 19
    x = rng.integers(0, 1 << 63, size=m, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=m, dtype=np.uint64)
    y = (rng.integers(0, 1 << 36, size=m, dtype=np.uint64) << np.uint64(28)) | np.uint64(20)
    h = CR.rec_fingerprint(x, y)
    o = np.argsort(h, kind="stable")
    at = np.flatnonzero((h[o][1:] == h[o][:-1]) & ((x[o][1:] != x[o][:-1]) | (y[o][1:] != y[o][:-1])))
    assert len(at), "no two records with one fingerprint among 2^19"
    a, b = o[at[0]], o[at[0] + 1]
    assert h[a] == h[b] and (x[a], y[a]) != (x[b], y[b])
    assert not np.any(S.junk_bits(x[[a, b]], y[[a, b]], K)[0]) and not np.any(S.junk_bits(x[[a, b]], y[[a, b]], K)[1])
    return (x[[a]], y[[a]]), (x[[b]], y[[b]])


def identical_records(case):
    rng = np.random.default_rng(sum(map(ord, case)))
    one = random_records(rng, 1, K, 13)
    if case == "x2048":                                    # C2_DD x SKM_CT: the whole unit is one record, weight 2048
        inp = Input(K, [times(one, CR.DD)])
        assert inp.plen[0] == CR.DD and np.all(inp.ref[0].counts == CR.DD) and inp.ref[0].n_all == 13
    elif case == "x2049":                                  # the extra record takes the plain rounds
        inp = Input(K, [times(one, CR.DD + 1)])
        assert np.all(inp.ref[0].counts == CR.DD + 1)
    elif case == "digits differ":                          # equal in bases, different digit fields (y bits 6 .. 27): identical
        x, y = times(one, 300)
        y = (y & ~np.uint64(((1 << S.DIGIT_BITS) - 1) << 6)) | (rng.integers(0, 1 << S.DIGIT_BITS, size=300, dtype=np.uint64) << np.uint64(6))
        inp = Input(K, [(x, y)])
        assert len(np.unique(y)) > 250 and np.all(inp.ref[0].counts == 300) and len(np.unique(CR.rec_fingerprint(x, y))) == 1
    elif case == "y bases differ":                         # equal in x, the bases in y differ: not identical
        x, y = times(random_records(rng, 1, K, 20), 256)
        y = (y & np.uint64((1 << 28) - 1)) | (np.arange(256, dtype=np.uint64) << np.uint64(28 + 8))
        inp = Input(K, [shuffled(rng, cat((x, y), (x, y), (x[:50], y[:50])))])
        assert len(np.unique(x)) == 1 and len(np.unique(y)) == 256 and inp.ref[0].counts.min() == 2 and inp.ref[0].counts.max() == 562
    elif case == "saturation":                             # 40,960 occurrences of key 0
        inp = Input(K, [times(text_record("A" * 50, K), CR.DD)])
        assert inp.occ[0] == 40960 and inp.ref[0].keys.tolist() == [0] and inp.ref[0].counts.tolist() == [CR.MAX_COUNT]
    elif case == "sentinels":                              # at the start, in the middle and at the end of a region; a region of sentinels only; plen = 0 between two full units
        a, b, c = random_records(rng, 150, K), random_records(rng, 150, K), random_records(rng, 300, K)
        inp = Input(K, [cat(sentinels(5), a, sentinels(7), times(a, 2), sentinels(6)), sentinels(8), b, sentinels(0), cat(c, a)], gap=3)
        assert inp.plen.tolist()[1:4] == [8, 152, 0] and inp.ref[1].n_all == 0 and inp.ref[3].n_all == 0 and np.all(inp.ref[0].counts % 3 == 0)
    else:
        raise KeyError(case)
    return inp


IDENTICAL = ["x2048", "x2049", "digits differ", "y bases differ", "saturation", "sentinels"]


def collision_units(m, kind="sorted"):
    """the two records of fingerprint_pair m times each, in both orders, among other records"""
    a, b = fingerprint_pair(kind)
    rng = np.random.default_rng(m)
    other = random_records(rng, 40, K)
    inp = Input(K, [cat(times(a, m), times(b, m), other), cat(times(b, m), other, times(a, m)), shuffled(rng, cat(times(a, m), times(b, m), times(other, 2)))])
    for u in inp.ref:
        ka, kb = (R.canonical(S.record_kmers(*r, K)[0], K) for r in (a, b))
        both = np.isin(ka, kb)                                 # (records that differ in one base share the k-mers that do not hold it)
        assert both.sum() == {"sorted": 0, "y only": 11, "x only": 0}[kind]
        assert np.all(u.counts[np.searchsorted(u.keys, ka)] == np.where(both, 2 * m, m)) and np.all(u.counts[np.searchsorted(u.keys, kb)] == np.where(np.isin(kb, ka), 2 * m, m))
    return inp


LONG = ["2052", "4096", "5000", "head repeated", "tail repeated"]


def long_unit(case):
    """beyond C2_DD x SKM_CT = 2048 records: the search covers the first 2048, the others follow in plain rounds"""
    rng = np.random.default_rng(len(case) * 131 + sum(map(ord, case)))
    if case in ("2052", "4096", "5000"):
        pool = random_records(rng, 250, K)
        pick = rng.integers(0, 250, size=int(case))
        rec = (pool[0][pick], pool[1][pick])
    else:
        rep, uniq = times(random_records(rng, 16, K), 128), random_records(rng, 700, K, 2)
        rec = cat(shuffled(rng, rep), uniq) if case == "head repeated" else cat(uniq, random_records(rng, CR.DD - 700, K, 1), shuffled(rng, rep))
    inp = Input(K, [rec])
    assert inp.plen[0] > CR.DD and inp.ref[0].n_all <= CR.FILL
    if case == "head repeated":
        assert len(np.unique(rec[0][:CR.DD])) == 16 and len(np.unique(rec[0][CR.DD:])) == 700
    if case == "tail repeated":
        assert len(np.unique(rec[0][:CR.DD])) == CR.DD and len(np.unique(rec[0][CR.DD:])) == 16
    return inp


@functools.lru_cache(maxsize=None)
def _slot_pool():
    rng = np.random.default_rng(4095)
    v = R.canonical(rng.integers(0, 1 << 62, size=1_600_000, dtype=np.uint64), K)
    return v, CR.c2_slot(v)


@functools.lru_cache(maxsize=None)
def distinct_kmers(count, seed):
    """`count` different canonical k-mers, one record of one k-mer each"""
    rng = np.random.default_rng(seed)
    v = np.unique(R.canonical(rng.integers(0, 1 << 62, size=count + 64, dtype=np.uint64), K))
    assert len(v) >= count
    return v[rng.permutation(len(v))[:count]]


PRESSURE = ["one home slot", "home slot 4095", "3400", "3401", "4097", "6000", "100000"]


@functools.lru_cache(maxsize=None)
def pressure_unit(case):
    rng = np.random.default_rng(sum(map(ord, case)))
    if case in ("one home slot", "home slot 4095"):        # a probe chain of 300 slots; from slot 4095 it wraps the table
        v, s = _slot_pool()
        slot = 4095 if case == "home slot 4095" else 1234
        keys = np.unique(v[s == slot])
        assert len(keys) >= 300
        keys = keys[:300]
        assert np.all(CR.c2_slot(keys) == slot)
        inp = Input(K, [cat(kmer_records(keys, K), kmer_records(keys[::3], K))])
        assert inp.ref[0].n_all == 300 and np.array_equal(inp.ref[0].keys, keys)
        return inp
    want = int(case)
    if want in (3400, 6000):                               # whole records of 20 k-mers
        inp = Input(K, [random_records(rng, want // 20, K, 20)])
    elif want in (3401, 4097):
        inp = Input(K, [cat(random_records(rng, want // 20, K, 20), random_records(rng, 1, K, want % 20))])
    else:                                                  # 5000 records: a long unit as well
        inp = Input(K, [random_records(rng, want // 20, K, 20)])
        u = inp.ref[0]
        assert want // 16 > CR.SLOTS                       # 16 passes cannot do: one of them has more k-mers than the table has slots
        assert np.bincount(CR.pass_of(u.keys) & 63, minlength=64).max() <= CR.FILL      # 64 can
    assert inp.ref[0].n_all == want, (case, inp.ref[0].n_all)
    return inp


@functools.lru_cache(maxsize=None)
def beyond_64_passes():
    """unit 0 has more than 64 x 4096 distinct k-mers; three ordinary units beside it"""
    rng = np.random.default_rng(64)
    inp = Input(K, [random_records(rng, 13200, K, 20)] + [random_records(rng, 80 + 10 * i, K) for i in range(3)])
    assert inp.ref[0].n_all > CR.MAX_PASSES * CR.SLOTS and inp.plen[0] == 13200
    return inp


@functools.lru_cache(maxsize=None)
def attempt_that_fails_late():
    """a unit whose attempt in FOUR passes gets through pass 0 (1000 k-mers, written and tallied) and fails in pass 1 (3600 k-mers of that class):
    sixteen passes do.  What pass 0 wrote and tallied must not show: counts 1, 2 and 3, so that every cut drops or keeps some of them.  An
    ordinary unit on either side"""
    rng = np.random.default_rng(16)
    v = distinct_kmers(60000, 16)
    c = CR.pass_of(v)
    keys = np.concatenate([v[(c & 3) == 0][:1000], v[(c & 3) == 1][:3600]])
    cls4, cls16 = np.bincount(CR.pass_of(keys) & 3, minlength=4), np.bincount(CR.pass_of(keys) & 15, minlength=16)
    assert cls4.tolist() == [1000, 3600, 0, 0] and len(keys) > CR.FILL and cls16.max() <= CR.FILL - 2000
    rec = kmer_records(keys, K)
    unit = shuffled(rng, cat(rec, (rec[0][::2], rec[1][::2]), (rec[0][::4], rec[1][::4])))
    inp = Input(K, [random_records(rng, 70, K), unit, random_records(rng, 90, K)])
    assert np.bincount(inp.ref[1].counts).tolist() == [0, 2300, 1150, 1150] and np.array_equal(inp.ref[1].keys, np.sort(keys))
    return inp


MULTS = [1, 2, 3, 5, 6, 63, 64, 65, 100]
THRS = [-1, 0, 1, 2, 5, 63]


@functools.lru_cache(maxsize=None)
def cut_units():
    """unit 0: counts 1, 2, 3, 5, 6, 63, 64, 65, 100 in one pass; unit 1: the same counts over more than 3400 distinct k-mers"""
    rng = np.random.default_rng(63)
    small = cat(*[times(random_records(rng, 3, K), m) for m in MULTS])
    big = cat(*[times(random_records(rng, 22, K, 20), m) for m in MULTS])
    inp = Input(K, [shuffled(rng, small), shuffled(rng, big), random_records(rng, 50, K)])
    assert sorted(set(inp.ref[0].counts.tolist())) == MULTS and sorted(set(inp.ref[1].counts.tolist())) == MULTS
    assert inp.ref[0].n_all <= CR.FILL < inp.ref[1].n_all == 22 * 20 * len(MULTS)
    return inp


def _pool_unit(kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "plain":                                    # no record twice
        return random_records(rng, 40 + seed % 50, K)
    if kind == "repeats":
        return shuffled(rng, times(random_records(rng, 6 + seed % 5, K), 30))
    if kind == "passes":                                   # more than 3400 distinct k-mers
        return random_records(rng, 172 + seed % 9, K, 20)
    if kind == "long":                                     # more than 2048 records
        return shuffled(rng, times(random_records(rng, 90, K, 4), 23))
    if kind == "sentinels":
        return sentinels(4)
    assert kind == "empty"
    return sentinels(0)


@functools.lru_cache(maxsize=None)
def forty_units(first):
    """40 units of different content.  first = "plain": a unit without repeats first (dedupe = 1: the next 15 units go without the search), then
    heavily repeated units, units of several passes next to units of one, a long unit, an empty unit last; first = "empty": an empty unit first"""
    kinds = ["plain", "repeats", "repeats", "repeats", "passes", "repeats", "passes", "passes", "plain", "long", "empty", "sentinels", "repeats", "passes",
             "repeats", "plain", "repeats", "repeats", "passes", "repeats", "long", "passes", "plain", "repeats", "repeats", "repeats", "passes", "passes",
             "repeats", "plain", "repeats", "repeats", "passes", "repeats", "repeats", "sentinels", "passes", "repeats", "repeats", "empty"]
    if first == "empty":
        kinds = ["empty"] + kinds[:-2] + ["repeats"]
    assert len(kinds) == 40
    inp = Input(K, [_pool_unit(kd, 100 + i) for i, kd in enumerate(kinds)], gap=4 if first == "empty" else 0)
    for kd, u, ln in zip(kinds, inp.ref, inp.plen):
        assert (u.n_all > CR.FILL) == (kd == "passes") and (ln > CR.DD) == (kd == "long") and (ln == 0) == (kd == "empty")
    nz = [u.keys.tobytes() for u in inp.ref if u.n_all]
    assert len(set(nz)) == len(nz) == 36                   # different content: a unit counted twice, skipped or swapped shows
    return inp


def prefix(inp, units):
    out = Input.__new__(Input)
    out.k, out.x, out.y, out.np = inp.k, inp.x, inp.y, units
    out.pstart, out.plen = inp.pstart[:units], inp.plen[:units]
    out.__dict__["ref"] = inp.ref[:units]
    out.__dict__["occ"] = inp.occ[:units]
    return out


GATHER_SIZES = [0, 1, 63, 64, 65, CR.GS_CAP, CR.GS_CAP + 1]


@functools.lru_cache(maxsize=None)
def gather_units():
    """units that keep 0, 1, 63, 64, 65, GS_CAP and GS_CAP + 1 entries at thr = -1 (the last one hashes twice instead of parking its bins), then units
    with counts above 1, the last of them not empty"""
    rng = np.random.default_rng(4096)
    units = [kmer_records(distinct_kmers(d, 500 + d), K) if d else sentinels(4) for d in GATHER_SIZES]
    units += [_pool_unit("repeats", 7), _pool_unit("plain", 8), sentinels(0), shuffled(rng, times(random_records(rng, 30, K), 3))]
    inp = Input(K, units)
    assert [u.n_all for u in inp.ref[:len(GATHER_SIZES)]] == GATHER_SIZES and inp.ref[-1].n_all > 0
    return inp


ALL_BUILDERS = ([lambda k=k: record_shapes(k) for k in range(20, 32)] + [lambda c=c: identical_records(c) for c in IDENTICAL]
                + [lambda m=m, kd=kd: collision_units(m, kd) for m in (1, 3) for kd in ("sorted", "y only", "x only")] + [attempt_that_fails_late]
                + [lambda c=c: long_unit(c) for c in LONG] + [lambda c=c: pressure_unit(c) for c in PRESSURE]
                + [beyond_64_passes, cut_units, lambda: forty_units("plain"), lambda: forty_units("empty"), gather_units])


# ---------------------------------------------------------------------------------------------------------------------------------
# the hook
# ---------------------------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data if a is not None else None


def count_stage(ctx, inp, thr=-1, dedupe=1, dyn=1, grid=2, n_batches=1, room=None, split_bits=-1, bit=0, k=None, pstart=None, plen=None):
    from metafast_amd import lib as L
    so = L.lib()
    fn, info, cp, free = so.mf_debug_skm_count, so.mf_debug_skm_count_info, so.mf_debug_skm_count_copy, so.mf_debug_skm_count_free
    fn.restype = info.restype = cp.restype = C.c_int
    free.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_int] * 6 + [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    info.argtypes = [C.c_void_p, C.c_void_p]
    cp.argtypes = [C.c_void_p] * 9
    free.argtypes = [C.c_void_p]
    rec = np.ascontiguousarray(np.stack([inp.x, inp.y], axis=1))
    ps = np.ascontiguousarray(inp.pstart if pstart is None else pstart, dtype=np.uint64)
    pl = np.ascontiguousarray(inp.plen if plen is None else plen, dtype=np.uint32)
    rm = None if room is None else np.ascontiguousarray(room, dtype=np.uint32)
    h = C.c_void_p()
    L._check(fn(ctx.h, _ptr(rec), len(rec), _ptr(ps), _ptr(pl), len(ps), inp.k if k is None else k, thr, dedupe, dyn, grid, n_batches, _ptr(rm), split_bits, bit, C.byref(h)))
    try:
        v = np.zeros(10, dtype=np.uint64)
        L._check(info(h, v.ctypes.data))
        npart, nlist, overflow, n_all, n_redo, gathered, nd, nfine, launches, n_cu = (int(t) for t in v)
        d = dict(overflow=overflow, n_all=n_all, n_redo=n_redo, gathered=bool(gathered), launches=launches, n_cu=n_cu, dcount=np.zeros(npart, dtype=np.uint32),
                 toff=np.zeros(npart + 1, dtype=np.uint64), tkeys=np.zeros(nlist, dtype=np.uint64), tcnt=np.zeros(nlist, dtype=np.uint16),
                 drop_hist=np.zeros(CR.LH, dtype=np.uint64), dk=np.zeros(nd, dtype=np.uint64), dc=np.zeros(nd, dtype=np.uint16), dfine=np.zeros(nfine, dtype=np.uint64))
        L._check(cp(h, *(_ptr(d[n]) for n in ("dcount", "toff", "tkeys", "tcnt", "drop_hist", "dk", "dc", "dfine"))))
        return d
    finally:
        free(h)


def check(inp, out, thr, dyn, where, skip=()):
    """(a) .. (e) for an input whose units all fit (overflow 0); skip: units left out of (a) and (b)"""
    ref = inp.ref
    dcount, n_all, hist, redo = CR.totals(ref, thr)
    assert out["overflow"] == 0, (where, "overflow", out["overflow"])
    toff = out["toff"].astype(np.int64)
    written = np.zeros(len(out["tkeys"]), dtype=bool)
    for p, u in enumerate(ref):
        if p in skip:
            written[toff[p]:toff[p + 1]] = True
            continue
        assert out["dcount"][p] == dcount[p], (where, f"unit {p}: dcount {out['dcount'][p]}, the reference keeps {dcount[p]} of {u.n_all} k-mers (thr {thr})")
        assert dcount[p] <= toff[p + 1] - toff[p], (where, p)
        s = slice(toff[p], toff[p] + dcount[p])
        got, want = CR.pairs(out["tkeys"][s], out["tcnt"][s]), CR.pairs(*u.kept(thr))
        if not np.array_equal(got, want):
            gs, ws = {tuple(r) for r in got.tolist()}, {tuple(r) for r in want.tolist()}
            raise AssertionError(f"{where}, unit {p} ({inp.plen[p]} records, {u.n_all} distinct k-mers, thr {thr}): {len(gs - ws)} (key, count) pairs not in the reference, e.g. "
                                 f"{[(S.decode(a, inp.k), b) for a, b in sorted(gs - ws)[:3]]}; {len(ws - gs)} missing, e.g. {[(S.decode(a, inp.k), b) for a, b in sorted(ws - gs)[:3]]}")
        written[s] = True
    bad = np.flatnonzero(~written & ((out["tkeys"] != np.uint64(CANARY_KEY)) | (out["tcnt"] != CANARY_CNT)))
    assert not len(bad), (where, f"{len(bad)} list entries written outside the units' kept entries, the first at {bad[0]} (unit starts: {toff[:8].tolist()} ...)")
    assert out["n_all"] == n_all, (where, "n_all", out["n_all"], n_all)
    assert out["n_redo"] == redo, (where, "n_redo", out["n_redo"], redo)
    if dyn and thr >= 0:
        assert np.array_equal(out["drop_hist"].astype(np.int64), hist), (where, "drop_hist", out["drop_hist"][:thr + 2].tolist(), hist[:thr + 2].tolist())
    else:
        assert not out["drop_hist"].any(), where


def check_gather(inp, out, thr, split_bits, bit, where):
    dfine, parts = CR.gather(inp.ref, thr, inp.k, split_bits, bit)
    assert out["gathered"], where
    assert np.array_equal(out["dfine"], dfine), (where, "dfine", np.flatnonzero(out["dfine"] != dfine)[:4].tolist())
    assert len(out["dk"]) == int(dfine[-1]), where
    for t, want in enumerate(parts):
        s = slice(int(dfine[t]), int(dfine[t + 1]))
        got = CR.pairs(out["dk"][s], out["dc"][s])
        assert np.array_equal(got, want), (where, f"table partition {t} (unit {t >> split_bits}, bin {t & ((1 << split_bits) - 1)}): {len(got)} entries, not the reference's")


def run_modes(ctx, inp, where, thr=-1, grids=(2,), modes=MODES, **kw):
    outs = []
    for dedupe, dyn in modes:
        for grid in grids:
            w = f"{where}: thr {thr}, dedupe {dedupe}, dyn {dyn}, grid {grid}, {kw}"
            out = count_stage(ctx, inp, thr=thr, dedupe=dedupe, dyn=dyn, grid=grid, **kw)
            check(inp, out, thr, dyn, w)
            outs.append(out)
    return outs


# ---------------------------------------------------------------------------------------------------------------------------------
# record shapes and extraction
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", range(20, 32))
def test_record_shapes_every_k(gpu_ctx, k):
    run_modes(gpu_ctx, record_shapes(k), f"k = {k}, every n")
    run_modes(gpu_ctx, record_shapes(k), f"k = {k}, every n", thr=2, modes=[(1, 1)])


# ---------------------------------------------------------------------------------------------------------------------------------
# identical records
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", IDENTICAL)
def test_identical_records(gpu_ctx, case):
    inp = identical_records(case)
    run_modes(gpu_ctx, inp, case, grids=(1, 3))
    run_modes(gpu_ctx, inp, case, thr=2, grids=(1,))


@gpu
@pytest.mark.parametrize("kind", ["sorted", "y only", "x only"])
@pytest.mark.parametrize("m", [1, 3])
def test_two_records_with_one_fingerprint(gpu_ctx, m, kind):
    """neither swallows the other, whichever claims the slot"""
    run_modes(gpu_ctx, collision_units(m, kind), f"one fingerprint ({kind}), {m} x each", grids=(1, 3))


@gpu
@pytest.mark.parametrize("case", LONG)
def test_long_units(gpu_ctx, case):
    run_modes(gpu_ctx, long_unit(case), f"long unit: {case}", grids=(1,))
    run_modes(gpu_ctx, long_unit(case), f"long unit: {case}", thr=1, grids=(1,), modes=[(1, 1), (5, 0)])


# ---------------------------------------------------------------------------------------------------------------------------------
# table pressure
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", PRESSURE)
def test_table_pressure(gpu_ctx, case):
    inp = pressure_unit(case)
    outs = run_modes(gpu_ctx, inp, f"table pressure: {case}", grids=(1,))
    want_redo = {"3400": 0, "3401": 1, "4097": 1, "6000": 1, "100000": 1}.get(case, 0)
    assert all(o["n_redo"] == want_redo for o in outs)
    run_modes(gpu_ctx, inp, f"table pressure: {case}", thr=0, grids=(1,), modes=[(1, 1)])


@gpu
@pytest.mark.parametrize("dedupe,dyn", [(0, 0), (1, 1), (5, 1)])
def test_beyond_64_passes_is_overflow_1(gpu_ctx, dedupe, dyn):
    """the workgroup that meets the unit stops there (units 0 and 2 are its own: unit 2 is never written); the other workgroup's units are right"""
    inp = beyond_64_passes()
    out = count_stage(gpu_ctx, inp, thr=-1, dedupe=dedupe, dyn=dyn, grid=2)
    assert out["overflow"] == 1 and out["n_redo"] == 1
    assert out["dcount"][0] == 0 and out["dcount"][2] == 0xFFFFFFFF
    toff = out["toff"].astype(np.int64)
    for p in (1, 3):
        u = inp.ref[p]
        assert out["dcount"][p] == u.n_all
        s = slice(toff[p], toff[p] + u.n_all)
        assert np.array_equal(CR.pairs(out["tkeys"][s], out["tcnt"][s]), CR.pairs(u.keys, u.counts)), p
    assert np.all(out["tkeys"][toff[2]:toff[3]] == np.uint64(CANARY_KEY))


# ---------------------------------------------------------------------------------------------------------------------------------
# cut and histogram
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("thr", THRS)
def test_cut_and_histogram(gpu_ctx, thr):
    """drop_hist, n_all and dcount show each k-mer once, nothing of the abandoned attempts at unit 1"""
    inp = cut_units()
    outs = run_modes(gpu_ctx, inp, "cut", thr=thr, grids=(1, 3))
    assert all(o["n_redo"] == 1 for o in outs)


@gpu
@pytest.mark.parametrize("thr", [-1, 0, 1, 2, 5])
def test_nothing_of_an_attempt_that_failed_after_a_good_pass(gpu_ctx, thr):
    """"What a failed attempt tallied is not committed": neither its entries, nor its share of n_all, nor its dropped counts"""
    outs = run_modes(gpu_ctx, attempt_that_fails_late(), "four passes fail in the second", thr=thr, grids=(1, 2))
    assert all(o["n_redo"] == 1 for o in outs)


# ---------------------------------------------------------------------------------------------------------------------------------
# the room guard
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("grid", [1, 3])
def test_room_guard_is_overflow_2(gpu_ctx, grid, last):
    rng = np.random.default_rng(2)
    units = [random_records(rng, 60, K), random_records(rng, 10, K, 20), random_records(rng, 2, K, 5)]
    inp = Input(K, units[:2] if last else units)
    assert inp.ref[1].n_all == 200
    room = inp.occ.copy()
    room[1] = 50
    for dedupe, dyn in MODES:
        out = count_stage(gpu_ctx, inp, thr=-1, dedupe=dedupe, dyn=dyn, grid=grid, room=room)
        where = f"room 50 for 200 entries, grid {grid}, dedupe {dedupe}, dyn {dyn}"
        assert out["overflow"] == 2, where
        toff = out["toff"].astype(np.int64)
        assert toff[2] - toff[1] == 50 and len(out["tkeys"]) >= toff[-1] + 150
        # the neighbours: complete and correct; behind them and behind the unit's room nothing but the fill
        ok = np.zeros(len(out["tkeys"]), dtype=bool)
        for p in [q for q in range(inp.np) if q != 1]:
            u = inp.ref[p]
            assert out["dcount"][p] == u.n_all, (where, p)
            s = slice(toff[p], toff[p] + u.n_all)
            assert np.array_equal(CR.pairs(out["tkeys"][s], out["tcnt"][s]), CR.pairs(u.keys, u.counts)), (where, p)
            ok[s] = True
        ok[toff[1]:toff[2]] = True
        assert np.all(out["tkeys"][~ok] == np.uint64(CANARY_KEY)) and np.all(out["tcnt"][~ok] == CANARY_CNT), where
        # what the unit did write inside its room is its own
        mine = out["tkeys"][toff[1]:toff[2]]
        mine = mine[mine != np.uint64(CANARY_KEY)]
        assert np.all(np.isin(mine, inp.ref[1].keys)) and len(np.unique(mine)) == len(mine), where


# ---------------------------------------------------------------------------------------------------------------------------------
# unit hand-out and the unit loop
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("units", [1, 2, 3, 4, 6, 7, 9, 10, 40])
@pytest.mark.parametrize("grid", [1, 2, 3])
def test_unit_hand_out(gpu_ctx, grid, units):
    """both sides of "the first three units by stride, every further one claimed three ahead" """
    inp = prefix(forty_units("plain"), units)
    run_modes(gpu_ctx, inp, f"{units} units on {grid} workgroups", thr=1, grids=(grid,))


@gpu
@pytest.mark.parametrize("first", ["plain", "empty"])
def test_forty_units_on_one_workgroup(gpu_ctx, first):
    inp = forty_units(first)
    for thr in (-1, 1):
        one = run_modes(gpu_ctx, inp, f"40 units, {first} first", thr=thr, grids=(1,))
        three = run_modes(gpu_ctx, inp, f"40 units, {first} first", thr=thr, grids=(1,), n_batches=3)
        assert all(o["launches"] == 1 for o in one) and all(o["launches"] == 3 for o in three)
        for a, b in zip(one, three):
            assert np.array_equal(a["dcount"], b["dcount"]) and a["n_all"] == b["n_all"] and a["n_redo"] == b["n_redo"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the gathers
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("split_bits", [0, 1, 2, 3, 4])
def test_gather(gpu_ctx, split_bits):
    """S = 1: k_gather_split, else k_gather_split_n; the bits sit where a plan of 10 counting bits puts them, and at the top of the hash"""
    bit10 = 31 - 10 if split_bits == 1 else min(31, 32 - 10 - split_bits)
    for inp, name in ((gather_units(), "sizes"), (prefix(forty_units("plain"), 14), "14 units")):
        for bit in (bit10, 32 - split_bits if split_bits else 31, 0):
            for thr, n_batches, grid, mode in ((-1, 1, 2, (1, 1)), (-1, 3, 3, (0, 1)), (1, 3, 1, (5, 0))):
                where = f"gather {name}: S {split_bits}, bit {bit}, thr {thr}, {n_batches} batches"
                out = count_stage(gpu_ctx, inp, thr=thr, dedupe=mode[0], dyn=mode[1], grid=grid, n_batches=n_batches, split_bits=split_bits, bit=bit)
                check(inp, out, thr, mode[1], where)
                check_gather(inp, out, thr, split_bits, bit, where)


# ---------------------------------------------------------------------------------------------------------------------------------
# the hook itself
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_hook_refuses_malformed_input_and_launches_nothing(gpu_ctx):
    from metafast_amd import lib as L
    rng = np.random.default_rng(1)
    inp = Input(K, [random_records(rng, 30, K), random_records(rng, 30, K)])
    gpu_ctx.set_option("profile", 1)
    try:
        check(inp, count_stage(gpu_ctx, inp), -1, 1, "a well-formed input")
        before = gpu_ctx.kernel_time("k_skm_count")[0]
        assert before >= 1

        def refused(match, **kw):
            bad = kw.pop("inp", inp)
            with pytest.raises(L.MetafastError, match=match):
                count_stage(gpu_ctx, bad, **kw)
        ps, pl = inp.pstart, inp.plen
        refused("inside or in front", pstart=ps[::-1].copy())                                # not ascending
        refused("inside or in front", pstart=np.array([0, pl[0] - 4], dtype=np.uint64))      # not disjoint
        refused("leaves the buffer", pstart=np.array([0, len(inp.x) - 4], dtype=np.uint64))
        refused("multiple of 4", plen=np.array([pl[0] - 1, pl[1]], dtype=np.uint32))
        for n in (0, S.rmax(K) + 1, 62):
            bad = Input(K, [random_records(rng, 8, K)])
            bad.y[3] = (bad.y[3] & ~np.uint64(63)) | np.uint64(n)
            refused("has n =", inp=bad)
        bad = Input(K, [random_records(rng, 8, K)])
        bad.x[2] &= np.uint64(0xFFFFFFFF)                                                    # n = 63 but not all ones
        bad.y[2] |= np.uint64(63)
        refused("has n = 63", inp=bad)
        bad = Input(K, [random_records(rng, 8, K, 3)])
        bad.y[5] |= np.uint64(1 << 28)                                                       # a bit behind the last base (33 bases)
        refused("behind its last base", inp=bad)
        bad = Input(K, [random_records(rng, 8, K, 1)])
        bad.x[5] |= np.uint64(1)                                                             # 31 bases: x bits 0 and 1 are behind them
        refused("behind its last base", inp=bad)
        refused("thr =", thr=CR.LH)
        refused("thr =", thr=-2)
        refused("k =", k=19)
        refused("k =", k=32)
        refused("grid =", grid=0)
        refused("grid =", grid=2 * count_stage(gpu_ctx, inp)["n_cu"] + 1)
        refused("n_batches", n_batches=0)
        refused("dyn =", dyn=2)
        refused("split_bits", split_bits=5, bit=0)
        refused("split_bits", split_bits=4, bit=29)
        assert gpu_ctx.kernel_time("k_skm_count")[0] == before + 1                           # (the one good call that asked for the CUs)
        check(inp, count_stage(gpu_ctx, inp), -1, 1, "a well-formed input, afterwards")
    finally:
        gpu_ctx.set_option("profile", 0)
