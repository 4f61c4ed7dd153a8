"""The super-k-mer records of the counting path (metafast_amd/csrc/mf_skm_scatter.h: S1 k_skm_hist, S2 k_skm_scatter; mf_skm_split.h: S3 k_skm_split) restated in
plain numpy for tests/test_skm_records_gpu.py.  The rule is stated from the reads, position by position; nothing here is shared with the
kernels' way of getting there (rolling reverse complements, a three-input sliding minimum, halo words from the next lane, run lists in LDS).
tests/test_skm_ref_cpu.py pins this file to the oracle's table and to tests/nbr_ref.py.

    valid start   a position inside a read of len >= max(k, min_len), at most len - k from the read's start
    minimizer     of a k-mer: the smallest mmer_hash(min(fwd, rc)) over its k - M + 1 M-mers (M = 13 for k <= 25, else 15)
    run           consecutive valid starts of one read with EQUAL minimizer hash (hashes are compared, not positions)
    RMAX          min(50 - (k - 1), 20) k-mers in a record
    exact form    a run is cut at every position of the base stream that is a multiple of 32 (a word of the scan), every piece is cut greedily
                  into records of at most RMAX k-mers from its start
    one-pass form a piece that ends at a word's last position takes up to min(head, RMAX - tail, 49 - k) k-mers of the next word's first piece
                  (head, tail: their lengths) when both have the same hash -- but not where the next word is the first of a wave's batch of 63
                  words, and not in a batch that holds a piece of more than RMAX k-mers or more than 384 pieces (that batch is cut as in the
                  exact form)
    record        n k-mers = n + k - 1 bases, two bits each (A G C T = 0 1 2 3, the project's order: mf_dec4), the first in the top bits of x; bases 32 .. 49 in the top 36
                  bits of y; every other base bit zero; y bits 6 .. 27 = ((ph << bits1) & 0xFFFFFFFF) >> 10 with ph = remix32(minimizer hash),
                  bits1 = the bits of level 1; y bits 0 .. 5 = n (63: a sentinel, all 128 bits set)
    partition     with B = the sum of the levels' bits: (ph >> (32 - B)) - (dlo << (B - bits1)) for a slice that starts at level-1 digit dlo"""
import numpy as np

import nbr_ref as R

_U = np.uint64
BASES = 50
DIGIT_BITS = 22
SENTINEL_N = 63
WAVE_WORDS = 63                    # words of a wave's batch (lane 63 only lends its word to lane 62)
WAVES = 16
LIST_CAP = 384                     # pieces a wave's batch can list
ALPHABET = "AGCT"                  # base codes 0 .. 3 (nbr_ref.encode / decode spell k-mer VALUES with another alphabet: not for reads)


def encode(s):
    v = 0
    for ch in s.upper():
        v = (v << 2) | ALPHABET.index(ch)
    return v


def decode(x, k):
    x = int(x)
    return "".join(ALPHABET[(x >> (2 * (k - 1 - i))) & 3] for i in range(k))


def rmax(k):
    return min(BASES - (k - 1), 20)


def base_codes(bases):
    """ASCII (either case) -> 0 .. 3"""
    lut = np.zeros(256, dtype=np.uint8)
    for i, c in enumerate(ALPHABET):
        lut[ord(c)] = lut[ord(c.lower())] = i
    return lut[np.asarray(bases, dtype=np.uint8)]


def valid_starts(off, k, min_len=0):
    """-> bool [n_bases]"""
    off = np.asarray(off).astype(np.int64)
    v = np.zeros(int(off[-1]) if len(off) else 0, dtype=bool)
    lens = np.diff(off)
    for s, ln in zip(off[:-1][lens >= max(k, min_len)], lens[lens >= max(k, min_len)]):
        v[s:s + ln - k + 1] = True
    return v


def windows(code, k):
    """the k-mer that starts at each position, uint64 [n]; 0 where fewer than k bases follow"""
    n = len(code)
    out = np.zeros(n, dtype=np.uint64)
    if n >= k:
        w = n - k + 1
        x = np.zeros(w, dtype=np.uint64)
        c = code.astype(np.uint64)
        for i in range(k):
            x = (x << _U(2)) | c[i:i + w]
        out[:w] = x
    return out


def minimizer_hashes(code, k):
    """the minimizer hash of the k-mer that starts at each position, uint64 [n] (32-bit values; meaningless where no k-mer fits)"""
    M = R.mmer_len(k)
    n = len(code)
    f = windows(code, M)
    h = R.mmer_hash(np.minimum(f, R.revcomp(f, M)), M)
    out = np.full(n, 0xFFFFFFFF, dtype=np.uint64)
    if n >= k:
        w = n - k + 1
        best = h[:w].copy()
        for j in range(1, k - M + 1):
            best = np.minimum(best, h[j:j + w])
        out[:w] = best
    return out


class Scan:
    """what the rule needs of one input: base codes, valid starts, minimizer hashes"""

    def __init__(self, bases, off, k, min_len=0):
        self.k = k
        self.code = base_codes(bases)
        self.valid = valid_starts(off, k, min_len)
        self.mh = minimizer_hashes(self.code, k)
        self.kmers = windows(self.code, k)

    def occurrences(self):
        """the forward k-mer of every valid start, sorted: the multiset the records must hold"""
        return np.sort(self.kmers[self.valid])

    def pieces(self, word_cut):
        """runs (word_cut: cut at the multiples of 32) -> (start positions, lengths), ascending"""
        v, mh = self.valid, self.mh
        pos = np.flatnonzero(v)
        if not len(pos):
            return pos, pos
        first = np.ones(len(pos), dtype=bool)
        first[1:] = (np.diff(pos) != 1) | (mh[pos[1:]] != mh[pos[:-1]])
        if word_cut:
            first |= (pos % 32) == 0
        at = np.flatnonzero(first)
        return pos[at], np.diff(np.append(at, len(pos)))

    def ideal_count(self):
        _, ln = self.pieces(False)
        r = rmax(self.k)
        return int(((ln + r - 1) // r).sum())

    def exact(self):
        """-> (start, n) of every record of the exact form"""
        return cut_rmax(*self.pieces(True), rmax(self.k))

    def one_pass(self, words_per_block):
        """-> (start, n) of every record of the one-pass form with the FAST scatter (words_per_block: the words of a workgroup)"""
        k, r = self.k, rmax(self.k)
        ps, pl = self.pieces(True)
        if not len(ps):
            return ps, pl
        word = ps // 32
        rel = word % words_per_block
        batch = (word // words_per_block) * (words_per_block // WAVE_WORDS + 1) + rel // WAVE_WORDS      # the wave's batch a piece belongs to
        lane = rel % WAVE_WORDS
        head = np.zeros(len(ps), dtype=bool)               # first piece of a word that goes on the piece before it
        head[1:] = ((ps[1:] % 32) == 0) & (ps[:-1] + pl[:-1] == ps[1:]) & (self.mh[ps[1:]] == self.mh[ps[:-1]]) & (lane[1:] > 0)
        tail = np.zeros(len(ps), dtype=np.int64)
        tail[1:] = pl[:-1]
        ext = np.where(head, np.minimum(pl, np.clip(np.minimum(r - tail, 49 - k), 0, None)), 0)
        nb = int(batch.max()) + 1
        long_piece = np.bincount(batch, weights=(pl > r), minlength=nb) > 0
        listed = np.bincount(batch, minlength=nb) - np.bincount(batch, weights=(ext > 0) & (ext == pl), minlength=nb)
        fast = (~long_piece & (listed <= LIST_CAP))[batch]
        ext = np.where(fast, ext, 0)
        start = ps + ext
        ln = pl - ext
        ln[:-1] += ext[1:]
        keep = ln > 0
        assert np.all(ln[fast] <= r)
        s1, n1 = start[keep & fast], ln[keep & fast]
        s2, n2 = cut_rmax(start[keep & ~fast], ln[keep & ~fast], r)
        s, n = np.concatenate([s1, s2]), np.concatenate([n1, n2])
        o = np.argsort(s, kind="stable")
        return s[o], n[o]


def cut_rmax(ps, pl, r):
    """pieces -> records of at most r k-mers, greedily from each piece's start"""
    cnt = (pl + r - 1) // r
    which = np.repeat(np.arange(len(ps)), cnt)
    j = np.arange(len(which)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return ps[which] + j * r, np.minimum(r, pl[which] - j * r)


def encode_records(code, start, n, mh, k, bits1):
    """records of n k-mers from position start, of a run with minimizer hash mh -> (x, y) uint64 arrays"""
    start, n = np.asarray(start, dtype=np.int64), np.asarray(n, dtype=np.int64)
    i = np.arange(BASES)
    keep = i[None, :] < (n + k - 1)[:, None]
    c = np.where(keep, code[np.minimum(start[:, None] + i[None, :], len(code) - 1)], 0).astype(np.uint64)
    x = np.zeros(len(start), dtype=np.uint64)
    y = np.zeros(len(start), dtype=np.uint64)
    for b in range(32):
        x |= c[:, b] << _U(62 - 2 * b)
    for b in range(32, BASES):
        y |= c[:, b] << _U(62 - 2 * (b - 32))
    y |= (digit_field(mh, bits1) << _U(6)) | n.astype(np.uint64)
    return x, y


def digit_field(mh, bits1):
    ph = R.remix32(mh)
    return ((ph << _U(bits1)) & _U(0xFFFFFFFF)) >> _U(32 - DIGIT_BITS)


def partition_of(mh, bits1, total_bits, dlo=0):
    ph = R.remix32(mh).astype(np.int64)
    return (ph >> (32 - total_bits)) - (dlo << (total_bits - bits1))


def rec_n(y):
    return (np.asarray(y, dtype=np.uint64) & _U(63)).astype(np.int64)


def rec_digits(y):
    return (np.asarray(y, dtype=np.uint64) >> _U(6)) & _U((1 << DIGIT_BITS) - 1)


def is_sentinel(x, y):
    return (np.asarray(x, dtype=np.uint64) == _U(0xFFFFFFFFFFFFFFFF)) & (np.asarray(y, dtype=np.uint64) == _U(0xFFFFFFFFFFFFFFFF))


def junk_bits(x, y, k):
    """the base bits behind each record's last base, (from x, from y): zero in a well-formed record"""
    x, y = np.asarray(x, dtype=np.uint64), np.asarray(y, dtype=np.uint64)
    nb = rec_n(y) + k - 1
    ones = _U(0xFFFFFFFFFFFFFFFF)
    bx = np.clip(64 - 2 * nb, 0, 64)                        # unused low bits of x
    by = np.clip(64 - 2 * (nb - 32), 28, 64)                # unused low bits of y, down to the digit field
    mx = np.where(bx >= 64, ones, (_U(1) << np.minimum(bx, 63).astype(np.uint64)) - _U(1))
    my = np.where(by >= 64, ones, (_U(1) << np.minimum(by, 63).astype(np.uint64)) - _U(1)) & ~_U((1 << 28) - 1)
    return x & mx, y & my


def record_kmers(x, y, k):
    """-> (forward k-mers of all records one after another, uint64; the record each belongs to)"""
    x, y = np.asarray(x, dtype=np.uint64), np.asarray(y, dtype=np.uint64)
    n = rec_n(y)
    c = np.empty((len(x), BASES), dtype=np.uint64)
    for b in range(32):
        c[:, b] = (x >> _U(62 - 2 * b)) & _U(3)
    for b in range(32, BASES):
        c[:, b] = (y >> _U(62 - 2 * (b - 32))) & _U(3)
    r = BASES - k + 1
    km = np.zeros((len(x), r), dtype=np.uint64)
    for i in range(k):
        km = (km << _U(2)) | c[:, i:i + r]
    m = np.arange(r)[None, :] < n[:, None]
    return km[m], np.repeat(np.arange(len(x)), np.minimum(n, r))


def decode_record(x, y, k):
    """one record -> (n, digit field, its forward k-mers as strings)"""
    km, _ = record_kmers(np.array([x], dtype=np.uint64), np.array([y], dtype=np.uint64), k)
    return int(rec_n(y)), int(rec_digits(y)), [decode(v, k) for v in km]


def sorted_pairs(x, y):
    """records as 128-bit values in ascending order, [n, 2]: equal multisets <=> equal arrays"""
    x, y = np.asarray(x, dtype=np.uint64), np.asarray(y, dtype=np.uint64)
    o = np.lexsort((y, x))
    return np.stack([x[o], y[o]], axis=1)
