"""The stages of the wide record path (metafast_amd/csrc/mf_wskm.hip: k_wskm_scan, the partition sort with k_wskm_offsets and k_wskm_units,
k_wskm_pack, k_wskm_count, mf_wide_order) restated in numpy and Python ints for tests/test_wskm_stages_gpu.py.  The rules are stated from the
base stream, position by position; nothing here is shared with the kernels' way of getting there (packed tiles in LDS, minima over windows of
7, ballots, rolling 128-bit registers, LDS tables, leading-bit runs).  tests/test_wskm_ref_cpu.py pins this file to the oracle's table.

    position      p counts the bases of the concatenated buffer (all reads one after the other)
    start         p is a k-mer start if it lies inside a read of len >= max(k, min_len), at most len - k from the read's start (skm_ref.valid_starts)
    minimizer     of the k-mer at p: the smallest mmer_hash(min(fwd, rc)) over its W = k - 14 15-mers (nbr_ref.mmer_hash; skm_ref.minimizer_hashes)
    run           starts where p is a start and p - 1 is not a start, or the hash differs from p - 1's, or p % 4096 == 0 (a tile of the scan); it goes
                  on over the starts that follow until the next run start or a position that is no start
    record        starts at every multiple of 48 (RMAX) from its run's start and holds min(48, rest of the run) k-mers
    words         w[0..6]: the 112 bases from p as they lie in the buffer, two bits each (A G C T = 0 1 2 3), the first in the top bits of w[0]; they
                  run on into whatever follows the record (the next read), code 0 behind the buffer's end.  w[7] = the number of k-mers
    partition     remix32(hash) >> (32 - pbits), 0 when pbits = 0; pbits is the smallest number with (n_occ >> pbits) <= the occurrences of a partition
    sort          the records' numbers in ascending order of their partitions; poff[q] = the first place whose partition is >= q (a search)
    units         G = max(8, int(max(unit, 64) * n_rec / n_occ)) records; uoff[j] = the first partition border at or behind j G, uoff[last] = n_rec;
                  uoff = poff when option wide_skm_merge is 0 or pbits is 0
    pack          per window of 1024 records in sorted order every class of identical 8-word records keeps ONE member with w[7] = len | size << 8, the
                  others get w[7] = 0.  Which member stays is a race: windows are compared as multisets
    count         the canonical 2k-bit k-mers of a list of records, each with its record's weight, cut by count > thr, clamped to 32767
    order         Python's sorted() on (hi << 64) | lo; an entry is SET ASIDE when more than 64 entries share its leading 32 bits"""
import numpy as np

import nbr_ref as R
import skm_ref as S

_U = np.uint64
TILE = 4096
HALO = 128
RMAX = 48
REC_BASES = 112
WINDOW = 1024
FILL = 2800                        # distinct k-mers a unit may hold before it is counted class by class
ORDER_RUN = 64
MAX_COUNT = 32767


class Scan:
    """what the cut rule needs of one input: base codes, k-mer starts, minimizer hashes"""

    def __init__(self, bases, off, k, min_len=0):
        assert 32 <= k <= 63 and R.mmer_len(k) == 15
        self.k = k
        self.code = S.base_codes(bases)
        self.valid = S.valid_starts(off, k, min_len)
        assert len(self.valid) == len(self.code)
        self.mh = S.minimizer_hashes(self.code, k)
        self.n_occ = int(self.valid.sum())

    def runs(self):
        """-> (start positions, lengths in k-mers), ascending"""
        pos = np.flatnonzero(self.valid)
        if not len(pos):
            return pos, pos
        first = np.ones(len(pos), dtype=bool)
        first[1:] = (np.diff(pos) != 1) | (self.mh[pos[1:]] != self.mh[pos[:-1]]) | (pos[1:] % TILE == 0)
        at = np.flatnonzero(first)
        return pos[at], np.diff(np.append(at, len(pos)))

    def records(self):
        """-> (start, n) of every record, ascending by position"""
        return S.cut_rmax(*self.runs(), RMAX)


def pbits_of(n_occ, unit=2400, fine=8, merge=1):
    per_part = max(64, unit // max(1, fine)) if merge else max(256, unit)
    b = 0
    while b < 28 and (n_occ >> b) > per_part:
        b += 1
    return b


def record_words(code, start, n):
    """-> uint32 [records, 8]"""
    start = np.asarray(start, dtype=np.int64)
    c = np.zeros(len(code) + REC_BASES, dtype=np.uint32)
    c[:len(code)] = code
    b = c[start[:, None] + np.arange(REC_BASES)[None, :]]
    w = np.zeros((len(start), 8), dtype=np.uint32)
    for i in range(REC_BASES):
        w[:, i // 16] |= b[:, i] << np.uint32(30 - 2 * (i % 16))
    w[:, 7] = np.asarray(n, dtype=np.uint32)
    return w


def partition(mh, pbits):
    mh = np.asarray(mh, dtype=np.uint64)
    return (R.remix32(mh) >> _U(32 - pbits)).astype(np.uint32) if pbits else np.zeros(len(mh), dtype=np.uint32)


def offsets(part_sorted, pbits):
    return np.searchsorted(part_sorted, np.arange((1 << pbits) + 1), side="left").astype(np.uint64)


def units(poff, n_rec, n_occ, pbits, unit=2400, merge=1):
    """-> uoff"""
    if not merge or not pbits:
        return poff.copy()
    G = max(8, int(float(max(unit, 64)) * float(n_rec) / float(n_occ)))
    nu = (n_rec + G - 1) // G
    first = np.searchsorted(poff, np.arange(nu, dtype=np.uint64) * _U(G), side="left")       # the first partition that starts at or behind j G
    return np.append(poff[first], _U(n_rec)).astype(np.uint64)


def rows_sorted(rows):
    """rows of words in ascending order: equal multisets <=> equal arrays"""
    rows = np.asarray(rows)
    return rows[np.lexsort(rows.T[::-1])] if len(rows) else rows


def pack(rows):
    """records [n, 8] in sorted order -> what k_wskm_pack may leave of them, every window's rows in ascending order (rows_sorted)"""
    out = np.empty_like(rows)
    for a in range(0, len(rows), WINDOW):
        w = rows[a:a + WINDOW]
        cls, size = np.unique(w, axis=0, return_counts=True)
        keep = cls.copy()
        keep[:, 7] = cls[:, 7] | (size.astype(np.uint32) << np.uint32(8))
        gone = np.repeat(cls, size - 1, axis=0)
        gone[:, 7] = 0
        out[a:a + WINDOW] = rows_sorted(np.concatenate([keep, gone]))
    return out


def windows_sorted(rows):
    out = np.empty_like(rows)
    for a in range(0, len(rows), WINDOW):
        out[a:a + WINDOW] = rows_sorted(rows[a:a + WINDOW])
    return out


def canonical_at(code, pos, k):
    """the canonical k-mers that start at the positions pos -> (hi, lo) uint64: hi = the bases in front of the last 32, lo = the last 32"""
    pos = np.asarray(pos, dtype=np.int64)
    n = len(code)

    def at(c, p):
        hi = S.windows(c, k - 32)[p] if k > 32 else np.zeros(len(p), dtype=np.uint64)
        return hi, S.windows(c, 32)[p + (k - 32)]
    fh, fl = at(code, pos)
    rh, rl = at((3 - code[::-1]).astype(code.dtype), n - pos - k)       # the other strand's k-mer of p starts at n - p - k of the turned buffer
    fwd = (fh < rh) | ((fh == rh) & (fl <= rl))
    return np.where(fwd, fh, rh), np.where(fwd, fl, rl)


def record_kmers(rows, k):
    """records as words -> (hi, lo) of their canonical k-mers one record after the other, the record each belongs to, its weight (w[7] >> 8, 0 = 1).
    Plain: base by base out of the words, the other strand by turning the bases round"""
    rows = np.asarray(rows, dtype=np.uint32)
    n = (rows[:, 7] & np.uint32(0xFF)).astype(np.int64)
    wgt = (rows[:, 7] >> np.uint32(8)).astype(np.int64)
    wgt[wgt == 0] = 1
    b = np.empty((len(rows), REC_BASES), dtype=np.uint64)
    for i in range(REC_BASES):
        b[:, i] = (rows[:, i // 16] >> np.uint32(30 - 2 * (i % 16))) & np.uint32(3)
    r = int(n.max()) if len(n) else 0
    assert r + k - 1 <= REC_BASES
    fh = np.zeros((len(rows), r), dtype=np.uint64); fl = fh.copy(); rh = fh.copy(); rl = fh.copy()
    for i in range(k):                                     # base i of the k-mer; base i of the other strand = 3 - base k - 1 - i
        f, t = b[:, i:i + r], _U(3) - b[:, k - 1 - i:k - 1 - i + r]
        if i < k - 32:
            fh = (fh << _U(2)) | f; rh = (rh << _U(2)) | t
        else:
            fl = (fl << _U(2)) | f; rl = (rl << _U(2)) | t
    fwd = (fh < rh) | ((fh == rh) & (fl <= rl))
    m = np.arange(r)[None, :] < n[:, None]
    rec = np.repeat(np.arange(len(rows)), n)
    return np.where(fwd, fh, rh)[m], np.where(fwd, fl, rl)[m], rec, wgt[rec]


def count(hi, lo, wgt=None, thr=0):
    """occurrences (with weights) -> (hi, lo, cnt int32) of the distinct k-mers with count > thr, ascending, clamped; the distinct k-mers before the cut"""
    hi, lo = np.asarray(hi, dtype=np.uint64), np.asarray(lo, dtype=np.uint64)
    if not len(hi):
        return hi, lo, np.zeros(0, dtype=np.int32), 0
    w = np.ones(len(hi), dtype=np.int64) if wgt is None else np.asarray(wgt, dtype=np.int64)
    o = np.lexsort((lo, hi))
    hi, lo, w = hi[o], lo[o], w[o]
    first = np.ones(len(hi), dtype=bool)
    first[1:] = (hi[1:] != hi[:-1]) | (lo[1:] != lo[:-1])
    at = np.flatnonzero(first)
    c = np.add.reduceat(w, at)
    keep = c > thr
    return hi[at][keep], lo[at][keep], np.minimum(c[keep], MAX_COUNT).astype(np.int32), len(at)


def distinct_per_group(hi, lo, group, n_groups):
    """distinct (hi, lo) per group -> int64 [n_groups]"""
    o = np.lexsort((lo, hi, group))
    hi, lo, g = np.asarray(hi)[o], np.asarray(lo)[o], np.asarray(group)[o]
    first = np.ones(len(g), dtype=bool)
    first[1:] = (g[1:] != g[:-1]) | (hi[1:] != hi[:-1]) | (lo[1:] != lo[:-1])
    return np.bincount(g[first], minlength=n_groups).astype(np.int64)


class Stages:
    """the reference's run of one input with one set of options: records, partitions, units and what the count must say"""

    def __init__(self, sc, unit=2400, fine=8, merge=1):
        self.sc = sc
        self.pbits = pbits_of(sc.n_occ, unit, fine, merge)
        self.start, self.n = sc.records()
        self.n_rec = len(self.start)
        self.part = partition(sc.mh[self.start], self.pbits)
        self.order = np.argsort(self.part, kind="stable")                        # (the kernels' order inside a partition is another one)
        self.poff = offsets(self.part[self.order], self.pbits)
        self.uoff = units(self.poff, self.n_rec, sc.n_occ, self.pbits, unit, merge)
        self._occ = None

    def words(self):
        return record_words(self.sc.code, self.start, self.n)

    def occurrences(self):
        """-> (hi, lo) of every occurrence's canonical k-mer, the unit that counts it"""
        if self._occ is None:
            pos = np.flatnonzero(self.sc.valid)
            hi, lo = canonical_at(self.sc.code, pos, self.sc.k)
            p = partition(self.sc.mh[pos], self.pbits).astype(np.int64)
            self._occ = hi, lo, np.searchsorted(self.uoff, self.poff[p], side="right") - 1      # (the last unit that starts at or before the partition: the one that is not empty)
        return self._occ

    def overflowing_units(self):
        hi, lo, unit = self.occurrences()
        return int((distinct_per_group(hi, lo, unit, len(self.uoff) - 1) > FILL).sum())

    def table(self, thr=0):
        hi, lo, _ = self.occurrences()
        return count(hi, lo, None, thr)


def order(hi, lo, cnt):
    """entries in any order -> ascending, by Python's sorted() on whole k-mers"""
    e = sorted(((int(h) << 64) | int(x), int(c)) for h, x, c in zip(hi, lo, cnt))
    return (np.array([v >> 64 for v, _ in e], dtype=np.uint64), np.array([v & 0xFFFFFFFFFFFFFFFF for v, _ in e], dtype=np.uint64),
            np.array([c for _, c in e], dtype=np.uint16))


def lead_runs(hi, lo, k):
    """the lengths of the runs of equal leading 32 bits (of the 2k), in ascending order of those bits"""
    lead = sorted((((int(h) << 64) | int(x)) >> (2 * k - 32)) for h, x in zip(hi, lo))
    out, i = [], 0
    while i < len(lead):
        j = i
        while j < len(lead) and lead[j] == lead[i]:
            j += 1
        out.append(j - i)
        i = j
    return out


def aside(hi, lo, k):
    return sum(r for r in lead_runs(hi, lo, k) if r > ORDER_RUN)
