"""The count stage of the super-k-mer path (metafast_amd/csrc/mf_skm_count.h: k_skm_count, k_gather_split, k_gather_split_n) restated in plain
numpy for tests/test_skm_count_units_gpu.py, on top of tests/skm_ref.py (the record) and tests/nbr_ref.py (canonical form, partition hash).
The rule is stated per counting unit, from the records the unit holds:

    k-mers      the forward k-mers of the unit's valid records (an all-ones sentinel holds none), each folded to min(forward, reverse complement)
    count       occurrences of a folded k-mer in the unit, at most MAX_COUNT
    n_all       the distinct k-mers of the unit, before the cut
    kept        the entries with count > thr, in no particular order: dcount = how many
    drop_hist   drop_hist[c] = the entries with count c <= thr
    gather      an entry of unit p goes to table partition (p << S) + ((part_hash(key) >> bit) & (2^S - 1)); dfine = where every table
                partition starts in the dense table (units in order, bins in order), dfine[np << S] = its size; no order inside a partition

Nothing here follows the kernel's way of getting there: no table, no items, no passes, no weights.  tests/test_skm_count_ref_cpu.py pins this
file to the oracle's table.

The three small hashes at the end (c2_slot, rec_fingerprint, pass_of) restate the kernel's own.  They serve ONLY to construct adversarial
inputs and to check on the CPU that an input has the property it is meant to have; no expected output is computed with them."""
import numpy as np

import nbr_ref as R
import skm_ref as S

_U = np.uint64
_M32 = _U(0xFFFFFFFF)
MAX_COUNT = 32767                  # MF_MAX_COUNT
LH = 64                            # C2_LH: bins of drop_hist (thr < LH)
FILL = 3400                        # C2_FILL: a unit with more distinct k-mers is counted again in several passes
SLOTS = 4096                       # C2_SLOTS
DD = 2048                          # C2_DD * SKM_CT: the records of a unit the search for identical records covers
MAX_PASSES = 64                    # SKM_MAX_PASSES
GS_CAP = 4096                      # k_gather_split_n parks the bins of a unit of up to this many entries


class Unit:
    """what one unit must come to: keys ascending with their counts (before the cut)"""

    def __init__(self, keys, counts):
        self.keys, self.counts = keys, counts

    @property
    def n_all(self):
        return len(self.keys)

    def kept(self, thr):
        m = self.counts > thr
        return self.keys[m], self.counts[m]

    def dropped_hist(self, thr):
        h = np.zeros(LH, dtype=np.int64)
        if thr >= 0:
            d = self.counts[self.counts <= thr]
            h[:thr + 1] = np.bincount(d, minlength=thr + 1)
        return h


def count_unit(x, y, k):
    """the records of one unit (sentinels among them) -> Unit"""
    x, y = np.asarray(x, dtype=np.uint64), np.asarray(y, dtype=np.uint64)
    v = ~S.is_sentinel(x, y)
    km, _ = S.record_kmers(x[v], y[v], k)
    keys, counts = np.unique(R.canonical(km, k), return_counts=True)
    return Unit(keys.astype(np.uint64), np.minimum(counts, MAX_COUNT).astype(np.int64))


def count_units(x, y, pstart, plen, k):
    return [count_unit(x[int(s):int(s) + int(n)], y[int(s):int(s) + int(n)], k) for s, n in zip(pstart, plen)]


def totals(units, thr):
    """-> dcount [np], n_all, drop_hist [LH], the units counted in several passes (more than FILL distinct k-mers)"""
    dcount = np.array([len(u.kept(thr)[0]) for u in units], dtype=np.int64)
    hist = np.zeros(LH, dtype=np.int64)
    for u in units:
        hist += u.dropped_hist(thr)
    return dcount, sum(u.n_all for u in units), hist, sum(u.n_all > FILL for u in units)


def gather(units, thr, k, S_bits, bit):
    """-> dfine [(np << S) + 1], and per table partition the (key, count) pairs in ascending order"""
    nb = 1 << S_bits
    dfine = [0]
    parts = []
    for u in units:
        keys, counts = u.kept(thr)
        b = ((R.part_hash(keys, k) >> _U(bit)) & _U(nb - 1)).astype(np.int64)
        for j in range(nb):
            m = b == j
            parts.append(np.stack([keys[m], counts[m].astype(np.uint64)], axis=1))
            dfine.append(dfine[-1] + int(m.sum()))
    return np.array(dfine, dtype=np.uint64), parts


def pairs(keys, counts):
    """(key, count) pairs in ascending order, [n, 2] uint64: equal multisets <=> equal arrays"""
    keys, counts = np.asarray(keys, dtype=np.uint64), np.asarray(counts).astype(np.uint64)
    o = np.lexsort((counts, keys))
    return np.stack([keys[o], counts[o]], axis=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel's hashes, restated for the input builders only
# ---------------------------------------------------------------------------------------------------------------------------------
def _rotr(v, r):
    v = np.asarray(v, dtype=np.uint64) & _M32
    return ((v >> _U(r)) | (v << _U(32 - r))) & _M32


def c2_slot(keys):
    """home slot of a k-mer in the LDS table"""
    keys = np.asarray(keys, dtype=np.uint64)
    hi, lo = keys >> _U(32), keys & _M32
    x = lo ^ _rotr(hi, 19)
    x ^= x >> _U(15)
    t = ((x & _U(0xFFFFFF)) * _U(0x9E3779)) & _M32
    return ((t >> _U(11)) & _U(SLOTS - 1)).astype(np.int64)


def rec_fingerprint(x, y):
    """the 32-bit fingerprint of a record in the search for identical records (the digit field, y bits 6 .. 27, is left out): slot = its low 12
    bits, tag = its bits 11 .. 31"""
    x, y = np.asarray(x, dtype=np.uint64), np.asarray(y, dtype=np.uint64)
    ym = y & ~_U(((1 << S.DIGIT_BITS) - 1) << 6)
    h = (x >> _U(32)) ^ _rotr(x & _M32, 11) ^ _rotr(ym >> _U(32), 21) ^ _rotr(ym & _M32, 5)
    h ^= h >> _U(16)
    h = (h * _U(0x9E3779B1)) & _M32
    return h ^ (h >> _U(15))


def pass_of(keys):
    """a k-mer of a unit counted in P passes is inserted in pass pass_of & (P - 1)"""
    keys = np.asarray(keys, dtype=np.uint64)
    g = (((keys >> _U(32)) * _U(0xC2B2AE35)) ^ ((keys & _M32) * _U(0x27D4EB2F))) & _M32
    g ^= g >> _U(15)
    g = (g * _U(0x165667B1)) & _M32
    return (g >> _U(24)).astype(np.int64)
