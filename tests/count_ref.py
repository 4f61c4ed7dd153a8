"""The one-record-per-k-mer counting path (metafast_amd/csrc/mf_count.hip: K0 k_mask_init / k_mask_reads, K1 k_l1_hist / k_scan / k_l1_scatter,
K2 k_split, K3 k_count, the table) restated in plain numpy for tests/test_count_stages_gpu.py.  Every rule is stated from the reads, position by
position, after the comments and definitions of that file; nothing here is shared with the kernels' way of getting there (clearing bit ranges
per read, a rolling reverse complement over 32-position words, staging lines in LDS, an open-addressed table).  tests/test_count_ref_cpu.py
pins this file to the oracle's table and shows that check() bites.

    bitmap        bit p (bit p % 32 of word p / 32) is set iff p lies in a read of length >= max(k, min_len) and p <= end - k; bits at and
                  beyond n_bases are clear; n_occ = the set bits
    k-mer         of a set position: the k bases from it, two bits each (A G C T = 0 1 2 3, either case), the first in the highest of the 2 k
                  bits; canonical = the smaller of it and its reverse complement
    hash          h = (x ^ (x >> 31)) * 0x9E3779B97F4A7C15 mod 2^64 (mf_phash)
    digit         of level i with `bits` bits behind `bits_used` bits of earlier levels: bits [64 - bits_used - bits, 64 - bits_used) of h
    level 1       workgroup g of G takes the words [g * wpb, (g + 1) * wpb), wpb = ceil(n_words / G); region (d, g) of the level-1 buffer
                  holds the k-mers of digit d that start in g's words, then all-ones sentinels up to a multiple of 8; the regions follow
                  each other in the order d * G + g from 0
    a K2 level    partition p (start, len of the level in front) gets room from start + p * 8 * nd on (nd = 2^bits); sub-region b holds p's
                  keys of digit b, padded with sentinels to a multiple of 8
    K3            keys[start .. start + dcount) = the distinct k-mers of the partition, cnt = min(occurrences, 32767)
    table         d_part_off = exclusive scan of dcount; part_bits = the plan's bits when they are 1 .. 30, else 0 and no offsets

A snapshot is a dict (test_count_stages_gpu.snapshot builds it from the hook, model() here from the reference): stage, n_words, n_occ, B, G, wpb,
staged, lv, vmask, blockhist, blockstart, buf1, pstart1, plen1, levels [bits_used, bits, buf, ostart, olen], keys, cnt, dcount, pstart, plen,
overflow, part_bits, n_dist, part_off, dk, dc.  Buffers a stage writes only in part are filled with 0xA5 bytes in front of it."""
import numpy as np

import nbr_ref as R

_U = np.uint64
EMPTY = 0xFFFFFFFFFFFFFFFF
FILL = 0xA5A5A5A5A5A5A5A5
FILL16 = 0xA5A5
LINE = 8
MAX_COUNT = 32767
MAX_DIGIT_BITS = 11
COUNT_SLOTS = 4096
PREFETCH = 3072                    # keys of a partition k_count holds in registers; the rest comes straight from HBM
PHASH_MULT = 0x9E3779B97F4A7C15
ALPHABET = "AGCT"


def base_codes(bases):
    """ASCII (either case) -> 0 .. 3"""
    lut = np.zeros(256, dtype=np.uint8)
    for i, c in enumerate(ALPHABET):
        lut[ord(c)] = lut[ord(c.lower())] = i
    return lut[np.asarray(bases, dtype=np.uint8)]


def encode(s):
    v = 0
    for ch in s.upper():
        v = (v << 2) | ALPHABET.index(ch)
    return v


def valid_starts(off, n_bases, k, min_len=0):
    """-> bool [n_bases]"""
    off = np.asarray(off).astype(np.int64)
    v = np.zeros(n_bases, dtype=bool)
    for s, e in zip(off[:-1].tolist(), off[1:].tolist()):
        if e - s >= max(k, min_len):
            v[s:e - k + 1] = True
    return v


def pack_bitmap(valid):
    """bool [n] -> uint32 [ceil(n / 32)], bit p % 32 of word p / 32"""
    n_words = (len(valid) + 31) // 32
    v = np.zeros(n_words * 32, dtype=np.uint8)
    v[:len(valid)] = valid
    w = (v.reshape(n_words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    return w.astype(np.uint32)


def kmers_at(code, pos, k):
    """the forward k-mer that starts at each position of pos"""
    pos = np.asarray(pos, dtype=np.int64)
    x = np.zeros(len(pos), dtype=np.uint64)
    c = code.astype(np.uint64)
    for i in range(k):
        x = (x << _U(2)) | c[pos + i]
    return x


def phash(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return (x ^ (x >> _U(31))) * _U(PHASH_MULT)


def digit(h, bits_used, bits):
    """bits [64 - bits_used - bits, 64 - bits_used) of h"""
    h = np.asarray(h, dtype=np.uint64)
    if bits == 0:
        return np.zeros(h.shape, dtype=np.int64)
    return ((h >> _U(64 - bits_used - bits)) & _U((1 << bits) - 1)).astype(np.int64)


def roundup8(x):
    return (np.asarray(x).astype(np.int64) + 7) // 8 * 8


def ceil_log2(x):
    b = 0
    while (1 << b) < x:
        b += 1
    return b


def plan_levels(n_occ, n_reads, n_bases, k, min_len, l1_bits, l2_bits, part_target, part_target_long=256):
    """(levels, B) of a forced plan (option l1_bits >= 0), after mf_count_plan's comments: partitions are sized by k-mer occurrences,
    part_target of them -- part_target_long for assembled sequences (mean length >= 8 k, or a caller that filters by length); level 1 takes
    l1_bits, the rest (l2_bits, or what B leaves) goes in levels of at most 11 bits"""
    assert l1_bits >= 0
    target = part_target
    if (n_bases // n_reads >= 8 * k or min_len > 0) and target > part_target_long:
        target = part_target_long
    B = ceil_log2((n_occ + target - 1) // target)
    lv = [l1_bits]
    rest = l2_bits if l2_bits >= 0 else max(0, B - l1_bits)
    while rest > 0:
        lv.append(min(rest, MAX_DIGIT_BITS))
        rest -= lv[-1]
    return lv, B


def level1_blocks(n_words, l1_blocks, n_cu):
    """(G, words per workgroup): l1_blocks workgroups (0: one per CU), at most ceil(n_words / 1024) -- a word per thread at least"""
    G = max(1, min(l1_blocks if l1_blocks > 0 else n_cu, (n_words + 1023) // 1024))
    return G, (n_words + G - 1) // G


class Reference:
    """what the rules need of one input: the bitmap, and position, canonical k-mer and hash of every set bit"""

    def __init__(self, bases, off, k, min_len=0):
        off = np.asarray(off).astype(np.int64)
        self.k, self.min_len = k, min_len
        self.n_reads = len(off) - 1
        self.n_bases = int(off[-1]) if len(off) else 0
        self.n_words = (self.n_bases + 31) // 32
        self.valid = valid_starts(off, self.n_bases, k, min_len)
        self.vmask = pack_bitmap(self.valid)
        self.pos = np.flatnonzero(self.valid)
        self.n_occ = len(self.pos)
        code = base_codes(np.asarray(bases, dtype=np.uint8)[:self.n_bases])
        self.keys = R.canonical(kmers_at(code, self.pos, k), k)
        self.hash = phash(self.keys)

    def table(self):
        """(ascending distinct canonical k-mers, min(occurrences, 32767))"""
        u, c = np.unique(self.keys, return_counts=True)
        return u, np.minimum(c, MAX_COUNT).astype(np.int32)

    def block_of(self, wpb):
        return (self.pos // 32) // wpb

    def partition_after(self, lv, levels):
        """the partition of every occurrence behind the first `levels` levels of the plan: its digits, one after the other"""
        p = np.zeros(self.n_occ, dtype=np.int64)
        used = 0
        for b in lv[:levels]:
            p = p * (1 << b) + digit(self.hash, used, b)
            used += b
        return p

    def final_sets(self, lv):
        """(partition, k-mer, clamped count) of the distinct k-mers, ascending by (partition, k-mer)"""
        p = self.partition_after(lv, len(lv))
        o = np.lexsort((self.keys, p))
        pk = np.stack([p[o].astype(np.uint64), self.keys[o]], axis=1)
        if not len(pk):
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64)
        first = np.concatenate([[True], np.any(pk[1:] != pk[:-1], axis=1)])
        idx = np.flatnonzero(first)
        c = np.diff(np.concatenate([idx, [len(pk)]]))
        return pk[idx, 0].astype(np.int64), pk[idx, 1], np.minimum(c, MAX_COUNT)


# ---------------------------------------------------------------------------------------------------------------------------------
# check
# ---------------------------------------------------------------------------------------------------------------------------------
def _fail(stage, msg):
    raise AssertionError(f"{stage}: {msg}")


def _flat(starts, lens):
    """regions -> (region of every entry, its place inside the region, its index in the buffer)"""
    starts, lens = np.asarray(starts).astype(np.int64), np.asarray(lens).astype(np.int64)
    rid = np.repeat(np.arange(len(lens)), lens)
    within = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
    return rid, within, np.repeat(starts, lens) + within


def _check_regions(stage, buf, starts, lens, counts, want_rid, want_keys, name):
    """region r = buf[starts[r] .. + lens[r]) holds counts[r] keys, the reference's multiset (want_rid, want_keys), then sentinels only;
    everything outside the regions is 0xA5 fill"""
    starts, lens, counts = np.asarray(starts).astype(np.int64), np.asarray(lens).astype(np.int64), np.asarray(counts).astype(np.int64)
    bad = np.flatnonzero((starts < 0) | (starts + lens > len(buf)))
    if len(bad):
        _fail(stage, f"region {name(bad[0])} = [{starts[bad[0]]}, + {lens[bad[0]]}) leaves the buffer of {len(buf)} entries")
    rid, within, idx = _flat(starts, lens)
    vals = buf[idx]
    iskey = within < np.repeat(counts, lens)
    for sel, what in ((~iskey & (vals != _U(EMPTY)), "where a sentinel belongs"), (iskey & (vals == _U(FILL)), "0xA5 fill left inside the region, among its keys"),
                      (iskey & (vals == _U(EMPTY)), "a sentinel among the region's keys")):
        bad = np.flatnonzero(sel)
        if len(bad):
            j = bad[0]
            v = int(vals[j])
            note = " (0xA5 fill left inside the region)" if v == FILL and not iskey[j] else ""
            _fail(stage, f"region {name(rid[j])} = [{starts[rid[j]]}, + {lens[rid[j]]}) with {counts[rid[j]]} keys, entry {within[j]}: {v:#018x} {what}{note} ({len(bad)} such entries)")
    kr, kv = rid[iskey], vals[iskey]
    o = np.lexsort((kv, kr))
    wo = np.lexsort((want_keys, want_rid))
    got, want = kv[o], np.asarray(want_keys, dtype=np.uint64)[wo]
    if len(got) != len(want):
        _fail(stage, f"the regions hold {len(got)} keys, the reference {len(want)}")
    bad = np.flatnonzero(got != want)
    if len(bad):
        j = bad[0]
        _fail(stage, f"region {name(kr[o][j])} does not hold the reference's multiset: it has {int(got[j]):#x} where the reference has {int(want[j]):#x} "
                     f"(both ascending; {len(bad)} entries differ)")
    covered = np.zeros(len(buf), dtype=bool)
    covered[idx] = True
    if covered.sum() != len(idx):
        _fail(stage, "regions overlap")
    bad = np.flatnonzero(~covered & (buf != _U(FILL)))
    if len(bad):
        _fail(stage, f"entry {bad[0]} outside every region was written: {int(buf[bad[0]]):#018x} ({len(bad)} such entries, 0xA5 fill expected)")


def _region_keys(buf, starts, lens):
    """(region, key) of the entries of the regions that are no sentinels, ascending"""
    rid, _, idx = _flat(starts, lens)
    v = buf[idx]
    m = v != _U(EMPTY)
    o = np.lexsort((v[m], rid[m]))
    return rid[m][o], v[m][o]


def check_k0(snap, ref):
    st = "K0"
    if snap["stage"] == 0:
        if ref.n_reads and ref.n_bases:
            _fail(st, "no bitmap although the input has reads and bases")
        return
    if snap["n_words"] != ref.n_words or len(snap["vmask"]) != ref.n_words:
        _fail(st, f"{snap['n_words']} words ({len(snap['vmask'])} copied), the reference has {ref.n_words}")
    bad = np.flatnonzero(snap["vmask"] != ref.vmask)
    if len(bad):
        w = int(bad[0])
        _fail(st, f"vmask[{w}] = {int(snap['vmask'][w]):#010x}, the reference has {int(ref.vmask[w]):#010x} (positions {32 * w} .. {32 * w + 31}; {len(bad)} words differ: {bad[:8].tolist()})")
    if snap["n_occ"] != ref.n_occ:
        _fail(st, f"n_occ = {snap['n_occ']}, the bitmap has {ref.n_occ} bits set")


def check_k1(snap, ref):
    st = "K1"
    lv, G, wpb = snap["lv"], snap["G"], snap["wpb"]
    nd1 = 1 << lv[0]
    if wpb != (ref.n_words + G - 1) // G:
        _fail(st, f"{wpb} words per workgroup for {ref.n_words} words on {G} workgroups")
    rid = digit(ref.hash, 0, lv[0]) * G + ref.block_of(wpb)
    hist = np.bincount(rid, minlength=nd1 * G)
    bh, bs = snap["blockhist"].astype(np.int64), snap["blockstart"].astype(np.int64)
    if len(bh) != nd1 * G or len(bs) != nd1 * G + 1:
        _fail(st, f"histogram of {len(bh)} entries, {len(bs)} region starts for {nd1} digits x {G} workgroups")
    bad = np.flatnonzero(bh != hist)
    if len(bad):
        i = int(bad[0])
        _fail(st, f"histogram: blockhist[{i // G} * G + {i % G}] = {bh[i]}, the reference counts {hist[i]} ({len(bad)} entries differ)")
    if bs[0] != 0 or np.any(bs % LINE) or np.any(np.diff(bs) < 0):
        _fail(st, "blockstart does not start at 0, is not ascending, or has an entry that is no multiple of 8")
    bad = np.flatnonzero(np.diff(bs) != roundup8(hist))
    if len(bad):
        i = int(bad[0])
        _fail(st, f"region ({i // G}, {i % G}) has room for {bs[i + 1] - bs[i]} entries, its {hist[i]} keys ask for {roundup8(hist[i])}")
    if snap["n_occ"] + LINE * nd1 * G != len(snap["buf1"]):
        _fail(st, f"the level-1 buffer has {len(snap['buf1'])} entries, n_occ + 8 * digits * G = {snap['n_occ'] + LINE * nd1 * G}")
    _check_regions(st, snap["buf1"], bs[:-1], np.diff(bs), hist, rid, ref.keys, lambda r: f"(digit {r // G}, workgroup {r % G})")
    ps, pl = snap["pstart1"].astype(np.int64), snap["plen1"].astype(np.int64)
    if len(ps) != nd1 or not np.array_equal(ps, bs[:-1:G]) or not np.array_equal(pl, bs[G::G] - bs[:-1:G]):
        _fail(st, "pstart / plen do not span the digits' regions")


def check_k2(snap, ref, li, buf_in, ps_in, pl_in):
    st = f"K2 level {li}"
    lv = snap["lv"]
    L = snap["levels"][li - 1]
    bits, used = L["bits"], L["bits_used"]
    if bits != lv[li] or used != sum(lv[:li]):
        _fail(st, f"{bits} bits behind {used}, the plan {lv} says {lv[li]} behind {sum(lv[:li])}")
    nd, np_in = 1 << bits, len(ps_in)
    if len(L["ostart"]) != np_in * nd or len(L["olen"]) != np_in * nd:
        _fail(st, f"{len(L['ostart'])} sub-regions for {np_in} partitions x {nd} digits")
    if len(L["buf"]) != len(buf_in) + np_in * LINE * nd:
        _fail(st, f"the level's buffer has {len(L['buf'])} entries, the one in front {len(buf_in)} + 8 * {nd} * {np_in} partitions")
    p_in = ref.partition_after(lv, li)
    rid = p_in * nd + digit(ref.hash, used, bits)
    counts = np.bincount(rid, minlength=np_in * nd)
    os_, ol = L["ostart"].astype(np.int64).reshape(np_in, nd), L["olen"].astype(np.int64).reshape(np_in, nd)
    bad = np.flatnonzero(ol.ravel() != roundup8(counts))
    if len(bad):
        i = int(bad[0])
        _fail(st, f"olen[{i // nd} * nd + {i % nd}] = {ol.ravel()[i]}, roundup8 of the reference's {counts[i]} keys is {roundup8(counts[i])} ({len(bad)} differ)")
    obase = ps_in + np.arange(np_in, dtype=np.int64) * (LINE * nd)
    if np.any(os_ % LINE):
        _fail(st, "a sub-region does not start at a multiple of 8")
    bad = np.flatnonzero((os_[:, 0] < obase) | np.any(os_[:, 1:] < os_[:, :-1] + ol[:, :-1], axis=1) | (os_[:, -1] + ol[:, -1] > obase + pl_in + LINE * nd))
    if len(bad):
        p = int(bad[0])
        _fail(st, f"the sub-regions of partition {p} are not ascending and disjoint inside [{obase[p]}, {obase[p] + pl_in[p] + LINE * nd}): they start at {os_[p].tolist()[:9]} ...")
    _check_regions(st, L["buf"], os_.ravel(), ol.ravel(), counts, rid, ref.keys, lambda r: f"(partition {r // nd}, digit {r % nd})")
    # the union over the digits is the partition's input
    gi, ki = _region_keys(buf_in, ps_in, pl_in)
    go, ko = _region_keys(L["buf"], os_.ravel(), ol.ravel())
    o = np.lexsort((ko, go // nd))
    if len(ki) != len(ko) or not np.array_equal(gi, (go // nd)[o]) or not np.array_equal(ki, ko[o]):
        _fail(st, "the sub-regions of a partition do not add up to the partition's input")
    return L["buf"], os_.ravel(), ol.ravel()


def check_k3(snap, ref, buf_in, ps_in, pl_in):
    st = "K3"
    lv = snap["lv"]
    npart = len(ps_in)
    if not np.array_equal(snap["pstart"].astype(np.int64), ps_in) or not np.array_equal(snap["plen"].astype(np.int64), pl_in):
        _fail(st, "k_count's directory is not the last level's")
    if snap["overflow"]:
        _fail(st, f"the overflow word is {snap['overflow']}")
    wp, wk, wc = ref.final_sets(lv)
    want_d = np.bincount(wp, minlength=npart)
    dc = snap["dcount"].astype(np.int64)
    bad = np.flatnonzero(dc != want_d) if len(dc) == npart else np.array([0])
    if len(bad):
        p = int(bad[0])
        _fail(st, f"dcount[{p}] = {dc[p] if len(dc) == npart else None}, partition {p} has {want_d[p]} distinct k-mers ({len(bad)} partitions differ)")
    keys, cnt = snap["keys"], snap["cnt"]
    if len(keys) != len(buf_in) or len(cnt) != len(buf_in):
        _fail(st, f"{len(keys)} keys, {len(cnt)} counts behind k_count, {len(buf_in)} entries in front")
    rid, _, idx = _flat(ps_in, dc)
    o = np.lexsort((keys[idx], rid))
    gk, gc = keys[idx][o], cnt[idx][o].astype(np.int64)
    bad = np.flatnonzero(gk != wk)
    if len(bad):
        j = int(bad[0])
        _fail(st, f"partition {rid[o][j]}: keys[start .. start + dcount) is not the set of its distinct k-mers: {int(gk[j]):#x} where the reference has {int(wk[j]):#x} (ascending)")
    bad = np.flatnonzero(gc != wc)
    if len(bad):
        j = int(bad[0])
        _fail(st, f"partition {rid[o][j]}, k-mer {int(gk[j]):#x}: cnt = {gc[j]}, min(occurrences, 32767) = {wc[j]} ({len(bad)} counts differ)")
    written = np.zeros(len(keys), dtype=bool)
    written[idx] = True
    bad = np.flatnonzero(~written & (cnt != np.uint16(FILL16)))
    if len(bad):
        _fail(st, f"cnt[{bad[0]}] = {int(cnt[bad[0]])} outside every [start, start + dcount) ({len(bad)} such entries, 0xA5 fill expected)")
    bad = np.flatnonzero(~written & (keys != buf_in))
    if len(bad):
        _fail(st, f"keys[{bad[0]}] outside every [start, start + dcount) is not what the level in front left there ({len(bad)} such entries)")
    return wp, wk, wc, want_d


def check_table(snap, ref, wp, wk, wc, want_d):
    st = "table"
    total_bits = sum(snap["lv"])
    npart = len(want_d)
    if snap["n_dist"] != len(wk) or len(snap["dk"]) != len(wk) or len(snap["dc"]) != len(wk):
        _fail(st, f"{snap['n_dist']} entries ({len(snap['dk'])} keys, {len(snap['dc'])} counts), the reference has {len(wk)}")
    off = np.concatenate([[0], np.cumsum(want_d)])
    if 1 <= total_bits <= 30:
        if snap["part_bits"] != total_bits:
            _fail(st, f"part_bits = {snap['part_bits']}, the plan has {total_bits} bits")
        po = snap["part_off"].astype(np.int64)
        bad = np.flatnonzero(po != off) if len(po) == npart + 1 else np.array([0])
        if len(bad):
            p = int(bad[0])
            _fail(st, f"d_part_off[{p}] = {po[p] if len(po) == npart + 1 else None}, the exclusive scan of dcount gives {off[p]} ({len(po)} entries for {npart} partitions)")
    elif snap["part_bits"] != 0 or len(snap["part_off"]):
        _fail(st, f"part_bits = {snap['part_bits']} with {len(snap['part_off'])} offsets for a plan of {total_bits} bits (no partition structure is kept then)")
    rid = np.repeat(np.arange(npart), want_d)
    o = np.lexsort((snap["dk"], rid))
    if not np.array_equal(snap["dk"][o], wk) or not np.array_equal(snap["dc"][o].astype(np.int64), wc):
        _fail(st, "a partition of the table is not the set k_count left for it")
    o = np.argsort(snap["dk"], kind="stable")
    tk, tc = ref.table()
    if not np.array_equal(snap["dk"][o], tk) or not np.array_equal(snap["dc"][o].astype(np.int32), tc):
        _fail(st, "the exported table is not the reference's")


def check(snap, ref, expect_overflow=False):
    """(a) K0, (b) K1, (c) every K2 level, (d) K3, (e) the table: bit-exact, an AssertionError that starts with the stage's name otherwise.
    expect_overflow: the count ended with `k_count: LDS table overflow` -- (a) to (c), then the overflow word must be set"""
    check_k0(snap, ref)
    if ref.n_occ == 0:
        if snap["stage"] > 1 or snap["n_dist"] or len(snap["dk"]) or len(snap["buf1"]) or len(snap["keys"]) or snap["levels"]:
            _fail("table", "no k-mer occurrence, but the snapshot is not empty")
        return
    if snap["stage"] != (4 if expect_overflow else 5):
        _fail("K1", f"the snapshot ends at stage {snap['stage']}")
    check_k1(snap, ref)
    cur = (snap["buf1"], snap["pstart1"].astype(np.int64), snap["plen1"].astype(np.int64))
    if len(snap["levels"]) != len(snap["lv"]) - 1:
        _fail("K2 level 1", f"{len(snap['levels'])} K2 levels for the plan {snap['lv']}")
    for li in range(1, len(snap["lv"])):
        cur = check_k2(snap, ref, li, *cur)
    if expect_overflow:
        if not snap["overflow"]:
            _fail("K3", "the overflow word is not set")
        return
    check_table(snap, ref, *check_k3(snap, ref, *cur))


# ---------------------------------------------------------------------------------------------------------------------------------
# a snapshot from the reference itself
# ---------------------------------------------------------------------------------------------------------------------------------
def _place(buf, starts, lens, rid, keys):
    """regions of sentinels, the keys of region r from its start on (in the order given)"""
    _, _, idx = _flat(starts, lens)
    buf[idx] = _U(EMPTY)
    o = np.argsort(rid, kind="stable")
    r = rid[o]
    first = np.searchsorted(r, r, side="left")
    buf[np.asarray(starts).astype(np.int64)[r] + (np.arange(len(r)) - first)] = keys[o]


def model(ref, lv, G, staged=1, B=0):
    """the snapshot of a count that does what the rules say, laid out as compactly as they allow"""
    s = dict(stage=0, n_words=0, n_occ=0, B=B, G=0, wpb=0, staged=staged, lv=[], vmask=np.zeros(0, dtype=np.uint32), blockhist=np.zeros(0, dtype=np.uint32),
             blockstart=np.zeros(0, dtype=np.uint64), buf1=np.zeros(0, dtype=np.uint64), pstart1=np.zeros(0, dtype=np.uint64), plen1=np.zeros(0, dtype=np.uint32),
             levels=[], keys=np.zeros(0, dtype=np.uint64), cnt=np.zeros(0, dtype=np.uint16), dcount=np.zeros(0, dtype=np.uint32), pstart=np.zeros(0, dtype=np.uint64),
             plen=np.zeros(0, dtype=np.uint32), overflow=0, part_bits=0, n_dist=0, part_off=np.zeros(0, dtype=np.uint64), dk=np.zeros(0, dtype=np.uint64),
             dc=np.zeros(0, dtype=np.uint16))
    if not ref.n_reads or not ref.n_bases:
        return s
    s.update(stage=1, n_words=ref.n_words, n_occ=ref.n_occ, vmask=ref.vmask.copy())
    if not ref.n_occ:
        return s
    wpb = (ref.n_words + G - 1) // G
    nd1 = 1 << lv[0]
    rid = digit(ref.hash, 0, lv[0]) * G + ref.block_of(wpb)
    hist = np.bincount(rid, minlength=nd1 * G)
    bs = np.concatenate([[0], np.cumsum(roundup8(hist))])
    buf = np.full(ref.n_occ + LINE * nd1 * G, FILL, dtype=np.uint64)
    _place(buf, bs[:-1], np.diff(bs), rid, ref.keys)
    ps, pl = bs[:-1:G].copy(), bs[G::G] - bs[:-1:G]
    s.update(stage=5, lv=list(lv), G=G, wpb=wpb, blockhist=hist.astype(np.uint32), blockstart=bs.astype(np.uint64), buf1=buf, pstart1=ps.astype(np.uint64),
             plen1=pl.astype(np.uint32))
    used = lv[0]
    for li in range(1, len(lv)):
        nd, np_in = 1 << lv[li], len(ps)
        rid = ref.partition_after(lv, li) * nd + digit(ref.hash, used, lv[li])
        ol = roundup8(np.bincount(rid, minlength=np_in * nd)).reshape(np_in, nd)
        os_ = (ps + np.arange(np_in) * LINE * nd)[:, None] + np.cumsum(ol, axis=1) - ol
        buf = np.full(len(buf) + np_in * LINE * nd, FILL, dtype=np.uint64)
        _place(buf, os_.ravel(), ol.ravel(), rid, ref.keys)
        s["levels"].append(dict(bits_used=used, bits=lv[li], buf=buf, ostart=os_.ravel().astype(np.uint64), olen=ol.ravel().astype(np.uint32)))
        ps, pl = os_.ravel(), ol.ravel()
        used += lv[li]
    wp, wk, wc = ref.final_sets(lv)
    dcount = np.bincount(wp, minlength=len(ps))
    keys, cnt = buf.copy(), np.full(len(buf), FILL16, dtype=np.uint16)
    _, _, idx = _flat(ps, dcount)
    keys[idx], cnt[idx] = wk, wc.astype(np.uint16)
    s.update(keys=keys, cnt=cnt, dcount=dcount.astype(np.uint32), pstart=ps.astype(np.uint64), plen=pl.astype(np.uint32), n_dist=len(wk), dk=wk.copy(),
             dc=wc.astype(np.uint16))
    if 1 <= sum(lv) <= 30:
        s.update(part_bits=sum(lv), part_off=np.concatenate([[0], np.cumsum(dcount)]).astype(np.uint64))
    return s
