"""The neighbour look-up of the k = 32 ... 63 tables (metafast_amd/csrc/mf_wgraph.hip: k_windex_build, w_side_walk / w_neighbours, k_w_ut_flags,
k_w_cc_adjacency, k_w_lookup; mf_wide.h: mf_windex_find) for its tests: a numpy port of the index hash, and the crafted tables of
tests/test_wnbr_gpu.py.

What is EXPECTED of the kernels never comes from the port: neighbours, flags and palindromes are ut_ref._neighbours_wide / ut_ref.flags (a
neighbour by a shift, its canonical form by a full reverse complement, its place from a dictionary), look-up values come from a dictionary.
The port (hash64 ... whash_key, home_tag) only says WHERE the index must keep a k-mer -- the index invariants of the GPU test -- and lets a
case be built for a place in the index: sixteen k-mers in one cluster, two interiors with one tag and one home slot, a cluster that runs over
the end of the index.  tests/test_wnbr_ref_cpu.py pins the port and asserts, from the reference alone, that every table has the property it was
made for.

A k-mer is a Python int with two bits per base, the first base in the highest of its 2 k bits, complement = 3 - code; the library prints code
c as "AGCT"[c], and so does everything here.  Arrays of k-mers are (hi, lo) pairs of uint64."""
import functools
import json
import os

import numpy as np

import nbr_ref as NR
import ut_ref as UR

_U = np.uint64
M64 = (1 << 64) - 1
KS = (32, 33, 34, 47, 62, 63)   # 32: the high word is 0 everywhere; 33: it holds the first base only; 34, 62: even (palindromes); 47: a middle case; 63: the widest
MIN_CAP = 1024                  # mf_wgraph.hip: mf_windex_build, "uint64_t cap = 1024; while (cap < 2 * n) cap <<= 1;"
EMPTY = 0xFFFFFFFFFFFFFFFF      # mf_wide.h: MF_WIDX_EMPTY
NONE = UR.NONE
MAX_COUNT = UR.MAX_COUNT
COLLISIONS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wnbr_collisions.json")
NUC = "AGCT"


# ---------------------------------------------------------------------------------------------------------------------------------
# the index hash (mf_common.h: mf_hash64; mf_wide.h: mf_whash, mf_whash_interior, mf_whash_key), on uint64 arrays
# ---------------------------------------------------------------------------------------------------------------------------------
def hash64(x):
    x = np.array(x, dtype=np.uint64, ndmin=1)
    x ^= x >> _U(33); x *= _U(0xff51afd7ed558ccd)
    x ^= x >> _U(33); x *= _U(0xc4ceb9fe1a85ec53)
    x ^= x >> _U(33)
    return x


def whash(hi, lo):
    hi, lo = np.array(hi, dtype=np.uint64, ndmin=1), np.array(lo, dtype=np.uint64, ndmin=1)
    return hash64((lo * _U(0x9E3779B97F4A7C15)) ^ hi)


def _shr(hi, lo, s):
    """(hi, lo) >> s, 0 <= s < 128"""
    if s == 0:
        return hi, lo
    if s >= 64:
        return np.zeros_like(hi), hi >> _U(s - 64)
    return hi >> _U(s), (lo >> _U(s)) | (hi << _U(64 - s))


def _low(hi, lo, bits):
    """the low `bits` bits of (hi, lo), bits <= 128"""
    if bits >= 64:
        return hi & _U((1 << (bits - 64)) - 1), lo
    return np.zeros_like(hi), lo & _U((1 << bits) - 1)


def revcomp(hi, lo, nb):
    """reverse complement of nb-base strings (nb <= 64) on whole words: either word turned round and complemented, the words swapped, the
    128 - 2 nb bits that were above the string dropped (held against ut_ref.rc_plain in the CPU test)"""
    hi, lo = np.array(hi, dtype=np.uint64, ndmin=1), np.array(lo, dtype=np.uint64, ndmin=1)
    return _shr(NR.revcomp(lo, 32), NR.revcomp(hi, 32), 128 - 2 * nb)


def _less(ahi, alo, bhi, blo):
    return (ahi < bhi) | ((ahi == bhi) & (alo < blo))


def canonical(hi, lo, nb):
    rhi, rlo = revcomp(hi, lo, nb)
    sw = _less(rhi, rlo, hi, lo)
    return np.where(sw, rhi, hi), np.where(sw, rlo, lo)


def whash_interior(whi, wlo, rhi, rlo):
    """the hash of the smaller of an interior and its reverse complement"""
    sw = _less(rhi, rlo, whi, wlo)
    return whash(np.where(sw, rhi, whi), np.where(sw, rlo, wlo))


def whash_key(hi, lo, k):
    """the hash the index keeps a k-mer under: that of its canonical interior, its middle k - 2 bases"""
    hi, lo = np.array(hi, dtype=np.uint64, ndmin=1), np.array(lo, dtype=np.uint64, ndmin=1)
    whi, wlo = _low(*_shr(hi, lo, 2), 2 * k - 4)
    rchi, rclo = revcomp(hi, lo, k)
    rhi, rlo = _low(*_shr(rchi, rclo, 2), 2 * k - 4)
    return whash_interior(whi, wlo, rhi, rlo)


def home_tag(h, cap):
    """-> (home slot in an index of `cap` slots, tag)"""
    h = np.asarray(h, dtype=np.uint64)
    return (h & _U(cap - 1)).astype(np.int64), (h >> _U(32)).astype(np.int64)


def cap_of(n):
    """slots of the index over n k-mers (0: none is built)"""
    if n == 0:
        return 0
    cap = MIN_CAP
    while cap < 2 * n:
        cap <<= 1
    return cap


def split(keys):
    """list of ints -> (hi, lo) uint64"""
    lo, hi = UR.split_words(keys)
    return hi, lo


def hash_of_keys(keys, k):
    return whash_key(*split(keys), k)


def hash_of_interior(w, k):
    """the port's hash of ONE interior ((k - 2)-base int, canonical or not)"""
    hi, lo = split([w])
    return int(whash(*canonical(hi, lo, k - 2))[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# k-mers as ints
# ---------------------------------------------------------------------------------------------------------------------------------
def bases(x, k):
    return "".join(NUC[(int(x) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def codes(s):
    return [NUC.index(c) for c in s]


def canon(x, k):
    return min(x, UR.rc_plain(x, k))


def interior(x, k):
    return (x >> 2) & ((1 << (2 * k - 4)) - 1)


def rand_int(rng, bits):
    return int.from_bytes(rng.bytes(16), "little") & ((1 << bits) - 1)


def join(a, w, b, k):
    """the k-mer a + w + b of an interior w of k - 2 bases"""
    return (a << (2 * k - 2)) | (w << 2) | b


def fan(w, k):
    """all sixteen a + w + b as read: {(a, b): k-mer}"""
    return {(a, b): join(a, w, b, k) for a in range(4) for b in range(4)}


def random_canonical(rng, k, count, avoid=()):
    out, seen = [], set(avoid)
    while len(out) < count:
        x = canon(rand_int(rng, 2 * k), k)
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# a crafted table
# ---------------------------------------------------------------------------------------------------------------------------------
class WTab:
    """name, k, keys (distinct canonical ints, ascending), counts (1 .. MAX_COUNT), note: what a case wants to be found again (interiors, chosen
    k-mers).  Everything expected of the kernels hangs here, computed once, never changed."""

    def __init__(self, name, k, kmers, seed, note=None):
        self.name, self.k = name, k
        self.keys = sorted({canon(int(x), k) for x in kmers})
        rng = np.random.default_rng(seed)
        self.counts = rng.integers(1, 51, size=len(self.keys)).astype(np.uint16)
        if len(self.keys):
            self.counts[int(rng.integers(0, len(self.keys)))] = MAX_COUNT
        self.note = note or {}
        self.hi, self.lo = split(self.keys)
        self.where = {x: i for i, x in enumerate(self.keys)}
        self.value = {x: int(c) for x, c in zip(self.keys, self.counts.tolist())}

    def __len__(self):
        return len(self.keys)

    @functools.cached_property
    def neighbours(self):
        """(nbr uint32 [n, 8], strand bool [n, 8]): slot 2 nuc = x[1..] + nuc (right), 2 nuc + 1 = nuc + x[..k-2] (left)"""
        if not self.keys:
            return np.zeros((0, 8), dtype=np.uint32), np.zeros((0, 8), dtype=bool)
        return UR._neighbours_wide(self.keys, self.k)

    @functools.cached_property
    def flags(self):
        """(info, ridx, lidx, pal) as k_w_ut_flags leaves them"""
        if not self.keys:
            return tuple(np.zeros(0, dtype=t) for t in (np.uint8, np.uint32, np.uint32, np.uint8))
        return UR.flags(self.keys, self.k)

    @functools.cached_property
    def hashes(self):
        return hash_of_keys(self.keys, self.k) if self.keys else np.zeros(0, dtype=np.uint64)

    def side_counts(self, side):
        """present neighbours per vertex on a side (0: right, 1: left)"""
        return (self.neighbours[0][:, side::2] != NONE).sum(axis=1)


def _outer(w, k, rng, right_counts=(1, 2, 3, 4), left_counts=(1, 2, 3, 4)):
    """the k-mers one step further out than the fan of w: right_counts[b] of the four w + b + c, left_counts[a] of the four d + a + w"""
    out = []
    for b in range(4):
        for c in rng.permutation(4)[:right_counts[b]].tolist():
            out.append((w << 4) | (b << 2) | c)
    for a in range(4):
        for d in rng.permutation(4)[:left_counts[a]].tolist():
            out.append((d << (2 * k - 2)) | (a << (2 * k - 4)) | w)
    return out


def _plain_interior(rng, k, accept=lambda h: True):
    """a random interior that is not its own reverse complement and whose port hash `accept`s"""
    nb = k - 2
    while True:
        raw = [rand_int(rng, 2 * nb) for _ in range(4096)]
        hi, lo = split(raw)
        chi, clo = canonical(hi, lo, nb)
        h = whash(chi, clo)
        for w, hh in zip(raw, h.tolist()):
            if accept(hh) and UR.rc_plain(w, nb) != w:
                return w


def case_fan(k, name="fan", accept=lambda h: True, pad_to=None):
    """1. one interior I that is not a palindrome, all sixteen a + I + b, and of the k-mers one step further out 1, 2, 3, 4 behind b = 0 .. 3 and in
    front of a = 0 .. 3: a member of the fan has 1 .. 4 neighbours on its outer side, an outer k-mer none on its own outer side and up to four
    -- on both strands -- on its inner side.  accept: a condition on I's hash (5. the wrap-around); pad_to: random k-mers up to that many keys"""
    rng = np.random.default_rng(7000 + 10 * k + len(name))
    w = _plain_interior(rng, k, accept)
    kmers = list(fan(w, k).values()) + _outer(w, k, rng)
    t = WTab(name, k, kmers, 7100 + k, note=dict(interior=w))
    if pad_to is not None:
        assert len(t) <= pad_to
        pad = random_canonical(rng, k, pad_to - len(t), avoid=t.keys)
        t = WTab(name, k, t.keys + pad, 7100 + k, note=dict(interior=w))
    return t


def self_rc(rng, nb):
    """a string of nb bases (even) equal to its reverse complement, as an int"""
    assert nb % 2 == 0
    h = rand_int(rng, nb)
    return (h << nb) | UR.rc_plain(h, nb // 2)


def case_palindromes(k):
    """2. (even k) P: a palindromic vertex with ONE neighbour x = P[1..] + c on either side -- the same k-mer, read on the two strands; seen from x, P
    is a neighbour that is its own reverse complement: reported once, strand bit 0.  P2: a palindrome with two such neighbours.  And the fan of a
    palindromic interior with its outer k-mers: sixteen strings, ten canonical k-mers"""
    assert k % 2 == 0
    rng = np.random.default_rng(7200 + k)
    mask = (1 << (2 * k)) - 1
    p, p2 = self_rc(rng, k), self_rc(rng, k)
    c0, (c1, c2) = int(rng.integers(0, 4)), rng.permutation(4)[:2].tolist()
    x = ((p << 2) | c0) & mask
    w = self_rc(rng, k - 2)
    kmers = [p, x, p2, ((p2 << 2) | c1) & mask, ((p2 << 2) | c2) & mask] + list(fan(w, k).values()) + _outer(w, k, rng)
    return WTab("palindromes", k, kmers, 7300 + k, note=dict(pal=p, pal2=p2, x=canon(x, k), interior=w))


def _windows(seq, k):
    return UR.seq_kmers(seq, k)[1]


def case_loops(k):
    """3. (odd k) the hairpin x = a + w, w = rc(w): its right neighbour w + (3 - a) is rc(x) -- x itself on the other strand --, with one more right
    and one left neighbour; G^k (code 0: the library's A), its own right and left neighbour, with a tail; the windows of (AC)^n, (AT)^n, (ACGT)^n,
    (AATT)^n, k + 8 bases each (for an even k the (AT), (ACGT) and (AATT) windows hold palindromes)"""
    rng = np.random.default_rng(7400 + k)
    kmers, note = [], {}
    if k % 2:
        w = self_rc(rng, k - 1)
        a = int(rng.integers(0, 4))
        x = (a << (2 * k - 2)) | w
        other = ((w << 2) | ((3 - a) ^ 1)) & ((1 << (2 * k)) - 1)              # a second right neighbour: w + another base
        left = (int(rng.integers(0, 4)) << (2 * k - 2)) | (x >> 2)
        kmers += [x, other, left]
        note["hairpin"] = canon(x, k)
    kmers += _windows([0] * (k + 3) + codes("CGTCAG"), k)
    for unit in ("AC", "AT", "ACGT", "AATT"):
        kmers += _windows(codes((unit * k)[:k + 8]), k)
    return WTab("loops", k, kmers, 7500 + k, note=note)


def collision_pairs(k):
    """the pairs of canonical interiors the fixed-seed search found for this k (tests/golden/make_wnbr_collisions.py): [(I1, I2)]"""
    with open(COLLISIONS) as f:
        d = json.load(f)
    return [(int(a, 16), int(b, 16)) for a, b in d["pairs"][str(k)]]


def collision_search(k, seed, draws=1 << 23, slot_bits=10, tag_bits=32, same_low=False):
    """a birthday search: `draws` random interiors of k - 2 bases, canonicalised -> the pairs of DIFFERENT canonical interiors whose port hashes agree in
    their high tag_bits bits and their low slot_bits bits (32 and 10: one tag and one home slot in an index of 1024 slots), as ints.  same_low: all
    draws share their last 31 bases (62 bits: with an end base, a whole low word) and are kept only where they are canonical as drawn"""
    rng = np.random.default_rng(seed)
    nb = k - 2
    hi = rng.integers(0, 1 << 63, size=draws, dtype=np.uint64) << _U(1) | rng.integers(0, 2, size=draws, dtype=np.uint64)
    lo = rng.integers(0, 1 << 63, size=draws, dtype=np.uint64) << _U(1) | rng.integers(0, 2, size=draws, dtype=np.uint64)
    hi, lo = _low(hi, lo, 2 * nb)
    if same_low:
        assert nb > 31
        lo = (lo & _U(3 << 62)) | (lo[0] & _U((1 << 62) - 1))
        chi, clo = canonical(hi, lo, nb)
        keep = (chi == hi) & (clo == lo)
        hi, lo = hi[keep], lo[keep]
    hi, lo = canonical(hi, lo, nb)
    h = whash(hi, lo)
    key = ((h >> _U(64 - tag_bits)) << _U(slot_bits)) | (h & _U((1 << slot_bits) - 1))
    order = np.argsort(key, kind="stable")
    ks = key[order]
    out = []
    for j in np.flatnonzero(ks[1:] == ks[:-1]).tolist():
        a, b = order[j], order[j + 1]
        x, y = (int(hi[a]) << 64) | int(lo[a]), (int(hi[b]) << 64) | int(lo[b])
        if x != y:
            out.append((min(x, y), max(x, y)))
    return sorted(set(out))


def case_collision(k):
    """4. two different canonical interiors with one tag and one home slot (1024 slots).  Of either fan every second string -- of I1 those with a + b
    even, of I2 those with a + b odd: a sibling that is missing behind one interior is there behind the other --, and all the outer k-mers, whose
    inner sides walk the cluster the two fans share"""
    w1, w2 = collision_pairs(k)[0]
    rng = np.random.default_rng(7600 + k)
    kmers = [x for (a, b), x in fan(w1, k).items() if (a + b) % 2 == 0] + [x for (a, b), x in fan(w2, k).items() if (a + b) % 2 == 1]
    kmers += _outer(w1, k, rng, (2, 2, 2, 2), (2, 2, 2, 2)) + _outer(w2, k, rng, (2, 2, 2, 2), (2, 2, 2, 2))
    return WTab("collision", k, kmers, 7700 + k, note=dict(interiors=(w1, w2)))


SEAM_KS = (47, 62, 63)          # two interiors that share their last 31 bases leave 2 (k - 33) bits to search a 42-bit collision in: 28 at k = 47, none worth the name at k = 34


def seam_pairs(k):
    with open(COLLISIONS) as f:
        d = json.load(f)
    return [(int(a, 16), int(b, 16)) for a, b in d["seam_pairs"][str(k)]]


def case_seam(k):
    """4b. two different canonical interiors with one tag, one home slot AND the same last 31 bases: a + I1 + b and a + I2 + b agree in their whole low
    word, in tag and in home slot and differ in the high word only, in the middle of the interior.  The table holds the fan of I1 and the outer k-mers
    of both; of I2's fan nothing: the outer k-mers of I2 walk I1's cluster and must find no neighbour there, a look-up of a + I2 + b must go past
    a + I1 + b"""
    w1, w2 = seam_pairs(k)[0]
    rng = np.random.default_rng(7900 + k)
    kmers = list(fan(w1, k).values()) + _outer(w1, k, rng, (2, 2, 2, 2), (2, 2, 2, 2)) + _outer(w2, k, rng, (2, 2, 2, 2), (2, 2, 2, 2))
    absent = list(fan(w2, k).values())
    return WTab("seam", k, kmers, 7950 + k, note=dict(interiors=(w1, w2), ask=absent + [UR.rc_plain(x, k) for x in absent]))


def case_wrap(k, big):
    """5. a fan whose home slot is one of the last three: its cluster of sixteen runs over the end of the index to slot 0.  big: 513 keys, an index of
    2048 slots -- the wrap at another mask"""
    cap = 2048 if big else 1024
    return case_fan(k, name="wrap%d" % cap, accept=lambda h: (h & (cap - 1)) >= cap - 3, pad_to=513 if big else None)


def case_empty(k):
    return WTab("empty", k, [], 1)


def case_broad(k):
    """7. the distinct k-mers of fifty reads of util.branchy_reads (about 5 000)"""
    from util import branchy_reads
    b, o = branchy_reads(900 + k, n=50)
    lut = np.zeros(256, dtype=np.uint8)
    for i, ch in enumerate(NUC.encode()):
        lut[ch] = i
    cs = lut[b]
    kmers = []
    for i in range(len(o) - 1):
        kmers += _windows(cs[int(o[i]):int(o[i + 1])], k)
    return WTab("broad", k, kmers, 7800 + k)


def case_names(k):
    return ["fan"] + (["palindromes"] if k % 2 == 0 else []) + ["loops", "collision"] + (["seam"] if k in SEAM_KS else []) + ["wrap1024", "wrap2048", "empty", "broad"]


_MAKE = {"seam": case_seam, "fan": case_fan, "palindromes": case_palindromes, "loops": case_loops, "collision": case_collision,
         "wrap1024": functools.partial(case_wrap, big=False), "wrap2048": functools.partial(case_wrap, big=True), "empty": case_empty, "broad": case_broad}
_built = {}


def get_case(name, k):
    """built once per process, never changed"""
    if (name, k) not in _built:
        _built[name, k] = _MAKE[name](k)
    return _built[name, k]


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. look-up queries
# ---------------------------------------------------------------------------------------------------------------------------------
def queries(t, seed=0, random_absent=200):
    """-> (queries: list of ints, wanted int32: the count or -1, kinds: list of str).  every key; `sibling`: a key with its last or its first base
    replaced (a present interior, another end base), as read and canonical; `hi` / `lo` (k >= 33): a key's low word under another key's high word and
    the converse; `random`: random canonical k-mers.  What is wanted comes from the dictionary"""
    k, keys = t.k, t.keys
    rng = np.random.default_rng(8000 + seed + k)
    q = [(x, "key") for x in keys]
    top = 2 * k - 2
    sib_of = keys if len(keys) <= 600 else [keys[i] for i in rng.choice(len(keys), size=600, replace=False).tolist()]
    for x in sib_of:
        for c in range(4):
            for y in ((x & ~3) | c, (x & ~(3 << top)) | (c << top)):
                if y != x:
                    q.append((y, "sibling"))
                    q.append((canon(y, k), "sibling"))
    if k >= 33 and len(keys) > 1:
        for i, x in enumerate(sib_of):
            other = keys[(t.where[x] + 1 + i % 7) % len(keys)]
            q.append((((other >> 64) << 64) | (x & M64), "hi"))
            q.append((((x >> 64) ^ 1) << 64 | (x & M64), "hi"))
            q.append((((x >> 64) << 64) | (other & M64), "lo"))
            q.append((x ^ (1 << int(rng.integers(0, 64))), "lo"))
    q += [(x, "asked") for x in t.note.get("ask", ())]                        # what a case wants asked on top
    q += [(x, "random") for x in random_canonical(rng, k, random_absent)]
    order = rng.permutation(len(q)).tolist()
    q = [q[i] for i in order]
    want = np.array([t.value.get(x, -1) for x, _ in q], dtype=np.int32)
    return [x for x, _ in q], want, [kind for _, kind in q]
