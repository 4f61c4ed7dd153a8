"""A model of the join core's union table (metafast_amd/csrc/mf_join.h, mf_join.hip) in Python integers and numpy, written from the kernels'
text; it shares no code with the library.

The table: `cap` (a power of two) slots of 16 bytes {key u64, cnt u32, row u32}, open-addressed with linear probing from home = hash64(key) &
(cap - 1); an empty slot holds the all-ones key.  The key space is cut into S slices by the TOP 32 bits of the hash, the home comes from the LOW
bits.  hash64 is fmix64, a bijection, and unhash64 is its inverse: tests/join_cases.py picks a key's home slot and slice at will.

Which slot of its cluster a key takes depends on the order in which the lanes of a launch win their compare-and-swaps, so a table is checked by
invariant (check_slots), not slot for slot:
  occupied    the multiset of non-empty keys is the set of keys of slice s that some sample holds with count > b (so no key is there twice)
  n_union     the counter equals that set's size
  reachable   a walk from a key's home reaches the key before any empty slot
  payload     per mode, what the samples add up to (expected_payloads)
  empty       every other slot holds the empty key and the initial payload
A failed check raises SlotError, whose text starts with the invariant's name."""
import math

import numpy as np

M64 = (1 << 64) - 1
EMPTY = M64
KEY_LIMIT = 1 << 62
NO_ROW = 0xFFFFFFFF
NOT_FOUND = M64
NOT_MINE = M64 - 1                      # mf_debug_join_find: a key >= 2^62 or of another slice
KNOCKED = 0x80000000
FIELD_MAX = (1 << 20) - 1
PRESENCE, SUM, FIELD, COLOR = 0, 1, 2, 3
P_NSAMPLES, P_KPS, P_COLOR, P_UKM, P_UK = 0, 1, 2, 3, 4
ALL = {P_NSAMPLES: True, P_KPS: False, P_COLOR: True, P_UKM: False, P_UK: True}

_C1, _C2 = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
_I1, _I2 = pow(_C1, -1, 1 << 64), pow(_C2, -1, 1 << 64)

SLOT = np.dtype([("key", "<u8"), ("cnt", "<u4"), ("row", "<u4")])


class SlotError(AssertionError):
    def __init__(self, invariant, text):
        super().__init__("%s: %s" % (invariant, text))
        self.invariant = invariant


def hash64(x):
    x &= M64
    x ^= x >> 33
    x = (x * _C1) & M64
    x ^= x >> 33
    x = (x * _C2) & M64
    x ^= x >> 33
    return x


def unhash64(h):
    """x ^= x >> 33 leaves the top 31 bits alone, so it undoes itself; the multipliers are odd"""
    h &= M64
    h ^= h >> 33
    h = (h * _I2) & M64
    h ^= h >> 33
    h = (h * _I1) & M64
    h ^= h >> 33
    return h


def slice_of(h, S):
    return ((h >> 32) * S) >> 32


def home(key, cap):
    return hash64(key) & (cap - 1)


def cap_of(total, S):
    """plan_slices' capacity for a set option stats_slices = S >= 1, in IEEE doubles"""
    per = float(total) / float(S)
    x = int(2.0 * (per + 6.0 * math.sqrt(per) + 1024.0))
    p = 1
    while p < x:
        p <<= 1
    return p


def index_cap_of(m):
    """the column index of kmers-per-sample: the power of two >= 2 m, at least 2"""
    c = 2
    while c < 2 * m:
        c <<= 1
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# what the samples add up to
# ---------------------------------------------------------------------------------------------------------------------------------
def initial_payload(mode):
    return (0, NO_ROW) if mode == PRESENCE else (0, 0)


def _add_entry(mode, add, c, cnt, row):
    """one entry (count c) of a sample with add word `add` on a slot's payload, as k_stats_union's atomics do it"""
    if mode == PRESENCE:
        return (cnt + add) & 0xFFFFFFFF, row
    if mode == SUM:
        return (cnt + 1) & 0xFFFFFFFF, (row + c) & 0xFFFFFFFF
    if mode == FIELD:
        if add == 2:
            return cnt, (row + c) & 0xFFFFFFFF
        return (cnt + ((c << (16 * add)) & 0xFFFFFFFF)) & 0xFFFFFFFF, row
    w = cnt | (row << 32)
    sh = 20 * (add & 3)
    f = (w >> sh) & FIELD_MAX
    nf = min(f + (c if add & 4 else 1), FIELD_MAX)
    w = (w & ~(FIELD_MAX << sh) & M64) | (nf << sh)
    return w & 0xFFFFFFFF, w >> 32


def expected_payloads(samples, b, mode, add, S=1, s=0):
    """{key: (cnt, row)} of slice s: every entry with count > b of sample j = (keys, counts) adds add[j] in `mode`.  A key >= 2^62 is the
    caller's mistake here (the pass refuses it)"""
    out = {}
    for j, (keys, counts) in enumerate(samples):
        for key, c in zip((int(x) for x in keys), (int(x) for x in counts)):
            if c <= b:
                continue
            assert key < KEY_LIMIT, key
            if slice_of(hash64(key), S) != s:
                continue
            out[key] = _add_entry(mode, int(add[j]), c, *out.get(key, initial_payload(mode)))
    return out


def union_keys(samples, b):
    return {int(k) for keys, counts in samples for k, c in zip(keys, counts) if int(c) > b}


# ---------------------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------------------
def empty_table(cap, mode=SUM):
    t = np.zeros(cap, dtype=SLOT)
    t["key"] = EMPTY
    t["cnt"], t["row"] = initial_payload(mode)
    return t


def insert(slots, key, payload=None):
    """linear probing: the slot that holds `key` or the first empty one of its walk (taken); None when the table is full"""
    cap = len(slots)
    p = home(key, cap)
    for _ in range(cap):
        k = int(slots["key"][p])
        if k == EMPTY or k == key:
            slots["key"][p] = key
            if payload is not None:
                slots["cnt"][p], slots["row"][p] = payload
            return p
        p = (p + 1) & (cap - 1)
    return None


def simulate(cap, samples, b, mode, add, S=1, s=0, rng=None):
    """the union of slice s by a plain linear-probing table, the entries of each sample in a shuffled order -> (slots, n_union)"""
    slots = empty_table(cap, mode)
    n = 0
    for j, (keys, counts) in enumerate(samples):
        order = np.arange(len(keys)) if rng is None else rng.permutation(len(keys))
        for i in order:
            key, c = int(keys[i]), int(counts[i])
            if c <= b or slice_of(hash64(key), S) != s:
                continue
            p = home(key, cap)
            while int(slots["key"][p]) not in (EMPTY, key):
                p = (p + 1) & (cap - 1)
            if int(slots["key"][p]) == EMPTY:
                n += 1
                slots["key"][p] = key
            slots["cnt"][p], slots["row"][p] = _add_entry(mode, int(add[j]), c, int(slots["cnt"][p]), int(slots["row"][p]))
    return slots, n


def walk(slots, key):
    """the read-only probe of mf_join_find -> (slot or NOT_FOUND, occupied slots looked at that do not hold the key)"""
    cap = len(slots)
    p = home(key, cap)
    for step in range(cap):
        k = int(slots["key"][p])
        if k == key:
            return p, step
        if k == EMPTY:
            return NOT_FOUND, step
        p = (p + 1) & (cap - 1)
    return NOT_FOUND, cap


def find(slots, key, S=1, s=0):
    """what mf_debug_join_find writes for `key`"""
    if key >= KEY_LIMIT or slice_of(hash64(key), S) != s:
        return NOT_MINE
    return walk(slots, key)[0]


def occupied_span_wraps(slots):
    """some run of occupied slots crosses cap - 1 -> 0"""
    return int(slots["key"][-1]) != EMPTY and int(slots["key"][0]) != EMPTY


def check_slots(slots, cap, S, s, samples, b, mode, add, n_union):
    """raises SlotError(invariant) unless `slots` (SLOT[cap]) and n_union are a union of slice s of S over the samples"""
    assert len(slots) == cap and cap >= 1 and cap & (cap - 1) == 0
    want = expected_payloads(samples, b, mode, add, S, s)
    keys = [int(k) for k in slots["key"]]
    held = sorted(k for k in keys if k != EMPTY)
    if held != sorted(want):
        twice = sorted({k for k in held if held.count(k) > 1})[:3] if len(held) < 5000 else []
        lost, extra = sorted(set(want) - set(held))[:3], sorted(set(held) - set(want))[:3]
        raise SlotError("occupied", "%d non-empty slots, %d keys expected; lost %s, not expected %s, twice %s" % (len(held), len(want), lost, extra, twice))
    if n_union != len(want):
        raise SlotError("n_union", "%d reported, %d keys in the slice" % (n_union, len(want)))
    for p, k in enumerate(keys):
        if k == EMPTY:
            continue
        q = home(k, cap)
        while keys[q] != k and keys[q] != EMPTY:          # (ends: k is in the table)
            q = (q + 1) & (cap - 1)
        if q != p:
            raise SlotError("reachable", "key %#x in slot %d, home %d: an empty slot lies between" % (k, p, home(k, cap)))
    init = initial_payload(mode)
    for p, k in enumerate(keys):
        got = (int(slots["cnt"][p]), int(slots["row"][p]))
        if k != EMPTY and got != want[k]:
            raise SlotError("payload", "key %#x in slot %d: cnt %#x row %#x, expected cnt %#x row %#x" % ((k, p) + got + want[k]))
    for p, k in enumerate(keys):
        got = (int(slots["cnt"][p]), int(slots["row"][p]))
        if k == EMPTY and got != init:
            raise SlotError("empty", "empty slot %d holds cnt %#x row %#x" % ((p,) + got))


# ---------------------------------------------------------------------------------------------------------------------------------
# the read-out
# ---------------------------------------------------------------------------------------------------------------------------------
def _i32(x):
    return x - (1 << 32) if x & 0x80000000 else x


def _i16(x):
    x &= 0xFFFF
    return x - (1 << 16) if x & 0x8000 else x


def project(cnt, row, proj, param=0):
    """an occupied slot through projection proj -> its value (widened to 64 bits) or None where the projection drops it"""
    if proj == P_NSAMPLES:
        return cnt & 0xFFFF
    if proj == P_KPS:
        return cnt & 0xFFFF if _i32(cnt) >= param else None
    if proj == P_COLOR:
        return cnt | (row << 32)
    if proj == P_UKM:
        if row & KNOCKED or _i16(row) <= param:
            return None
        return ((row & 0xFFFF) | (cnt << 16)) & 0xFFFFFFFF
    return 0 if row & KNOCKED else min(row, 32767)


def read(slots, proj, param=0):
    """the (key, value) pairs of the read-out, sorted (the kernel writes them in any order)"""
    out = []
    for k, c, r in zip(slots["key"], slots["cnt"], slots["row"]):
        if int(k) != EMPTY:
            v = project(int(c), int(r), proj, param)
            if v is not None:
                out.append((int(k), v))
    return sorted(out)
