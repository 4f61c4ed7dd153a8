"""Crafted keys for the join core's union table (tests/join_ref.py): families of distinct keys below 2^62 whose home slot and slice are chosen
through the inverse of the hash, and the cohorts the GPU tests feed to the union pass.  No GPU needed: tests/test_join_ref_cpu.py asserts
every property the cases rest on.

A family fixes the top 32 hash bits (the slice) and the low 20 (the home slot in every table of up to 2^20 slots, `home & (cap - 1)` in a smaller
one) and walks through the 12 bits between them; about a quarter of the 4096 candidates invert to a key below 2^62.  `skip` leaves out a family's
first candidates: ghosts (keys no sample holds) are taken far behind the keys that are held."""
import numpy as np

import join_ref as J

LOW = 20
LOW_MASK = (1 << LOW) - 1
TOPS = (0x12345678, 0x6789ABCD, 0xC0FFEE11)            # one per third of the hash's top 32 bits: slices 0, 1, 2 of 3
GHOST_SKIP = 500

_cache = {}


def candidates(v, top32):
    """every key below 2^62 whose hash is top32 << 32 | mid << 20 | v, in the order of mid"""
    if (v, top32) not in _cache:
        _cache[v, top32] = [k for k in (J.unhash64((top32 << 32) | (mid << LOW) | v) for mid in range(1 << 12)) if k < J.KEY_LIMIT]
    return _cache[v, top32]


def at(v, n, top32=TOPS[0], skip=0):
    c = candidates(v & LOW_MASK, top32)
    assert len(c) >= skip + n, (v, top32, len(c), skip, n)
    return c[skip:skip + n]


def last(n, top32=TOPS[0], skip=0):
    """the low 20 hash bits all ones: home cap - 1 in every table up to 2^20 slots, so the cluster runs over the end of the table"""
    return at(LOW_MASK, n, top32, skip)


def first(n, top32=TOPS[0], skip=0):
    return at(0, n, top32, skip)


def stair(v, steps, per, top32=TOPS[0], skip=0):
    """homes v, v + 1, ... with `per` keys each: the clusters merge, and a probe passes through other homes' keys"""
    return [k for i in range(steps) for k in at(v + i, per, top32, skip)]


def edge_tops(S):
    """the top-32 hash values on either side of every slice border, and the two ends"""
    t = [0, 0xFFFFFFFF]
    for s in range(1, S):
        c = -((-s << 32) // S)                            # ceil(s 2^32 / S): the first value of slice s
        t += [c - 1, c]
    return sorted(t)


def edges(S, per=8):
    """[(top32, key)]: `per` keys for every value of edge_tops(S); the low 32 hash bits are taken in turn"""
    out = []
    for t in edge_tops(S):
        got, low = 0, 0x9E3779B1
        while got < per:
            k = J.unhash64((t << 32) | low)
            if k < J.KEY_LIMIT:
                out.append((t, k))
                got += 1
            low = (low * 0x2545F491 + 0x3C6EF35F) & 0xFFFFFFFF
    return out


SPECIAL = (0, J.KEY_LIMIT - 1)

# ---------------------------------------------------------------------------------------------------------------------------------
# the cohorts of the union tests
# ---------------------------------------------------------------------------------------------------------------------------------
B = 2                                                   # entries with count <= 2 bring nothing
# cap -> keys per family and top: (last, first, stair steps, stair per, keys per edge value, edges at S = 1, keys 0 and 2^62 - 1)
SPEC = {1: (1, 0, 0, 0, 0, False, False), 8: (3, 1, 0, 0, 1, False, True), 64: (20, 6, 3, 3, 2, True, True), 512: (300, 20, 6, 5, 8, True, True),
        4096: (300, 20, 6, 5, 8, True, True)}
STAIR_AT = 37                                           # the stair's first home (below every capacity from 64 on)
CAPS = tuple(SPEC)
# what a sample adds, per mode variant: (name, mode, add words of samples 0 .. 4; FIELD takes the first three samples, one per field)
#   (sample 2's counts are 65535: it fills nonibd, cd or uc to the last bit in the three FIELD variants)
VARIANTS = (("presence", J.PRESENCE, (1, 1 << 16, 1 << 10, 1 << 20, 0)), ("sum", J.SUM, (0, 0, 0, 0, 0)), ("field", J.FIELD, (0, 1, 2)),
            ("field, 65535 in cd", J.FIELD, (1, 2, 0)), ("field, 65535 in uc", J.FIELD, (2, 0, 1)), ("color counts", J.COLOR, (0, 1, 2, 0, 1)),
            ("color values", J.COLOR, (4, 5, 6, 4, 5)))


def held_keys(cap, S):
    """-> dict(last, first, stair, edges, special, low_only): the keys of the cohort for a table of `cap` slots cut into S slices; at S = 3 every
    family is there once per slice.  low_only: keys held only with counts <= B, homes inside the `last` cluster"""
    nl, nf, steps, per, ne, e1, sp = SPEC[cap]
    tops = TOPS[:S]
    lo_n = 0 if cap == 1 else 3
    d = dict(last=[k for t in tops for k in last(nl, t)], first=[k for t in tops for k in first(nf, t)],
             stair=[k for t in tops for k in stair(STAIR_AT, steps, per, t)], edges=[k for _, k in edges(3, ne)] if ne and (S == 3 or e1) else [],
             special=list(SPECIAL) if sp else [], low_only=[k for t in tops for k in last(lo_n, t, skip=nl)])
    return d


def cohort(cap, S):
    """five samples (keys uint64, counts uint16) over held_keys(cap, S), every sample's keys distinct:
      0  the whole `last` family (one launch contends for one home slot) and every second key of the rest
      1  every key but each third one
      2  every second key, each with count 65535
      3  every key: counts 1 and 2 (<= B) on two of three, and the low_only keys
      4  the first, stair and special keys, and every fourth `last` key"""
    d = held_keys(cap, S)
    rest = d["first"] + d["stair"] + d["edges"] + d["special"]
    allk = d["last"] + rest
    rng = np.random.default_rng(7000 + 10 * cap + S)

    def sample(keys, counts=None):
        keys = np.array(keys, dtype=np.uint64)
        if counts is None:
            counts = rng.integers(B + 1, 60, size=len(keys))
        return keys, np.asarray(counts, dtype=np.uint16)

    s3 = allk + d["low_only"]
    c3 = [(1, 2, 40)[i % 3] for i in range(len(allk))] + [1 + i % 2 for i in range(len(d["low_only"]))]
    if cap == 1:                                          # (one key a slice: every sample that holds it counts it)
        c3 = [7] * len(allk)
    return [sample(d["last"] + rest[::2]), sample([k for i, k in enumerate(allk) if i % 3 != 2] if cap > 1 else allk), sample(allk[::2], [65535] * len(allk[::2])),
            sample(s3, c3), sample(d["first"] + d["stair"] + d["special"] + d["last"][::4])]


def ghosts(cap, S):
    """[(key, why, walk)]: keys of no sample whose homes lie at the head of, inside and in front of the clusters of cohort(cap, S); walk: the
    occupied slots its probe passes, at least, before it meets an empty one (the `last` keys lie in the slots cap - 1, 0, 1, ... whatever the
    order they came in, the `first` keys behind them, a stair's keys in the slots from its first home on)"""
    nl, nf, steps, per, ne, e1, sp = SPEC[cap]
    out = []
    for t in TOPS[:S]:
        out += [(k, "home cap - 1, the head of the wrapped cluster", nl) for k in last(3, t, GHOST_SKIP)]
        out += [(k, "home 0, inside the wrapped cluster", max(1, nl - 1 + nf)) for k in first(3, t, GHOST_SKIP)]
        if steps:
            out += [(k, "home in the stair", per) for k in stair(STAIR_AT, steps, 1, t, GHOST_SKIP)]
            out += [(k, "the empty slot in front of the stair", 0) for k in at(STAIR_AT - 1, 2, t, GHOST_SKIP)]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the cohort of the tools' test
# ---------------------------------------------------------------------------------------------------------------------------------
CRAFTED_N = 6


def crafted_pool():
    """-> dict(last, rest, ghosts): about 600 keys -- per third of the hash space 100 `last` keys, 20 `first` keys and a stair of 6 x 5, the border
    keys of 3 and of 7 slices, keys 0 and 2^62 - 1 -- and ghosts at the head of, inside and in front of their clusters.  The homes hold in every
    table of up to 2^20 slots"""
    lastk = [k for t in TOPS for k in last(100, t)]
    rest = [k for t in TOPS for k in first(20, t) + stair(STAIR_AT, 6, 5, t)]
    rest += sorted({k for S in (3, 7) for _, k in edges(S)}) + list(SPECIAL)
    gh = [k for t in TOPS for k in last(8, t, GHOST_SKIP) + first(4, t, GHOST_SKIP) + stair(STAIR_AT, 6, 1, t, GHOST_SKIP) + at(STAIR_AT - 1, 2, t, GHOST_SKIP)]
    assert len(set(lastk + rest + gh)) == len(lastk + rest + gh)
    return dict(last=lastk, rest=rest, ghosts=gh)


def crafted_cohort(seed=1, lo=1, hi=40, kps=False):
    """CRAFTED_N samples (keys uint64, counts int16 in lo .. hi - 1) over crafted_pool(), each of at most about 600 entries.
    kps = False: every sample holds about two thirds of the `last` keys and of the rest.
    kps = True: every sample holds every `last` key, and a key of the rest lies in at most three samples -- at percent = 80 (thresh 4 of the five
    samples behind the first) the selected columns are the `last` keys, all of them"""
    p = crafted_pool()
    rng = np.random.default_rng(seed)
    lastk, rest = np.array(p["last"], np.uint64), np.array(p["rest"], np.uint64)
    owners = np.stack([rng.permutation(CRAFTED_N)[:3] for _ in rest])                   # the (at most) three samples of a key of the rest
    out = []
    for j in range(CRAFTED_N):
        if kps:
            keys = np.concatenate([lastk, rest[(owners == j).any(axis=1) & (rng.random(len(rest)) < 0.8)]])
        else:
            keys = np.concatenate([lastk[rng.random(len(lastk)) < 0.66], rest[rng.random(len(rest)) < 0.66]])
        keys = keys[rng.permutation(len(keys))]
        out.append((keys, rng.integers(lo, hi, size=len(keys)).astype(np.int16)))
    return out


def with_ghosts(sample, seed=2):
    """the sample and every ghost of crafted_pool(), shuffled"""
    rng = np.random.default_rng(seed)
    g = np.array(crafted_pool()["ghosts"], np.uint64)
    keys = np.concatenate([sample[0], g])
    counts = np.concatenate([sample[1], rng.integers(3, 30, size=len(g)).astype(np.int16)])
    order = rng.permutation(len(keys))
    return keys[order], counts[order]


def fill(cap, n, top32=TOPS[0]):
    """n distinct keys of one top32 with homes spread over a table of `cap` slots, three to a home"""
    return [k for v in range((n + 2) // 3) for k in at(v * 0x10001 + 5, 3, top32)][:n]
