"""tests/wnbr_ref.py without a GPU: the numpy port of the wide index hash pinned to hand-worked values, to a restatement on Python ints and to the
property the neighbour look-up rests on (a + I + b and its reverse complement hash alike for every a, b); and, case by case, the property every
crafted table of tests/test_wnbr_gpu.py is made for, asserted from the reference (ut_ref) and the port alone.  A case that loses its property fails
here, not silently on the GPU."""
import numpy as np
import pytest

import ut_ref as UR
import wnbr_ref as W

M64 = (1 << 64) - 1


# ---- the port -------------------------------------------------------------------------------------------------------------------
def _h64(x):
    """mf_hash64 on a Python int"""
    x ^= x >> 33; x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33; x = (x * 0xc4ceb9fe1a85ec53) & M64
    return x ^ (x >> 33)


def _key_hash(x, k):
    """mf_whash_key on a Python int, base by base: the middle k - 2 bases, the smaller of them and their reverse complement, one multiply, one mix"""
    w = (x >> 2) & ((1 << (2 * k - 4)) - 1)
    c = min(w, UR.rc_plain(w, k - 2))
    return _h64((((c & M64) * 0x9E3779B97F4A7C15) & M64) ^ (c >> 64))


def test_hashes_pinned():
    # the finaliser of MurmurHash3: 0 -> 0, 1 -> b456bcfc34c2cb2c (worked by hand in 128-bit integer arithmetic, like the other two)
    assert W.hash64([0, 1]).tolist() == [0, 0xb456bcfc34c2cb2c]
    assert W.whash([1, 0, 0x123456789ABCDEF], [0, 1, 0xFEDCBA9876543210]).tolist() == [0xb456bcfc34c2cb2c, 0x9ca066f1a4ab2eea, 0xc3a091ce77ab2539]
    for k in W.KS:
        # code 0 k times: the interior is 0, its reverse complement all threes: hash 0, home slot 0, tag 0 -- and so for every first and last base
        keys = [W.join(a, 0, b, k) for a in range(4) for b in range(4)]
        assert W.hash_of_keys(keys, k).tolist() == [0] * 16
        home, tag = W.home_tag(W.hash_of_keys(keys, k), 1024)
        assert home.tolist() == [0] * 16 and tag.tolist() == [0] * 16
        # interior = code 0 ... 0 1 (canonical: it starts with 0, its reverse complement with 2): the hash of the one-word number 1
        assert W.hash_of_keys([W.join(3, 1, 2, k)], k).tolist() == [0x9ca066f1a4ab2eea]
    h = np.array([0xFFFFFFFF000003FF, 0x0000000100000400], dtype=np.uint64)
    assert [x.tolist() for x in W.home_tag(h, 1024)] == [[1023, 0], [0xFFFFFFFF, 1]]
    assert [x.tolist() for x in W.home_tag(h, 2048)] == [[1023, 1024], [0xFFFFFFFF, 1]]
    assert [W.cap_of(n) for n in (0, 1, 512, 513, 1024, 1025)] == [0, 1024, 1024, 2048, 2048, 4096]


@pytest.mark.parametrize("nb", [1, 2, 30, 31, 32, 33, 45, 60, 61, 62, 63, 64])
def test_revcomp_port_against_the_plain_one(nb):
    rng = np.random.default_rng(nb)
    xs = [W.rand_int(rng, 2 * nb) for _ in range(200)] + [0, (1 << (2 * nb)) - 1, 1, 1 << (2 * nb - 1)]
    hi, lo = W.split(xs)
    rhi, rlo = W.revcomp(hi, lo, nb)
    assert [(int(a) << 64) | int(b) for a, b in zip(rhi, rlo)] == [UR.rc_plain(x, nb) for x in xs]
    chi, clo = W.canonical(hi, lo, nb)
    assert [(int(a) << 64) | int(b) for a, b in zip(chi, clo)] == [min(x, UR.rc_plain(x, nb)) for x in xs]


@pytest.mark.parametrize("k", range(32, 64))
def test_key_hash_port_against_python_ints(k):
    rng = np.random.default_rng(100 + k)
    xs = [W.rand_int(rng, 2 * k) for _ in range(300)]
    assert W.hash_of_keys(xs, k).tolist() == [_key_hash(x, k) for x in xs]
    assert [W.hash_of_interior(W.interior(x, k), k) for x in xs[:20]] == [_key_hash(x, k) for x in xs[:20]]


@pytest.mark.parametrize("k", range(32, 64))
def test_a_fan_and_its_reverse_complements_hash_alike(k):
    """what w_side_walk rests on: one probe sequence meets a + I + b and rc(a + I + b) for every a, b"""
    rng = np.random.default_rng(200 + k)
    seen = set()
    for _ in range(20):
        w = W.rand_int(rng, 2 * k - 4)
        xs = list(W.fan(w, k).values())
        xs += [UR.rc_plain(x, k) for x in xs]
        h = set(W.hash_of_keys(xs, k).tolist())
        assert len(h) == 1
        seen |= h
    assert len(seen) == 20                                 # (another interior, another hash)


# ---- the tables -----------------------------------------------------------------------------------------------------------------
ALL = [(name, k) for k in W.KS for name in W.case_names(k)]


@pytest.mark.parametrize("name,k", ALL)
def test_every_table_is_a_table(name, k):
    t = W.get_case(name, k)
    assert t.keys == sorted(set(t.keys)) and all(0 <= x < (1 << (2 * k)) and x <= UR.rc_plain(x, k) for x in t.keys)
    assert len(t.counts) == len(t) and (len(t) == 0 or (t.counts.min() >= 1 and t.counts.max() == W.MAX_COUNT))
    assert [(int(h) << 64) | int(l) for h, l in zip(t.hi, t.lo)] == t.keys
    if k == 32:
        assert not t.hi.any()
    if k == 33 and len(t):
        assert int(t.hi.max()) <= 3
    want_cap = {"wrap2048": 2048, "broad": W.cap_of(len(t)), "empty": 0}.get(name, 1024)
    assert W.cap_of(len(t)) == want_cap and (name == "broad" or len(t) <= 513)
    nbr, strand = t.neighbours
    info, ridx, lidx, pal = t.flags
    if k % 2:
        assert not pal.any()                               # 2. an odd k has no palindromes
    # the adjacency is symmetric: every present neighbour has the vertex among its own eight
    for v, s in np.argwhere(nbr != W.NONE).tolist():
        assert v in nbr[nbr[v, s]].tolist()
    # 6. the queries hold what they are made for
    q, want, kinds = W.queries(t)
    ks = set(kinds)
    assert "random" in ks and all(want[i] == -1 for i, kd in enumerate(kinds) if kd == "random")
    if len(t):
        assert [want[i] for i, kd in enumerate(kinds) if kd == "key"].count(-1) == 0 and kinds.count("key") == len(t)
        sib = [(q[i], int(want[i])) for i, kd in enumerate(kinds) if kd == "sibling"]
        present_interiors = {min(W.interior(x, k), UR.rc_plain(W.interior(x, k), k - 2)) for x in t.keys}
        assert all(min(W.interior(x, k), UR.rc_plain(W.interior(x, k), k - 2)) in present_interiors for x, _ in sib)
        assert any(w == -1 for _, w in sib)
        if k >= 33:
            for kd in ("hi", "lo"):
                sel = [i for i, x in enumerate(kinds) if x == kd]
                assert any(want[i] == -1 for i in sel)
                lows, highs = {x & M64 for x in t.keys}, {x >> 64 for x in t.keys}
                assert any(want[i] == -1 and ((q[i] & M64) in lows if kd == "hi" else (q[i] >> 64) in highs) for i in sel)
    else:
        assert (want == -1).all()


def _fan_keys(t, w=None):
    w = t.note["interior"] if w is None else w
    return sorted({W.canon(x, t.k) for x in W.fan(w, t.k).values()})


def _check_fan(t):
    """1. sixteen keys in one cluster, every number of neighbours on a side, both strands on one side of one vertex, the seam between the words"""
    k = t.k
    fk = _fan_keys(t)
    assert len(fk) == 16 and all(x in t.where for x in fk)
    h = W.hash_of_keys(fk, k)
    home, tag = W.home_tag(h, W.cap_of(len(t)))
    assert len(set(home.tolist())) == 1 and len(set(tag.tolist())) == 1
    nbr, strand = t.neighbours
    present = nbr != W.NONE
    for side in (0, 1):
        assert set(t.side_counts(side).tolist()) == {0, 1, 2, 3, 4}, side
        both = [(present[v, side::2] & strand[v, side::2]).any() and (present[v, side::2] & ~strand[v, side::2]).any() for v in range(len(t))]
        assert any(both), side
    if k >= 33:
        pairs = [(x, y) for x in fk for y in fk if x < y and (x & M64) == (y & M64)]
        assert pairs and all(x >> 64 != y >> 64 for x, y in pairs)
    else:
        assert not t.hi.any()
    return home[0]


@pytest.mark.parametrize("k", W.KS)
def test_case_fan(k):
    _check_fan(W.get_case("fan", k))


@pytest.mark.parametrize("k", [k for k in W.KS if k % 2 == 0])
def test_case_palindromes(k):
    t = W.get_case("palindromes", k)
    nbr, strand = t.neighbours
    info, ridx, lidx, pal = t.flags
    for name in ("pal", "pal2"):
        p = t.note[name]
        assert UR.rc_plain(p, k) == p and pal[t.where[p]] == 1
    p, x = t.where[t.note["pal"]], t.where[t.note["x"]]
    # P has one neighbour on either side, the same k-mer: forward on one side, as its reverse complement on the other
    assert t.side_counts(0)[p] == 1 and t.side_counts(1)[p] == 1 and ridx[p] == x and lidx[p] == x
    assert ((info[p] >> 6) & 1) != ((info[p] >> 7) & 1)
    # seen from x, P is reported once, with strand bit 0 -- in the adjacency and in the info byte of the side it is the only neighbour of
    at = np.argwhere(nbr[x] == p).reshape(-1).tolist()
    assert len(at) == 1 and not strand[x, at[0]]
    side = at[0] & 1
    assert t.side_counts(side)[x] == 1 and (lidx if side else ridx)[x] == p and ((info[x] >> (7 if side else 6)) & 1) == 0
    assert t.side_counts(0)[t.where[t.note["pal2"]]] == 2
    w = t.note["interior"]
    assert UR.rc_plain(w, k - 2) == w
    fk = _fan_keys(t)
    assert len(fk) == 10 and all(y in t.where for y in fk)
    assert len(set(W.hash_of_keys(fk, k).tolist())) == 1
    assert int(pal.sum()) >= 2 + 4                          # P, P2 and the four a + I + (3 - a)


@pytest.mark.parametrize("k", W.KS)
def test_case_loops(k):
    t = W.get_case("loops", k)
    nbr, strand = t.neighbours
    info, ridx, lidx, pal = t.flags
    assert t.keys[0] == 0 and nbr[0, 0] == 0 and nbr[0, 1] == 0 and not strand[0, 0] and not strand[0, 1]       # code 0 k times: its own right and left neighbour
    loops = int((nbr == np.arange(len(t), dtype=np.uint32)[:, None]).sum())
    if k % 2:
        v = t.where[t.note["hairpin"]]
        at = np.argwhere(nbr[v] == v).reshape(-1).tolist()
        assert len(at) == 1 and strand[v, at[0]]            # the hairpin: itself, on the other strand
        assert t.side_counts(at[0] & 1)[v] == 2 and t.side_counts(1 - (at[0] & 1))[v] == 1
        assert loops >= 3
    else:
        assert int(pal.sum()) >= 3                          # windows of (AT)^n, (ACGT)^n, (AATT)^n
        assert loops >= 2
    # the windows of a sequence of period p are p k-mers in a cycle (or fewer canonical ones)
    assert len(t) <= 3 + 10 + 2 + 2 + 4 + 4


@pytest.mark.parametrize("k", W.KS)
def test_collision_fixture_and_case(k):
    pairs = W.collision_pairs(k)
    assert pairs
    for w1, w2 in pairs:
        assert w1 != w2 and all(w < (1 << (2 * k - 4)) and w <= UR.rc_plain(w, k - 2) for w in (w1, w2))
        h1, h2 = _key_hash(W.join(0, w1, 0, k), k), _key_hash(W.join(0, w2, 0, k), k)
        assert h1 >> 32 == h2 >> 32 and h1 & 1023 == h2 & 1023
        assert (W.hash_of_interior(w1, k), W.hash_of_interior(w2, k)) == (h1, h2)
    t = W.get_case("collision", k)
    w1, w2 = t.note["interiors"]
    assert (w1, w2) == pairs[0]
    home, tag = W.home_tag(t.hashes, 1024)
    for w in (w1, w2):
        assert UR.rc_plain(w, k - 2) != w
    mine = {w: [x for x in t.keys if min(W.interior(x, k), UR.rc_plain(W.interior(x, k), k - 2)) == w] for w in (w1, w2)}
    assert len(mine[w1]) == 8 and len(mine[w2]) == 8
    both = [t.where[x] for x in mine[w1] + mine[w2]]
    assert len(set(home[both].tolist())) == 1 and len(set(tag[both].tolist())) == 1
    # a sibling that is missing behind one interior is there behind the other, and the vertex that would find it walks the shared cluster
    nbr, _ = t.neighbours
    crossed = 0
    for wa, wb in ((w1, w2), (w2, w1)):
        for (a, b), x in W.fan(wa, k).items():
            if W.canon(x, k) not in t.where and W.canon(W.join(a, wb, b, k), k) in t.where:
                crossed += 1
                around = [((x << 2) | c) & ((1 << (2 * k)) - 1) for c in range(4)] + [(x >> 2) | (d << (2 * k - 2)) for d in range(4)]
                assert sum(W.canon(y, k) in t.where for y in around) == 4          # (two outer k-mers on either side would find it)
    assert crossed == 16
    absent_slots = int(((nbr == W.NONE) & np.isin(np.arange(len(t)), [i for i in range(len(t)) if i not in both])[:, None]).sum())
    assert absent_slots > 0


@pytest.mark.parametrize("k", W.SEAM_KS)
def test_case_seam(k):
    """4b. one tag, one home slot, one low word: a + I1 + b and a + I2 + b differ in the high word only, inside the interior.  (The low halves of
    w_side_walk's two compares alone cannot tell them apart; for k = 33, 34 no such pair can be built: see wnbr_ref.SEAM_KS)"""
    pairs = W.seam_pairs(k)
    assert pairs
    for w1, w2 in pairs:
        assert w1 != w2 and (w1 ^ w2) & ((1 << 62) - 1) == 0 and all(w < (1 << (2 * k - 4)) and w <= UR.rc_plain(w, k - 2) for w in (w1, w2))
        h1, h2 = _key_hash(W.join(0, w1, 0, k), k), _key_hash(W.join(0, w2, 0, k), k)
        assert h1 >> 32 == h2 >> 32 and h1 & 1023 == h2 & 1023
    t = W.get_case("seam", k)
    w1, w2 = t.note["interiors"]
    assert (w1, w2) == pairs[0] and W.cap_of(len(t)) == 1024
    f1, f2 = W.fan(w1, k), W.fan(w2, k)
    assert all(W.canon(x, k) in t.where for x in f1.values()) and not any(W.canon(x, k) in t.where for x in f2.values())
    forward = [ab for ab, x in f1.items() if W.canon(x, k) == x and W.canon(f2[ab], k) == f2[ab]]
    assert len(forward) >= 4 and all(f1[ab] & M64 == f2[ab] & M64 and f1[ab] >> 64 != f2[ab] >> 64 for ab in forward)
    # the outer k-mers of I2 are there, and their inner side -- the walk through I1's cluster -- finds nothing
    nbr, _ = t.neighbours
    lonely = 0
    for b in range(4):
        for c in range(4):
            y = (w2 << 4) | (b << 2) | c                    # I2 + b + c: its left neighbours are the a + I2 + b
            if W.canon(y, k) in t.where:
                v, side = t.where[W.canon(y, k)], (1 if W.canon(y, k) == y else 0)
                assert (nbr[v, side::2] == W.NONE).all()
                lonely += 1
    assert lonely == 8
    q, want, kinds = W.queries(t)
    asked = [i for i, kd in enumerate(kinds) if kd == "asked"]
    assert len(asked) == 32 and all(want[i] == -1 for i in asked) and {q[i] for i in asked} >= set(f2.values())


@pytest.mark.parametrize("k", W.KS)
@pytest.mark.parametrize("big", [False, True])
def test_case_wrap(k, big):
    t = W.get_case("wrap2048" if big else "wrap1024", k)
    cap = W.cap_of(len(t))
    assert cap == (2048 if big else 1024) and len(t) == (513 if big else 36)
    home = _check_fan(t)
    assert home >= cap - 3                                  # sixteen keys from there on: at least thirteen lie behind the end, from slot 0 on


@pytest.mark.parametrize("k", W.KS)
def test_case_broad_and_empty(k):
    t = W.get_case("broad", k)
    assert 4000 <= len(t) <= 6500
    nbr, strand = t.neighbours
    present = nbr != W.NONE
    assert present.sum() > len(t) and (present & strand).any() and (present & ~strand).any()
    e = W.get_case("empty", k)
    assert len(e) == 0 and W.cap_of(0) == 0


def test_collision_search_finds_what_it_says():
    """the search itself, at a size that takes no time: 12 tag bits and 4 slot bits"""
    k = 47
    pairs = W.collision_search(k, 5, draws=1 << 13, slot_bits=4, tag_bits=12)
    assert len(pairs) > 50
    for a, b in pairs:
        ha, hb = W.hash_of_interior(a, k), W.hash_of_interior(b, k)
        assert a < b and ha >> 52 == hb >> 52 and ha & 15 == hb & 15
        assert a <= UR.rc_plain(a, k - 2) and b <= UR.rc_plain(b, k - 2)
