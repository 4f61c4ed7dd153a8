"""tests/join_ref.py and tests/join_cases.py without a GPU: the hash and its inverse, every key family's property, what each named case of
tests/test_join_slots_gpu.py and tests/test_join_crafted_gpu.py promises, the capacity formula, and check_slots itself -- it accepts every
table a plain linear-probing simulator makes in shuffled orders and rejects each doctored table with the invariant's name."""
import numpy as np
import pytest

import join_cases as JC
import join_ref as J


def test_hash_pins_and_round_trip():
    assert J.hash64(0) == 0 and J.hash64(1) == 0xb456bcfc34c2cb2c
    rng = np.random.default_rng(1)
    for x in [0, 1, J.M64, J.KEY_LIMIT - 1, J.KEY_LIMIT, 1 << 63] + [int(v) for v in rng.integers(0, 1 << 63, size=2000, dtype=np.uint64)]:
        assert J.unhash64(J.hash64(x)) == x and J.hash64(J.unhash64(x)) == x
    # numpy's wrapping arithmetic agrees with the integers
    v = rng.integers(0, 1 << 63, size=500, dtype=np.uint64)
    h = v.copy()
    h ^= h >> np.uint64(33)
    h *= np.uint64(0xff51afd7ed558ccd)
    h ^= h >> np.uint64(33)
    h *= np.uint64(0xc4ceb9fe1a85ec53)
    h ^= h >> np.uint64(33)
    assert [int(x) for x in h] == [J.hash64(int(x)) for x in v]


def test_slice_of_borders():
    for S in (1, 3, 7, 16):
        assert J.slice_of(0, S) == 0 and J.slice_of(J.M64, S) == S - 1
        for s in range(1, S):
            c = -((-s << 32) // S)
            assert J.slice_of(c << 32, S) == s and J.slice_of(((c - 1) << 32) | 0xFFFFFFFF, S) == s - 1


def test_cap_of_pins():
    # 2 (per + 6 sqrt(per) + 1024), truncated, then the power of two at or above it
    assert J.cap_of(0, 1) == 2048 and J.cap_of(1, 1) == 4096 and J.cap_of(0, 7) == 2048
    assert J.cap_of(1000, 1) == 8192                    # 2 (1000 + 189.7 + 1024) = 4427
    assert J.cap_of(1000, 3) == 4096                    # 2 (333.3 + 109.5 + 1024) = 2933
    assert J.cap_of(3000, 7) == 4096                    # 2 (428.6 + 124.2 + 1024) = 3153
    assert J.cap_of(1 << 20, 1) == 1 << 22              # 2 (1048576 + 6144 + 1024) = 2111488
    assert J.cap_of(1_000_000, 3) == 1 << 20            # 2 (333333.3 + 3464.1 + 1024) = 675642
    assert [J.index_cap_of(m) for m in (0, 1, 2, 3, 300, 512, 513)] == [2, 2, 4, 8, 1024, 1024, 2048]


def _family_ok(keys, n, v=None, top32=None):
    assert len(keys) == n and len(set(keys)) == n and all(0 <= k < J.KEY_LIMIT for k in keys)
    for k in keys:
        h = J.hash64(k)
        assert v is None or h & JC.LOW_MASK == v
        assert top32 is None or h >> 32 == top32


def test_families():
    for t in JC.TOPS:
        assert len(JC.candidates(JC.LOW_MASK, t)) >= JC.GHOST_SKIP + 3 and len(JC.candidates(0, t)) >= JC.GHOST_SKIP + 3
    assert [J.slice_of(t << 32, 3) for t in JC.TOPS] == [0, 1, 2]
    _family_ok(JC.last(300), 300, JC.LOW_MASK, JC.TOPS[0])
    _family_ok(JC.first(20, JC.TOPS[2]), 20, 0, JC.TOPS[2])
    _family_ok(JC.at(12345, 9, JC.TOPS[1]), 9, 12345, JC.TOPS[1])
    for cap in (1, 8, 64, 512, 4096, 1 << 20):
        assert {J.home(k, cap) for k in JC.last(50)} == {cap - 1} and {J.home(k, cap) for k in JC.first(50)} == {0}
        assert {J.home(k, cap) for k in JC.at(37, 5)} == {37 & (cap - 1)}
    st = JC.stair(37, 6, 5)
    _family_ok(st, 30, None, JC.TOPS[0])
    assert [J.home(k, 512) for k in st] == [37 + i for i in range(6) for _ in range(5)]
    assert not set(JC.last(300)) & set(JC.last(3, skip=JC.GHOST_SKIP)) and not set(JC.last(300)) & set(JC.last(3, skip=300))
    for S in (3, 7):
        e = JC.edges(S)
        tops = JC.edge_tops(S)
        assert len(tops) == 2 * S and len(e) == 8 * 2 * S
        _family_ok([k for _, k in e], len(e))
        for t, k in e:
            assert J.hash64(k) >> 32 == t
        for s in range(1, S):
            below = [t for t in tops if J.slice_of(t << 32, S) == s - 1]
            above = [t for t in tops if J.slice_of(t << 32, S) == s]
            assert max(below) + 1 == min(above)                        # the two values of border s are neighbours, one a slice
        assert J.slice_of(0, S) == 0 and J.slice_of(0xFFFFFFFF << 32, S) == S - 1
    assert J.hash64(0) == 0 and J.KEY_LIMIT - 1 < J.KEY_LIMIT
    f = JC.fill(8, 9)
    _family_ok(f, 9, None, JC.TOPS[0])


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("cap", JC.CAPS)
def test_cohorts_hold_what_their_names_promise(cap, S):
    d = JC.held_keys(cap, S)
    samples = JC.cohort(cap, S)
    assert len(samples) == 5
    for keys, counts in samples:
        assert len(set(int(k) for k in keys)) == len(keys) == len(counts) and all(int(k) < J.KEY_LIMIT for k in keys)
    union = J.union_keys(samples, JC.B)
    every = d["last"] + d["first"] + d["stair"] + d["edges"] + d["special"]
    assert len(set(every)) == len(every) and union == set(every)
    assert not set(d["low_only"]) & union and (cap == 1 or len(d["low_only"]) == 3 * S)
    assert {int(c) for c in samples[2][1]} == {65535} and len(samples[0][0]) >= len(d["last"])
    if cap >= 512:
        assert len(d["last"]) == 300 * S and set(d["last"]) <= {int(k) for k in samples[0][0]}       # 300 lanes of one launch, one home slot
    per_slice = [sum(1 for k in union if J.slice_of(J.hash64(k), S) == s) for s in range(S)]
    assert all(1 <= n <= cap for n in per_slice), per_slice
    for s in range(S):
        slots, n = J.simulate(cap, samples, JC.B, J.SUM, (0,) * 5, S, s)
        assert n == per_slice[s]
        if cap > 1:
            assert J.occupied_span_wraps(slots)                                                       # the `last` cluster crosses cap - 1 -> 0
        lo = [k for k in d["low_only"] if J.slice_of(J.hash64(k), S) == s]
        assert all(int(slots["key"][J.home(k, cap)]) != J.EMPTY and J.walk(slots, k)[0] == J.NOT_FOUND for k in lo)
        # every ghost is absent, and its probe passes the occupied slots its case states
        for k, why, least in JC.ghosts(cap, S):
            if J.slice_of(J.hash64(k), S) != s:
                continue
            assert k not in union
            pos, steps = J.walk(slots, k)
            assert pos == J.NOT_FOUND and steps >= least, (why, steps, least)
        if cap == 512:
            assert max(J.walk(slots, k)[1] for k in union if J.slice_of(J.hash64(k), S) == s) >= 299    # a long chain
    if S == 3 and d["edges"]:
        tops = {J.hash64(k) >> 32 for k in d["edges"]}
        assert tops == set(JC.edge_tops(3))


def test_crafted_cohort_of_the_tools():
    """what tests/test_join_crafted_gpu.py rests on: sizes, ghosts in no sample, clusters that wrap in every slice of the tables the plan gives
    (2048 .. 16384 slots for 1200 .. 2400 entries in 1, 3 or 7 slices), the rule behind kmers-per-sample's selection"""
    p = JC.crafted_pool()
    pool = p["last"] + p["rest"]
    assert 550 <= len(pool) <= 620 and len(p["last"]) == 300 and all(k < J.KEY_LIMIT for k in pool + p["ghosts"])
    plain, kps = JC.crafted_cohort(), JC.crafted_cohort(seed=3, kps=True)
    for s in plain + kps + [JC.with_ghosts(plain[0])]:
        assert len(s[0]) == len(set(int(k) for k in s[0])) <= 620 and int(s[1].min()) >= 1
    for s in plain + kps:
        assert not set(int(k) for k in s[0]) & set(p["ghosts"])
    assert set(p["ghosts"]) <= set(int(k) for k in JC.with_ghosts(plain[0])[0])
    assert {J.slice_of(J.hash64(k), 3) for k in p["last"]} == {0, 1, 2} and len({J.slice_of(J.hash64(k), 7) for k in pool}) == 7
    assert {J.hash64(k) >> 32 for k in pool} >= set(JC.edge_tops(3)) | set(JC.edge_tops(7))
    for S in (1, 3, 7):
        for total in (1200, 2400):
            cap = J.cap_of(total, S)
            assert 2048 <= cap <= 16384
            for s in range(S):
                slots, n = J.simulate(cap, plain, 0, J.SUM, (0,) * 6, S, s)
                mine = [k for k in p["last"] if J.slice_of(J.hash64(k), S) == s]
                if mine:
                    assert J.occupied_span_wraps(slots) and max(J.walk(slots, k)[1] for k in mine) >= 50
                for g in p["ghosts"]:
                    if J.slice_of(J.hash64(g), S) == s:
                        assert J.walk(slots, g)[0] == J.NOT_FOUND
                heads = [g for g in p["ghosts"] if J.hash64(g) & JC.LOW_MASK == JC.LOW_MASK and J.slice_of(J.hash64(g), S) == s]
                assert all(J.walk(slots, g)[1] >= 50 for g in heads) and (not mine or heads)
    # kmers-per-sample at percent 80: a `last` key is in all six samples, no other key in more than three
    held = {}
    for s in kps:
        for k in s[0]:
            held[int(k)] = held.get(int(k), 0) + 1
    assert all(held[k] == 6 for k in p["last"]) and all(held.get(k, 0) <= 3 for k in p["rest"])
    assert J.index_cap_of(300) == 1024


def _shuffled_tables(cap, S, mode, add, seeds=(0, 1, 2)):
    samples = JC.cohort(cap, S)[:len(add)]
    for s in range(S):
        for seed in seeds:
            slots, n = J.simulate(cap, samples, JC.B, mode, add, S, s, np.random.default_rng(seed))
            yield samples, s, slots, n


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("cap", [1, 8, 64, 512])
def test_check_slots_accepts_the_simulator(cap, S):
    placed = set()
    for _, mode, add in JC.VARIANTS:
        for samples, s, slots, n in _shuffled_tables(cap, S, mode, add):
            J.check_slots(slots, cap, S, s, samples, JC.B, mode, add, n)
            placed.add((s, slots["key"].tobytes()))
            # the model of the probe finds every key where it lies
            for p, k in enumerate(slots["key"]):
                if int(k) != J.EMPTY:
                    assert J.find(slots, int(k), S, s) == p and (S == 1 or J.find(slots, int(k), S, (s + 1) % S) == J.NOT_MINE)
    if cap >= 64:
        assert len(placed) > S                          # the orders really place keys differently


def _doctor(slots, what, mode):
    """-> a doctored copy of the cap-64 cohort's table ("n_union off by one" leaves the table alone)"""
    t = slots.copy()
    occ = [p for p in range(len(t)) if int(t["key"][p]) != J.EMPTY]
    emp = [p for p in range(len(t)) if int(t["key"][p]) == J.EMPTY]
    if what == "moved behind an empty slot":
        p = occ[0]
        q = next(e for e in emp if (e - 1) % len(t) in emp)              # an empty slot behind an empty slot
        t[q] = t[p]
        t["key"][p] = J.EMPTY
        t["cnt"][p], t["row"][p] = J.initial_payload(mode)
    elif what == "present twice":
        t[emp[0]] = t[occ[0]]
    elif what == "lost":
        t["key"][occ[-1]] = J.EMPTY
        t["cnt"][occ[-1]], t["row"][occ[-1]] = J.initial_payload(mode)
    elif what == "payloads swapped":
        a = occ[0]
        b = next(p for p in occ if (t["cnt"][p], t["row"][p]) != (t["cnt"][a], t["row"][a]))
        t["cnt"][[a, b]] = t["cnt"][[b, a]]
        t["row"][[a, b]] = t["row"][[b, a]]
    elif what == "empty payload dirtied":
        t["cnt"][emp[0]] += 1
    elif what == "carry":
        # FIELD: cd ran over into uc; COLOR: field 0 ran over into field 1
        p = occ[0]
        if mode == J.FIELD:
            t["cnt"][p] = (int(t["cnt"][p]) + 0x10000) & 0xFFFFFFFF
        else:
            w = (int(t["cnt"][p]) | (int(t["row"][p]) << 32)) + (1 << 20)
            t["cnt"][p], t["row"][p] = w & 0xFFFFFFFF, (w >> 32) & 0xFFFFFFFF
    return t


@pytest.mark.parametrize("what,invariant", [("moved behind an empty slot", "reachable"), ("present twice", "occupied"), ("lost", "occupied"),
                                            ("payloads swapped", "payload"), ("empty payload dirtied", "empty"), ("n_union off by one", "n_union"),
                                            ("carry", "payload")])
def test_check_slots_rejects_doctored_tables(what, invariant):
    cap = 64
    for _, mode, add in JC.VARIANTS:
        if what == "carry" and mode not in (J.FIELD, J.COLOR):
            continue
        samples = JC.cohort(cap, 1)[:len(add)]
        slots, n = J.simulate(cap, samples, JC.B, mode, add, rng=np.random.default_rng(5))
        J.check_slots(slots, cap, 1, 0, samples, JC.B, mode, add, n)
        for dn in ((1, -1) if what == "n_union off by one" else (0,)):
            with pytest.raises(J.SlotError) as e:
                J.check_slots(_doctor(slots, what, mode), cap, 1, 0, samples, JC.B, mode, add, n + dn)
            assert e.value.invariant == invariant and str(e.value).startswith(invariant + ":"), (what, mode, str(e.value))


def test_payload_model_edges():
    k = np.array([5], np.uint64)
    full = (k, np.array([65535], np.uint16))
    # SUM: the sum's carry never reaches the sample count; FIELD: each field filled to the last bit, none runs over
    assert J.expected_payloads([full] * 3, 0, J.SUM, (0, 0, 0)) == {5: (3, 3 * 65535)}
    assert J.expected_payloads([full] * 3, 0, J.FIELD, (0, 1, 2)) == {5: (0xFFFFFFFF, 65535)}
    # COLOR: 17 x 65535 = 1114095 stops at 2^20 - 1 in the middle field, the neighbours keep 3 and 1
    low = (k, np.array([3], np.uint16))
    one = (k, np.array([1], np.uint16))
    got = J.expected_payloads([low] + [full] * 17 + [one], 0, J.COLOR, (4,) + (5,) * 17 + (6,))
    w = got[5][0] | (got[5][1] << 32)
    assert (w & J.FIELD_MAX, (w >> 20) & J.FIELD_MAX, (w >> 40) & J.FIELD_MAX, w >> 60) == (3, J.FIELD_MAX, 1, 0)
    assert J.expected_payloads([full, one], 1, J.PRESENCE, (1, 1 << 16)) == {5: (1, J.NO_ROW)}       # count 1 <= b brings nothing


def test_projections():
    # kps: the count as a signed word against thresh; thresh <= 0 keeps count 0
    assert J.project(0, J.NO_ROW, J.P_KPS, 0) == 0 and J.project(0, J.NO_ROW, J.P_KPS, 1) is None and J.project(3, J.NO_ROW, J.P_KPS, -2) == 3
    # ukm: Java shorts -- 0x7FFF = 32767, 0x8000 = -32768, 0xFFFF = -1
    assert J.project(2, 0x7FFF, J.P_UKM, 32766) == 0x7FFF | 2 << 16 and J.project(2, 0x7FFF, J.P_UKM, 32767) is None
    assert J.project(2, 0x8000, J.P_UKM, 0) is None and J.project(2, 0x8000, J.P_UKM, -32769) == 0x8000 | 2 << 16
    assert J.project(1, 0xFFFF, J.P_UKM, -2) == 0xFFFF | 1 << 16 and J.project(1, 0xFFFF, J.P_UKM, -1) is None
    assert J.project(1, 5 | J.KNOCKED, J.P_UKM, 0) is None and J.project(0x12345, 5, J.P_UKM, 0) == 5 | 0x2345 << 16
    # uk: bounded at 32767, 0 where knocked out
    assert [J.project(1, r, J.P_UK) for r in (0, 32766, 32767, 32768, 3 * 65535, 9 | J.KNOCKED)] == [0, 32766, 32767, 32767, 32767, 0]
    assert J.project(0x10007, 9, J.P_NSAMPLES) == 7 and J.project(0x10007, 9, J.P_COLOR) == 0x10007 | 9 << 32
