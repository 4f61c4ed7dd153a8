"""The join core's union table (metafast_amd/csrc/mf_join.h, mf_join.hip: k_stats_init, k_stats_union in its four modes, mf_join_mine,
mf_join_find, k_join_read with its five projections) slot by slot against tests/join_ref.py, bit-exact, on the crafted keys of
tests/join_cases.py: clusters that run over the end of the table, a chain of 300, 300 lanes of one launch on one home slot, ghosts that walk
a whole cluster, keys on the slice borders, tables exactly full and over-full, a table of one slot.

The hooks mf_debug_join_plan / _union / _find / _read (mf_join.hip; bound here with ctypes, not part of the C-ABI) run the production functions
with a capacity the host would never pick.  The inputs need no GPU: tests/test_join_ref_cpu.py asserts what every case rests on.

The over-full table and the key >= 2^62 are defined error returns, not faults: both probe loops (k_stats_union, mf_join_find) end at
`probe <= mask`, and the pass reads its flag word afterwards.

Left out: a read-out with `nu` below the number of occupied slots (mf_join_read's piece has nu entries and the kernel writes one per kept slot:
the hook refuses it before the launch); the wide join (mf_wjoin.hip: no hash table)."""
import ctypes as C
import gc

import numpy as np
import pytest

import join_cases as JC
import join_ref as J

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------------
# the hooks
# ---------------------------------------------------------------------------------------------------------------------------------
def _so():
    from metafast_amd import lib as L
    so = L.lib()
    if getattr(so, "_join_hooks", None) is None:
        so.mf_debug_join_plan.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        so.mf_debug_join_union.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p,
                                           C.POINTER(C.c_uint64)]
        so.mf_debug_join_find.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
        so.mf_debug_join_read.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        for f in (so.mf_debug_join_plan, so.mf_debug_join_union, so.mf_debug_join_find, so.mf_debug_join_read):
            f.restype = C.c_int
        so._join_hooks = True
    return so


def plan(ctx, total):
    from metafast_amd import lib as L
    S, cap = C.c_uint32(), C.c_uint64()
    L._check(_so().mf_debug_join_plan(ctx.h, total, C.byref(S), C.byref(cap)))
    return S.value, cap.value


def union(ctx, tabs, b, mode, add, S, s, cap):
    """-> (slots SLOT[cap], n_union)"""
    from metafast_amd import lib as L
    h = (C.c_void_p * len(tabs))(*[t.h for t in tabs])
    a = np.asarray(add, dtype=np.uint32)
    assert len(a) == len(tabs)
    slots = np.zeros(cap, dtype=J.SLOT)
    n = C.c_uint64()
    L._check(_so().mf_debug_join_union(ctx.h, h, len(tabs), b, mode, a.ctypes.data, S, s, cap, slots.ctypes.data, C.byref(n)))
    return slots, n.value


def find(ctx, slots, keys, S=1, s=0):
    from metafast_amd import lib as L
    slots = np.ascontiguousarray(slots, dtype=J.SLOT)
    keys = np.array(keys, dtype=np.uint64)
    pos = np.zeros(len(keys), dtype=np.uint64)
    L._check(_so().mf_debug_join_find(ctx.h, slots.ctypes.data, len(slots), keys.ctypes.data, len(keys), S, s, pos.ctypes.data))
    return [int(p) for p in pos]


def read(ctx, slots, nu, proj, param=0):
    """-> the (key, value) pairs, sorted"""
    from metafast_amd import lib as L
    slots = np.ascontiguousarray(slots, dtype=J.SLOT)
    keys, vals = np.zeros(max(nu, 1), dtype=np.uint64), np.zeros(max(nu, 1), dtype=np.uint64)
    m = C.c_uint64()
    L._check(_so().mf_debug_join_read(ctx.h, slots.ctypes.data, len(slots), nu, proj, param, keys.ctypes.data, vals.ctypes.data, C.byref(m)))
    return sorted(zip((int(k) for k in keys[:m.value]), (int(v) for v in vals[:m.value])))


def raw_table(ctx, keys, counts):
    """a table that holds `counts` as they are, 65535 included.  mf_table_from_host sums a small or unordered input's duplicates through its index
    and bounds the sums at 32767; 4096 strictly ascending keys or more are taken as a k-mers file's records, counts untouched.  So the sample
    is filled up with keys of count 0 (no pass looks at an entry with count <= b, b >= 0) and sorted"""
    keys, counts = np.asarray(keys, np.uint64), np.asarray(counts, np.uint16)
    have = {int(k) for k in keys}
    pad = np.array([x for x in range(1, 2 * 4200, 2) if x not in have][:max(0, 4100 - len(keys))], dtype=np.uint64)
    k = np.concatenate([keys, pad])
    c = np.concatenate([counts, np.zeros(len(pad), np.uint16)])
    order = np.argsort(k)
    t = ctx.table_from_host(k[order], c[order], 31)
    gk, gc = t.export(-1)
    o2 = np.argsort(gk)
    assert np.array_equal(gk[o2], k[order]) and np.array_equal(gc[o2].astype(np.uint16), c[order]), "the table does not hold the counts as given"
    return t


def tables(ctx, samples):
    return [raw_table(ctx, k, c) if len(c) and int(np.max(c)) > 32767 else ctx.table_from_host(k, c, 31) for k, c in samples]


def live_bytes(ctx):
    return ctx.stat("arena_bytes") - ctx.stat("arena_idle_bytes")


def occupied(slots):
    return [int(k) for k in slots["key"] if int(k) != J.EMPTY]


# ---------------------------------------------------------------------------------------------------------------------------------
# union
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("cap", JC.CAPS)
def test_union_every_mode(gpu_ctx, cap, S):
    """the cohort of join_cases.cohort: 300 `last` keys in one sample (caps 512 and 4096: one launch contends for slot cap - 1 and the cluster
    wraps), the stair, the slice borders of S = 3, keys 0 and 2^62 - 1, entries with count <= b inside the clusters, counts of 65535"""
    samples = JC.cohort(cap, S)
    tabs = tables(gpu_ctx, samples)
    want_all = J.union_keys(samples, JC.B)
    for name, mode, add in JC.VARIANTS:
        seen = []
        for s in range(S):
            slots, n = union(gpu_ctx, tabs[:len(add)], JC.B, mode, add, S, s, cap)
            try:
                J.check_slots(slots, cap, S, s, samples[:len(add)], JC.B, mode, add, n)
            except J.SlotError as e:
                raise AssertionError("cap %d, S %d, s %d, %s: %s" % (cap, S, s, name, e)) from None
            seen.append(occupied(slots))
            if cap > 1:
                assert J.occupied_span_wraps(slots)
        # every key in exactly one slice: the slices' unions are disjoint and complete (the border keys of edges(3) among them)
        flat = [k for o in seen for k in o]
        assert len(flat) == len(set(flat)) and (len(add) < 5 or set(flat) == want_all), (cap, S, name)


def test_color_values_saturate(gpu_ctx):
    """17 samples of 65535 in value mode: 1 114 095 stops at 2^20 - 1 in its field, whichever field, and the neighbours keep what they had"""
    keys = np.array(JC.last(5) + JC.first(2) + [0], dtype=np.uint64)
    big = (keys, np.full(len(keys), 65535, np.uint16))
    small = [(keys, np.full(len(keys), c, np.uint16)) for c in (3, 1)]
    tabs = tables(gpu_ctx, [big] + small)
    for field in (0, 1, 2):
        others = [f for f in (0, 1, 2) if f != field]
        samples = [small[0]] + [big] * 17 + [small[1]]
        add = (others[0] | 4,) + (field | 4,) * 17 + (others[1] | 4,)
        slots, n = union(gpu_ctx, [tabs[1]] + [tabs[0]] * 17 + [tabs[2]], 0, J.COLOR, add, 1, 0, 8)
        J.check_slots(slots, 8, 1, 0, samples, 0, J.COLOR, add, n)
        assert n == 8
        for c, r in zip(slots["cnt"], slots["row"]):
            w = int(c) | (int(r) << 32)
            assert [(w >> (20 * f)) & J.FIELD_MAX for f in (field, others[0], others[1])] == [J.FIELD_MAX, 3, 1] and w >> 60 == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# exact fill, over-fill, key limit
# ---------------------------------------------------------------------------------------------------------------------------------
def test_exact_fill_overfill_and_key_limit(gpu_ctx):
    from metafast_amd import lib as L
    ctx = gpu_ctx
    right = JC.cohort(64, 3)
    right_tabs = tables(ctx, right)
    add5 = (1, 1 << 16, 1 << 10, 1 << 20, 0)

    def still_right():
        for s in range(3):
            slots, n = union(ctx, right_tabs, JC.B, J.PRESENCE, add5, 3, s, 64)
            J.check_slots(slots, 64, 3, s, right, JC.B, J.PRESENCE, add5, n)

    still_right()
    base = live_bytes(ctx)
    for cap in (1, 8):
        keys = JC.fill(cap, cap + 1)
        assert len(keys) == cap + 1
        halves = [(np.array(keys[:cap][::2], np.uint64), np.full(len(keys[:cap][::2]), 9, np.uint16)),
                  (np.array(keys[:cap], np.uint64), np.full(cap, 4, np.uint16))]
        over = (np.array(keys[cap:] + keys[:1], np.uint64), np.array([5, 6], np.uint16))         # the key too many, and one that is there already
        tabs = tables(ctx, halves + [over])
        before = live_bytes(ctx)
        for _, mode, add in JC.VARIANTS[:3] + JC.VARIANTS[5:]:
            slots, n = union(ctx, tabs[:2], 0, mode, add[:2], 1, 0, cap)
            J.check_slots(slots, cap, 1, 0, halves, 0, mode, add[:2], n)
            assert n == cap and len(occupied(slots)) == cap                                       # cap keys into cap slots: every slot occupied
            with pytest.raises(L.MetafastError, match="the union table of a slice is full"):
                union(ctx, tabs, 0, mode, add[:3], 1, 0, cap)
            assert live_bytes(ctx) == before
            still_right()
        del tabs
    # a key >= 2^62 is refused for every slice: mf_join_mine raises the flag before it looks at the slice
    for bad_key in (J.KEY_LIMIT, J.M64 - 1):
        big = ctx.table_from_host(np.array([5, bad_key], np.uint64), np.array([3, 3], np.uint16), 31)
        for S in (1, 3):
            for s in range(S):
                for _, mode, add in JC.VARIANTS[:2] + JC.VARIANTS[5:6]:
                    with pytest.raises(L.MetafastError, match=r"a k-mer key >= 2\^62"):
                        union(ctx, right_tabs[:2] + [big], 0, mode, add[:3], S, s, 64)
        # ... unless its count is <= b: the entry is dropped before its key is looked at
        for s in range(3):
            slots, n = union(ctx, right_tabs[:2] + [big], 3, J.SUM, (0, 0, 0), 3, s, 64)
            J.check_slots(slots, 64, 3, s, right[:2] + [(np.zeros(0, np.uint64), np.zeros(0, np.uint16))], 3, J.SUM, (0, 0, 0), n)
        del big
        still_right()
    gc.collect()
    assert live_bytes(ctx) == base
    # the hook's own refusals
    for cap in (0, 3, 48, 1 << 25):
        with pytest.raises(L.MetafastError, match="not a power of two"):
            union(ctx, right_tabs, 0, J.SUM, (0,) * 5, 1, 0, cap)
    with pytest.raises(L.MetafastError, match="slice 3 of 3"):
        union(ctx, right_tabs, 0, J.SUM, (0,) * 5, 3, 3, 64)


# ---------------------------------------------------------------------------------------------------------------------------------
# find
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("cap", [8, 64, 512])
def test_find_on_union_tables(gpu_ctx, cap, S):
    samples = JC.cohort(cap, S)
    tabs = tables(gpu_ctx, samples)
    held = sorted(J.union_keys(samples, JC.B))
    ghosts = JC.ghosts(cap, S)
    low_only = JC.held_keys(cap, S)["low_only"]
    for s in range(S):
        slots, n = union(gpu_ctx, tabs, JC.B, J.SUM, (0,) * 5, S, s, cap)
        J.check_slots(slots, cap, S, s, samples, JC.B, J.SUM, (0,) * 5, n)
        at = {int(k): p for p, k in enumerate(slots["key"]) if int(k) != J.EMPTY}
        queries = held + [k for k, _, _ in ghosts] + low_only + [J.KEY_LIMIT, J.KEY_LIMIT + 5, J.M64 - 1, J.M64]
        got = find(gpu_ctx, slots, queries, S, s)
        for k, p in zip(queries, got):
            mine = k < J.KEY_LIMIT and J.slice_of(J.hash64(k), S) == s
            want = J.NOT_MINE if not mine else at.get(k, J.NOT_FOUND)
            assert p == want == J.find(slots, k, S, s), (cap, S, s, hex(k), p, want)
        assert sum(1 for p in got if p == J.NOT_FOUND) == sum(1 for k in [g for g, _, _ in ghosts] + low_only if J.slice_of(J.hash64(k), S) == s)
        assert sum(1 for p in got if p < cap) == n


def test_find_on_hand_built_tables(gpu_ctx):
    # a full table of 8 slots and an absent key, home by home: the probe ends after 8 steps
    keys = JC.fill(8, 8)
    full = J.empty_table(8)
    for i, k in enumerate(keys):
        assert J.insert(full, k, (i, 100 + i)) is not None
    assert len(occupied(full)) == 8
    absent = [JC.at(v, 1, skip=JC.GHOST_SKIP)[0] for v in range(8)] + JC.last(2, skip=JC.GHOST_SKIP)
    assert sorted(J.home(k, 8) for k in absent[:8]) == list(range(8))
    got = find(gpu_ctx, full, keys + absent)
    assert got == [J.walk(full, k)[0] for k in keys] + [J.NOT_FOUND] * len(absent) and sorted(got[:8]) == list(range(8))
    # one slot, mask 0: the key it holds, an absent key, and the empty table
    one = J.empty_table(1)
    J.insert(one, keys[0], (1, 2))
    assert find(gpu_ctx, one, [keys[0], keys[1], 0, J.KEY_LIMIT]) == [0, J.NOT_FOUND, J.NOT_FOUND, J.NOT_MINE]
    assert find(gpu_ctx, J.empty_table(1), [keys[0], 0]) == [J.NOT_FOUND, J.NOT_FOUND]
    assert find(gpu_ctx, one, [keys[0]], 3, J.slice_of(J.hash64(keys[0]), 3)) == [0]
    assert find(gpu_ctx, one, [keys[0]], 3, (J.slice_of(J.hash64(keys[0]), 3) + 1) % 3) == [J.NOT_MINE]
    # a table the union kernel would not build: a key behind an empty slot is not found (the probe stops at the empty slot)
    t = J.empty_table(64)
    k0, k1 = JC.at(10, 2)
    t["key"][10], t["key"][12] = k0, k1
    assert find(gpu_ctx, t, [k0, k1]) == [10, J.NOT_FOUND]
    # the wrapped cluster by hand: 5 keys of home 63 in 63, 0, 1, 2, 3; a ghost of home 63 walks all of them, one of home 4 none
    w = J.empty_table(64)
    lk = JC.last(5)
    assert [J.insert(w, k) for k in lk] == [63, 0, 1, 2, 3]
    g = JC.last(1, skip=JC.GHOST_SKIP) + JC.at(4, 1, skip=JC.GHOST_SKIP) + JC.at(2, 1, skip=JC.GHOST_SKIP)
    assert find(gpu_ctx, w, lk + g) == [63, 0, 1, 2, 3] + [J.NOT_FOUND] * 3
    # slice borders: each border key is its own slice's and no other's
    e = JC.edges(3, 2)
    for s in range(3):
        got = find(gpu_ctx, J.empty_table(8), [k for _, k in e], 3, s)
        assert got == [J.NOT_FOUND if J.slice_of(tp << 32, 3) == s else J.NOT_MINE for tp, _ in e]


# ---------------------------------------------------------------------------------------------------------------------------------
# read
# ---------------------------------------------------------------------------------------------------------------------------------
def _hand_table(cap, payloads):
    """`cap` slots with len(payloads) occupied ones scattered over it (a read-out looks at no home): keys 0, 2^62 - 1 and crafted ones"""
    t = J.empty_table(cap, J.PRESENCE)
    keys = ([0, J.KEY_LIMIT - 1] + JC.last(len(payloads)))[:len(payloads)]
    where = np.random.default_rng(cap).permutation(cap)[:len(payloads)]
    for p, k, (c, r) in zip(where, keys, payloads):
        t["key"][p], t["cnt"][p], t["row"][p] = k, c, r
    return t


@pytest.mark.parametrize("cap", [1, 8, 32, 64, 128, 512, 4096])
def test_read_projections(gpu_ctx, cap):
    """every projection on hand-built slots.  A capacity is a power of two, so `no multiple of 256` means below 256: at 1, 8, 32 a part of one
    wave holds slots, at 64 and 128 whole waves of a workgroup hold none, and all of them reach mf_wave_reserve"""
    from metafast_amd import lib as L
    sums = [0, 1, 0x7FFE, 0x7FFF, 0x8000, 0x8001, 0xFFFE, 0xFFFF, 0x10000, 3 * 65535, 32766, 32767, 32768, 5 | J.KNOCKED, 0x7FFF | J.KNOCKED,
            0xFFFF | J.KNOCKED, J.KNOCKED]
    cnts = [0, 1, 2, 0xFFFF, 0x10000, 0x10007, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 20, 300, 1 << 16, 1 << 20, 1 << 10, 5, 6, 7]
    payloads = [(c, r) for c, r in zip(cnts, sums)] + [(c, J.NO_ROW) for c in cnts] + [(0xABCDE | 0x123 << 20, 0x45 | 0xFFFFF << 8)]
    payloads = payloads[:max(1, min(len(payloads), cap - cap // 4))]
    t = _hand_table(cap, payloads)
    nu = len(payloads)
    for proj, params in ((J.P_NSAMPLES, (0,)), (J.P_KPS, (-3, 0, 1, 2, 7, 301, 0x7FFFFFFF)), (J.P_COLOR, (0,)),
                         (J.P_UKM, (-32769, -32768, -2, -1, 0, 1, 32765, 32766, 32767)), (J.P_UK, (0,))):
        for param in params:
            want = J.read(t, proj, param)
            assert read(gpu_ctx, t, nu, proj, param) == want, (cap, proj, param)
            if J.ALL[proj]:
                assert len(want) == nu
                # a claimed size that the table does not have
                with pytest.raises(L.MetafastError, match="%d union entries written, %d claimed" % (nu, nu + 1)):
                    read(gpu_ctx, t, nu + 1, proj, param)
            else:
                assert read(gpu_ctx, t, nu + 3, proj, param) == want                   # (a bound: fewer may come out)
    if cap >= 8:
        # kps keeps the count-0 entries at thresh <= 0 and drops them at 1
        zero = {int(k) for k, c in zip(t["key"], t["cnt"]) if int(k) != J.EMPTY and int(c) == 0}
        assert zero and zero <= {k for k, _ in read(gpu_ctx, t, nu, J.P_KPS, 0)} and not zero & {k for k, _ in read(gpu_ctx, t, nu, J.P_KPS, 1)}
        # ukm: the packed value, and the three sum words as Java shorts against thr = 0: 0x7FFF stays, 0x8000 and 0xFFFF go
        got = dict(read(gpu_ctx, t, nu, J.P_UKM, 0))
        by_sum = {int(r): (int(k), int(c)) for k, c, r in zip(t["key"], t["cnt"], t["row"]) if int(k) != J.EMPTY}
        if 0x7FFF in by_sum and 0xFFFF in by_sum:
            k, c = by_sum[0x7FFF]
            assert got[k] == 0x7FFF | ((c << 16) & 0xFFFFFFFF) and by_sum[0x8000][0] not in got and by_sum[0xFFFF][0] not in got
            assert by_sum[5 | J.KNOCKED][0] not in got
            uk = dict(read(gpu_ctx, t, nu, J.P_UK))
            assert uk[by_sum[32766][0]] == 32766 and uk[by_sum[32768][0]] == 32767 and uk[by_sum[3 * 65535][0]] == 32767 and uk[by_sum[5 | J.KNOCKED][0]] == 0
    # the empty table
    e = J.empty_table(cap)
    for proj in range(5):
        assert read(gpu_ctx, e, 0, proj) == []
    with pytest.raises(L.MetafastError, match="would write past its piece"):
        read(gpu_ctx, t, nu - 1, J.P_COLOR)


def test_plan_hook(gpu_ctx):
    try:
        for S in (1, 3, 7):
            gpu_ctx.set_option("stats_slices", S)
            for total in (0, 1, 1000, 3000, 123457, 1_000_000):
                assert plan(gpu_ctx, total) == (S, J.cap_of(total, S))
    finally:
        gpu_ctx.set_option("stats_slices", 0)
    S, cap = plan(gpu_ctx, 1000)                          # (0: as many slices as free memory asks for -- one, for a table of 128 KiB)
    assert (S, cap) == (1, J.cap_of(1000, 1))
