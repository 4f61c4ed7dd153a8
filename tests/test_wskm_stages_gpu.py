"""The wide record path (metafast_amd/csrc/mf_wskm.hip: 32 <= k <= 63) stage by stage against tests/wskm_ref.py: k_wskm_scan's records, the partition
sort with k_wskm_offsets and k_wskm_units, k_wskm_pack, k_wskm_count's raw output and counters, and mf_wide_order with k_wskm_place's run bound.

mf_debug_wskm_records (mf_wskm.hip; bound here with ctypes, not part of the C-ABI) runs what mf_count_wide_device_above runs with the context's
options and hands over what every stage left for the next one; mf_debug_wide_order runs mf_wide_order on entries given from the host and says how
many it set aside and whether the leading-bits route was kept.  Every comparison is bit-exact.  tests/test_wskm_ref_cpu.py asserts, from the
reference alone, that every crafted input below has the property it is there for.

The issue asked for counters[2] > 0 "on the small-unit case": a small unit cannot overflow the table (it holds fewer k-mers, not more), so the
case that must overflow here is random reads counted in units of 20000 occurrences, beside the crafted heavy partition."""
import ctypes as C

import numpy as np
import pytest

import nbr_ref as R
import skm_ref as S
import wskm_ref as W
from test_wide_gpu import _reads
from util import pack_reads

gpu = pytest.mark.gpu

# (tests/test_count_gpu.py: OPTION_DEFAULTS)
DEFAULTS = (("wide_skm", 1), ("wide_skm_min", 1 << 20), ("wide_skm_lazy_order", 1), ("wide_skm_fine", 8), ("wide_skm_pack", 1), ("wide_skm_merge", 1),
            ("wide_skm_lead", 1), ("wide_skm_unit", 2400))
SCAN_KS = [32, 33, 34, 35, 47, 48, 62, 63]        # W = k - 14 15-mers: 18, 19, 20, 21 (= 3 x 7: the last window of 7 lands on the one before), 33, 34, 48, 49


@pytest.fixture(autouse=True)
def _wide_options_back(request):
    yield
    if "gpu_ctx" in request.fixturenames:
        ctx = request.getfixturevalue("gpu_ctx")
        for name, v in DEFAULTS:
            ctx.set_option(name, v)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs (no GPU needed: tests/test_wskm_ref_cpu.py runs the reference on them)
# ---------------------------------------------------------------------------------------------------------------------------------
def _random(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(n))].tobytes()


def ragged(k, n=3000):
    """reads of 20 .. 220 bases from a genome of 4000 at 1 % error: many shorter than k, a poly-A stretch, (AT)n"""
    return _reads(np.random.default_rng(900 + k), n, 20, 220)


def long_read(k):
    """one read of 10000 bases -- it crosses two whole tiles -- beside short ones"""
    rng = np.random.default_rng(1000 + k)
    return pack_reads([_random(rng, n) for n in (70, 130, 10000, 64, 90, 200)])


BORDER_STARTS = (4095, 2 * 4096, 3 * 4096 + 1)        # reads that start at tile positions 4095, 4096 (= 0) and 4097 (= 1)
BORDER_LAST = (4 * 4096 - 1, 5 * 4096)                # reads whose last k-mer starts at tile positions 4095 and 4096 (= 0)


def tile_borders(k):
    rng = np.random.default_rng(1100 + k)
    reads, at = [], 0

    def fill_to(p):
        nonlocal at
        while at < p:
            n = p - at if p - at < 260 else int(rng.integers(40, 200))
            reads.append(_random(rng, n)); at += n
    for s in BORDER_STARTS:
        fill_to(s)
        reads.append(_random(rng, 150)); at += 150
    for s in BORDER_LAST:
        fill_to(s + k - 150)
        reads.append(_random(rng, 150)); at += 150
        assert at == s + k
    fill_to(at + 300)
    return pack_reads(reads)


def long_runs(k):
    """poly-A and (AT)n of 300 bases: one minimizer from end to end, runs of 301 - k k-mers in front of the first tile border"""
    rng = np.random.default_rng(1200 + k)
    return pack_reads(["A" * 300, "AT" * 150, _random(rng, 100), "T" * 120, _random(rng, 180)])


def short_and_empty(k):
    """reads shorter than k and empty reads between long ones (with min_len = 100: the reads of 64 .. 99 bases give nothing either)"""
    rng = np.random.default_rng(1300 + k)
    lens = [150, 0, k - 1, 0, 0, 120, k, 99, 100, 1, k + 1, 64, 0, 210, 31, 101, 0]
    return pack_reads([_random(rng, n) for n in lens] * 12)


def one_kmer_reads(k, n=6000):
    """reads of exactly k bases: a record per k-mer occurrence, more than the scan's first room takes"""
    rng = np.random.default_rng(1400 + k)
    return np.frombuffer(_random(rng, n * k), dtype=np.uint8).copy(), np.arange(n + 1, dtype=np.uint64) * np.uint64(k)


def many_copies(k, copies=1500):
    """20 reads of 40 .. 70 bases, `copies` of each one after the other: identical records by the thousand (a record holds the 112 bases from its
    start, whatever read they belong to: the copies of a read give identical records where the same read follows them)"""
    rng = np.random.default_rng(1500 + k)
    reads = [_random(rng, n) for n in rng.integers(max(40, k), max(71, k + 20), size=20)]
    return pack_reads([reads[i] for i in np.repeat(np.arange(20), copies)])


def unique_reads(k, n=600):
    """random reads of 150 bases: every k-mer once (units hold as many distinct k-mers as occurrences)"""
    rng = np.random.default_rng(1600 + k)
    return pack_reads([_random(rng, 150) for _ in range(n)])


def heavy_partition(k=47, n=400):
    """random(47) + LOW + random(47), LOW the 15-mer with the smallest hash of the order: the 33 k-mers of a read that hold LOW whole have it as
    their minimizer -- 13200 distinct k-mers in one partition, more than 4 x 2800: two levels of class splitting"""
    rng = np.random.default_rng(1700 + k)
    low = S.decode(R.low_mmers(15, 1)[0][0], 15).encode()
    return pack_reads([_random(rng, 47) + low + _random(rng, 47) for _ in range(n)])


def saturating_copies(k=63, n=70000):
    rng = np.random.default_rng(1800 + k)
    return pack_reads([_random(rng, 64)] * n)


def tiny(k):
    """fewer occurrences than one partition takes: pbits = 0"""
    rng = np.random.default_rng(1900 + k)
    return pack_reads([_random(rng, k + 40), _random(rng, k - 1), _random(rng, k + 99)])


def order_entries(k, seed, runs, background):
    """distinct entries in random order: `background` random ones + runs of equal leading 32 bits, runs = [(leading value, length)] -> hi, lo, cnt"""
    rng = np.random.default_rng(seed)
    tail_bits = 2 * k - 32

    def tail():
        return int.from_bytes(rng.bytes(12), "little") % (1 << tail_bits)
    vals = set()
    for lead, n in runs:
        got = set()
        while len(got) < n:
            got.add((lead << tail_bits) | tail())
        vals |= got
    taken = {lead for lead, _ in runs}
    while len(vals) < background + sum(n for _, n in runs):
        lead = int(rng.integers(0, 1 << 32))
        if lead not in taken:
            vals.add((lead << tail_bits) | tail())
    vals = sorted(vals)
    vals = [vals[i] for i in rng.permutation(len(vals))]
    hi = np.array([v >> 64 for v in vals], dtype=np.uint64)
    lo = np.array([v & 0xFFFFFFFFFFFFFFFF for v in vals], dtype=np.uint64)
    return hi, lo, rng.integers(1, 32768, size=len(vals)).astype(np.uint16)


TOP = (1 << 32) - 1
# lengths 1, 2, 63, 64, 65, 66, 128, 129, 1000; two long runs with neighbouring leading values; a long run at the very start and one at the very end
ORDER_RUNS = [(0, 70), (5000, 1), (6000, 2), (7000, 63), (8000, 64), (9000, 65), (10000, 66), (11000, 128), (12000, 129), (13000, 1000), (20000, 100), (20001, 90), (TOP, 70)]


def order_case(k, which):
    if which == "random":
        return order_entries(k, 2000 + k, [], 5000)
    if which == "runs":
        return order_entries(k, 2100 + k, ORDER_RUNS, 20000)
    if which == "short runs":                                # nothing goes aside: the longest run has 64 entries
        return order_entries(k, 2200 + k, [(0, 64), (1, 64), (7000, 63), (TOP, 64)], 3000)
    if which == "too many aside":                            # 2130 of 4330 entries stand in long runs: more than n / 8 + 1024 = 1565
        return order_entries(k, 2300 + k, [(0, 1000), (1, 1000), (TOP, 130)], 2200)
    raise KeyError(which)


# ---------------------------------------------------------------------------------------------------------------------------------
# the hooks
# ---------------------------------------------------------------------------------------------------------------------------------
def snapshot(ctx, bases, off, k, min_len=0, thr=0, shift=0):
    """-> dict: pbits, n_occ, n_rec, n_units, n_parts, packed, scans, first_room, counters [4], rec [n_rec, 8], part, order, poff, uoff, pack, hi, lo, cnt.
    shift: the bases handed in from that many bytes behind a 256-byte-aligned address; behind their end lie 'T's, not zeros"""
    import torch
    from metafast_amd import lib as L
    so = L.lib()
    fn, info, cp, free = so.mf_debug_wskm_records, so.mf_debug_wskm_info, so.mf_debug_wskm_copy, so.mf_debug_wskm_free
    fn.restype = info.restype = cp.restype = C.c_int
    free.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    info.argtypes = [C.c_void_p, C.c_void_p]
    cp.argtypes = [C.c_void_p] * 10
    free.argtypes = [C.c_void_p]
    tb = torch.full((len(bases) + 64 + shift,), ord("T"), dtype=torch.uint8, device="cuda")
    assert tb.data_ptr() % 256 == 0
    if len(bases):
        tb[shift:shift + len(bases)] = torch.from_numpy(np.ascontiguousarray(bases))
    to = torch.from_numpy(np.ascontiguousarray(off).view(np.int64)).to("cuda")
    h = C.c_void_p()
    L._check(fn(ctx.h, tb.data_ptr() + shift, to.data_ptr(), len(off) - 1, int(off[-1]), k, min_len, thr, C.byref(h)))
    try:
        v = np.zeros(13, dtype=np.uint64)
        L._check(info(h, v.ctypes.data))
        pbits, n_occ, n_rec, n_units, n_parts, packed, scans, room = (int(t) for t in v[:8])
        d = dict(pbits=pbits, n_occ=n_occ, n_rec=n_rec, n_units=n_units, n_parts=n_parts, packed=bool(packed), scans=scans, first_room=room, counters=[int(t) for t in v[8:12]],
                 rec=np.zeros((n_rec, 8), dtype=np.uint32), part=np.zeros(n_rec, dtype=np.uint32), order=np.zeros(n_rec, dtype=np.uint32),
                 poff=np.zeros(n_parts + 1 if n_rec else 0, dtype=np.uint64), uoff=np.zeros(n_units + 1 if n_rec else 0, dtype=np.uint64),
                 pack=np.zeros((n_rec if packed else 0, 8), dtype=np.uint32), hi=np.zeros(int(v[12]), dtype=np.uint64), lo=np.zeros(int(v[12]), dtype=np.uint64),
                 cnt=np.zeros(int(v[12]), dtype=np.uint16))
        L._check(cp(h, *(d[n].ctypes.data for n in ("rec", "part", "order", "poff", "uoff", "pack", "hi", "lo", "cnt"))))
        return d
    finally:
        free(h)


def wide_order(ctx, k, hi, lo, cnt):
    """-> (hi, lo, cnt) as mf_wide_order leaves them, entries set aside, leading-bits route kept"""
    from metafast_amd import lib as L
    fn = L.lib().mf_debug_wide_order
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_uint64] + [C.c_void_p] * 3 + [C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    n = len(hi)
    oh, ol, oc = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint16)
    aside, placed = C.c_uint64(12345), C.c_int(-1)
    L._check(fn(ctx.h, k, hi.ctypes.data, lo.ctypes.data, cnt.ctypes.data, n, oh.ctypes.data, ol.ctypes.data, oc.ctypes.data, C.byref(aside), C.byref(placed)))
    return oh, ol, oc, int(aside.value), int(placed.value)


class options:
    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        assert set(self.kw) <= {n for n, _ in DEFAULTS}
        for name, v in DEFAULTS:
            self.ctx.set_option(name, self.kw.get(name, 1 if name == "wide_skm_min" else v))     # (every input here is far smaller than 2^20 occurrences)

    def __exit__(self, *a):
        for name, v in DEFAULTS:
            self.ctx.set_option(name, v)


_refs = {}


def ref_of(key, make, k, min_len=0, unit=2400, fine=8, merge=1):
    """(bases, offsets, the reference's stages), built once per input and set of options and left unchanged"""
    if (key, k, min_len) not in _refs:
        b, o = make()
        _refs[(key, k, min_len)] = (b, o, W.Scan(b, o, k, min_len))
    b, o, sc = _refs[(key, k, min_len)]
    if (key, k, min_len, unit, fine, merge) not in _refs:
        _refs[(key, k, min_len, unit, fine, merge)] = W.Stages(sc, unit, fine, merge)
    return b, o, _refs[(key, k, min_len, unit, fine, merge)]


def device_table(ctx, bases, off, k, min_len=0):
    from util import to_device
    db, do = to_device(bases, off)
    return ctx.count_wide_device(db.data_ptr(), do.data_ptr(), len(off) - 1, len(bases), k, min_len)


# ---------------------------------------------------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------------------------------------------------
def spell(row, k):
    n = int(row[7]) & 0xFF
    b = "".join(S.ALPHABET[(int(row[i // 16]) >> (30 - 2 * (i % 16))) & 3] for i in range(W.REC_BASES))
    return f"{n} k-mers (weight {int(row[7]) >> 8}) from {b[:min(W.REC_BASES, n + k - 1)]}|{b[n + k - 1:][:8]}..."


def check_scan(snap, st, where):
    """the records and their partitions as k_wskm_scan wrote them = the reference's, as multisets"""
    k = st.sc.k
    assert snap["n_occ"] == st.sc.n_occ and snap["pbits"] == st.pbits, (where, snap["n_occ"], st.sc.n_occ, snap["pbits"], st.pbits)
    got = W.rows_sorted(np.column_stack([snap["rec"], snap["part"]]))
    ref = W.rows_sorted(np.column_stack([st.words(), st.part]))
    if got.shape == ref.shape and np.array_equal(got, ref):
        assert snap["n_rec"] == st.n_rec
        return
    gs, rs = {tuple(r) for r in got.tolist()}, {tuple(r) for r in ref.tolist()}
    msg = [f"{where}: {snap['n_rec']} records, the reference has {st.n_rec}"]
    msg += [f"not in the reference: partition {r[8]}, {spell(r, k)}" for r in sorted(gs - rs)[:3]]
    msg += [f"missing: partition {r[8]}, {spell(r, k)}" for r in sorted(rs - gs)[:3]]
    raise AssertionError("\n".join(msg))


def check_sort(snap, st, where, merge=1):
    n = snap["n_rec"]
    assert np.array_equal(np.sort(snap["order"]), np.arange(n, dtype=np.uint32)), (where, "order is no permutation")
    ps = snap["part"][snap["order"]]
    assert np.all(ps[1:] >= ps[:-1]), (where, "partitions do not ascend along order")
    assert snap["n_parts"] == 1 << snap["pbits"]
    assert np.array_equal(snap["poff"], W.offsets(ps, snap["pbits"])), (where, "poff")
    assert np.array_equal(snap["poff"], st.poff), (where, "poff against the reference's records")
    u = snap["uoff"]
    assert len(u) == snap["n_units"] + 1 and u[0] == 0 and u[-1] == n and np.all(u[1:] >= u[:-1]), (where, "uoff is not monotone from 0 to n_rec")
    assert np.all(np.isin(u, snap["poff"])), (where, "a unit starts inside a partition")
    if not merge or not snap["pbits"]:
        assert np.array_equal(u, snap["poff"]), (where, "uoff != poff without merging")
    assert np.array_equal(u, st.uoff), (where, "uoff against the reference's units")


def check_pack(snap, where, mode):
    rows = snap["rec"][snap["order"]]
    if mode == 0:
        assert not snap["packed"] and len(snap["pack"]) == 0, where
        return None
    assert snap["packed"] and snap["pack"].shape == rows.shape, where
    if mode == 2:
        want = rows.copy()
        want[:, 7] |= np.uint32(1 << 8)
        assert np.array_equal(snap["pack"], want), (where, "order only: every record at its sorted place with weight 1")
        return None
    got, want = W.windows_sorted(snap["pack"]), W.pack(rows)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (where, f"window {bad[0] // W.WINDOW if len(bad) else 0}: got {spell(got[bad[0]], 0) if len(bad) else ''}, want {spell(want[bad[0]], 0) if len(bad) else ''}")
    wgt = (snap["pack"][:, 7] >> np.uint32(8)).astype(np.int64)
    for a in range(0, len(rows), W.WINDOW):
        assert int(wgt[a:a + W.WINDOW].sum()) == len(rows[a:a + W.WINDOW]), (where, "the weights of a window do not add up to its records")
    return wgt


def check_count(snap, st, thr, where):
    """k_wskm_count's raw output = the reference's cut table as multisets, and its counters"""
    hi, lo, cnt, n_all = st.table(thr)
    o = np.lexsort((snap["lo"], snap["hi"]))
    assert len(o) == len(hi) and np.array_equal(snap["hi"][o], hi) and np.array_equal(snap["lo"][o], lo), (where, f"{len(o)} entries, the reference keeps {len(hi)}")
    assert np.array_equal(snap["cnt"][o].astype(np.int32), cnt), (where, "counts")
    c = snap["counters"]
    assert c[0] == len(hi) and c[1] == n_all and c[3] == 0, (where, c, len(hi), n_all)
    assert c[2] == st.overflowing_units(), (where, "units counted in several passes", c[2], st.overflowing_units())


def check_table(ctx, b, o, k, oracle, where, min_len=0):
    got = device_table(ctx, b, o, k, min_len)
    hi, lo, cnt, n_occ = oracle.count_wide(b, o, k, min_len)
    assert got["n_occ"] == n_occ, where
    assert np.array_equal(got["hi"], hi) and np.array_equal(got["lo"], lo) and np.array_equal(got["counts"].astype(np.int32), cnt), where


# ---------------------------------------------------------------------------------------------------------------------------------
# scan
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", SCAN_KS)
def test_scan_ragged_reads_every_window_size(gpu_ctx, oracle, k):
    b, o, st = ref_of("ragged", lambda: ragged(k), k)
    with options(gpu_ctx):
        snap = snapshot(gpu_ctx, b, o, k)
        check_scan(snap, st, f"k = {k}, ragged reads")
        assert snap["n_occ"] == oracle.count_wide(b, o, k, 0)[3]
        check_sort(snap, st, f"k = {k}, ragged reads")


CRAFTED = {"long read": long_read, "tile borders": tile_borders, "long runs": long_runs, "short and empty": short_and_empty}


@gpu
@pytest.mark.parametrize("k", [32, 35, 63])
@pytest.mark.parametrize("name", list(CRAFTED))
def test_scan_crafted_reads(gpu_ctx, oracle, name, k):
    b, o, st = ref_of(name, lambda: CRAFTED[name](k), k)
    with options(gpu_ctx):
        snap = snapshot(gpu_ctx, b, o, k)
        check_scan(snap, st, f"k = {k}, {name}")
        check_table(gpu_ctx, b, o, k, oracle, f"k = {k}, {name}")


@gpu
@pytest.mark.parametrize("k", [32, 63])
def test_scan_reads_filtered_by_length(gpu_ctx, oracle, k):
    b, o, st = ref_of("short and empty", lambda: short_and_empty(k), k, min_len=100)
    with options(gpu_ctx, wide_skm=2):
        snap = snapshot(gpu_ctx, b, o, k, min_len=100)
        check_scan(snap, st, f"k = {k}, min_len 100")
        assert snap["n_occ"] == oracle.count_wide(b, o, k, 100)[3]
        check_table(gpu_ctx, b, o, k, oracle, f"k = {k}, min_len 100", min_len=100)


@gpu
@pytest.mark.parametrize("shift", [1, 5])
@pytest.mark.parametrize("k", [32, 63])
def test_scan_unaligned_base_pointer(gpu_ctx, k, shift):
    """k_wskm_scan packs 16 bases with one 16-byte load where the pointer allows it and byte by byte where not"""
    for name in ("tile borders", "long read"):
        b, o, st = ref_of(name, lambda: CRAFTED[name](k), k)
        with options(gpu_ctx):
            check_scan(snapshot(gpu_ctx, b, o, k, shift=shift), st, f"k = {k}, {name}, bases at + {shift}")


@gpu
@pytest.mark.parametrize("k", [32, 63])
def test_scan_second_attempt_when_the_record_room_is_too_small(gpu_ctx, k):
    b, o, st = ref_of("one k-mer reads", lambda: one_kmer_reads(k), k)
    with options(gpu_ctx):
        snap = snapshot(gpu_ctx, b, o, k)
    assert snap["first_room"] < st.n_rec and snap["scans"] == 2, (snap["first_room"], st.n_rec, snap["scans"])
    check_scan(snap, st, f"k = {k}, a record per k-mer")


# ---------------------------------------------------------------------------------------------------------------------------------
# sort and units
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fine", [1, 8, 32])
@pytest.mark.parametrize("unit", [64, 300, 4000])
def test_sort_and_units(gpu_ctx, unit, fine):
    k = 47
    for merge in (1, 0):
        b, o, st = ref_of("ragged", lambda: ragged(k), k, unit=unit, fine=fine, merge=merge)
        with options(gpu_ctx, wide_skm_unit=unit, wide_skm_fine=fine, wide_skm_merge=merge):
            snap = snapshot(gpu_ctx, b, o, k)
        where = f"unit {unit}, fine {fine}, merge {merge}"
        check_scan(snap, st, where)
        check_sort(snap, st, where, merge)
        check_count(snap, st, 0, where)


@gpu
def test_sort_and_units_of_one_partition(gpu_ctx, oracle):
    k = 33
    b, o, st = ref_of("tiny", lambda: tiny(k), k)
    with options(gpu_ctx):
        snap = snapshot(gpu_ctx, b, o, k)
        assert snap["pbits"] == 0 and snap["n_parts"] == 1 and snap["n_units"] == 1 and (snap["part"] == 0).all()
        check_scan(snap, st, "pbits 0")
        check_sort(snap, st, "pbits 0")
        assert snap["order"].tolist() == list(range(snap["n_rec"])) and snap["uoff"].tolist() == [0, snap["n_rec"]]
        check_count(snap, st, 0, "pbits 0")
        check_table(gpu_ctx, b, o, k, oracle, "pbits 0")


# ---------------------------------------------------------------------------------------------------------------------------------
# pack
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", [1, 2, 0])
def test_pack(gpu_ctx, oracle, mode):
    k = 32
    b, o, st = ref_of("many copies", lambda: many_copies(k), k)
    with options(gpu_ctx, wide_skm_pack=mode):
        snap = snapshot(gpu_ctx, b, o, k)
        where = f"wide_skm_pack {mode}"
        check_scan(snap, st, where)
        wgt = check_pack(snap, where, mode)
        if mode == 1:
            assert wgt.max() > 255 and (wgt == 0).sum() > len(wgt) // 2, (wgt.max(), (wgt == 0).sum())
            rows = snap["rec"][snap["order"]]
            assert any((rows[a - 1] == rows[a]).all() for a in range(W.WINDOW, len(rows), W.WINDOW)), "no class spans a window border"
        check_count(snap, st, 3, where)
        check_table(gpu_ctx, b, o, k, oracle, where)


# ---------------------------------------------------------------------------------------------------------------------------------
# count
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("thr", [0, 1, 3])
@pytest.mark.parametrize("k", [32, 47, 63])
def test_count_raw_output_and_counters(gpu_ctx, k, thr):
    b, o, st = ref_of("ragged", lambda: ragged(k), k)
    with options(gpu_ctx):
        snap = snapshot(gpu_ctx, b, o, k, thr=thr)
    check_count(snap, st, thr, f"k = {k}, threshold {thr}")
    assert snap["counters"][2] == 0


@gpu
@pytest.mark.parametrize("thr", [0, 1])
def test_count_units_that_overflow_the_table(gpu_ctx, oracle, thr):
    """units of 20000 occurrences of reads without repeats: every one holds more distinct k-mers than the table takes and is counted class by class"""
    k = 47
    b, o, st = ref_of("unique", lambda: unique_reads(k), k, unit=20000)
    with options(gpu_ctx, wide_skm_unit=20000):
        snap = snapshot(gpu_ctx, b, o, k, thr=thr)
        check_count(snap, st, thr, f"units of 20000, threshold {thr}")
        assert snap["counters"][2] > 0
        check_table(gpu_ctx, b, o, k, oracle, "units of 20000")


@gpu
def test_count_heavy_partition_in_two_levels_of_classes(gpu_ctx, oracle):
    k = 47
    b, o, st = ref_of("heavy", lambda: heavy_partition(k), k)
    with options(gpu_ctx):
        snap = snapshot(gpu_ctx, b, o, k)
        check_scan(snap, st, "heavy partition")
        check_count(snap, st, 0, "heavy partition")
        assert snap["counters"][2] >= 1
        check_table(gpu_ctx, b, o, k, oracle, "heavy partition")


@gpu
def test_count_saturates_by_weight(gpu_ctx, oracle):
    k = 63
    b, o, st = ref_of("saturating", lambda: saturating_copies(k), k)
    with options(gpu_ctx):
        snap = snapshot(gpu_ctx, b, o, k)
        check_pack(snap, "70000 copies", 1)
        check_count(snap, st, 0, "70000 copies")
        assert sorted(snap["cnt"].tolist()) == [32767, 32767]
        check_table(gpu_ctx, b, o, k, oracle, "70000 copies")


# ---------------------------------------------------------------------------------------------------------------------------------
# order
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [32, 33, 48, 63])
@pytest.mark.parametrize("which", ["random", "runs", "short runs", "too many aside"])
def test_order(gpu_ctx, k, which):
    hi, lo, cnt = order_case(k, which)
    want = W.order(hi, lo, cnt)
    n_aside = W.aside(hi, lo, k)
    for lead in (1, 0, 2):
        with options(gpu_ctx, wide_skm_lead=lead):
            gh, gl, gc, aside, placed = wide_order(gpu_ctx, k, hi, lo, cnt)
        where = f"k = {k}, {which}, wide_skm_lead {lead}"
        assert np.array_equal(gh, want[0]) and np.array_equal(gl, want[1]), (where, "not ascending")
        assert np.array_equal(gc, want[2]), (where, "the counts did not travel with their keys")
        if lead == 0:
            assert (aside, placed) == (0, 0), (where, aside, placed)
        else:
            room = len(hi) // 8 + 1024 if lead == 1 else 0
            assert aside == n_aside and placed == (1 if n_aside <= room else 0), (where, aside, n_aside, placed)
    if which == "too many aside":
        assert n_aside > len(hi) // 8 + 1024


@gpu
@pytest.mark.parametrize("k", [32, 63])
def test_order_of_one_entry_and_of_none(gpu_ctx, k):
    for lead in (1, 0, 2):
        with options(gpu_ctx, wide_skm_lead=lead):
            hi, lo, cnt = np.array([3 if k > 32 else 0], dtype=np.uint64), np.array([1 << 63], dtype=np.uint64), np.array([7], dtype=np.uint16)
            gh, gl, gc, aside, placed = wide_order(gpu_ctx, k, hi, lo, cnt)
            assert (gh.tolist(), gl.tolist(), gc.tolist(), aside, placed) == (hi.tolist(), lo.tolist(), [7], 0, 1 if lead else 0)
            e = np.zeros(0, dtype=np.uint64)
            assert wide_order(gpu_ctx, k, e, e, np.zeros(0, dtype=np.uint16))[3:] == (0, 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# options through the whole path, and the hook itself
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [35, 62])
def test_options_through_the_whole_path(gpu_ctx, oracle, k):
    from util import to_device
    b, o = ragged(k, n=5000)
    db, do = to_device(b, o)
    hi, lo, cnt, n_occ = oracle.count_wide(b, o, k, 0)
    for pack in (0, 1, 2):
        for merge in (0, 1):
            for lazy in (0, 1):
                with options(gpu_ctx, wide_skm_pack=pack, wide_skm_merge=merge, wide_skm_lazy_order=lazy):
                    got = gpu_ctx.count_wide_device(db.data_ptr(), do.data_ptr(), len(o) - 1, len(b), k, 0)
                where = f"k = {k}, pack {pack}, merge {merge}, lazy_order {lazy}"
                assert got["n_occ"] == n_occ, where
                assert np.array_equal(got["hi"], hi) and np.array_equal(got["lo"], lo) and np.array_equal(got["counts"].astype(np.int32), cnt), where


@gpu
def test_hook_refuses_what_it_cannot_show_and_leaves_the_count_alone(gpu_ctx, oracle):
    from metafast_amd import lib as L
    k = 40
    b, o, st = ref_of("ragged", lambda: ragged(k), k)
    with options(gpu_ctx, wide_skm=0):
        with pytest.raises(L.MetafastError, match="does not reach the record path"):
            snapshot(gpu_ctx, b, o, k)
    with options(gpu_ctx):
        with pytest.raises(L.MetafastError, match="does not reach the record path"):          # (wide_skm = 1 leaves inputs filtered by length to the sort path)
            snapshot(gpu_ctx, b, o, k, min_len=100)
    with options(gpu_ctx, wide_skm_min=1 << 20):
        with pytest.raises(L.MetafastError, match="handed the input back .*wide_skm_min"):
            snapshot(gpu_ctx, b, o, k)
    big = (np.full(150 * 200000, ord("A"), dtype=np.uint8), np.arange(200001, dtype=np.uint64) * np.uint64(150))       # 2.2e7 occurrences
    with options(gpu_ctx):
        with pytest.raises(L.MetafastError, match="k-mer occurrences .*at most"):
            snapshot(gpu_ctx, *big, k)
        check_scan(snapshot(gpu_ctx, b, o, k), st, "after the refusals")
        check_table(gpu_ctx, b, o, k, oracle, "the next count on the same context")          # an ordinary one
