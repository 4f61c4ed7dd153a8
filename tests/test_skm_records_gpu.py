"""The super-k-mer scan, scatter and split (metafast_amd/csrc/mf_skm_scan.h, mf_skm_scatter.h, mf_skm_split.h: k_skm_hist, k_skm_scatter, k_skm_split) record by record against
tests/skm_ref.py.

mf_debug_skm_records (mf_skm.hip; bound here with ctypes, not part of the C-ABI) runs what mf_count_device runs with the context's options and
hands over, per slice, the record buffer and the directory (pstart / plen / pocc) as they stand in front of k_skm_count, the plan (levels, digit
range, workgroups and words per workgroup of level 1, one-pass or exact, FAST scatter or not), the level-1 directory and the valid-record
counter.  Every comparison is bit-exact.  Every case asserts the plan it is about from what the hook reports, then

    a  regions ascending, disjoint, inside the buffer, plen a multiple of 4
    b  a region holds valid records and all-ones sentinels only; after a split level plen = roundup4(valid records); a one-level plan has
       at most 3 G sentinels per region (every workgroup pads its share of a digit to a line); the level-1 regions of the one-pass form
       are whole chunks of 256 records
    c  1 <= n <= RMAX, zero bits behind the last base, digit field and partition as the reference derives them from the record's k-mers
    d  all k-mers of a record share one minimizer hash
    e  pocc[p] = the k-mers of the valid records of p
    f  the valid-record counter = the valid records -- for plans with a split level; a one-level plan leaves it at 0 (mf_table_records
       then reports the padded level-1 count), which is asserted as such
    g  the forward k-mers of all records = the forward k-mer occurrences of the reads, as multisets (no folding, no saturation)
    h  records >= the ideal count (runs cut by RMAX alone)

and the multiset of whole records of every partition against the reference: the exact form wherever level 1 has exact ranges or the scatter
is not the FAST one, the one-pass form (runs go on across word borders, skm_ref.Scan.one_pass) otherwise.

Left out: the RECORDS of level 1 in front of a split (only its directory is looked at); the streamed level 1 (mf_stream.hip).  The 32-byte
records of the wide path (mf_wskm.hip) have tests/test_wskm_stages_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import nbr_ref as R
import skm_ref as S
from util import genome_reads, pack_reads

gpu = pytest.mark.gpu

DEFAULTS = (("l1_bits", -1), ("l2_bits", -1), ("part_target", 3072), ("scatter_staged", 1), ("scatter_fast", 1), ("l1_blocks", 0), ("skm", 1),
            ("skm_batches", 0), ("skm_dyn", 1), ("skm_slices", 0), ("skm_shared", 1), ("skm_dedupe", 1), ("arena_cap_gb", 0), ("skm_pilot", 1),
            ("skm_unit_distinct", 2200))
CHUNK = 256                        # records of a chunk of the one-pass level 1


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs (no GPU needed: tests/test_skm_ref_cpu.py runs the reference on them)
# ---------------------------------------------------------------------------------------------------------------------------------
def genome_and_ragged(k, n_genome=2000, n_ragged=500):
    """reads of 150 bases from one genome at 1 % error (both strands, ~10-fold: identical records occur) among ragged reads of 0 .. 120
    bases, the empty read and reads of k - 1, k and k + 1 bases among them"""
    rng = np.random.default_rng(3100 + k)
    gb, go = genome_reads(rng, 30000, n_genome, 150, err=0.01)
    reads = [gb[go[i]:go[i + 1]].tobytes() for i in range(n_genome)]
    lens = rng.integers(0, 121, size=n_ragged)
    lens[:8] = [0, k - 1, k, k + 1, 0, k, 120, 1]
    al = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads += [al[rng.integers(0, 4, size=int(n))].tobytes() for n in lens]
    return pack_reads([reads[i] for i in rng.permutation(len(reads))])


def low_complexity(k):
    """runs far longer than RMAX (homopolymers and microsatellites have one minimizer hash from end to end)"""
    return pack_reads(["A" * 500, "AC" * 200, "ACG" * 150, "T" * 33, "acgtacgtacgtaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaacgtacgt" * 3, "C" * (k - 1), "C" * k,
                       "G" * 131, "TTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTC" * 5, "a" * 257])


def border_reads(seed):
    """every read a multiple of 32 bases long: reads begin and end on word borders.  One of 2112 bases crosses a wave's batch of 63 words,
    one of 33024 a workgroup's batch of 16 x 63 words (and, from word 1000 on, the border between two workgroups where level 1 runs on two
    or three)"""
    rng = np.random.default_rng(seed)
    al = np.frombuffer(b"ACGT", dtype=np.uint8)
    lens = [32] * 40 + [64] * 30 + [96] * 20 + [160] * 30 + [2112] + [320] * 62 + [128] + [33024] + [128] * 40 + [2112, 640, 32, 32] + [992] * 30
    assert sum(lens[:lens.index(33024)]) == 32 * 1000 and all(n % 32 == 0 for n in lens)
    return pack_reads([al[rng.integers(0, 4, size=n)].tobytes() for n in lens])


def one_run_read(k):
    """a read of k + 8 bases whose 9 k-mers all hold the smallest M-mer of the order and share no other minimizer: one run of 9 k-mers"""
    M = R.mmer_len(k)
    m, _ = R.low_mmers(M, 1)[0]
    rng = np.random.default_rng(k)
    while True:
        read = "".join("ACGT"[i] for i in rng.integers(0, 4, size=8)) + S.decode(m, M) + "".join("ACGT"[i] for i in rng.integers(0, 4, size=k - M))
        sc = S.Scan(*pack_reads([read]), k)
        if len(sc.pieces(False)[0]) == 1 and len(read) == k + 8:
            return read


def straddle_reads(k, first_pos):
    """the read of one_run_read from position first_pos of the base stream, behind reads too short to hold a k-mer"""
    pad = [("ACGT" * 8)[:k - 1]] * (first_pos // (k - 1)) + ["G" * (first_pos % (k - 1))]
    b, o = pack_reads(pad + [one_run_read(k), "T" * 40])
    assert int(o[-3]) == first_pos
    return b, o


# ---------------------------------------------------------------------------------------------------------------------------------
# the hook
# ---------------------------------------------------------------------------------------------------------------------------------
def snapshot(ctx, bases, off, k, min_len=0):
    """-> the slices of the run: dicts of rec [cap, 2] (x, y), pstart, plen, pocc, l1_pstart, l1_plen and the plan"""
    from metafast_amd import lib as L
    from util import to_device
    so = L.lib()
    fn, info, cp, free = so.mf_debug_skm_records, so.mf_debug_skm_info, so.mf_debug_skm_copy, so.mf_debug_skm_free
    fn.restype = info.restype = cp.restype = C.c_int
    free.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    info.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    cp.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
    free.argtypes = [C.c_void_p]
    tb, to = to_device(bases, off)
    h = C.c_void_p()
    L._check(fn(ctx.h, tb.data_ptr(), to.data_ptr(), len(off) - 1, int(off[-1]), k, min_len, C.byref(h)))
    try:
        v = np.zeros(20, dtype=np.uint64)
        L._check(info(h, -1, v.ctypes.data))
        out = []
        for s in range(int(v[0])):
            L._check(info(h, s, v.ctypes.data))
            cap, np_, dlo, dhi, G, wpb, one_pass, repeated, n_valid, nlv = (int(t) for t in v[:10])
            d = dict(cap=cap, np=np_, dlo=dlo, dhi=dhi, G=G, wpb=wpb, one_pass=bool(one_pass), repeated=bool(repeated), n_valid=n_valid,
                     lv=[int(t) for t in v[10:10 + nlv]], fast=bool(v[18]), rec=np.zeros((cap, 2), dtype=np.uint64), pstart=np.zeros(np_, dtype=np.uint64),
                     plen=np.zeros(np_, dtype=np.uint32), pocc=np.zeros(np_, dtype=np.uint32), l1_pstart=np.zeros(int(v[19]), dtype=np.uint64),
                     l1_plen=np.zeros(int(v[19]), dtype=np.uint32))
            L._check(cp(h, s, *(d[n].ctypes.data for n in ("rec", "pstart", "plen", "pocc", "l1_pstart", "l1_plen"))))
            out.append(d)
        return out
    finally:
        free(h)


class options:
    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        assert set(self.kw) <= {n for n, _ in DEFAULTS}
        for name, v in DEFAULTS:
            self.ctx.set_option(name, self.kw.get(name, v))

    def __exit__(self, *a):
        for name, v in DEFAULTS:
            self.ctx.set_option(name, v)


_scans = {}


def scan_of(key, make, k, min_len=0):
    """(input, reference scan), built once per input, k and min_len and left unchanged"""
    if (key, k, min_len) not in _scans:
        b, o = make()
        _scans[(key, k, min_len)] = (b, o, S.Scan(b, o, k, min_len))
    return _scans[(key, k, min_len)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------------------------------------------------
def describe(sl):
    return (f"levels {sl['lv']} digits [{sl['dlo']}, {sl['dhi']}) G {sl['G']} x {sl['wpb']} words "
            f"{'one-pass' if sl['one_pass'] else 'exact'}{' (repeated after an overflow)' if sl['repeated'] else ''} {'FAST' if sl['fast'] else 'per-lane'}")


def explain(k, sl, p, x, y, what):
    n, digits, kmers = S.decode_record(x, y, k)
    return f"{what}: partition {p} of [{describe(sl)}], record {int(x):#018x} {int(y):#018x}: n = {n}, digits {digits:#x}, k-mers {kmers[:3]}{' ...' if n > 3 else ''}"


def check_slice(k, sl, where):
    """(a) .. (f) on one slice -> (partition, x, y) of its valid records"""
    lv, cap, npart = sl["lv"], sl["cap"], sl["np"]
    bits1, B = lv[0], sum(lv)
    assert npart == (sl["dhi"] - sl["dlo"]) << (B - bits1), where
    ps, pl = sl["pstart"].astype(np.int64), sl["plen"].astype(np.int64)
    # a
    assert np.all(pl % 4 == 0), where
    assert np.all(ps >= 0) and np.all(ps + pl <= cap), (where, "a region leaves the buffer")
    assert np.all(ps[1:] >= (ps + pl)[:-1]), (where, "regions overlap or are out of order")
    part = np.repeat(np.arange(npart), pl)
    idx = np.repeat(ps, pl) + (np.arange(len(part)) - np.repeat(np.cumsum(pl) - pl, pl))
    x, y = sl["rec"][idx, 0], sl["rec"][idx, 1]
    n = S.rec_n(y)
    sent = n == S.SENTINEL_N
    # b
    bad = np.flatnonzero(sent & ~S.is_sentinel(x, y))
    assert not len(bad), (where, f"partition {part[bad[0]]}: a record with n = 63 that is not all ones: {int(x[bad[0]]):#x} {int(y[bad[0]]):#x}")
    nvalid = np.bincount(part[~sent], minlength=npart)
    if len(lv) > 1:
        assert np.array_equal(pl, (nvalid + 3) // 4 * 4), (where, "plen != roundup4(valid records) after a split level")
    else:
        assert np.all(pl - nvalid <= 3 * sl["G"]), (where, "more than 3 G sentinels in a level-1 region")
    if sl["one_pass"]:
        assert np.all(sl["l1_plen"] % CHUNK == 0) and np.all(sl["l1_pstart"] % CHUNK == 0), (where, "level-1 regions of the one-pass form are whole chunks")
    else:
        assert np.all(sl["l1_plen"] % 4 == 0), where
    x, y, n, part = x[~sent], y[~sent], n[~sent], part[~sent]
    if not len(x):
        return part, x, y
    # c
    bad = np.flatnonzero((n < 1) | (n > S.rmax(k)))
    assert not len(bad), (where, f"partition {part[bad[0]]}: n = {n[bad[0]]} (1 .. {S.rmax(k)})")
    jx, jy = S.junk_bits(x, y, k)
    bad = np.flatnonzero((jx != 0) | (jy != 0))
    assert not len(bad), (where, explain(k, sl, part[bad[0]], x[bad[0]], y[bad[0]], f"{len(bad)} record(s) with bits set behind the last base (stage: record assembly, skm_make_rec)"))
    km, rec = S.record_kmers(x, y, k)
    ph = R.part_hash(km, k)
    first = np.cumsum(n) - n
    ph0 = ph[first]
    # d
    bad = np.flatnonzero(ph != ph0[rec])
    assert not len(bad), (where, explain(k, sl, part[rec[bad[0]]], x[rec[bad[0]]], y[rec[bad[0]]], "k-mers of one record with different minimizer hashes (stage: run detection)"))
    want = ((ph0 << np.uint64(bits1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(10)
    bad = np.flatnonzero(S.rec_digits(y) != want)
    assert not len(bad), (where, explain(k, sl, part[bad[0]], x[bad[0]], y[bad[0]], f"{len(bad)} record(s) whose digit field is not the partition hash's (want {int(want[bad[0]]) if len(bad) else 0:#x}; stage: skm_route)"))
    wantp = (ph0.astype(np.int64) >> (32 - B)) - (sl["dlo"] << (B - bits1))
    bad = np.flatnonzero(part != wantp)
    assert not len(bad), (where, explain(k, sl, part[bad[0]], x[bad[0]], y[bad[0]], f"{len(bad)} record(s) in the wrong partition (want {int(wantp[bad[0]]) if len(bad) else 0}; stage: scatter / split)"))
    # e
    occ = np.bincount(part, weights=n, minlength=npart).astype(np.int64)
    bad = np.flatnonzero(occ != sl["pocc"].astype(np.int64))
    assert not len(bad), (where, f"pocc[{bad[0] if len(bad) else 0}] = {sl['pocc'][bad[0]] if len(bad) else 0}, its valid records hold {occ[bad[0]] if len(bad) else 0} k-mers ({len(bad)} partitions differ; stage: the last level's occupancy)")
    # f
    assert sl["n_valid"] == (len(x) if len(lv) > 1 else 0), (where, "valid-record counter", sl["n_valid"], len(x))
    return part, x, y


def check_run(k, slices, sc, form, where):
    """every slice, then (g), (h) and the record multisets per partition over the whole run -> (x, y) of all valid records"""
    assert slices, where
    parts = [check_slice(k, sl, f"{where}, slice {i}: {describe(sl)}") for i, sl in enumerate(slices)]
    lv = slices[0]["lv"]
    assert all(sl["lv"] == lv for sl in slices) and slices[0]["dlo"] == 0 and slices[-1]["dhi"] == 1 << lv[0], where
    assert all(a["dhi"] == b["dlo"] for a, b in zip(slices, slices[1:])), where
    x = np.concatenate([p[1] for p in parts])
    y = np.concatenate([p[2] for p in parts])
    # g
    km, _ = S.record_kmers(x, y, k)
    want = sc.occurrences()
    assert len(km) == len(want) and np.array_equal(np.sort(km), want), (where, f"the records hold {len(km)} k-mer occurrences, the reads {len(want)}, or other ones")
    # h
    assert len(x) >= sc.ideal_count(), where
    if form is None:
        return x, y
    start, n = sc.exact() if form == "exact" else sc.one_pass(slices[0]["wpb"])
    rx, ry = S.encode_records(sc.code, start, n, sc.mh[start], k, lv[0])
    d1 = (R.remix32(sc.mh[start]) >> np.uint64(32 - lv[0])).astype(np.int64) if lv[0] else np.zeros(len(start), dtype=np.int64)
    for i, (sl, (part, gx, gy)) in enumerate(zip(slices, parts)):
        m = (d1 >= sl["dlo"]) & (d1 < sl["dhi"])
        rp = S.partition_of(sc.mh[start[m]], lv[0], sum(lv), sl["dlo"])
        got = np.stack([part.astype(np.uint64), gx, gy], axis=1)[np.lexsort((gy, gx, part))]
        ref = np.stack([rp.astype(np.uint64), rx[m], ry[m]], axis=1)[np.lexsort((ry[m], rx[m], rp))]
        if got.shape == ref.shape and np.array_equal(got, ref):
            continue
        gs, rs = {tuple(r) for r in got.tolist()}, {tuple(r) for r in ref.tolist()}
        extra, missing = sorted(gs - rs)[:2], sorted(rs - gs)[:2]
        msg = [f"{where}, slice {i} [{describe(sl)}]: {len(got)} records, the {form} form of the reference has {len(ref)}"]
        msg += [explain(k, sl, p, a, b, "not in the reference") for p, a, b in extra] + [explain(k, sl, p, a, b, "missing") for p, a, b in missing]
        raise AssertionError("\n".join(msg))
    return x, y


def run(ctx, k, inp, form, where, min_len=0, plan=None, **opts):
    b, o, sc = inp
    with options(ctx, **opts):
        slices = snapshot(ctx, b, o, k, min_len)
    print(f"{where}: " + "; ".join(describe(sl) for sl in slices))
    if plan:
        plan(slices)
    return slices, check_run(k, slices, sc, form, where)


def levels(n, one_pass=False, fast=None):
    def f(slices):
        for sl in slices:
            assert len(sl["lv"]) == n and sl["one_pass"] == one_pass and not sl["repeated"], describe(sl)
            assert fast is None or sl["fast"] == fast, describe(sl)
    return f


# ---------------------------------------------------------------------------------------------------------------------------------
# exact form
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", range(20, 32))
def test_exact_every_k(gpu_ctx, k):
    inp = scan_of("genome", lambda: genome_and_ragged(k), k)
    run(gpu_ctx, k, inp, "exact", f"k = {k}, two levels", plan=levels(2, fast=True), skm_dyn=0, l1_bits=5, l2_bits=5)
    run(gpu_ctx, k, inp, "exact", f"k = {k}, one level", plan=levels(1, fast=True), skm_dyn=0, l1_bits=6, l2_bits=0)


@gpu
@pytest.mark.parametrize("k", [21, 31])
def test_exact_scatter_forms_and_level1_widths(gpu_ctx, k):
    inp = scan_of("genome", lambda: genome_and_ragged(k), k)
    _, a = run(gpu_ctx, k, inp, "exact", f"k = {k}, scatter_fast 1", plan=levels(2, fast=True), skm_dyn=0, l1_bits=5, l2_bits=5, scatter_fast=1)
    _, b = run(gpu_ctx, k, inp, "exact", f"k = {k}, scatter_fast 0", plan=levels(2, fast=False), skm_dyn=0, l1_bits=5, l2_bits=5, scatter_fast=0)
    assert np.array_equal(S.sorted_pairs(*a), S.sorted_pairs(*b))
    # 11 bits: the staging lines leave no LDS for the FAST form; 2 and 3 bits: many records per line and workgroup
    run(gpu_ctx, k, inp, "exact", f"k = {k}, l1_bits 11", plan=levels(2, fast=False), skm_dyn=0, l1_bits=11, l2_bits=2)
    run(gpu_ctx, k, inp, "exact", f"k = {k}, l1_bits 11, one level", plan=levels(1, fast=False), skm_dyn=0, l1_bits=11, l2_bits=0)
    run(gpu_ctx, k, inp, "exact", f"k = {k}, l1_bits 2", plan=levels(2, fast=True), skm_dyn=0, l1_bits=2, l2_bits=7)
    run(gpu_ctx, k, inp, "exact", f"k = {k}, l1_bits 3", plan=levels(1, fast=True), skm_dyn=0, l1_bits=3, l2_bits=0)
    run(gpu_ctx, k, inp, "exact", f"k = {k}, l1_bits 0", plan=levels(2, fast=True), skm_dyn=0, l1_bits=0, l2_bits=6)


@gpu
@pytest.mark.parametrize("k", [21, 31])
def test_exact_three_levels(gpu_ctx, k):
    """the third level writes into the first level's buffer"""
    inp = scan_of("genome", lambda: genome_and_ragged(k), k)
    slices, _ = run(gpu_ctx, k, inp, "exact", f"k = {k}, three levels", plan=levels(3), skm_dyn=0, l1_bits=3, part_target=1)
    assert slices[0]["lv"][1] == 11 and sum(slices[0]["lv"]) >= 17


@gpu
def test_exact_planned_by_the_pilot(gpu_ctx):
    """no forced plan: the levels after the first come from the pilot's count of a few level-1 regions"""
    k = 31
    inp = scan_of("genome", lambda: genome_and_ragged(k), k)
    pilots = gpu_ctx.stat("pilot_runs")
    slices, _ = run(gpu_ctx, k, inp, "exact", "k = 31, the pilot's plan", skm_dyn=0, part_target=16)
    assert len(slices) == 1 and len(slices[0]["lv"]) >= 2 and not slices[0]["one_pass"]
    assert gpu_ctx.stat("pilot_runs") == pilots + 1


@gpu
@pytest.mark.parametrize("min_len", [0, 100])
@pytest.mark.parametrize("k", [20, 27, 31])
def test_exact_low_complexity(gpu_ctx, k, min_len):
    """runs far longer than RMAX: the batches take the per-lane loop, not the run list"""
    inp = scan_of("low", lambda: low_complexity(k), k, min_len)
    assert inp[2].pieces(True)[1].max() == 32 and inp[2].pieces(False)[1].max() >= 500 - k + 1 - 8
    run(gpu_ctx, k, inp, "exact", f"k = {k}, low complexity, min_len {min_len}, two levels", min_len=min_len, plan=levels(2), skm_dyn=0, l1_bits=3, l2_bits=3)
    run(gpu_ctx, k, inp, "exact", f"k = {k}, low complexity, min_len {min_len}, one level", min_len=min_len, plan=levels(1), skm_dyn=0, l1_bits=4, l2_bits=0)


def _straddles(o, wpb):
    """a read that has words in two workgroups' ranges"""
    s, e = o[:-1].astype(np.int64) // 32, (o[1:].astype(np.int64) - 1) // 32
    return bool(np.any((o[1:] > o[:-1]) & (s // wpb != e // wpb)))


@gpu
@pytest.mark.parametrize("blocks", [0, 2, 3])
@pytest.mark.parametrize("k", [20, 26, 31])
def test_exact_borders(gpu_ctx, k, blocks):
    inp = scan_of("borders", lambda: border_reads(41), k)
    lens = np.diff(inp[1].astype(np.int64))
    assert np.all(lens % 32 == 0) and lens.max() > 16 * 63 * 32 and np.sort(lens)[-2] >= 2100

    def plan(slices):
        levels(2, fast=True)(slices)
        assert blocks == 0 or slices[0]["G"] == blocks
        assert slices[0]["G"] >= 2 and _straddles(inp[1], slices[0]["wpb"])
    run(gpu_ctx, k, inp, "exact", f"k = {k}, word borders, l1_blocks {blocks}", plan=plan, skm_dyn=0, l1_bits=4, l2_bits=4, l1_blocks=blocks)


@gpu
@pytest.mark.parametrize("shared", [2, 0])
@pytest.mark.parametrize("nslices", [2, 4])
def test_exact_slices(gpu_ctx, nslices, shared):
    """each slice holds exactly the reference's records of its digit range (shared: split out of one level 1 over all digits, the rebase
    path); together they are the unsliced run"""
    k = 31
    inp = scan_of("genome", lambda: genome_and_ragged(k), k)
    _, whole = run(gpu_ctx, k, inp, "exact", "k = 31, unsliced", plan=levels(2), skm_dyn=0, l1_bits=5, l2_bits=5)

    def plan(slices):
        levels(2)(slices)
        assert len(slices) == nslices and [sl["dhi"] - sl["dlo"] for sl in slices] == [32 // nslices] * nslices
    _, parts = run(gpu_ctx, k, inp, "exact", f"k = 31, {nslices} slices, skm_shared {shared}", plan=plan, skm_dyn=0, l1_bits=5, l2_bits=5, skm_slices=nslices, skm_shared=shared)
    assert np.array_equal(S.sorted_pairs(*parts), S.sorted_pairs(*whole))


# ---------------------------------------------------------------------------------------------------------------------------------
# one-pass form
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [20, 21, 25, 26, 31])
def test_one_pass_against_the_model(gpu_ctx, k):
    inp = scan_of("genome", lambda: genome_and_ragged(k), k)
    _, (x, _) = run(gpu_ctx, k, inp, "one-pass", f"k = {k}, one-pass", plan=levels(2, one_pass=True, fast=True), skm_dyn=2, l1_bits=5, l2_bits=5)
    n_exact = len(inp[2].exact()[0])
    assert len(x) < n_exact, (len(x), n_exact)             # strictly fewer records than the exact form on reads of 150 bases
    # without the FAST scatter the one-pass form has chunked regions but the exact form's records
    _, (x2, _) = run(gpu_ctx, k, inp, "exact", f"k = {k}, one-pass, scatter_fast 0", plan=levels(2, one_pass=True, fast=False), skm_dyn=2, l1_bits=5, l2_bits=5, scatter_fast=0)
    assert len(x2) == n_exact


@gpu
def test_one_pass_other_plans(gpu_ctx):
    k = 31
    inp = scan_of("genome", lambda: genome_and_ragged(k), k)
    run(gpu_ctx, k, inp, "exact", "k = 31, one-pass, l1_bits 11", plan=levels(2, one_pass=True, fast=False), skm_dyn=2, l1_bits=11, l2_bits=2)
    run(gpu_ctx, k, inp, "one-pass", "k = 31, one-pass, l1_bits 10", plan=levels(2, one_pass=True, fast=True), skm_dyn=2, l1_bits=10, l2_bits=2)
    run(gpu_ctx, k, inp, "one-pass", "k = 31, one-pass, three levels", plan=levels(3, one_pass=True, fast=True), skm_dyn=2, l1_bits=3, part_target=1)
    for nslices, shared in ((2, 2), (4, 0)):
        _, (x, _) = run(gpu_ctx, k, inp, "one-pass", f"k = 31, one-pass, {nslices} slices, skm_shared {shared}", plan=levels(2, one_pass=True, fast=True), skm_dyn=2, l1_bits=5, l2_bits=5,
                        skm_slices=nslices, skm_shared=shared)
        assert len(x) <= len(inp[2].exact()[0])
    # a one-level plan never takes the one-pass form
    run(gpu_ctx, k, inp, "exact", "k = 31, skm_dyn 2, one level", plan=levels(1, one_pass=False), skm_dyn=2, l1_bits=6, l2_bits=0)


@gpu
@pytest.mark.parametrize("k", [20, 27, 31])
def test_one_pass_low_complexity_and_borders(gpu_ctx, k):
    """a batch with a run of more than RMAX k-mers takes the per-lane loop: no extension there"""
    inp = scan_of("low", lambda: low_complexity(k), k)
    _, (x, _) = run(gpu_ctx, k, inp, "one-pass", f"k = {k}, one-pass, low complexity", plan=levels(2, one_pass=True, fast=True), skm_dyn=2, l1_bits=3, l2_bits=3)
    assert len(x) <= len(inp[2].exact()[0])
    for blocks in (2, 3):
        inp = scan_of("borders", lambda: border_reads(41), k)
        _, (x, _) = run(gpu_ctx, k, inp, "one-pass", f"k = {k}, one-pass, word borders, l1_blocks {blocks}", plan=levels(2, one_pass=True, fast=True), skm_dyn=2, l1_bits=4, l2_bits=4, l1_blocks=blocks)
        assert len(x) < len(inp[2].exact()[0])


@gpu
@pytest.mark.parametrize("k", [21, 31])
def test_one_run_across_a_word_border(gpu_ctx, k):
    """one run of 9 k-mers, 2 in front of a word border and 7 behind it: one record in the one-pass form, two in the exact form -- unless the
    word behind the border is the first of a wave's batch: then two in both"""
    nk = 9
    assert 7 <= min(S.rmax(k) - 2, 49 - k)                 # (the whole head of 7 k-mers fits the record of the 2 in front of the border)
    read = one_run_read(k)
    run_kmers = S.windows(S.base_codes(np.frombuffer(read.encode(), dtype=np.uint8)), k)[:nk]
    for word, want_one_pass in ((40, [9]), (S.WAVE_WORDS * 2, [2, 7]), (S.WAVE_WORDS * S.WAVES, [2, 7]), (S.WAVE_WORDS * S.WAVES + 1, [9])):
        b, o = straddle_reads(k, 32 * word - 2)
        inp = (b, o, S.Scan(b, o, k))
        assert inp[2].pieces(False)[1].tolist()[0] == nk and inp[2].pieces(False)[0].tolist()[0] == 32 * word - 2
        for dyn, want in ((2, want_one_pass), (0, [2, 7])):
            def plan(slices):
                levels(2, one_pass=dyn == 2, fast=True)(slices)
                # the batch geometry as the hook reports it: one workgroup over all words, so a wave's batches start at the multiples of 63
                assert slices[0]["G"] == 1 and slices[0]["wpb"] > word
                assert ((word % slices[0]["wpb"]) % S.WAVE_WORDS == 0) == (want_one_pass == [2, 7])
            _, (x, y) = run(gpu_ctx, k, inp, "one-pass" if dyn == 2 else "exact", f"k = {k}, one run across the border of word {word}, skm_dyn {dyn}", plan=plan, skm_dyn=dyn, l1_bits=3, l2_bits=3)
            km, rec = S.record_kmers(x, y, k)
            run_recs = np.unique(rec[np.isin(km, run_kmers)])
            got = sorted(((km[rec == r] == run_kmers[0]).any(), int(S.rec_n(y[r]))) for r in run_recs)[::-1]       # the record of the run's first k-mer first
            assert [n for _, n in got] == want and got[0][0], (word, dyn, got)


# ---------------------------------------------------------------------------------------------------------------------------------
# the hook itself
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_hook_refuses_other_paths_and_leaves_the_count_alone(gpu_ctx, oracle):
    from metafast_amd import lib as L
    from util import gpu_count
    k = 31
    b, o, sc = scan_of("genome", lambda: genome_and_ragged(k), k)
    with pytest.raises(L.MetafastError, match="super-k-mer path"):
        snapshot(gpu_ctx, b, o, 19)
    with options(gpu_ctx, skm=0):
        with pytest.raises(L.MetafastError, match="super-k-mer path"):
            snapshot(gpu_ctx, b, o, k)
    with options(gpu_ctx):
        assert snapshot(gpu_ctx, *pack_reads(["ACGT", ""]), k) == []
        slices = snapshot(gpu_ctx, b, o, k)
        check_run(k, slices, sc, "exact", "k = 31, the context's defaults")
        # the next count on the same context is an ordinary one
        t = gpu_count(gpu_ctx, b, o, k)
        gk, gc = t.export()
        ok, ov = oracle.Table().count_buffer(b, o, k).export()
        assert np.array_equal(gk, ok) and np.array_equal(gc.astype(np.int32), ov) and t.records()[1] == 16
