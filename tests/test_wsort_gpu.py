"""The wide sort path (metafast_amd/csrc/mf_wide.hip: 32 <= k <= 63) at its borders, against tests/wsort_ref.py and tests/wskm_ref.py.

mf_debug_wide_pass (mf_wide.hip; bound here with ctypes, not part of the C-ABI) runs the body count_wide_impl runs per pass -- the radix passes over the
leading bits, k_wide_finish, k_wide_big<64> / <256>, the side sort or the full sort, the run lengths -- on entries given from the host with the
context's options, and hands back the ordered occurrences, the distinct k-mers with their counts and the routing numbers.  Every crafted case of
wsort_ref.py goes through it in four input orders (the radix passes are stable: the order inside a bucket is the input's) at k = 32, 33, 43, 44, 47,
48, 62, 63; tests/test_wsort_ref_cpu.py asserts what each case is there for.  The generation kernel k_wide_kmers is reached through the public
count with the record path switched off.  Every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import skm_ref as S
import wskm_ref as W
import wsort_ref as R
from util import pack_reads

gpu = pytest.mark.gpu
KS = R.KS
# (tests/test_count_gpu.py: OPTION_DEFAULTS)
DEFAULTS = R.OPTION_DEFAULTS + (("wide_skm", 1), ("wide_passes", 0))


@pytest.fixture(autouse=True)
def _wide_options_back(request):
    yield
    if "gpu_ctx" in request.fixturenames:
        ctx = request.getfixturevalue("gpu_ctx")
        for name, v in DEFAULTS:
            ctx.set_option(name, v)


def wide_pass(ctx, k, hi, lo):
    """-> (hi, lo) ordered, (hi, lo, cnt) distinct, info[10]"""
    from metafast_amd import lib as L
    fn = L.lib().mf_debug_wide_pass
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 7
    n = len(hi)
    hi, lo = np.ascontiguousarray(hi, dtype=np.uint64), np.ascontiguousarray(lo, dtype=np.uint64)
    oh, ol, dh, dl = (np.full(n, 0xDEADBEEF, dtype=np.uint64) for _ in range(4))
    dc = np.zeros(n, dtype=np.uint16)
    nd = C.c_uint64(12345)
    info = np.full(10, 99, dtype=np.uint64)
    L._check(fn(ctx.h, k, hi.ctypes.data, lo.ctypes.data, n, oh.ctypes.data, ol.ctypes.data, dh.ctypes.data, dl.ctypes.data, dc.ctypes.data, C.byref(nd), info.ctypes.data))
    m = int(nd.value)
    return oh, ol, dh[:m], dl[:m], dc[:m], [int(v) for v in info]


def check_pass(ctx, name, k, how, finish=1):
    hi, lo, opts = R.case(name, k)
    (eh, el, dh, dl, dc), rt = R.reference(name, k)
    if not finish:
        rt = R.route(hi, lo, k, finish=0)
    a, b = R.ordered(hi, lo, how)
    for o, v in opts.items():
        ctx.set_option(o, v)
    ctx.set_option("wide_finish", finish)
    before = ctx.stat("wide_big_entries"), ctx.stat("wide_hashed_entries")
    oh, ol, gh, gl, gc, info = wide_pass(ctx, k, a, b)
    after = ctx.stat("wide_big_entries"), ctx.stat("wide_hashed_entries")
    where = (name, k, how, finish)
    print(where, dict(zip(R.INFO, info)))
    bad = np.flatnonzero((oh != eh) | (ol != el))
    assert not len(bad), (where, f"{len(bad)} of {len(eh)} ordered occurrences differ, the first at {int(bad[0])}: {int(oh[bad[0]]):x} {int(ol[bad[0]]):x}, expected {int(eh[bad[0]]):x} {int(el[bad[0]]):x}")
    assert len(gh) == len(dh), (where, len(gh), len(dh))
    assert np.array_equal(gh, dh) and np.array_equal(gl, dl), where
    assert np.array_equal(gc, dc), (where, "counts")
    assert info == R.info_vector(rt), (where, dict(zip(R.INFO, info)), rt)
    assert (after[0] - before[0], after[1] - before[1]) == (rt["big_total"], rt["hashed_entries"]), where


@gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(R.CASES))
def test_pass_equals_the_model(gpu_ctx, name, k):
    for how in R.ORDERS:
        check_pass(gpu_ctx, name, k, how)


@gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(R.CASES))
def test_pass_without_the_finish(gpu_ctx, name, k):
    check_pass(gpu_ctx, name, k, "shuffled", finish=0)


@gpu
def test_pass_refuses(gpu_ctx):
    from metafast_amd import lib as L
    one = np.zeros(1, dtype=np.uint64)
    for k in (31, 64):
        with pytest.raises(L.MetafastError, match="32 .. 63"):
            wide_pass(gpu_ctx, k, one, one)
    for k in KS:
        with pytest.raises(L.MetafastError, match="high word"):
            wide_pass(gpu_ctx, k, np.array([1 << (2 * k - 64)], dtype=np.uint64), one)
        if k > 32:
            oh, ol, dh, dl, dc, _ = wide_pass(gpu_ctx, k, np.array([(1 << (2 * k - 64)) - 1], dtype=np.uint64), one)
            assert oh.tolist() == dh.tolist() == [(1 << (2 * k - 64)) - 1] and dc.tolist() == [1]


# ---------------------------------------------------------------------------------------------------------------------------------
# the generation kernel, through the public count with the record path off
# ---------------------------------------------------------------------------------------------------------------------------------
def _random(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(n))].tobytes()


def _rc(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def model_table(bases, off, k, min_len=0, thr=0):
    """-> (hi, lo, cnt uint16) of the k-mers with count > thr, distinct k-mers in all, occurrences"""
    code = S.base_codes(bases)
    pos = np.flatnonzero(S.valid_starts(off, k, min_len))
    hi, lo = W.canonical_at(code, pos, k)
    dh, dl, c, n_all = W.count(hi, lo, None, thr)
    return dh, dl, c.astype(np.uint16), n_all, len(pos)


def device_reads(bases, off, shift=0):
    """the bases `shift` bytes behind a 256-byte-aligned address, 'T's (a base, not a zero) in front of them and behind their end"""
    import torch
    tb = torch.full((len(bases) + 64 + shift,), ord("T"), dtype=torch.uint8, device="cuda")
    assert tb.data_ptr() % 256 == 0
    if len(bases):
        tb[shift:shift + len(bases)] = torch.from_numpy(np.ascontiguousarray(bases))
    view = tb[shift:]
    assert view.data_ptr() == tb.data_ptr() + shift
    return view, torch.from_numpy(np.ascontiguousarray(off).view(np.int64)).to("cuda")


def check_count(ctx, bases, off, k, min_len=0, shift=0, where=None):
    db, do = device_reads(bases, off, shift)
    ctx.set_option("wide_skm", 0)
    got = ctx.count_wide_device(db.data_ptr(), do.data_ptr(), len(off) - 1, len(bases), k, min_len)
    dh, dl, c, _, n_occ = model_table(bases, off, k, min_len)
    assert got["n_occ"] == n_occ, (where, got["n_occ"], n_occ)
    assert np.array_equal(got["hi"], dh) and np.array_equal(got["lo"], dl) and np.array_equal(got["counts"], c), where
    return got


def fill_reads(rng, reads, at, to):
    """random reads of 40 .. 200 bases up to position `to` exactly -> the new position"""
    while at < to:
        n = to - at if to - at < 260 else int(rng.integers(40, 200))
        reads.append(_random(rng, n)); at += n
    return at


@gpu
@pytest.mark.parametrize("k", KS)
def test_kmers_at_tile_borders(gpu_ctx, k):
    """a tile of the generation kernel holds 8192 positions, 32 per thread, + the 64 bases that follow"""
    rng = np.random.default_rng(3000 + k)
    # one read over 8000 .. 17000: every position 8159 .. 8192 and 16383 .. 16385 starts a k-mer
    reads = []
    at = fill_reads(rng, reads, 0, 8000)
    reads.append(_random(rng, 9000))
    fill_reads(rng, reads, at + 9000, at + 9300)
    bases, off = pack_reads(reads)
    v = S.valid_starts(off, k)
    assert v[8159:8193].all() and v[16383:16386].all()
    check_count(gpu_ctx, bases, off, k, where="long")
    # reads that end and start there: the last k-mer of a read at 8191, at 16383; a read from 8192, 16384, 16385
    for ends in ((8191 + k, 16384), (8192, 16383 + k), (8192 + k, 16385), (8159 + k, 16385 + k)):
        reads, at = [], 0
        for e in ends:
            at = fill_reads(rng, reads, at, e - 150)
            reads.append(_random(rng, 150)); at += 150
            reads.append(_random(rng, 150)); at += 150
        bases, off = pack_reads(reads)
        assert all(e in off.tolist() for e in ends)
        check_count(gpu_ctx, bases, off, k, where=ends)


@gpu
@pytest.mark.parametrize("k", KS)
def test_kmers_at_the_end_of_the_bases(gpu_ctx, k):
    """a read that ends exactly at n_bases, n_bases = 1, 15, 16, 17, 31 (mod 32); reads of k - 1, k and k + 1 bases with min_read_len = k + 1"""
    rng = np.random.default_rng(3100 + k)
    for r in (1, 15, 16, 17, 31, 0):
        reads = []
        fill_reads(rng, reads, 0, 32 * 30 + r - 100)
        reads.append(_random(rng, 100))
        bases, off = pack_reads(reads)
        assert len(bases) % 32 == r and int(off[-1]) == len(bases)
        check_count(gpu_ctx, bases, off, k, where=("end", r))
    lens = [k - 1, k, k + 1, 150, k, k + 1, k - 1, k + 1]
    bases, off = pack_reads([_random(rng, n) for n in lens])
    got = check_count(gpu_ctx, bases, off, k, min_len=k + 1, where="min_len")
    assert got["n_occ"] == 2 * 3 + (150 - k + 1)
    got = check_count(gpu_ctx, bases, off, k, min_len=k, where="min_len = k")
    assert got["n_occ"] == 2 * 3 + 2 * 1 + (150 - k + 1)


@gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("shift", [1, 8, 15])
def test_kmers_from_an_unaligned_pointer(gpu_ctx, k, shift):
    rng = np.random.default_rng(3200 + k)
    reads = []
    fill_reads(rng, reads, 0, 9000 + shift)
    bases, off = pack_reads(reads)
    check_count(gpu_ctx, bases, off, k, shift=shift, where=shift)


@gpu
@pytest.mark.parametrize("k", KS)
def test_kmers_of_one_class(gpu_ctx, k):
    """poly-A next to poly-T, 40 000 bases each: every k-mer is code 0 k times -- class 0, the LDS stage filled between any two looks -- and saturates"""
    bases, off = pack_reads([b"A" * 40000, b"T" * 40000])
    got = check_count(gpu_ctx, bases, off, k, where="poly")
    assert got["n_occ"] == 2 * (40000 - k + 1) and got["hi"].tolist() == [0] and got["lo"].tolist() == [0] and got["counts"].tolist() == [32767]
    if k % 2 == 0:                                              # reads that are their own reverse complement
        rng = np.random.default_rng(3300 + k)
        reads = []
        for n in (k // 2, k // 2 + 1, 40, 100):
            w = _random(rng, n)
            reads += [w + _rc(w)] * 3
        reads.append(b"AT" * 60)
        bases, off = pack_reads(reads)
        for r in reads:
            assert r == _rc(r)
        check_count(gpu_ctx, bases, off, k, where="palindromes")


def _repeated_reads(k):
    """reads in 4, 5, 6 and 7 copies (k-mers with exactly those counts) and single ones"""
    rng = np.random.default_rng(3400 + k)
    reads = []
    for copies in (4, 5, 6, 7, 1, 5):
        for _ in range(6):
            reads += [_random(rng, int(rng.integers(k, 200)))] * copies
    order = rng.permutation(len(reads))
    return pack_reads([reads[i] for i in order])


@gpu
@pytest.mark.parametrize("k", KS)
def test_count_in_passes_and_cut(gpu_ctx, k):
    bases, off = _repeated_reads(k)
    dh, dl, c, n_all, n_occ = model_table(bases, off, k)
    assert {1, 4, 5, 6, 7} <= set(c.tolist())
    db, do = device_reads(bases, off)
    n = len(off) - 1
    gpu_ctx.set_option("wide_skm", 0)
    for passes in (1, 3, 1024):                                 # (1024: a class per pass, empty passes skipped)
        gpu_ctx.set_option("wide_passes", passes)
        got = gpu_ctx.count_wide_device(db.data_ptr(), do.data_ptr(), n, len(bases), k, 0)
        assert got["n_occ"] == n_occ and np.array_equal(got["hi"], dh) and np.array_equal(got["lo"], dl) and np.array_equal(got["counts"], c), passes
        t = gpu_ctx.count_wide_table(db.data_ptr(), do.data_ptr(), n, len(bases), k, 0)
        try:
            m = len(t.pieces())
            assert (m == 1) if passes == 1 else (2 <= m <= 6) if passes == 3 else (6 < m <= 1024), (passes, m)      # (passes are cut at class borders)
            if passes == 3:
                for thr in (4, 5, 6):
                    f = t.filter(thr)
                    try:
                        fh, fl, fc = f.export()
                        keep = c > thr
                        assert np.array_equal(fh, dh[keep]) and np.array_equal(fl, dl[keep]) and np.array_equal(fc, c[keep]), thr
                    finally:
                        f.close()
        finally:
            t.close()
    for passes in (0, 3):
        gpu_ctx.set_option("wide_passes", passes)
        for thr in (4, 5, 6):                                   # c - 1, c, c + 1 around c = 5
            t, all_ = gpu_ctx.count_wide_above(db.data_ptr(), do.data_ptr(), n, len(bases), k, thr)
            try:
                gh, gl, gc = t.export()
            finally:
                t.close()
            keep = c > thr
            assert all_ == n_all and 0 < keep.sum() < len(c)
            assert np.array_equal(gh, dh[keep]) and np.array_equal(gl, dl[keep]) and np.array_equal(gc, c[keep]), (passes, thr)
