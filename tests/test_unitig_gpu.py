"""Steps U1 .. U5 of the unitig builder (metafast_amd/csrc/mf_unitig.hip) on crafted tables, against tests/ut_ref.py and the oracle.

mf_debug_unitigs (mf_unitig.hip; bound here with ctypes, not part of the C-ABI) runs mf_ut_build -- links, jump words, chunked walks, doubling,
emission rule, segment cuts, the second walk -- on a table, U1 arrays and minimizer partitions given from the host, and returns the ordinary
sequences plus a trace of what the host saw: start nodes, walk rounds, whether the jump words were doubled, entries, doubling rounds, longest
path, candidates, paths, segment slots.  Every crafted case (ut_ref.CASES; tests/test_ut_ref_cpu.py asserts on the CPU that each reaches the
path it was made for)

    * compares the sequences (strand-normalised, as test_pipeline_gpu._norm_seqs) with their (avg, min, max) and Seqs.stats() with the oracle's,
    * compares the trace with ut_ref.predict, field by field (the doubling rounds: inside the interval predict() derives),
    * does both under every (ut_double_after, ut_plain_rounds) the case names.

mf_debug_unitig_flags returns U1 of a real table by k_ut_flags (path 0) or by the launches of k_ut_flags_part (path 1): both against
ut_ref.flags, byte for byte, on the crafted tables of tests/test_nbr_gpu.py.

Out of scope: the sharded cutter; the order of mf_seqs_export beyond what export() gives."""
import ctypes as C

import numpy as np
import pytest

import ut_ref as R
from util import branchy_reads, canon_seq, gpu_count

pytestmark = pytest.mark.gpu


def _norm_seqs(seqs):
    return sorted((canon_seq(s), a, mn, mx) for s, a, mn, mx in seqs)


def _ptr(a):
    return None if a is None or a.size == 0 else a.ctypes.data


def debug_unitigs(ctx, keys, counts, info, ridx, lidx, pal, k, min_len, part_bits=0, off=None, n=None, hi=None):
    """-> (Seqs.export(), Seqs.stats(), trace dict).  keys: ints (any k) -- or a uint64 array of low words with `hi` given explicitly"""
    from metafast_amd import lib as L
    fn = L.lib().mf_debug_unitigs
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 7 + [C.c_int] * 3 + [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]
    if isinstance(keys, np.ndarray):
        lo = np.ascontiguousarray(keys, dtype=np.uint64)
    else:
        lo, hi_words = R.split_words(keys)
        hi = hi_words if (k >= 33 and hi is None) else hi
    counts = np.ascontiguousarray(counts, dtype=np.uint16)
    info = np.ascontiguousarray(info, dtype=np.uint8)
    ridx, lidx = np.ascontiguousarray(ridx, dtype=np.uint32), np.ascontiguousarray(lidx, dtype=np.uint32)
    pal = None if pal is None else np.ascontiguousarray(pal, dtype=np.uint8)
    off = None if off is None else np.ascontiguousarray(off, dtype=np.uint64)
    trace = np.zeros(len(R.TRACE_FIELDS), dtype=np.uint64)
    h = C.c_void_p()
    L._check(fn(ctx.h, len(lo) if n is None else n, _ptr(lo), _ptr(hi), _ptr(counts), _ptr(info), _ptr(ridx), _ptr(lidx), _ptr(pal), k, min_len,
                part_bits, _ptr(off), C.byref(h), trace.ctypes.data))
    seqs = L.Seqs(ctx, h)
    try:
        return seqs.export(), seqs.stats(), dict(zip(R.TRACE_FIELDS, map(int, trace)))
    finally:
        seqs.close()


def debug_flags(ctx, t, path, part_bits=None):
    """-> (keys in table order, info, ridx, lidx, pal or None, part_bits, partition offsets or None)"""
    from metafast_amd import lib as L
    fn = L.lib().mf_debug_unitig_flags
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.POINTER(C.c_int), C.c_void_p, C.c_uint64]
    n = len(t)
    keys, info = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint8)
    ridx, lidx, pal = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    pb = C.c_int(-1)
    off = np.zeros((1 << part_bits) + 1, dtype=np.uint64) if part_bits else None
    L._check(fn(ctx.h, t.h, path, keys.ctypes.data, info.ctypes.data, ridx.ctypes.data, lidx.ctypes.data, pal.ctypes.data, C.byref(pb),
                off.ctypes.data if part_bits else None, len(off) if part_bits else 0))
    return keys, info, ridx, lidx, pal, pb.value, off


def check_trace(trace, want, what):
    for f in R.TRACE_FIELDS:
        if f == "double_rounds":
            lo, hi = want[f]
            assert lo <= trace[f] <= hi, (what, f, trace, want[f])
        else:
            assert trace[f] == want[f], (what, f, trace[f], want[f], trace)
    assert sum(want["segments"]) <= trace["seg_slots"], what


def run(ctx, k, keys, counts, flags, part_bits, off, min_len, settings, want_seqs, predict=None):
    """every setting against the oracle's sequences (and predict(double_after, plain_rounds)) -> [raw export per setting]"""
    info, ridx, lidx, pal = flags
    outs = []
    try:
        for after, plain in settings:
            ctx.set_option("ut_double_after", after)
            ctx.set_option("ut_plain_rounds", plain)
            what = f"ut_double_after = {after}, ut_plain_rounds = {plain}"
            got, stats, trace = debug_unitigs(ctx, keys, counts, info, ridx, lidx, pal if k % 2 == 0 else None, k, min_len, part_bits, off)
            print(what, trace)
            assert len(got) == len(want_seqs), (what, len(got), len(want_seqs))
            g, w = _norm_seqs(got), _norm_seqs(want_seqs)
            bad = [i for i in range(len(g)) if g[i] != w[i]]
            assert not bad, (what, len(bad), "first:", g[bad[0]][1:], w[bad[0]][1:], len(g[bad[0]][0]), len(w[bad[0]][0]),
                             next((j for j, (a, b) in enumerate(zip(g[bad[0]][0], w[bad[0]][0])) if a != b), None))
            assert stats == (len(want_seqs), sum(len(s[0]) for s in want_seqs)), what
            if predict is not None:
                check_trace(trace, predict(after, plain), what)
            outs.append(got)
    finally:
        ctx.set_option("ut_double_after", 4)
        ctx.set_option("ut_plain_rounds", 3)
    return outs


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_crafted_case(gpu_ctx, oracle, name):
    c = R.get_case(name)
    want, _ = c.oracle_unitigs(oracle)
    outs = run(gpu_ctx, c.k, c.keys, c.counts, c.flags, c.part_bits, c.off, c.min_len, c.settings, want, c.predict)
    if name == "f_store_alignment":                         # the paths' places in the output: every residue mod 8 (in the order export() gives)
        lens = np.array([len(s[0]) for s in outs[0]])
        assert set((np.cumsum(lens) % 8).tolist()) == set(range(8))


@pytest.mark.parametrize("seed", [7, 9])
def test_layout_independence(gpu_ctx, oracle, seed):
    """j. one read-derived table (branches, tips, bubbles: paths printed 0, 1 and 2 times) under four partition assignments: the same output"""
    k, b, min_len = 31, 1, 100
    bases, off = branchy_reads(seed)
    keys, vals = oracle.Table().count_buffer(bases, off, k).export(b)
    g = oracle.Table()
    for x, v in zip(keys.tolist(), vals.tolist()):
        g.add(x, v)
    want = oracle.build_unitigs(g, k, b, min_len).all()
    assert len(want) > 40
    outs = {}
    for name, a in R.random_assignments(len(keys), seed).items():
        order, bits, poff = R.layout(keys, a)
        tkeys = keys[order]
        outs[name] = run(gpu_ctx, k, tkeys.tolist(), vals[order], R.flags(tkeys, k), bits, poff, min_len, ((4, 3), (1, 3)), want)
    for name in outs:
        assert outs[name][0] == outs[name][1] == outs["none"][0], name


def test_arguments_are_checked(gpu_ctx):
    from metafast_amd import lib as L
    c = R.get_case("c_cycle_across")
    info, ridx, lidx, _ = c.flags
    lo = np.array(c.keys, dtype=np.uint64)
    n, k = len(lo), c.k
    args = dict(keys=lo, counts=c.counts, info=info, ridx=ridx, lidx=lidx, pal=None, k=k, min_len=k, part_bits=c.part_bits, off=c.off)

    def refused(match, **change):
        with pytest.raises(L.MetafastError, match=match):
            debug_unitigs(gpu_ctx, **{**args, **change})

    refused("fewer than 2\\^31", n=0x7FFFFFFF)
    for v in (0, R.MAX_COUNT + 1):
        cnt = c.counts.copy()
        cnt[3] = v
        refused("count .* of k-mer 3", counts=cnt)
    bad = lo.copy()
    bad[5] = np.uint64(1) << np.uint64(2 * k)
    refused("k-mer 5 does not fit 42 bits", keys=bad)
    refused("high words are given exactly when k >= 33", hi=np.zeros(n, dtype=np.uint64))
    refused("high words are given exactly when k >= 33", k=33)
    refused("palindrome flags are given exactly when k is even", pal=np.zeros(n, dtype=np.uint8))
    refused("palindrome flags are given exactly when k is even", k=20)
    refused("k = 64", k=64)
    i = int(np.flatnonzero((info & 7) < 4)[0])
    bad = ridx.copy()
    bad[i] = n
    refused(f"right neighbour {n} of k-mer {i}", ridx=bad)
    j = int(np.flatnonzero(((info >> 3) & 7) < 4)[0])
    bad = lidx.copy()
    bad[j] = 0xFFFFFFFF
    refused(f"left neighbour 4294967295 of k-mer {j}", lidx=bad)
    bad = info.copy()
    bad[0] = 6
    refused("info byte 0x6 of k-mer 0", info=bad)
    bad = ridx.copy()                                       # a right neighbour that does not point back: two links into one node
    both = np.flatnonzero(((info & 7) < 4) & (((info >> 3) & 7) < 4))
    bad[i] = next(int(g) for g in both if g != ridx[i] and g != i)
    refused("the links are not mutual", ridx=bad)
    for change, match in (((0, 1), "start at 1"), ((1, int(c.off[2]) + 1), "decrease at partition 1"), ((-1, n - 1), "end at")):
        bad = c.off.copy()
        bad[change[0]] = change[1]
        refused(match, off=bad)
    refused("partition offsets are given exactly when part_bits > 0", off=None)
    refused("partition offsets are given exactly when part_bits > 0", part_bits=0)
    refused("part_bits = 27", part_bits=27)
    got, stats, trace = debug_unitigs(gpu_ctx, **args)      # ... and the unchanged arguments pass
    assert stats[0] == 1 and trace["paths"] == 1
    got, stats, trace = debug_unitigs(gpu_ctx, np.zeros(0, dtype=np.uint64), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), None, 21, 21)
    assert got == [] and stats == (0, 0) and trace["n_starts"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# U1
# ---------------------------------------------------------------------------------------------------------------------------------
def explain_flags(got, want, tkeys, k, off):
    """the first mismatches, each with the size class of its k-mer's partition (as test_nbr_gpu.explain)"""
    from test_nbr_gpu import size_class
    import nbr_ref as NR
    (gi, gr, gl, gp), (wi, wr, wl, wp) = got, want
    r_u, l_u = (wi & 7) < 4, ((wi >> 3) & 7) < 4
    bad = np.flatnonzero((gi != wi) | (r_u & (gr != wr)) | (l_u & (gl != wl)) | ((gp != wp) if k % 2 == 0 else False))
    if not len(bad):
        return ""
    sizes = np.diff(off.astype(np.int64))
    part = np.searchsorted(off.astype(np.int64), bad, side="right") - 1
    lines = [f"{len(bad)} wrong k-mers of {len(wi)}"]
    for v, p in zip(bad[:12].tolist(), part[:12].tolist()):
        lines.append(f"k-mer {v} {NR.decode(tkeys[v], k)} in partition {p} of {sizes[p]} keys [{size_class(sizes[p])}]: info {gi[v]:#x} want {wi[v]:#x}, "
                     f"ridx {gr[v]:#x} want {wr[v]:#x}, lidx {gl[v]:#x} want {wl[v]:#x}, pal {gp[v]} want {wp[v]}")
    return "\n".join(lines)


@pytest.mark.parametrize("k", [21, 22, 25, 26, 31])
def test_flags_byte_for_byte(gpu_ctx, k):
    from test_nbr_gpu import PART_BITS, SIZES, crafted_table
    keys, counts, wanted = crafted_table(k)
    t = gpu_ctx.table_from_host(keys, counts, k)
    got = {path: debug_flags(gpu_ctx, t, path, PART_BITS) for path in (0, 1)}
    tkeys, off = got[0][0], got[0][6]
    assert got[0][5] == got[1][5] == PART_BITS and np.array_equal(tkeys, got[1][0]) and np.array_equal(np.sort(tkeys), keys)
    sizes = np.diff(off.astype(np.int64))
    assert sorted(sizes[list(wanted)].tolist()) == sorted(SIZES)
    want = R.flags(tkeys, k)
    wi = want[0]
    assert ((wi & 7) == R.CODE_MANY).any() and ((wi & 7) == R.CODE_NONE).any() and ((wi >> 3) & 7 == R.CODE_MANY).any() and (wi >> 6 & 1).any() and (wi >> 7).any()
    assert (k % 2 == 1) or want[3].any()
    for path in (1, 0):
        msg = explain_flags(got[path][1:5], want, tkeys, k, off)
        assert not msg, f"k = {k}, path {path}: " + msg


@pytest.mark.parametrize("k", [31, 21])
def test_front_end_to_back_end(gpu_ctx, k):
    """the flags a counted table gives (path 1), fed back through mf_debug_unitigs with the table's own partitions = build_unitigs on that table"""
    from metafast_amd import lib as L
    bases, off = L.synth_reads_host(0x4D45544146415354, 0, 0, 20000, 150, 4000)
    t = gpu_count(gpu_ctx, bases, off, k)
    _, _, _, _, _, bits, _ = debug_flags(gpu_ctx, t, 0)
    assert bits > 0
    tkeys, info, ridx, lidx, pal, _, poff = debug_flags(gpu_ctx, t, 1, bits)
    want = R.flags(tkeys, k)
    assert not explain_flags((info, ridx, lidx, pal), want, tkeys, k, poff)
    counts = t.lookup(tkeys).astype(np.uint16)
    ref = gpu_ctx.build_unitigs(t, 0, k).export()
    got, stats, trace = debug_unitigs(gpu_ctx, tkeys, counts, info, ridx, lidx, pal if k % 2 == 0 else None, k, k, bits, poff)
    assert len(ref) > 20 and got == ref and trace["paths"] == len(ref)
