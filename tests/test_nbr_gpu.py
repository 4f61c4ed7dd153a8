"""The partition-local neighbour lookup (metafast_amd/csrc/mf_nbr.h, nb_for_each) neighbour by neighbour against tests/nbr_ref.py.

mf_debug_neighbours (mf_cc.hip; bound here with ctypes, not part of the C-ABI) returns the adjacency of a table by a chosen path -- 0:
k_cc_adjacency, eight lookups in the HBM index; 1: the MODE 1 + MODE 2 launches of k_cc_adjacency_part exactly as
mf_cut_components_device makes them -- with the keys in table order and the partition offsets.  The crafted tables put one partition at
each of the sizes where the code changes its path:

    352 / 353     NB_CAP: a wave's LDS table / the workgroup form (MODE 2)
    1408 / 1409   NB_CAP * NB_WAVES: MODE 2 / every lookup through the HBM index (and every batch of 64 k-mers asks for more than NB_RQ = 64
                  requests: the rest is looked up on the spot)
    511 / 512     2 c + 1 <= MF_IDX_WAVE_SLOTS: index region built by a wave / by a workgroup (k_index_build_part<64> / <256>)
    4095 / 4096   2 c + 1 <= 8192: region built in LDS by a workgroup / in place in HBM (k_index_build_huge)

and every case asserts, from the reference's result alone, that it held what each path needs (present and absent neighbours, in the same
and in other partitions, on both strands, grouped and ungrouped requests, a self loop, a palindrome for even k).  A failure names the
partition's size class, the slot and whether the neighbour lives in another partition.

Out of scope: k_dcc_adjacency_part with lw > 0 (the `foreign` bits of a sharded table) stays with tests/test_distributed_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import nbr_ref as R
from util import canon_seq, gpu_count

gpu = pytest.mark.gpu

KS = [21, 22, 25, 26, 31]          # 21 / 25 / 31: k a compile-time constant (25: the five-wave build); 22 / 26: the generic build, even k (palindromes), 26: M = 15
SIZES = (352, 353, 511, 512, 1408, 1409, 4095, 4096)
NB_CAP, NB_BIGCAP, NB_RQ = 352, 1408, 64
PART_BITS = 9


def size_class(c):
    return "wave-local LDS table (<= 352 keys)" if c <= NB_CAP else "workgroup LDS table, MODE 2 (353 .. 1408 keys)" if c <= NB_BIGCAP else "HBM index for every lookup (> 1408 keys)"


def region_class(c):
    return "index region built by a wave" if 2 * c + 1 <= 1024 else "index region built by a workgroup" if 2 * c + 1 <= 8192 else "index region built in HBM"


def table_part_bits(n):
    """the partition bits mf_table_from_host gives a table of n distinct ascending keys (k >= 20, n >= 4096): at most 96 keys a partition"""
    bits = 1
    while bits < 26 and (n >> bits) > 96:
        bits += 1
    return bits


def _windows(seqs, k):
    """seqs: uint8 [m, L] of base codes -> the canonical k-mers of all windows, uint64 [m * (L - k + 1)]"""
    seqs = np.asarray(seqs, dtype=np.uint64)
    w = seqs.shape[1] - k + 1
    x = np.zeros((seqs.shape[0], w), dtype=np.uint64)
    for i in range(k):
        x = (x << np.uint64(2)) | seqs[:, i:i + w]
    return R.canonical(x.reshape(-1), k)


def _codes(s):
    return np.array(["ACGT".index(c) for c in s], dtype=np.uint8)


def _family_seqs(rng, mmer, M, k, m, ext, variants=0.4):
    """m sequences that hold the M-mer in every one of their middle k - M + 1 windows (random bases around it, `ext` more on either side:
    those windows lie in other partitions); two in five are single-base variants of an earlier one (branches)"""
    mb = np.array([(mmer >> (2 * (M - 1 - i))) & 3 for i in range(M)], dtype=np.uint8)
    fl = k - M + ext
    seqs = rng.integers(0, 4, size=(m, 2 * fl + M), dtype=np.uint8)
    for i in np.flatnonzero(rng.random(m) < variants):
        if i:
            seqs[i] = seqs[rng.integers(0, i)]
            p = int(rng.integers(0, 2 * fl))
            p = p if p < fl else p + M                      # (not inside the M-mer)
            seqs[i, p] = (seqs[i, p] + rng.integers(1, 4)) & 3
    seqs[:, fl:fl + M] = mb
    return seqs


def crafted_table(k):
    """-> (keys ascending canonical uint64, counts uint16 in 1 .. 50, {partition: wanted size}) for 2^9 partitions"""
    rng = np.random.default_rng(1000 + k)
    M = R.mmer_len(k)
    shift = np.uint64(32 - PART_BITS)
    picked, seen = [], set()
    for m, h in R.low_mmers(M, 64):                         # eight minimizers in eight different partitions
        p = int(R.remix32(h) >> shift)
        if p not in seen and len(picked) < len(SIZES):
            seen.add(p)
            picked.append((m, p))
    specials = [_windows(_codes(s)[None, :], k) for s in (
        "A" * (k + 3) + "CGTCAG", ("AC" * k)[:k + 8], ("ACGT" * k)[:k + 8], ("AATT" * k)[:k + 8])]
    genome = rng.integers(0, 4, size=(1, 27000 + k), dtype=np.uint8)
    pool = [_windows(genome, k)] + specials
    for (m, p), want in zip(picked, SIZES):
        fam = np.zeros(0, dtype=np.uint64)
        while True:                                         # until the partition could be filled by the family alone
            fam = np.unique(np.concatenate([fam, _windows(_family_seqs(rng, m, M, k, 12, 2), k)]))
            if int(((R.part_hash(fam, k) >> shift) == np.uint64(p)).sum()) >= want + 16:
                break
        pool.append(fam)
    keys = np.unique(np.concatenate(pool))
    part = (R.part_hash(keys, k) >> shift).astype(np.int64)
    keep = np.ones(len(keys), dtype=bool)
    special = np.isin(keys, np.concatenate(specials))
    wanted = {}
    for (m, p), want in zip(picked, SIZES):                 # trim every target partition to its size
        idx = np.flatnonzero((part == p) & ~special)
        excess = int((part == p).sum()) - want
        assert 0 <= excess <= len(idx)
        keep[rng.choice(idx, size=excess, replace=False)] = False
        wanted[p] = want
    keys = keys[keep]
    assert table_part_bits(len(keys)) == PART_BITS
    counts = rng.integers(1, 51, size=len(keys)).astype(np.uint16)
    return keys, counts, wanted


def table_order(keys, k, bits):
    """a table order of ascending keys for the checks that need no GPU: by partition, ascending inside"""
    part = (R.part_hash(keys, k) >> np.uint64(32 - bits)).astype(np.int64)
    return keys[np.argsort(part, kind="stable")]


def coverage(tkeys, k, bits, wanted):
    """what a table (keys in table order: partitions contiguous) offers the lookup's paths, from the numpy reference alone.
    -> ({wanted size: counts of its partition}, counts of the whole table)"""
    tkeys = np.asarray(tkeys, dtype=np.uint64)
    shift = np.uint64(32 - bits)
    own = R.part_hash(tkeys, k)
    part = (own >> shift).astype(np.int64)
    ref, rc = R.neighbours(tkeys, k, with_strand=True)
    present = ref != R.NONE
    y = R.neighbour_kmers(tkeys, k)
    per = {}
    for p, want in wanted.items():
        rows = np.flatnonzero(part == p)
        pr = present[rows]
        npart = np.where(pr, part[np.where(pr, ref[rows], 0)], -1)
        nph = R.part_hash(y[rows].reshape(-1), k).reshape(len(rows), 8)
        # requests: a neighbour is remote if its minimizer is not the k-mer's own (or its partition is too large for LDS: all are); the
        # remote neighbours of a side with one minimizer are one (grouped) request, else one request each
        remote = (nph != own[rows][:, None]) | (len(rows) > NB_BIGCAP)
        nreq = np.zeros(len(rows), dtype=np.int64)
        grouped = ungrouped = 0
        for side in (0, 1):
            rs, hs = remote[:, side::2], nph[:, side::2]
            cnt = rs.sum(axis=1)
            lo = np.where(rs, hs, np.uint64(1 << 40)).min(axis=1)
            hi = np.where(rs, hs, np.uint64(0)).max(axis=1)
            same = (cnt > 0) & (lo == hi)
            diff = (cnt > 0) & (lo != hi)
            grouped += int(same.sum())
            ungrouped += int(diff.sum())
            nreq += np.where(same, 1, np.where(diff, cnt, 0))
        batches = [int(nreq[j:j + 64].sum()) for j in range(0, len(rows), 64)] if len(rows) > NB_BIGCAP else [0]
        per[want] = dict(keys=len(rows), present=int(pr.sum()), absent=int((~pr).sum()), same_part=int((pr & (npart == p)).sum()),
                         other_part=int((pr & (npart != p)).sum()), reverse=int((pr & rc[rows]).sum()), forward=int((pr & ~rc[rows]).sum()),
                         grouped=grouped, ungrouped=ungrouped, batches_over_rq=sum(b > NB_RQ for b in batches))
    whole = dict(self_loops=int((ref == np.arange(len(tkeys), dtype=np.uint32)[:, None]).sum()),
                 palindromes=int((present & (y == R.revcomp(y.reshape(-1), k).reshape(y.shape))).sum()))
    return per, whole


def check_coverage(per, whole, k):
    assert sorted(per) == sorted(SIZES)
    for want, c in per.items():
        assert c["keys"] == want, (want, c)
        assert c["present"] >= 50 and c["absent"] >= 50, (want, c)
        assert c["same_part"] >= 10 and c["other_part"] >= 10, (want, c)          # (asked of all eight, not only of the LDS sizes)
        assert c["reverse"] >= 1 and c["forward"] >= 1, (want, c)
        assert c["grouped"] >= 1 and c["ungrouped"] >= 1, (want, c)
        if want > NB_BIGCAP:                                # every lane has two requests or more: each full batch overflows the request buffer
            assert c["batches_over_rq"] >= want // 64, (want, c)
    assert whole["self_loops"] >= 1, whole
    if k % 2 == 0:
        assert whole["palindromes"] >= 1, whole


def debug_neighbours(ctx, t, path, part_bits=None):
    """-> (keys in table order, neighbour ids [n, 8], part_bits, partition offsets or None)"""
    from metafast_amd import lib as L
    fn = L.lib().mf_debug_neighbours
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_uint64]
    n = len(t)
    keys = np.empty(n, dtype=np.uint64)
    nbr = np.empty((n, 8), dtype=np.uint32)
    pb = C.c_int(-1)
    off = np.zeros((1 << part_bits) + 1, dtype=np.uint64) if part_bits else None
    L._check(fn(ctx.h, t.h, path, keys.ctypes.data, nbr.ctypes.data, C.byref(pb), off.ctypes.data if part_bits else None, len(off) if part_bits else 0))
    return keys, nbr, pb.value, off


def both_paths(ctx, t):
    k0, n0, bits, _ = debug_neighbours(ctx, t, 0)
    k1, n1, bits1, off = debug_neighbours(ctx, t, 1, bits)
    assert bits1 == bits and np.array_equal(k0, k1)
    return k0, n0, n1, bits, off


def explain(got, want, tkeys, k, bits, off):
    """the first mismatches, each with the path it took: size class of the k-mer's partition, slot, same / other partition"""
    bad = np.argwhere(got != want)
    if not len(bad):
        return ""
    shift = np.uint64(32 - bits)
    sizes = np.diff(off.astype(np.int64))
    lines = [f"{len(bad)} wrong neighbours of {got.size}"]
    for v, s in bad[:12]:
        x = tkeys[v]
        p = int(R.part_hash(x, k) >> shift)
        y = R.neighbour_kmers(np.array([x], dtype=np.uint64), k)[0, s]
        q = int(R.part_hash(y, k) >> shift)
        lines.append(f"vertex {v} {R.decode(x, k)} in partition {p} of {sizes[p]} keys [{size_class(sizes[p])}], slot {s} "
                     f"({'left' if s & 1 else 'right'} {'ACGT'[s >> 1]}): neighbour in {'the same' if q == p else 'another'} partition ({q}, {sizes[q]} keys, {region_class(sizes[q])}), "
                     f"{'palindrome, ' if int(R.revcomp(y, k)) == int(y) else ''}got {got[v, s]:#x} want {want[v, s]:#x}")
    return "\n".join(lines)


_cases = {}


@pytest.fixture(params=KS)
def case(request, gpu_ctx):
    """per k, built once: the crafted table on the GPU, its adjacency by both paths, the reference"""
    k = request.param
    if k not in _cases:
        keys, counts, wanted = crafted_table(k)
        t = gpu_ctx.table_from_host(keys, counts, k)
        tkeys, nbr0, nbr1, bits, off = both_paths(gpu_ctx, t)
        _cases[k] = dict(k=k, keys=keys, counts=counts, wanted=wanted, table=t, tkeys=tkeys, nbr0=nbr0, nbr1=nbr1, bits=bits, off=off)
    return _cases[k]


@gpu
def test_layout(case):
    k, tkeys, bits, off = case["k"], case["tkeys"], case["bits"], case["off"]
    assert bits == PART_BITS
    assert np.array_equal(np.sort(tkeys), case["keys"])                                  # a permutation of the input (ascending, distinct)
    part = (R.part_hash(tkeys, k) >> np.uint64(32 - bits)).astype(np.int64)
    assert off[0] == 0 and off[-1] == len(tkeys) and np.all(np.diff(off.astype(np.int64)) >= 0)
    assert np.array_equal(part, np.repeat(np.arange(1 << bits), np.diff(off.astype(np.int64))))      # key i lies in the partition of its minimizer
    sizes = np.diff(off.astype(np.int64))
    assert {p: int(sizes[p]) for p in case["wanted"]} == case["wanted"]
    assert sorted(sizes[list(case["wanted"])].tolist()) == sorted(SIZES)


@gpu
def test_coverage_of_the_crafted_table(case):
    per, whole = coverage(case["tkeys"], case["k"], case["bits"], case["wanted"])
    print(case["k"], per, whole)
    check_coverage(per, whole, case["k"])


@gpu
@pytest.mark.parametrize("path", [1, 0])
def test_adjacency_neighbour_by_neighbour(case, path):
    want = R.neighbours(case["tkeys"], case["k"])
    got = case["nbr1" if path else "nbr0"]
    assert np.array_equal(got, want), f"k = {case['k']}, path {path}: " + explain(got, want, case["tkeys"], case["k"], case["bits"], case["off"])


@gpu
def test_lookup_present_and_absent(case):
    """Table.lookup (mf_index_find_ph, the third walker of the index) on all three region builds: every key, and as many k-mers the table
    does not hold -- absent NEIGHBOURS of its keys first (they share their interior, i.e. home slot and tag, with keys that are there)"""
    k, keys, counts = case["k"], case["keys"], case["counts"]
    rng = np.random.default_rng(k)
    near = np.unique(R.canonical(R.neighbour_kmers(keys, k).reshape(-1), k))
    near = rng.permutation(near[~np.isin(near, keys)])[:len(keys) - 1000]
    far = R.canonical(rng.integers(0, 1 << (2 * k), size=1000, dtype=np.uint64), k)
    far = far[~np.isin(far, keys)]
    q = np.concatenate([keys, near, far])
    want = np.concatenate([counts.astype(np.int32), np.full(len(near) + len(far), -1, dtype=np.int32)])
    order = rng.permutation(len(q))
    got = case["table"].lookup(q[order])
    bad = np.flatnonzero(got != want[order])
    assert not len(bad), (len(bad), [(R.decode(q[order][i], k), int(got[i]), int(want[order][i])) for i in bad[:8]])


def _norm_seqs(seqs):
    return sorted((canon_seq(s), a, mn, mx) for s, a, mn, mx in seqs)


def _same_comps(got, want):
    assert [(a, b, c) for a, b, c, _ in got] == [(a, b, c) for a, b, c, _ in want]
    for (_, _, _, gk), (_, _, _, wk) in zip(got, want):
        assert np.array_equal(gk, wk)


@gpu
def test_consumers_local_and_global(case, gpu_ctx, oracle):
    """k_ut_flags_part's flip bits and k_cc_adjacency_part behind their consumers: unitigs and components of the crafted table with the
    partition-local lookup forced (nbr_global = -1: the table's 80 keys a partition would not take it) and with the HBM index alone (1),
    both against the oracle on the same (k-mer, count) pairs"""
    k, t = case["k"], case["table"]
    b1, b2 = 5, 2000               # the background genome is one path of 27000 k-mers: above b2, split at threshold 2 and higher
    ot = oracle.Table()
    for key, c in zip(case["keys"].tolist(), case["counts"].tolist()):
        ot.add(key, c)
    want_seqs = _norm_seqs(oracle.build_unitigs(ot, k, 0, k).all())
    want_comps = oracle.cut_components(ot, k, b1, b2).all()
    assert len(want_comps) >= 2 and max(c[2] for c in want_comps) >= 2 and min(c[2] for c in want_comps) == 1
    out = {}
    try:
        for mode in (-1, 1):
            gpu_ctx.set_option("nbr_global", mode)
            out[mode] = (_norm_seqs(gpu_ctx.build_unitigs(t, 0, k).export()), gpu_ctx.cut_components(t, b1, b2).export())
    finally:
        gpu_ctx.set_option("nbr_global", 0)
    for mode in (-1, 1):
        assert out[mode][0] == want_seqs, (k, mode)
        _same_comps(out[mode][1], want_comps)
    assert out[-1][0] == out[1][0]
    _same_comps(out[-1][1], out[1][1])


@gpu
@pytest.mark.parametrize("k", [31, 21])
def test_counted_sample_both_paths(gpu_ctx, k):
    """a table out of the counting pass carries the plan's own partition bits and split (mf_table_from_host never makes such a table)"""
    from metafast_amd import lib as L
    bases, off = L.synth_reads_host(0x4D45544146415354, 0, 0, 20000, 150, 4000)
    t = gpu_count(gpu_ctx, bases, off, k)
    tkeys, nbr0, nbr1, bits, poff = both_paths(gpu_ctx, t)
    assert bits > 0 and poff[-1] == len(tkeys) == len(t)
    assert np.array_equal(np.sort(tkeys), t.export()[0])
    want = R.neighbours(tkeys, k)
    assert (want != R.NONE).sum() > len(tkeys)
    for path, got in ((1, nbr1), (0, nbr0)):
        assert np.array_equal(got, want), f"k = {k}, path {path}: " + explain(got, want, tkeys, k, bits, poff)


@gpu
def test_oversized_partition_gets_the_generic_index(gpu_ctx):
    """2^20 + 8 keys around one minimizer: a position inside the partition no longer fits the compact index's 20 bits, the table gets the
    generic index.  The partition-local lookup is refused on it, the lookups through the generic index are right (the adjacency on one
    vertex in 16)."""
    from metafast_amd import lib as L
    k, M = 31, 15
    rng = np.random.default_rng(31)
    m, _ = R.low_mmers(M, 1)[0]
    fam = np.unique(_windows(_family_seqs(rng, m, M, k, 66000, 0, variants=0.0), k))
    assert np.all(R.part_hash(fam[::97], k) == R.part_hash(fam[0], k))
    fam = rng.permutation(fam)[:(1 << 20) + 8]
    assert len(fam) == (1 << 20) + 8
    keys = np.unique(np.concatenate([fam, _windows(rng.integers(0, 4, size=(1, 6000), dtype=np.uint8), k)]))
    counts = rng.integers(1, 51, size=len(keys)).astype(np.uint16)
    t = gpu_ctx.table_from_host(keys, counts, k)
    tkeys, nbr0, bits, _ = debug_neighbours(gpu_ctx, t, 0)
    _, _, _, off = debug_neighbours(gpu_ctx, t, 0, bits)
    assert bits == table_part_bits(len(keys)) and int(np.diff(off.astype(np.int64)).max()) >= (1 << 20) + 8
    with pytest.raises(L.MetafastError, match="no index over minimizer partitions"):
        debug_neighbours(gpu_ctx, t, 1, bits)
    assert np.array_equal(np.sort(tkeys), keys)
    rows = np.arange(0, len(tkeys), 16)
    want = R.neighbours(tkeys, k, rows=rows)
    assert (want != R.NONE).sum() > len(rows) and np.array_equal(nbr0[rows], want)
    absent = R.canonical(rng.integers(0, 1 << (2 * k), size=100_000, dtype=np.uint64), k)
    absent = absent[~np.isin(absent, keys)]
    got = t.lookup(np.concatenate([keys, absent]))
    assert np.array_equal(got[:len(keys)], counts.astype(np.int32)) and np.all(got[len(keys):] == -1)
