"""The one-record-per-k-mer counting path (metafast_amd/csrc/mf_count.hip: k_mask_init / k_mask_reads, k_l1_hist, k_l1_scatter, k_split, k_count, the
table) stage by stage against tests/count_ref.py.

mf_debug_count_stages (mf_count.hip; bound here with ctypes, not part of the C-ABI) runs what mf_count_device runs with the context's options and
hands over what every stage left for the next: the valid-start bitmap and n_occ, the plan (levels, workgroups and words per workgroup of level 1,
staged scatter or not), the level-1 histogram, region starts and buffer, every K2 level's buffer and directory, keys / cnt / dcount and the
overflow word behind k_count, d_part_off and the table.  Buffers a stage writes only in part hold 0xA5 bytes in front of it.  Every comparison
is bit-exact (count_ref.check, (a) .. (e)); every case asserts the plan it is about from what the hook reports.

The inputs need no GPU: tests/test_count_ref_cpu.py runs the reference on them and asserts the properties the cases rest on.

Left out: the streamed level 1 (mf_stream.hip), k_presence, bytes other than ACGT / acgt (the parsers split reads there)."""
import ctypes as C

import numpy as np
import pytest

import count_ref as CR
from util import genome_reads, gpu_count, pack_reads

pytestmark = pytest.mark.gpu

DEFAULTS = (("l1_bits", -1), ("l2_bits", -1), ("part_target", 3072), ("scatter_staged", 1), ("l1_blocks", 0), ("skm", 1), ("skm_batches", 0), ("skm_dyn", 1),
            ("skm_slices", 0), ("skm_shared", 1), ("skm_dedupe", 1), ("arena_cap_gb", 0), ("skm_pilot", 1), ("skm_unit_distinct", 2200))
PART_TARGET = 3072
N_CU = 256                         # compute units of an MI355X: level 1 runs on one workgroup each unless option l1_blocks or the input's size says otherwise
BITMAP_KS = (1, 2, 5, 16, 19, 31)
MIN_LENS = (0, 40, 64, 65)
# (l1_bits, l2_bits, scatter_staged, l1_blocks, part_target).  The last one is the three-level plan 2 + 11 + 2: option l2_bits takes 11 at the most, so the 13
# bits behind level 1 come from the plan itself -- 15 bits for these reads at 8 occurrences per partition
PLANS = ((0, 0, 1, 0, 3072), (3, -1, 1, 1, 3072), (11, -1, 1, 0, 3072), (2, 11, 1, 5, 3072), (5, 5, 0, 3, 3072), (6, 6, 1, 2, 3072), (2, -1, 1, 2, 8))
PATTERNS = ("plain", "next63", "next_short", "next_below_min_len", "empty_between")
_AL = np.frombuffer(b"ACGT", dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs (no GPU needed)
# ---------------------------------------------------------------------------------------------------------------------------------
def _random_reads(rng, lens):
    return pack_reads([_AL[rng.integers(0, 4, size=int(n))].tobytes() for n in lens])


def ragged_reads(k, n=400):
    """reads of 0 .. 120 bases, with k - 1, k, k + 1, 31, 32, 33, 63, 64 and 65 among them; n_bases is no multiple of 32"""
    rng = np.random.default_rng(4100 + k)
    lens = rng.integers(0, 121, size=n)
    lens[:12] = [k - 1, k, k + 1, 31, 32, 33, 63, 64, 65, 0, 120, 1]
    lens = lens[rng.permutation(n)]
    if lens.sum() % 32 == 0:
        lens[-1] += 1
    return _random_reads(rng, lens)


def neighbour_run(k, min_len, cycles=150):
    """the neighbour patterns the plain read-modify-write of k_mask_reads rests on, `cycles` times each, at every alignment to the 32-base
    words (a cycle has an odd number of bases): a read of A = max(64, min_len) bases in front of one of A, of 63, of k - 1, of 64 (below
    min_len when that is 65), and of an empty one with a read of A behind it; the last read has 64 bases or more"""
    A = max(64, min_len)
    cycle = [A, A, A, 63, A, k - 1, A, 64, A, 0, A, A + 32, 33, 31, 1, 96, 64, 64]
    if sum(cycle) % 2 == 0:
        cycle.append(1)
    lens = cycle * cycles + [A + 7]
    if sum(lens) % 32 == 0:
        lens[-1] += 1
    return _random_reads(np.random.default_rng(4200 + 100 * k + min_len), lens)


def pattern_counts(off, k, min_len):
    """how often each neighbour pattern occurs: this read has 64 bases or more and holds k-mers, the next one ..."""
    ln = np.diff(np.asarray(off).astype(np.int64))
    this, nxt = ln[:-1], ln[1:]
    nn = np.concatenate([ln[2:], [0]])
    ok = (this >= 64) & (this >= max(k, min_len))
    return dict(plain=int((ok & (nxt >= 64) & (nxt >= min_len)).sum()), next63=int((ok & (nxt == 63)).sum()), next_short=int((ok & (nxt < k)).sum()),
                next_below_min_len=int((ok & (nxt >= 64) & (nxt < min_len)).sum()), empty_between=int((ok & (nxt == 0) & (nn >= 64)).sum()))


def border_counts(off, k, min_len):
    """reads of 64 bases or more that hold k-mers and end on a word border, one base behind it, one base in front of it"""
    off = np.asarray(off).astype(np.int64)
    ln = np.diff(off)
    e = off[1:][(ln >= 64) & (ln >= max(k, min_len))]
    return int((e % 32 == 0).sum()), int((e % 32 == 1).sum()), int((e % 32 == 31).sum())


def plan_reads():
    """2000 reads of 100 bases from one genome at 1 % error (both strands, ~10-fold) among ragged reads of 0 .. 120 bases"""
    rng = np.random.default_rng(4300)
    gb, go = genome_reads(rng, 20000, 2000, 100, err=0.01)
    reads = [gb[go[i]:go[i + 1]].tobytes() for i in range(2000)]
    lens = rng.integers(0, 121, size=500)
    lens[:10] = [0, 10, 11, 12, 30, 31, 32, 120, 1, 0]
    reads += [_AL[rng.integers(0, 4, size=int(n))].tobytes() for n in lens]
    b, o = pack_reads([reads[i] for i in rng.permutation(len(reads))])
    assert int(o[-1]) % 32 != 0
    return b, o


def flush_reads():
    """random sequence: at k = 16 the 32 k-mers of a word go to 32 different digits of 2048"""
    return _random_reads(np.random.default_rng(4400), [1000] * 200 + [37])


def heavy_inputs(k):
    """name -> reads: few distinct k-mers, many occurrences each"""
    rng = np.random.default_rng(4500 + k)
    low = bytes(_AL[rng.integers(0, 4, size=60000)]).lower()
    return {"A x 32766": ["A" * (32766 + k - 1)], "A x 32767": ["A" * (32767 + k - 1)], "A x 32768": ["A" * (32768 + k - 1)], "A * 40000": ["A" * 40000],
            "AC": ["AC" * 9000, "A" * 3500], "ACG": ["ACG" * 6500, "T" * 3300], "lower case": [low[:30000], low[30000:]]}


def distinct_read(k, n_distinct):
    """a random read of n_distinct + k - 1 bases whose canonical k-mers are all different"""
    for seed in range(4600, 4700):
        b, o = _random_reads(np.random.default_rng(seed), [n_distinct + k - 1])
        if len(CR.Reference(b, o, k).table()[0]) == n_distinct:
            return b, o
    raise AssertionError("no such read")


def few_distinct_read(k, n_occ):
    return pack_reads([("ACGGT" * (n_occ // 5 + k))[:n_occ + k - 1]])


_refs = {}


def ref_of(key, make, k, min_len=0):
    """(bases, offsets, reference), built once per input, k and min_len and left unchanged"""
    if (key, k, min_len) not in _refs:
        b, o = make()
        _refs[(key, k, min_len)] = (b, o, CR.Reference(b, o, k, min_len))
    return _refs[(key, k, min_len)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the hook
# ---------------------------------------------------------------------------------------------------------------------------------
_TOP = (("vmask", np.uint32), ("blockhist", np.uint32), ("blockstart", np.uint64), ("buf1", np.uint64), ("pstart1", np.uint64), ("plen1", np.uint32),
        ("keys", np.uint64), ("cnt", np.uint16), ("dcount", np.uint32), ("pstart", np.uint64), ("plen", np.uint32), ("part_off", np.uint64), ("dk", np.uint64),
        ("dc", np.uint16))


def snapshot(ctx, bases, off, k, min_len=0):
    """-> the snapshot of count_ref's docstring"""
    from metafast_amd import lib as L
    from util import to_device
    so = L.lib()
    fn, info, cp, free = so.mf_debug_count_stages, so.mf_debug_count_info, so.mf_debug_count_copy, so.mf_debug_count_free
    fn.restype = info.restype = cp.restype = C.c_int
    free.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    info.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    cp.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint64]
    free.argtypes = [C.c_void_p]
    tb, to = to_device(bases, off)
    h = C.c_void_p()
    L._check(fn(ctx.h, tb.data_ptr(), to.data_ptr(), len(off) - 1, int(off[-1]), k, min_len, C.byref(h)))
    try:
        v = np.zeros(24, dtype=np.uint64)
        L._check(info(h, -1, v.ctypes.data))
        stage, n_words, n_occ, B, G, wpb, staged, nlv, n_buf1, np_, cap, overflow, part_bits, n_dist, n_off = (int(t) for t in v[:15])
        nd1G = (1 << int(v[16])) * G if stage >= 2 else 0
        sizes = dict(vmask=n_words if stage else 0, blockhist=nd1G, blockstart=nd1G + 1 if stage >= 2 else 0, buf1=n_buf1, pstart1=nd1G // G if G else 0,
                     plen1=nd1G // G if G else 0, keys=cap, cnt=cap, dcount=np_, pstart=np_, plen=np_, part_off=n_off, dk=n_dist if stage == 5 else 0,
                     dc=n_dist if stage == 5 else 0)
        s = dict(stage=stage, n_words=n_words, n_occ=n_occ, B=B, G=G, wpb=wpb, staged=staged, lv=[int(t) for t in v[16:16 + nlv]], overflow=overflow,
                 part_bits=part_bits, n_dist=n_dist, levels=[])
        for what, (name, dt) in enumerate(_TOP):
            s[name] = np.zeros(sizes[name], dtype=dt)
            L._check(cp(h, -1, what, s[name].ctypes.data, s[name].nbytes))
        for li in range(1, nlv if stage >= 3 else 1):
            L._check(info(h, li, v.ctypes.data))
            lev = dict(bits_used=int(v[0]), bits=int(v[1]), buf=np.zeros(int(v[2]), dtype=np.uint64), ostart=np.zeros(int(v[4]), dtype=np.uint64),
                       olen=np.zeros(int(v[4]), dtype=np.uint32))
            for what, name in enumerate(("buf", "ostart", "olen")):
                L._check(cp(h, li, what, lev[name].ctypes.data, lev[name].nbytes))
            s["levels"].append(lev)
        return s
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


def describe(s):
    return f"levels {s['lv']} (B {s['B']}), G {s['G']} x {s['wpb']} words, {'staged' if s['staged'] else 'unstaged'}, stage {s['stage']}"


def overflows(ref, lv):
    """a partition of the plan holds more distinct k-mers than k_count's LDS table has slots: the count is the defined error
    `k_count: LDS table overflow` then, and only then"""
    return ref.n_occ > 0 and int(np.bincount(ref.final_sets(lv)[0]).max()) > CR.COUNT_SLOTS


def run(ctx, k, inp, where, min_len=0, oracle=None, **opts):
    """snapshot under the options, (a) .. (e), the table against the oracle's -> the snapshot.  A plan with a partition of more distinct k-mers
    than the LDS table takes: (a) .. (c) and the overflow word"""
    b, o, ref = inp
    with options(ctx, skm=0 if k >= 20 else 1, **opts):
        s = snapshot(ctx, b, o, k, min_len)
    print(f"{where}: {describe(s)}")
    over = s["stage"] >= 2 and overflows(ref, s["lv"])
    try:
        CR.check(s, ref, expect_overflow=over)
    except AssertionError as e:
        raise AssertionError(f"{where} [{describe(s)}]: {e}") from None
    if oracle is not None and not over:
        ok, ov = oracle.Table().count_buffer(b, o, k, min_len).export()
        order = np.argsort(s["dk"], kind="stable")
        assert np.array_equal(s["dk"][order], ok) and np.array_equal(s["dc"][order].astype(np.int32), ov), (where, "the table is not the oracle's")
    return s


def forced(ref, l1, l2, staged, blocks, target=PART_TARGET):
    """the plan the options ask for on this input: (levels, G, words per workgroup, staged)"""
    lv, _ = CR.plan_levels(ref.n_occ, ref.n_reads, ref.n_bases, ref.k, ref.min_len, l1, l2, target)
    return (lv,) + CR.level1_blocks(ref.n_words, blocks, N_CU) + (staged,)


def assert_plan(s, ref, l1, l2, staged, blocks, where, target=PART_TARGET):
    assert (s["lv"], s["G"], s["wpb"], s["staged"]) == forced(ref, l1, l2, staged, blocks, target), (where, describe(s))


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_len", MIN_LENS)
@pytest.mark.parametrize("k", BITMAP_KS)
def test_bitmap_edges(gpu_ctx, oracle, k, min_len):
    """ragged reads, and the neighbour patterns of k_mask_reads' plain read-modify-write at every alignment.  A failure of check (a) on the
    crafted run names the word: with the read lengths of neighbour_run that is the pattern -- it is a finding, not something to run again"""
    run(gpu_ctx, k, ref_of("ragged", lambda: ragged_reads(k), k, min_len), f"k = {k}, min_len = {min_len}, ragged reads", min_len, oracle)
    run(gpu_ctx, k, ref_of(("run", min_len), lambda: neighbour_run(k, min_len), k, min_len), f"k = {k}, min_len = {min_len}, neighbour patterns", min_len, oracle)


@pytest.mark.parametrize("l1,l2,staged,blocks,target", PLANS)
@pytest.mark.parametrize("k", [11, 31])
def test_plans(gpu_ctx, oracle, k, l1, l2, staged, blocks, target):
    inp = ref_of("plan", plan_reads, k)
    where = f"k = {k}, plan ({l1}, {l2}, {staged}, {blocks}), part_target {target}"
    s = run(gpu_ctx, k, inp, where, oracle=oracle, l1_bits=l1, l2_bits=l2, scatter_staged=staged, l1_blocks=blocks, part_target=target)
    assert_plan(s, inp[2], l1, l2, staged, blocks, where, target)
    if target == 8:
        assert s["lv"] == [2, 11, 2] and [(v["bits_used"], v["bits"]) for v in s["levels"]] == [(2, 11), (13, 2)]
    if (l1, l2) == (0, 0):
        # one partition of far more than 4096 distinct k-mers: K0 .. K1 as ever, then the defined error, from the hook and from the production call
        from metafast_amd import lib as L
        assert s["lv"] == [0] and s["part_bits"] == 0 and len(s["dcount"]) == 1 and s["stage"] == 4 and s["overflow"] != 0
        with options(gpu_ctx, skm=0 if k >= 20 else 1, l1_bits=l1, l2_bits=l2, scatter_staged=staged, l1_blocks=blocks, part_target=target):
            with pytest.raises(L.MetafastError, match="k_count: LDS table overflow"):
                gpu_count(gpu_ctx, inp[0], inp[1], k)
    else:
        assert s["stage"] == 5 and s["overflow"] == 0


def test_flush_queue(gpu_ctx, oracle):
    """2048 staging lines fed by random 16-mers on one workgroup: many lanes of a wave complete different lines in the same step, more than
    the 16 entries of the wave's flush queue among them (tests/test_count_ref_cpu.py asserts the necessary condition on the input)"""
    inp = ref_of("flush", flush_reads, 16)
    for blocks in (1, 0):
        where = f"k = 16, random sequence, plan (11, -1), l1_blocks {blocks}"
        s = run(gpu_ctx, 16, inp, where, oracle=oracle, l1_bits=11, l2_bits=-1, l1_blocks=blocks)
        assert_plan(s, inp[2], 11, -1, 1, blocks, where)
        assert s["lv"] == [11] and s["staged"] == 1


@pytest.mark.parametrize("k", [5, 2])
def test_heavy_partitions(gpu_ctx, oracle, k):
    """partitions longer than k_count's prefetch window with few distinct keys: the rest of the partition comes straight from HBM; the
    clamp at 32767"""
    want_a = {"A x 32766": 32766, "A x 32767": 32767, "A x 32768": 32767, "A * 40000": 32767}
    for name, reads in heavy_inputs(k).items():
        inp = ref_of(("heavy", name), lambda: pack_reads(reads), k)
        for l1 in (0, 1):
            s = run(gpu_ctx, k, inp, f"k = {k}, {name}, plan ({l1}, 0)", oracle=oracle, l1_bits=l1, l2_bits=0)
            assert s["lv"] == [l1] and np.all(s["plen"][s["dcount"] > 0] > CR.PREFETCH) and s["dcount"].max() <= 512
            if name in want_a:
                assert s["dk"].tolist() == [0] and s["dc"].tolist() == [want_a[name]]


def test_table_limit_and_overflow(gpu_ctx, oracle):
    """one partition (plan (0, 0)) at k = 16: 4096 distinct k-mers fill the LDS table to the last slot; 4097 are the defined error
    `k_count: LDS table overflow` of the production call, the hook reports the overflow word set, and the context counts on afterwards"""
    from metafast_amd import lib as L
    k = 16
    full = ref_of("4096", lambda: distinct_read(k, CR.COUNT_SLOTS), k)
    over = ref_of("4097", lambda: distinct_read(k, CR.COUNT_SLOTS + 1), k)
    s = run(gpu_ctx, k, full, "k = 16, 4096 distinct k-mers in one partition", oracle=oracle, l1_bits=0, l2_bits=0)
    assert s["lv"] == [0] and s["dcount"].tolist() == [CR.COUNT_SLOTS] and s["plen"].tolist() == [CR.COUNT_SLOTS]
    with options(gpu_ctx, l1_bits=0, l2_bits=0):
        with pytest.raises(L.MetafastError, match="k_count: LDS table overflow"):
            gpu_count(gpu_ctx, over[0], over[1], k)
        s = snapshot(gpu_ctx, over[0], over[1], k)
        assert s["stage"] == 4 and s["overflow"] != 0 and s["n_dist"] == 0 and len(s["dk"]) == 0, describe(s)
        CR.check(s, over[2], expect_overflow=True)
        t = gpu_count(gpu_ctx, full[0], full[1], k)
        gk, gc = t.export()
        ok, ov = oracle.Table().count_buffer(full[0], full[1], k).export()
        assert np.array_equal(gk, ok) and np.array_equal(gc.astype(np.int32), ov)
    # the loop over what lies beyond the prefetch window: one key of 3073, none of 3072
    for n_occ in (CR.PREFETCH + 1, CR.PREFETCH):
        inp = ref_of(("few", n_occ), lambda: few_distinct_read(k, n_occ), k)
        s = run(gpu_ctx, k, inp, f"k = 16, {n_occ} keys, few distinct", oracle=oracle, l1_bits=0, l2_bits=0)
        assert s["plen"].tolist() == [int(CR.roundup8(n_occ))] and s["dcount"][0] <= 5


def test_nothing_to_do(gpu_ctx):
    for reads, k, min_len, stage in (([], 5, 0, 0), ([""] * 3, 5, 0, 0), (["ACG", "AC", "", "ACGT"], 5, 0, 1), (["ACGT" * 25] * 40, 19, 101, 1)):
        b, o = pack_reads(reads)
        s = run(gpu_ctx, k, (b, o, CR.Reference(b, o, k, min_len)), f"k = {k}, min_len = {min_len}, {len(reads)} reads without a k-mer", min_len)
        assert s["stage"] == stage and s["n_occ"] == 0 and s["n_dist"] == 0 and not s["vmask"].any() and len(s["buf1"]) == 0 and len(s["dk"]) == 0
        with options(gpu_ctx):
            t = gpu_count(gpu_ctx, b, o, k, min_len)
            assert len(t) == 0 and t.occurrences() == 0


def test_hook_refuses_the_other_path_and_leaves_the_count_alone(gpu_ctx, oracle):
    from metafast_amd import lib as L
    k = 31
    b, o, ref = ref_of("plan", plan_reads, k)
    with options(gpu_ctx):
        with pytest.raises(L.MetafastError, match="super-k-mer path"):
            snapshot(gpu_ctx, b, o, k)
        CR.check(snapshot(gpu_ctx, b, o, 19), CR.Reference(b, o, 19))          # k < 20: this path whatever option skm says
        t = gpu_count(gpu_ctx, b, o, k)                                         # the next count on the same context is an ordinary one
        gk, gc = t.export()
        ok, ov = oracle.Table().count_buffer(b, o, k).export()
        assert np.array_equal(gk, ok) and np.array_equal(gc.astype(np.int32), ov) and t.records()[1] == 16
