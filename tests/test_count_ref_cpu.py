"""tests/count_ref.py (the reference of tests/test_count_stages_gpu.py) without a GPU: its table is the pinned oracle's on every input of the GPU
cases, its check passes a snapshot built from the reference itself and rejects that snapshot with one thing wrong, naming the stage, and the
inputs have the properties the GPU cases rest on."""
import copy

import numpy as np
import pytest

import count_ref as CR
import nbr_ref as R
import test_count_stages_gpu as G
from util import pack_reads


def _inputs():
    """(name, make, k, min_len) of every input of the GPU cases"""
    out = []
    for k in G.BITMAP_KS:
        for min_len in G.MIN_LENS:
            out.append((f"ragged k {k} min_len {min_len}", lambda k=k: G.ragged_reads(k), k, min_len))
            out.append((f"run k {k} min_len {min_len}", lambda k=k, m=min_len: G.neighbour_run(k, m), k, min_len))
    out += [(f"plan k {k}", G.plan_reads, k, 0) for k in (11, 31)] + [("flush", G.flush_reads, 16, 0)]
    for k in (5, 2):
        out += [(f"heavy {name} k {k}", lambda r=reads: pack_reads(r), k, 0) for name, reads in G.heavy_inputs(k).items()]
    out += [(f"{n} distinct", lambda n=n: G.distinct_read(16, n), 16, 0) for n in (4096, 4097)]
    out += [(f"{n} keys", lambda n=n: G.few_distinct_read(16, n), 16, 0) for n in (3072, 3073)]
    out += [("short reads", lambda: pack_reads(["ACG", "AC", "", "ACGT"]), 5, 0), ("below min_len", lambda: pack_reads(["ACGT" * 25] * 40), 19, 101)]
    return out


INPUTS = _inputs()


@pytest.mark.parametrize("name,make,k,min_len", INPUTS, ids=[i[0] for i in INPUTS])
def test_reference_table_is_the_oracles(oracle, name, make, k, min_len):
    b, o = make()
    ref = CR.Reference(b, o, k, min_len)
    ok, ov = oracle.Table().count_buffer(b, o, k, min_len).export()
    tk, tc = ref.table()
    assert np.array_equal(tk, ok) and np.array_equal(tc, ov)
    # the union of the partitions of a plan, sorted, is the same table
    _, wk, wc = ref.final_sets([3, 2])
    order = np.argsort(wk, kind="stable")
    assert np.array_equal(wk[order], ok) and np.array_equal(wc[order].astype(np.int32), ov)
    lens = np.diff(o.astype(np.int64))
    assert ref.n_occ == int(np.maximum(lens - k + 1, 0)[lens >= max(k, min_len)].sum()) == int(sum(bin(int(w)).count("1") for w in ref.vmask))


def test_definitions_by_hand():
    assert CR.encode("AGCT") == 0b00011011 and CR.base_codes(np.frombuffer(b"AaGgCcTt", dtype=np.uint8)).tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    # reads of 5, 2 and 4 bases at k = 3, then with min_len = 5: valid starts 0 1 2 | - | 7 8
    b, o = pack_reads(["ACGTA", "GG", "ttga"])
    r = CR.Reference(b, o, 3)
    assert r.valid.tolist() == [1, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0] and r.vmask.tolist() == [0b110000111] and r.n_occ == 5
    assert CR.Reference(b, o, 3, 5).vmask.tolist() == [0b111]
    # ACG -> its reverse complement CGT is larger in the order A G C T; TTG <-> CAA
    assert r.keys.tolist() == [min(CR.encode(x), CR.encode(y)) for x, y in (("ACG", "CGT"), ("CGT", "ACG"), ("GTA", "TAC"), ("TTG", "CAA"), ("TGA", "TCA"))]
    assert int(R.revcomp(CR.encode("TTG"), 3)) == CR.encode("CAA")
    # bit 32 of a 40-base read is bit 0 of word 1; bits from n_bases on are clear
    b, o = pack_reads(["A" * 40])
    assert CR.Reference(b, o, 8).vmask.tolist() == [0xFFFFFFFF, 1]
    h = CR.phash(np.array([0, 1, 0x123456789ABCDEF], dtype=np.uint64))
    x = 0x123456789ABCDEF
    assert h.tolist() == [0, CR.PHASH_MULT, ((x ^ (x >> 31)) * CR.PHASH_MULT) % (1 << 64)]
    hh = np.array([0xF123456789ABCDEF], dtype=np.uint64)
    assert CR.digit(hh, 0, 4).tolist() == [0xF] and CR.digit(hh, 4, 8).tolist() == [0x12] and CR.digit(hh, 12, 11).tolist() == [0x345 >> 1] and CR.digit(hh, 0, 0).tolist() == [0]
    assert CR.plan_levels(200000, 2000, 200000, 11, 0, 2, -1, 8) == ([2, 11, 2], 15) and CR.plan_levels(200000, 2000, 200000, 31, 0, 3, -1, 3072) == ([3, 4], 7)
    assert CR.plan_levels(200000, 2000, 200000, 31, 0, 11, -1, 3072)[0] == [11] and CR.plan_levels(10, 1, 100, 16, 0, 0, 0, 3072)[0] == [0]
    assert CR.level1_blocks(7200, 5, 256) == (5, 1440) and CR.level1_blocks(7200, 0, 256) == (8, 900) and CR.level1_blocks(100, 3, 256) == (1, 100)


# ---------------------------------------------------------------------------------------------------------------------------------
# check bites
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(9)
    lens = [70, 0, 64, 33, 5, 4, 120] * 12 + [400]
    b, o = pack_reads([np.frombuffer(b"ACG", dtype=np.uint8)[rng.integers(0, 3, size=n)].tobytes() for n in lens])       # three letters: 5-mers repeat
    ref = CR.Reference(b, o, 5)
    return ref, CR.model(ref, [2, 3], 2)


@pytest.mark.parametrize("l1,l2,staged,blocks,target", G.PLANS)
@pytest.mark.parametrize("k", [11, 31])
def test_model_of_every_plan_passes(k, l1, l2, staged, blocks, target):
    b, o, ref = G.ref_of("plan", G.plan_reads, k)
    lv, g, wpb, _ = G.forced(ref, l1, l2, staged, blocks, target)
    s = CR.model(ref, lv, g, staged)
    assert s["wpb"] == wpb
    CR.check(s, ref)


def test_model_passes_and_empty_snapshots(small):
    ref, s = small
    assert len(s["levels"]) == 1 and s["part_bits"] == 5 and s["stage"] == 5 and s["dc"].max() > 1
    CR.check(s, ref)
    for reads, k, min_len, stage in (([], 5, 0, 0), (["", ""], 5, 0, 0), (["ACG", "AC"], 5, 0, 1), (["ACGTACGT"], 5, 9, 1)):
        b, o = pack_reads(reads)
        r = CR.Reference(b, o, k, min_len)
        e = CR.model(r, [2, 3], 2)
        assert e["stage"] == stage
        CR.check(e, r)
        full = copy.deepcopy(s)
        with pytest.raises(AssertionError):
            CR.check(full, r)


def _region(s, i):
    bs = s["blockstart"].astype(np.int64)
    return int(bs[i]), int(bs[i + 1]), int(s["blockhist"][i])


def test_check_rejects_one_wrong_thing_at_a_time(small):
    ref, good = small
    CR.check(good, ref)

    def doctored():
        return copy.deepcopy(good)

    # a bitmap bit: set where it should be clear, clear where it should be set
    for w, bit in ((0, 31), (2, 0)):
        s = doctored()
        s["vmask"][w] ^= np.uint32(1 << bit)
        with pytest.raises(AssertionError, match=rf"^K0: vmask\[{w}\]"):
            CR.check(s, ref)
    s = doctored()
    s["n_occ"] += 1
    with pytest.raises(AssertionError, match="^K0: n_occ"):
        CR.check(s, ref)
    # a key moved to the neighbouring region (a sentinel in its place)
    i = next(i for i in range(len(good["blockhist"]) - 1) if _region(good, i)[2] >= 1 and _region(good, i + 1)[2] % 8 != 0)
    s = doctored()
    a0, _, ac = _region(s, i)
    b0, _, bc = _region(s, i + 1)
    s["buf1"][b0 + bc] = s["buf1"][a0 + ac - 1]
    s["buf1"][a0 + ac - 1] = CR.EMPTY
    with pytest.raises(AssertionError, match="^K1: region"):
        CR.check(s, ref)
    # ... swapped with a key of the neighbouring region: only the multisets tell
    j = next(j for j in range(len(good["blockhist"]) - 1) if _region(good, j)[2] >= 1 and _region(good, j + 1)[2] >= 1)
    s = doctored()
    a0, b0 = _region(s, j)[0], _region(s, j + 1)[0]
    s["buf1"][[a0, b0]] = s["buf1"][[b0, a0]]
    with pytest.raises(AssertionError, match="^K1: region .* does not hold the reference's multiset"):
        CR.check(s, ref)
    # a sentinel replaced by a key's duplicate
    s = doctored()
    b0, _, bc = _region(s, i + 1)
    s["buf1"][b0 + bc] = s["buf1"][b0]
    with pytest.raises(AssertionError, match="^K1: region .* where a sentinel belongs"):
        CR.check(s, ref)
    # 0xA5 inside a region: among the keys, in the padding
    s = doctored()
    s["buf1"][_region(s, i)[0]] = CR.FILL
    with pytest.raises(AssertionError, match="^K1: region .* 0xA5 fill left inside"):
        CR.check(s, ref)
    s = doctored()
    s["buf1"][b0 + bc] = CR.FILL
    with pytest.raises(AssertionError, match="^K1: region .* where a sentinel belongs .0xA5 fill left inside"):
        CR.check(s, ref)
    # a write behind the last region; a histogram entry; a region start
    s = doctored()
    s["buf1"][-1] = 7
    with pytest.raises(AssertionError, match="^K1: entry .* outside every region"):
        CR.check(s, ref)
    s = doctored()
    s["blockhist"][i] += 1
    with pytest.raises(AssertionError, match="^K1: histogram"):
        CR.check(s, ref)
    s = doctored()
    s["blockstart"][1] += 4
    with pytest.raises(AssertionError, match="^K1: blockstart"):
        CR.check(s, ref)
    s = doctored()
    s["plen1"][0] -= 8
    with pytest.raises(AssertionError, match="^K1: pstart / plen"):
        CR.check(s, ref)
    # the K2 level: the same things, and the directory
    lev = good["levels"][0]
    q = next(q for q in range(len(lev["olen"]) - 1) if lev["olen"][q] and lev["olen"][q + 1])
    s = doctored()
    a0, b0 = int(lev["ostart"][q]), int(lev["ostart"][q + 1])
    s["levels"][0]["buf"][[a0, b0]] = s["levels"][0]["buf"][[b0, a0]]
    with pytest.raises(AssertionError, match="^K2 level 1: region"):
        CR.check(s, ref)
    s = doctored()
    s["levels"][0]["olen"][q] += 8
    with pytest.raises(AssertionError, match="^K2 level 1: olen"):
        CR.check(s, ref)
    s = doctored()
    s["levels"][0]["ostart"][1] -= 8
    with pytest.raises(AssertionError, match="^K2 level 1: the sub-regions of partition 0"):
        CR.check(s, ref)
    s = doctored()
    s["levels"][0]["bits_used"] = 3
    with pytest.raises(AssertionError, match="^K2 level 1: 3 bits behind 3"):
        CR.check(s, ref)
    s = doctored()
    s["levels"][0]["buf"][int(lev["ostart"][0]) - 1] = 0
    with pytest.raises(AssertionError, match="^K2 level 1: entry .* outside every region"):
        CR.check(s, ref)
    # K3: a count raised by 1; 32768 where 32767 belongs; dcount; a count behind the set; the overflow word
    p = int(np.flatnonzero(good["dcount"])[0])
    at = int(good["pstart"][p])
    s = doctored()
    s["cnt"][at] += 1
    with pytest.raises(AssertionError, match="^K3: partition .* cnt = "):
        CR.check(s, ref)
    s = doctored()
    s["dcount"][p] -= 1
    with pytest.raises(AssertionError, match=rf"^K3: dcount\[{p}\]"):
        CR.check(s, ref)
    s = doctored()
    s["cnt"][at + int(good["dcount"][p])] = 1
    with pytest.raises(AssertionError, match="^K3: cnt"):
        CR.check(s, ref)
    s = doctored()
    s["keys"][at] ^= np.uint64(1 << 9)
    with pytest.raises(AssertionError, match="^K3: partition .* is not the set of its distinct k-mers"):
        CR.check(s, ref)
    s = doctored()
    s["overflow"] = 1
    with pytest.raises(AssertionError, match="^K3: the overflow word"):
        CR.check(s, ref)
    with pytest.raises(AssertionError, match="^K1: the snapshot ends at stage 5"):
        CR.check(s, ref, expect_overflow=True)
    s["stage"] = 4
    CR.check(s, ref, expect_overflow=True)
    s["overflow"] = 0
    with pytest.raises(AssertionError, match="^K3: the overflow word is not set"):
        CR.check(s, ref, expect_overflow=True)
    # the table: d_part_off shifted by one; part_bits; an entry in another partition
    s = doctored()
    s["part_off"][1:] += 1
    with pytest.raises(AssertionError, match=r"^table: d_part_off\[1\]"):
        CR.check(s, ref)
    s = doctored()
    s["part_bits"] = 4
    with pytest.raises(AssertionError, match="^table: part_bits"):
        CR.check(s, ref)
    s = doctored()
    s["dk"][[0, -1]] = s["dk"][[-1, 0]]
    with pytest.raises(AssertionError, match="^table: a partition of the table"):
        CR.check(s, ref)
    s = doctored()
    s["dc"][0] += 1
    with pytest.raises(AssertionError, match="^table: "):
        CR.check(s, ref)


def test_check_rejects_a_count_beyond_the_clamp():
    """32768 where 32767 belongs"""
    b, o = pack_reads(["A" * 40000, "ACGTTGCA" * 8])
    ref = CR.Reference(b, o, 5)
    s = CR.model(ref, [1], 1)
    CR.check(s, ref)
    at = int(np.flatnonzero(s["cnt"] == 32767)[0])
    assert s["keys"][at] == 0
    s["cnt"][at] = 32768
    with pytest.raises(AssertionError, match="^K3: partition .* cnt = 32768, min\\(occurrences, 32767\\) = 32767"):
        CR.check(s, ref)
    # a plan of 0 bits keeps no partition structure
    s = CR.model(ref, [0], 1)
    assert s["part_bits"] == 0 and len(s["part_off"]) == 0
    CR.check(s, ref)
    s["part_off"] = np.array([0, s["n_dist"]], dtype=np.uint64)
    with pytest.raises(AssertionError, match="^table: part_bits = 0 with 2 offsets"):
        CR.check(s, ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# what the GPU cases rest on
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_len", G.MIN_LENS)
@pytest.mark.parametrize("k", G.BITMAP_KS)
def test_bitmap_inputs(k, min_len):
    b, o = G.ragged_reads(k)
    lens = np.diff(o.astype(np.int64)).tolist()
    assert {k - 1, k, k + 1, 31, 32, 33, 63, 64, 65, 0, 120} <= set(lens) and max(lens) <= 121 and int(o[-1]) % 32 != 0 and len(lens) < 3000
    b, o = G.neighbour_run(k, min_len)
    lens = np.diff(o.astype(np.int64))
    assert len(lens) < 3000 and int(o[-1]) % 32 != 0 and lens[-1] >= 64 and lens[-1] >= min_len
    n = G.pattern_counts(o, k, min_len)
    for name in G.PATTERNS:
        # (a next read of 64 bases or more below min_len needs min_len > 64)
        assert n[name] >= 50 or (name == "next_below_min_len" and min_len <= 64 and n[name] == 0), (name, n)
    if min_len <= 64:
        # the lengths the patterns are named after
        pairs = set(zip(lens[:-1].tolist(), lens[1:].tolist()))
        assert {(64, 64), (64, 63), (64, k - 1), (64, 0)} <= pairs and (min_len == 65 or (64, 0, 64) in set(zip(lens[:-2].tolist(), lens[1:-1].tolist(), lens[2:].tolist())))
    assert min(G.border_counts(o, k, min_len)) >= 10, G.border_counts(o, k, min_len)


def test_plan_inputs():
    for k in (11, 31):
        b, o, ref = G.ref_of("plan", G.plan_reads, k)
        assert ref.n_reads < 3000 and ref.n_bases % 32 != 0
        for l1, l2, staged, blocks, target in G.PLANS:
            lv, g, wpb, _ = G.forced(ref, l1, l2, staged, blocks, target)
            # the asked G stands: the input has more than 1024 words for each (no l1_blocks: the cap itself, one workgroup per 1024 words)
            assert g == (blocks if blocks else (ref.n_words + 1023) // 1024) and (ref.n_words + 1023) // 1024 > 5, (blocks, g)
            assert lv[0] == l1 and (l2 < 0 or sum(lv[1:]) == l2) and max(lv) <= 11
            # one partition for all of these reads is the LDS table's overflow (the table-limit case has the single partition that fits); every other plan fits
            assert G.overflows(ref, lv) == ((l1, l2) == (0, 0))
        assert G.forced(ref, 2, -1, 1, 2, 8)[0] == [2, 11, 2] and G.forced(ref, 11, -1, 1, 0)[0] == [11] and G.forced(ref, 0, 0, 1, 0)[0] == [0]
        assert len(G.forced(ref, 3, -1, 1, 1)[0]) == 2


def test_flush_queue_input():
    """necessary for more than 16 lanes of a wave to complete different lines in one step (the interleaving itself cannot be pinned): a
    workgroup fills eight or more slots -- a whole line -- in more than 16 distinct digits.  Here every workgroup does in nearly all 2048, and
    the 32 k-mers of a word go to about 32 different digits"""
    b, o, ref = G.ref_of("flush", G.flush_reads, 16)
    for blocks in (1, 0):
        lv, g, wpb, _ = G.forced(ref, 11, -1, 1, blocks)
        assert lv == [11] and g == (1 if blocks else 7)
        hist = np.bincount(CR.digit(ref.hash, 0, 11) * g + ref.block_of(wpb), minlength=2048 * g).reshape(2048, g)
        assert ((hist >= 8).sum(axis=0) > 16).any() and ((hist >= 8).sum(axis=0) > 1024).all()
    d, w = CR.digit(ref.hash, 0, 11), ref.pos // 32
    per_word = np.array([len(set(d[w == x].tolist())) for x in range(100, 120)])
    assert per_word.min() >= 28


def test_heavy_inputs():
    for k in (5, 2):
        for name, reads in G.heavy_inputs(k).items():
            b, o = pack_reads(reads)
            ref = CR.Reference(b, o, k)
            for l1 in (0, 1):
                p = ref.partition_after([l1], 1)
                n = np.bincount(p, minlength=1 << l1)
                wp, _, wc = ref.final_sets([l1])
                assert np.all(n[n > 0] > CR.PREFETCH) and np.bincount(wp).max() <= 512, (k, name, n)
        want = {"A x 32766": 32766, "A x 32767": 32767, "A x 32768": 32767, "A * 40000": 32767}
        for name, c in want.items():
            b, o = pack_reads(G.heavy_inputs(k)[name])
            tk, tc = CR.Reference(b, o, k).table()
            assert tk.tolist() == [0] and tc.tolist() == [c]
        assert G.heavy_inputs(k)["lower case"][0].islower()


def test_table_limit_inputs():
    for n in (4096, 4097):
        b, o = G.distinct_read(16, n)
        ref = CR.Reference(b, o, 16)
        assert ref.n_occ == n and len(ref.table()[0]) == n and ref.n_words <= 1024
    assert CR.COUNT_SLOTS == 4096
    for n in (3072, 3073):
        b, o = G.few_distinct_read(16, n)
        ref = CR.Reference(b, o, 16)
        assert ref.n_occ == n and len(ref.table()[0]) <= 5 and int(CR.roundup8(n)) - CR.PREFETCH == (8 if n == 3073 else 0)
