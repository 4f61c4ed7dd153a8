"""k_skm_scatter (metafast_amd/csrc/mf_skm_scatter.h) where its run list and its staging protocol work under lane masks: a descriptor is written
only by the lanes that start a run at a position (skm_runlist8), and only pending lanes peek, reserve, write and commit in
skm_stage_insert.  Every partition's record multiset and the directory invariants against tests/skm_ref.py, with the checks and the hook
of tests/test_skm_records_gpu.py, bit-exact, in the exact and in the one-pass form.

What an input is for is asserted from the reference before the GPU sees it (a wave's batch is 63 words = 2016 positions of the base
stream; NR, the descriptors a batch lists, is counted by batch_runs below as the kernel counts it):

    two short reads        k = 20, 25, 26, 31: both minimizer lengths, the smallest and the largest RMAX; a batch of two or three runs
    one run                a batch that lists ONE descriptor (rl[0] is read by all 64 lanes), its other words without a run start -- words
                           without a k-mer, and in the one-pass form the word whose whole head went to the run of the word in front of it
    dense words            two neighbouring words in which EVERY valid position starts a run (reads whose consecutive k-mers all differ in
                           their minimizer hash: 9 to 13 starts per word at k = 20, 5 or 6 at k = 31), followed by a word without any start: a
                           descriptor too many or too few lands in the neighbour's part of the list
    NR = 255 .. 385        the last slot of the first four-wide iteration, the first of the second, the last of the list, and one run too
                           many (that batch takes the per-lane loop: in the one-pass form its runs do not go on across word borders)
    one hot digit          1500 copies of a read: a staging line closes again and again while the other lanes wait, several flush blocks per
                           turn; one workgroup and three
    slices                 four slices of 8 of the 32 digits each: three quarters of the records are predicated out in front of the insert,
                           with the hot digit inside the slice and outside it
    ragged end             17 bases behind the last k-mer, a read across the border of the first wave's batch"""
import numpy as np
import pytest

import skm_ref as S
import test_skm_records_gpu as T
from util import genome_reads, pack_reads

gpu = pytest.mark.gpu
BATCH = S.WAVE_WORDS * 32
AL = np.frombuffer(b"ACGT", dtype=np.uint8)
FORMS = (("exact", 0), ("one-pass", 2))


def rand_read(rng, n):
    return AL[rng.integers(0, 4, size=n)].tobytes()


def batch_runs(sc, wpb, one_pass):
    """-> (descriptors listed per wave batch, batches that hold a piece of more than RMAX k-mers): NR and the run-length check of the kernel"""
    k, r = sc.k, S.rmax(sc.k)
    ps, pl = sc.pieces(True)
    word = ps // 32
    rel = word % wpb
    batch = (word // wpb) * (wpb // S.WAVE_WORDS + 1) + rel // S.WAVE_WORDS
    nb = int(batch.max()) + 1
    n = np.bincount(batch, minlength=nb)
    if one_pass:                                           # a head that goes to the run in front of it whole is not listed
        head = np.zeros(len(ps), dtype=bool)
        head[1:] = ((ps[1:] % 32) == 0) & (ps[:-1] + pl[:-1] == ps[1:]) & (sc.mh[ps[1:]] == sc.mh[ps[:-1]]) & ((rel % S.WAVE_WORDS)[1:] > 0)
        tail = np.zeros(len(ps), dtype=np.int64)
        tail[1:] = pl[:-1]
        ext = np.where(head, np.minimum(pl, np.clip(np.minimum(r - tail, 49 - k), 0, None)), 0)
        n = n - np.bincount(batch, weights=(ext > 0) & (ext == pl), minlength=nb).astype(np.int64)
    return n.astype(np.int64), np.bincount(batch, weights=(pl > r), minlength=nb) > 0


def fillers(k, n_bases):
    """reads too short for a k-mer that cover at least n_bases"""
    return [("ACGT" * 8)[:k - 1]] * (n_bases // (k - 1) + 1)


def run_forms(ctx, k, inp, what, G=1, check=None, **opts):
    """both forms on G workgroups (G = 1: one workgroup over all words, a wave's batches start at the multiples of 63 words)"""
    for form, dyn in FORMS:
        def plan(slices):
            T.levels(2, one_pass=dyn == 2, fast=True)(slices)
            assert slices[0]["G"] == G, T.describe(slices[0])
            if check:
                check(slices, dyn == 2)
        kw = dict(l1_bits=4, l2_bits=4)
        kw.update(opts)
        T.run(ctx, k, inp, form, f"k = {k}, {what}, G = {G}, {form}", plan=plan, skm_dyn=dyn, l1_blocks=G, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def two_short_reads(k):
    rng = np.random.default_rng(5200 + k)
    return pack_reads([rand_read(rng, k + 3), rand_read(rng, k + 40)])


def one_run(k):
    """one read = one run of 9 k-mers, 2 of them in front of the border of word 40; nothing else holds a k-mer"""
    first = 32 * 40 - 2
    b, o = pack_reads([("ACGT" * 8)[:k - 1]] * (first // (k - 1)) + ["G" * (first % (k - 1)), T.one_run_read(k)])
    assert int(o[-2]) == first
    sc = S.Scan(b, o, k)
    for one_pass, want in ((False, 2), (True, 1)):
        n, long_piece = batch_runs(sc, 10 ** 9, one_pass)
        assert n.tolist() == [want] and not long_piece.any()
    assert sc.valid[32 * 40:32 * 41].any() and int(sc.valid.sum()) == 9
    return b, o, sc


_dense = {}


def dense_reads(k, r, count):
    """`count` reads of r k-mers each of which has another minimizer hash than the one in front of it"""
    if (k, r) not in _dense:
        rng = np.random.default_rng(6100 + k)
        code = rng.integers(0, 4, size=3_000_000).astype(np.uint8)
        mh = S.minimizer_hashes(code, k)
        change = mh[1:] != mh[:-1]
        ok = np.ones(len(change) - r, dtype=bool)
        for i in range(r - 1):
            ok &= change[i:i + len(ok)]
        at = np.flatnonzero(ok)
        at = at[np.concatenate([[True], np.diff(at) > k + r])]
        _dense[(k, r)] = [np.frombuffer(b"AGCT", dtype=np.uint8)[code[a:a + k + r - 1]].tobytes() for a in at]
    assert len(_dense[(k, r)]) >= count, (k, r, len(_dense[(k, r)]))
    return _dense[(k, r)][:count]


DENSE_WORD = 7                     # the first of the two dense words


def dense_words(k):
    r = 8 if k == 20 else 6
    rng = np.random.default_rng(6300 + k)
    gb, go = genome_reads(rng, 20000, 40, 150, err=0.01)
    normal = [gb[go[i]:go[i + 1]].tobytes() for i in range(40)]
    pad = 32 * DENSE_WORD - 150
    front = normal[:1] + [("ACGT" * 8)[:k - 1]] * (pad // (k - 1)) + ["G" * (pad % (k - 1))]
    dense = dense_reads(k, r, 8)
    reads, n = list(front), 32 * DENSE_WORD
    for d in dense:                                        # dense reads back to back while their k-mers start inside the two words
        if n + r - 1 >= 32 * (DENSE_WORD + 2):
            break
        reads.append(d)
        n += len(d)
    reads += fillers(k, 32 * (DENSE_WORD + 3) - n) + normal[1:]
    b, o = pack_reads(reads)
    sc = S.Scan(b, o, k)
    ps, _ = sc.pieces(True)
    for w in (DENSE_WORD, DENSE_WORD + 1):
        v = np.flatnonzero(sc.valid[32 * w:32 * w + 32]) + 32 * w
        assert len(v) >= (9 if k == 20 else 5) and np.array_equal(v, ps[(ps >= 32 * w) & (ps < 32 * w + 32)]), (k, w, len(v))
        assert np.all(sc.mh[v[1:]][np.diff(v) == 1] != sc.mh[v[:-1]][np.diff(v) == 1])
    assert not sc.valid[32 * (DENSE_WORD + 2):32 * (DENSE_WORD + 3)].any() and sc.valid[32 * (DENSE_WORD + 3):].any()
    return b, o, sc


NR_K = 20


def batch_of(nr, one_pass):
    """k = 20: a first wave batch that lists exactly nr descriptors in the given form (a random read cut to length), quiet words behind it,
    a few reads in the batches after"""
    k = NR_K
    for seed in range(400):
        rng = np.random.default_rng(7000 + seed)
        long_read = rand_read(rng, BATCH)
        later = [rand_read(rng, 100) for _ in range(6)]
        ps, _ = S.Scan(*pack_reads([long_read]), k).pieces(True)
        for j in range(nr - 1, min(nr + 60, len(ps))):
            cut = int(ps[j]) + k
            b, o = pack_reads([long_read[:cut]] + fillers(k, BATCH + 96 - cut) + later)
            sc = S.Scan(b, o, k)
            n, long_piece = batch_runs(sc, 10 ** 9, one_pass)
            if long_piece[0] or n[0] > nr:
                break
            if n[0] == nr:
                assert not long_piece.any() and int(o[1]) <= BATCH
                return b, o, sc
    raise AssertionError(f"no batch of {nr} runs found")


NRS = (255, 256, 257, S.LIST_CAP, S.LIST_CAP + 1)
COPIES = 1500


def hot_digit(k):
    """40 reads of a genome, 1500 copies of one of them, 17 bases behind the last k-mer; a read of 300 bases across position 2016"""
    rng = np.random.default_rng(7900 + k)
    gb, go = genome_reads(rng, 20000, 60, 150, err=0.01)
    reads = [gb[go[i]:go[i + 1]].tobytes() for i in range(60)]
    head = reads[:12] + [reads[12][:100]]                  # 1900 bases
    all_reads = head + [rand_read(rng, 300)] + reads[13:40] + [reads[40]] * COPIES + reads[41:] + [rand_read(rng, 17)]
    b, o = pack_reads(all_reads)
    sc = S.Scan(b, o, k)
    n = int(o[-1])
    assert int(o[13]) == 1900 < BATCH < 2200 - k and sc.valid[1900:2200 - k + 1].all()
    assert n % 16 and n % 32 and not sc.valid[n - 17:].any() and sc.valid[n - 17 - k]
    return b, o, sc


def hot_share(sc, bits):
    """the exact form's records in the fullest level-1 digit (every copy of the read has at least one there), and that digit"""
    start, _ = sc.exact()
    d1 = (T.R.remix32(sc.mh[start]) >> np.uint64(32 - bits)).astype(np.int64)
    c = np.bincount(d1, minlength=1 << bits)
    return int(c.max()), int(c.argmax())


# ---------------------------------------------------------------------------------------------------------------------------------
# no GPU: the inputs are what the docstring says (the builders assert it)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (20, 31))
def test_inputs_one_run_and_dense_words(k):
    T.scan_of("runlist_one", lambda: one_run(k + (k == 20))[:2], k + (k == 20))
    T.scan_of("runlist_dense", lambda: dense_words(k)[:2], k)
    assert hot_share(T.scan_of("runlist_hot", lambda: hot_digit(k)[:2], k)[2], 4)[0] >= COPIES


@pytest.mark.parametrize("one_pass", (False, True))
@pytest.mark.parametrize("nr", NRS)
def test_inputs_batches_of_nr_runs(nr, one_pass):
    sc = T.scan_of(("runlist_nr", nr, one_pass), lambda: batch_of(nr, one_pass)[:2], NR_K)[2]
    assert batch_runs(sc, 10 ** 9, one_pass)[0][0] == nr


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", (20, 25, 26, 31))
def test_two_short_reads(gpu_ctx, k):
    run_forms(gpu_ctx, k, T.scan_of("runlist_two", lambda: two_short_reads(k), k), "two short reads", l1_bits=3, l2_bits=3)


@gpu
@pytest.mark.parametrize("k", (21, 31))                   # (the read of T.one_run_read holds its minimizer in all 9 k-mers from k = 21 on)
def test_one_run_in_a_batch(gpu_ctx, k):
    run_forms(gpu_ctx, k, T.scan_of("runlist_one", lambda: one_run(k)[:2], k), "a batch of one run", l1_bits=3, l2_bits=3)


@gpu
@pytest.mark.parametrize("k", (20, 31))
def test_every_valid_position_starts_a_run(gpu_ctx, k):
    run_forms(gpu_ctx, k, T.scan_of("runlist_dense", lambda: dense_words(k)[:2], k), "two dense words in front of an empty one")


@gpu
@pytest.mark.parametrize("nr", NRS)
def test_batches_of_nr_runs(gpu_ctx, nr):
    for form, dyn in FORMS:
        inp = T.scan_of(("runlist_nr", nr, dyn == 2), lambda: batch_of(nr, dyn == 2)[:2], NR_K)

        def plan(slices):
            T.levels(2, one_pass=dyn == 2, fast=True)(slices)
            assert slices[0]["G"] == 1 and slices[0]["wpb"] >= S.WAVE_WORDS
            assert batch_runs(inp[2], slices[0]["wpb"], dyn == 2)[0][0] == nr         # with the batch geometry the hook reports
        T.run(gpu_ctx, NR_K, inp, form, f"k = {NR_K}, a batch of {nr} runs, {form}", plan=plan, skm_dyn=dyn, l1_bits=4, l2_bits=4, l1_blocks=1)


@gpu
@pytest.mark.parametrize("G", (1, 3))
@pytest.mark.parametrize("k", (20, 31))
def test_one_hot_digit_and_a_ragged_end(gpu_ctx, k, G):
    run_forms(gpu_ctx, k, T.scan_of("runlist_hot", lambda: hot_digit(k)[:2], k), "one hot digit", G=G)


@gpu
@pytest.mark.parametrize("k", (20, 31))
def test_slices_with_and_without_the_hot_digit(gpu_ctx, k):
    inp = T.scan_of("runlist_hot", lambda: hot_digit(k)[:2], k)
    share, hot = hot_share(inp[2], 5)
    assert share >= COPIES
    for form, dyn in FORMS:
        def plan(slices):
            T.levels(2, one_pass=dyn == 2, fast=True)(slices)
            assert [(sl["dlo"], sl["dhi"]) for sl in slices] == [(8 * i, 8 * i + 8) for i in range(4)]
            assert sum(sl["dlo"] <= hot < sl["dhi"] for sl in slices) == 1
        T.run(gpu_ctx, k, inp, form, f"k = {k}, four slices, hot digit {hot}, {form}", plan=plan, skm_dyn=dyn, l1_bits=5, l2_bits=5, skm_slices=4, skm_shared=0)
