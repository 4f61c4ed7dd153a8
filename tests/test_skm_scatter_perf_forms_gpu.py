"""k_skm_scatter / k_skm_hist (metafast_amd/csrc/mf_skm_scatter.h) at the edges of the cheaper scan: reverse complements cut out of reversed words, the
sliding minimum's partial results handed over by the next lane, record tails cleared with 64-bit masks.  Every partition's record multiset
against tests/skm_ref.py, with the checks and the hook of tests/test_skm_records_gpu.py, bit-exact.

One input per (k, tail), a few thousand reads:
    k = 20, 25, 26, 31     both minimizer lengths; windows of 8, 13, 12 and 17 M-mers (the three-minimum form without and with a second pass)
    tail = 1, 15, 17, 33   bases behind the last read that holds a k-mer: the base count is no multiple of 16, 32 or 64 and the last words are
                           zeroed beyond the last base at every one of the four 16-base loads
    a read of 2300 bases from base 1900: it crosses from lane 62 to lane 63 of the first wave's batch (base 2016) and lies in three batches
    2000 copies of one read: every workgroup's batch of 1008 words holds > 200 records of one digit -- its staging line closes and re-opens
                           while all sixteen waves insert into it
each run on G = 1 and G = 3 workgroups, in the exact and in the one-pass form."""
import numpy as np
import pytest

import skm_ref as S
import test_skm_records_gpu as T
from util import genome_reads, pack_reads

gpu = pytest.mark.gpu
KS = (20, 25, 26, 31)
TAILS = (1, 15, 17, 33)
LONG_AT, LONG_LEN, COPIES = 1900, 2300, 2000


def make_input(k, tail):
    rng = np.random.default_rng(7700 + 64 * k + tail)
    al = np.frombuffer(b"ACGT", dtype=np.uint8)
    gb, go = genome_reads(rng, 20000, 300, 150, err=0.01)
    reads = [gb[go[i]:go[i + 1]].tobytes() for i in range(300)]
    head = reads[:12] + [reads[12][:100]]                                   # 1900 bases
    long_read = al[rng.integers(0, 4, size=LONG_LEN)].tobytes()
    copied = reads[13]
    pads = {1: [1], 15: [15], 17: [17], 33: [16, 17]}[tail]                  # reads too short for a k-mer (k >= 20)
    last = reads[14][:150 - (5 if tail == 1 else 0)]
    all_reads = head + [long_read] + reads[15:] + [copied] * COPIES + [last] + [al[rng.integers(0, 4, size=n)].tobytes() for n in pads]
    b, o = pack_reads(all_reads)
    assert int(o[13]) == LONG_AT and int(o[-1]) - int(o[-1 - len(pads)]) == tail
    return b, o


def inp_of(k, tail):
    return T.scan_of(("perf_forms", tail), lambda: make_input(k, tail), k)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("tail", TAILS)
def test_the_inputs_reach_the_edges(k, tail):
    """no GPU: what the docstring says of the inputs, from the reference"""
    b, o, sc = inp_of(k, tail)
    n = int(o[-1])
    assert n % 16 and n % 32 and n % 64
    assert not sc.valid[n - tail:].any() and sc.valid[n - tail - k]          # the last k-mer ends `tail` bases before the end
    batch = S.WAVE_WORDS * 32
    assert LONG_AT < batch < 2 * batch < LONG_AT + LONG_LEN - k and sc.valid[LONG_AT:LONG_AT + LONG_LEN - k + 1].all()
    # records of the copies per level-1 digit (4 bits) inside one workgroup batch of 16 x 63 words
    start, cnt = sc.exact()
    first_copy = int(o[13 + 1 + 285])
    in_batch = start[(start >= first_copy) & (start < first_copy + S.WAVES * batch - 150)]
    d1 = (T.R.remix32(sc.mh[in_batch]) >> np.uint64(28)).astype(np.int64)
    assert np.bincount(d1, minlength=16).max() > 4 * 16 * 3


@gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("tail", TAILS)
def test_records_at_the_edges(gpu_ctx, k, tail):
    inp = inp_of(k, tail)
    for G in (1, 3):
        def plan(one_pass):
            def f(slices):
                T.levels(2, one_pass=one_pass, fast=True)(slices)
                assert slices[0]["G"] == G, T.describe(slices[0])
                assert slices[0]["wpb"] > 3 * S.WAVE_WORDS                  # the long read's three batches belong to the first workgroup
            return f
        T.run(gpu_ctx, k, inp, "exact", f"k = {k}, tail {tail}, G = {G}, exact", plan=plan(False), skm_dyn=0, l1_bits=4, l2_bits=4, l1_blocks=G)
        T.run(gpu_ctx, k, inp, "one-pass", f"k = {k}, tail {tail}, G = {G}, one-pass", plan=plan(True), skm_dyn=2, l1_bits=4, l2_bits=4, l1_blocks=G)
