"""The inputs of tests/test_wseq2comp_gpu.py with their references (tests/wseq2comp_ref.py), built once per process.  The CPU test
(tests/test_wseq2comp_cpu.py) asserts on the references alone the conditions the GPU cases rely on."""
import functools
import os
import re

import numpy as np

import wide_files_ref as WF
import wseq2comp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (32, 33, 47, 63)


def lds_max_in_source():
    """WS2C_T as the device code defines it (on the GPU: ctx.stat("ws2c_lds_max"))"""
    text = open(os.path.join(ROOT, "metafast_amd", "csrc", "mf_wseq2comp.hip")).read()
    return int(re.search(r"^#define WS2C_T (\d+)", text, re.M).group(1))


def rnd(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


@functools.lru_cache(maxsize=None)
def edges(k):
    rng = np.random.default_rng(2000 + k)
    s, twice, w = rnd(rng, 100), rnd(rng, 120), rnd(rng, (k + 1) // 2)
    pal = w + R.rc_str(w)                                  # an even-length palindrome: of length k where k is even, k + 1 where it is odd
    assert R.rc_str(pal) == pal and len(pal) in (k, k + 1)
    seqs = ["", rnd(rng, k - 1), rnd(rng, k), rnd(rng, k + 1), "A" * (k + 5), "T" * (k + 20), ("ACG" * 167)[:500], s + R.rc_str(s), twice, twice,
            rnd(rng, 7) + pal + rnd(rng, 9), pal, rnd(rng, 300).lower()]
    return seqs, R.components(seqs, k)


@functools.lru_cache(maxsize=None)
def both_words(k):
    """"A" + S and "G" + S (the same low word, another high word for k >= 33), P + "A" and P + "G" (the other way round), and both pairs in
    one sequence; every one of the four k-mers is its own canonical form"""
    rng = np.random.default_rng(3000 + k)
    S = rnd(rng, k - 2) + "A"                              # ends in A: the reverse complement starts with T, above A... and G...
    P = "A" + rnd(rng, k - 2)                              # starts with A: the reverse complements start with T (P + A) and C (P + G)
    seqs = ["A" + S + "G" + S, P + "A" + P + "G", "A" + S + "G" + S + P + "A" + P + "G"]
    return seqs, R.components(seqs, k), (R.encode("A" + S), R.encode("G" + S), R.encode(P + "A"), R.encode(P + "G"))


@functools.lru_cache(maxsize=None)
def borders(T):
    k = 33
    rng = np.random.default_rng(T)
    unit50 = rnd(rng, 50)
    seqs = []
    for n in (T // 4 - 1, T // 4, T // 4 + 1, T - 1, T, T + 1, 2 * T):      # occurrences: the wave / workgroup / sort classes, on both sides
        seqs.append(rnd(rng, n + k - 1))
        seqs.append((unit50 * (n // 50 + 3))[: n + k - 1])
    seqs.append(rnd(rng, 20000))
    return k, seqs, R.components(seqs, k)


@functools.lru_cache(maxsize=None)
def many():
    k = 63
    rng = np.random.default_rng(63000)
    lens = rng.integers(33, 401, 2500)
    for at in (0, 1200, 2499):
        lens[at] = 6000 + at % 7
    pool = rnd(rng, int(lens.sum()))
    ends = np.cumsum(lens)
    seqs = [pool[int(e - n): int(e)] for e, n in zip(ends, lens)]
    return k, seqs, R.components(seqs, k)


@functools.lru_cache(maxsize=None)
def roundtrip():
    k = 33
    rng = np.random.default_rng(33200)
    seqs = [rnd(rng, 200) for _ in range(40)]
    return k, seqs, R.components(seqs, k)


def canon(x, k):
    return min(x, WF.revcomp(x, k))


def sample_of(comps, k, rng):
    """a sample that holds about a third of the members (counts 1 .. 9) and 40 canonical k-mers of its own"""
    members = sorted({x for c in comps for x in c[0]})
    sample = {x: int(v) for x, v in zip(members, rng.integers(1, 10, len(members))) if rng.random() < 0.33}
    for _ in range(40):
        x = canon(int.from_bytes(rng.bytes(16), "big") & ((1 << (2 * k)) - 1), k)
        sample.setdefault(x, 5)
    return sample
