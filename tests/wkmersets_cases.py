"""The crafted cohort of the wide set tools' tests: a few dozen canonical k-mers per k that meet every rule of unique-kmers-multi's definition
(tests/test_wkmersets_cpu.py checks on the reference that they do; tests/test_wkmersets_gpu.py runs the library on them)."""
import numpy as np

import wfeatures_ref as FR
import wkmersets_ref as R

B = 1          # the threshold the case is made for


def largest_canonical(k):
    """T..T A..A (an odd k: G in the middle).  A canonical k-mer that starts with h T's ends with h A's (its reverse complement starts with the
    complements of its last bases), and the middle base of an odd k is at most its own complement: A or G"""
    h = k // 2
    return FR.encode("T" * h + ("G" if k % 2 else "") + "A" * h)


def _pair(rng, k, bit):
    """two canonical k-mers that differ in one bit"""
    mask = (1 << (2 * k)) - 1
    while True:
        x = int.from_bytes(rng.bytes(16), "big") & mask
        y = x ^ (1 << bit)
        if x == R.canonical(x, k) and y == R.canonical(y, k):
            return x, y


def crafted(k):
    """-> (inputs, filters, names): four inputs (the last one empty), two filters, and the k-mers by what they are there for"""
    rng = np.random.default_rng(k)
    mask = (1 << (2 * k)) - 1
    rnd = sorted({R.canonical(int.from_bytes(rng.bytes(16), "big") & mask, k) for _ in range(26)})
    rng.shuffle(rnd)
    everywhere, wrap, sat, at_b, above_b, f_small, f_only, f_hit = rnd[:8]
    top = largest_canonical(k)
    lo_x, lo_y = _pair(rng, k, 2)                                    # equal in hi, different in lo
    hi_x, hi_y = _pair(rng, k, 64) if k > 32 else _pair(rng, k, 63)  # equal in lo, different in hi (k = 32 has no high word)
    i0 = {0: 3, top: 2, hi_x: 2, lo_x: 4, everywhere: 5, wrap: 20000, sat: 32767, at_b: B, above_b: B + 1, f_small: 7, f_hit: 9}
    i1 = {0: 4, hi_y: 6, lo_y: 3, everywhere: 5, wrap: 20000, sat: 32767, f_hit: 2}
    i2 = {top: 9, everywhere: 5, wrap: 20000, hi_x: 1}
    for j, x in enumerate(rnd[8:]):
        (i0, i1, i2)[j % 3][x] = 2 + j
        if j % 4 == 0:
            (i1, i2, i0)[j % 3][x] = 3
    f0 = {everywhere: 2, f_small: 1, f_only: 30, hi_y: 1}
    f1 = {f_hit: 5, f_only: 2}
    names = dict(everywhere=everywhere, wrap=wrap, sat=sat, at_b=at_b, above_b=above_b, f_small=f_small, f_only=f_only, f_hit=f_hit, top=top,
                 lo_pair=(lo_x, lo_y), hi_pair=(hi_x, hi_y))
    return [i0, i1, i2, {}], [f0, f1], names
