"""The crafted cohort of the wide kmers-per-sample tests: the six tables of tests/wkmersets_cases.py (four inputs, the last one empty, and two
filters) taken as six samples, and the few k-mers the tool's own rules still need (tests/test_wkps_cpu.py checks on the reference that the
cohort meets them; tests/test_wkps_gpu.py runs the library on it)."""
import numpy as np

import wkmersets_cases as CASES
import wkmersets_ref as WR


def cohort(k):
    """-> (six samples as {kmer: count}, the added k-mers by what they are there for).  At percent 50 of six samples thresh is 3"""
    ins, flt, names = CASES.crafted(k)
    samples = [dict(t) for t in ins + flt]
    assert samples[3] == {}
    rng = np.random.default_rng(5000 + k)
    mask = (1 << (2 * k)) - 1
    taken = set().union(*samples)
    fresh = []
    while len(fresh) < 4:
        x = WR.canonical(int.from_bytes(rng.bytes(16), "big") & mask, k)
        if x not in taken:
            taken.add(x)
            fresh.append(x)
    only0, below, at, only_last = fresh
    samples[0][only0] = 123                            # sample 0 alone: a candidate with n = 0 (n = 1 when the first sample is counted)
    for j, c in ((1, 100), (2, 999)):                  # n = 2 = thresh - 1
        samples[j][below] = c
    for j, c in ((1, 1000), (2, 9999), (4, 10000)):    # n = 3 = thresh
        samples[j][at] = c
    samples[5][only_last] = 4567
    names = dict(names, only0=only0, below=below, at=at, only_last=only_last)
    return samples, names
