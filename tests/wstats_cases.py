"""The cohorts of the wide stats-kmers tests (tests/test_wstats_cpu.py checks on the reference that the crafted one meets every rule it is
made for; tests/test_wstats_gpu.py runs the library on them).

crafted(k): four samples in A and four in B at max_bad = 2, p_chi2 = 0.3, p_mw = 0.05.  With N = 8 a k-mer that at most ceil(0.4) = 1 sample
holds is scarce; Mann-Whitney at 4 x 4 keeps a row with 2 Umin <= 2 (p = 0.021, 0.043) and rejects one with 2 Umin >= 4 (p = 0.083)."""
import numpy as np

import wkmersets_cases as WC
import wkmersets_ref as WR

MAX_BAD = 2
P_CHI2, P_MW = 0.3, 0.05
NA = NB = 4


def slice_of(x, k, S):
    """mf_wjoin_slice: the leading 24 bits of the 2k-bit k-mer scaled to [0, S)"""
    return ((x >> (2 * k - 24)) * S) >> 24


def border_keys(k, S):
    """for every border between two slices the largest leading-bits value of the lower slice and the smallest of the upper one, each with the
    rest of the k-mer all A (canonical: its reverse complement starts with T's) and with a G in front of the last A"""
    out = []
    for s in range(1, S):
        t = -((-s << 24) // S)                               # the smallest t with t * S >> 24 == s
        for top in (t - 1, t):
            for low in (0, 4):
                x = (top << (2 * k - 24)) | low
                assert x == WR.canonical(x, k) and slice_of(x, k, S) == (s - 1 if top < t else s)
                out.append(x)
    return out


def _fresh(rng, k, n, taken):
    mask = (1 << (2 * k)) - 1
    out = []
    while len(out) < n:
        x = WR.canonical(int.from_bytes(rng.bytes(16), "big") & mask, k)
        if x not in taken:
            taken.add(x)
            out.append(x)
    return out


def crafted(k, empty=None):
    """-> (A samples, B samples, names: the k-mers by what they are there for).  empty = "A" / "B": one more, empty sample at the end of that
    group (N = 9: scarce is still at most one sample)"""
    rng = np.random.default_rng(7000 + k)
    b = MAX_BAD
    A = [dict() for _ in range(NA)]
    B = [dict() for _ in range(NB)]
    S = A + B
    names = {}

    def put(name, x, counts):
        """counts: one per sample, 0 = absent"""
        assert len(counts) == NA + NB and x not in names.values()
        names[name] = x
        for t, c in zip(S, counts):
            if c:
                t[x] = c

    taken = set()
    top = WC.largest_canonical(k)
    lo_x, lo_y = WC._pair(rng, k, 2)                                       # equal in hi, different in lo
    hi_x, hi_y = WC._pair(rng, k, 64) if k > 32 else WC._pair(rng, k, 63)  # equal in lo, different in hi (k = 32 has no high word)
    borders = sorted(set(border_keys(k, 3) + border_keys(k, 7)))
    taken.update([0, top, lo_x, lo_y, hi_x, hi_y], borders)
    f = _fresh(rng, k, 12, taken)
    big = 32767
    # scarce: one sample holds it; a second one has it, but at max_bad
    put("scarce", f[0], [b + 1, 0, 0, 0, b, 0, 0, 0])
    put("scarce_smallest", 0, [0, 0, 0, 0, 0, 0, 77, 0])
    # in all
    put("in_all", f[1], [b + 1, 3, 3, 4, 5, 6, 7, 8])
    put("in_all_largest", top, [3] * 8)
    # unique on either side and kept by both tests: every holder above every sample of the other group (2 Umin = 0)
    put("unique_a", f[2], [3, 4, 5, 6, 0, 0, 0, 0])
    put("unique_b", f[3], [0, 0, 0, 0, 30, 40, 50, 60])
    # chi-squared rejected: as many holders on either side (at p_chi2 = 0.3 and 4 x 4 exactly these are)
    put("chi_rejected", lo_x, [5, 5, 0, 0, 0, 9, 9, 0])
    # chi-squared kept (4 : 1), Mann-Whitney rejected: B's one holder is the largest value of the row -> 2 Umin = 8
    put("mw_rejected", lo_y, [3, 3, 3, 3, 0, 0, 0, 2000])
    # group A: every A above every B (2 Umin = 0)
    put("group_a", hi_x, [100, 200, 300, 400, 3, 0, 0, 0])
    # tied means (v = 38, 38 against 76: both means 19): to B.  Mann-Whitney rejects the row (no 4 x 4 row with equal means has 2 Umin <= 2),
    # so the tie shows at p_mw = 0
    put("tie", hi_y, [8, 8, 0, 0, 16, 0, 0, 0])
    # a mean that truncates to 0: the two holders are the samples with F_j = 64000, v = 3 * 19000 / 64000 = 0.89, mean 0.45 (kept at p_mw = 0)
    put("mean_zero", f[6], [0, 0, 3, 3, 0, 0, 0, 0])
    # ... and counts of 32767 in a row that is kept (at p_mw = 0)
    put("big_counts", f[4], [0, 0, big, 20000, 0, 0, 0, 0])
    # presence is cut at max_bad, the gathered counts are not: no sample of A holds it, yet A's counts of 1 and max_bad reach the row -- the
    # mean of A is not 0 and the row is not "unique left"
    put("low_counts", f[7], [1, b, 1, b, 300, 300, 300, 300])
    # the keys at the slice borders of S = 3 and 7: rows of group A and of group B in turn
    for i, x in enumerate(borders):
        put("border%d" % i, x, [0, 0, 0, 0, 3 + i, 4 + i, 5 + i, 6 + i] if i % 2 else [7 + i, 8 + i, 9 + i, 10 + i, 0, 0, 0, 0])
    # every sample is filled up to F_j = 4000 by one private k-mer (scarce, like every private k-mer), samples 2 and 3 to 64000 by two: M = 19000
    # and v_j = c_j * 4.75 exactly, but for samples 2 and 3
    pad = _fresh(rng, k, 2 * (NA + NB), taken)
    for j, t in enumerate(S):
        rest = (64000 if j in (2, 3) else 4000) - sum(t.values())
        assert b < rest <= 2 * big and (rest <= big or rest - big > b), (j, rest)
        t[pad[2 * j]] = min(rest, big)
        if rest > big:
            t[pad[2 * j + 1]] = rest - big
    if empty == "A":
        A.append({})
    elif empty == "B":
        B.append({})
    names["borders"] = borders
    return A, B, names


def random_cohort(k, na, nb, n_kmers=300, base=5, seed=0, max_bad=MAX_BAD):
    """`base` distinct samples per group (fewer where the group is smaller), repeated to fill the groups: a k-mer leans to A, to B, to
    neither, or is rare; counts of 1, max_bad, max_bad + 1 and 32767 among them.  -> (A samples, B samples)"""
    rng = np.random.default_rng(9000 + 131 * k + 7 * na + nb + seed)
    keys = _fresh(rng, k, n_kmers, set())
    counts = np.array([1, max_bad, max_bad + 1, 5, 17, 250, 4000, 32767])
    ba, bb = min(base, na), min(base, nb)
    lean = rng.integers(0, 4, n_kmers)                      # 0 A, 1 B, 2 neither, 3 rare
    pa = np.array([0.9, 0.15, 0.6, 0.06])[lean]
    pb = np.array([0.15, 0.9, 0.6, 0.06])[lean]
    groups = []
    for n_base, p, hot in ((ba, pa, 0), (bb, pb, 1)):
        out = []
        for _ in range(n_base):
            has = rng.random(n_kmers) < p
            c = rng.choice(counts, n_kmers, p=[0.1, 0.1, 0.15, 0.2, 0.2, 0.15, 0.07, 0.03])
            c = np.where(lean == hot, np.maximum(c, 5) * 3 % 32768, c)      # the group a k-mer leans to holds it with larger counts
            out.append({keys[i]: int(max(c[i], 1)) for i in range(n_kmers) if has[i]})
        groups.append(out)
    A = [groups[0][j % ba] for j in range(na)]
    B = [groups[1][j % bb] for j in range(nb)]
    return A, B


# (nA, nB, p_chi2, p_mw) of every library run of tests/test_wstats_gpu.py: tests/test_wstats_cpu.py holds the margin guard over them.
# p_chi2 = 0: the quantile is infinite and no k-mer survives the chi-squared test (m = 0 rows in every slice)
RANDOM_SHAPES = [(1, 1), (16, 16), (16, 17), (35, 35)]     # N = 2; 32: the last shape of the thread-per-row kernel; 33: the first of the wave-per-row kernel; 70: a wave's lanes loop twice
RANDOM_PS = [(0.05, 0.05), (0.05, 0.0), (0.0, 0.05)]
GPU_SHAPES = ([(NA, NB, P_CHI2, P_MW), (NA, NB, P_CHI2, 0.0), (NA + 1, NB, P_CHI2, P_MW), (NA + 1, NB, P_CHI2, 0.0), (NA, NB + 1, P_CHI2, P_MW),
               (NA, NB + 1, P_CHI2, 0.0), (3, 3, 0.3, 0.0), (5, 5, 0.05, 0.05), (20, 20, 0.05, 0.05)] + [(na, nb, pc, pm) for na, nb in RANDOM_SHAPES for pc, pm in RANDOM_PS])
