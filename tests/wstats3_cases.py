"""The cohorts of the wide stats-kmers-3 / kmers-grouped-counter tests (tests/test_wstats3_cpu.py checks on the reference that the crafted one
meets every rule it is made for; tests/test_wstats3_gpu.py runs the library on them).

crafted(k): three samples in each of A, B and C at max_bad = 2, p_chi2 = 0.05, p_mw = 0.05.  With N = 9 a k-mer that at most ceil(0.45) = 1
sample holds is scarce; the chi-squared statistic of 3 x 3 x 3 is 0.034 where the three groups hold a k-mer equally often and above 40 everywhere
else (q = 5.99); Mann-Whitney at 3 x 3 keeps a pair with 2 Umin = 0 (p = 0.0495) and rejects one with 2 Umin >= 1 (p = 0.081)."""
import numpy as np

import wkmersets_cases as WC
import wstats_cases as W2

MAX_BAD = 2
P_CHI2, P_MW = 0.05, 0.05
NA = NB = NC = 3
slice_of = W2.slice_of
border_keys = W2.border_keys


def crafted(k, empty=None):
    """-> (A samples, B samples, C samples, names: the k-mers by what they are there for).  empty = "A" / "B" / "C": one more, empty sample at the
    end of that group (N = 10: scarce is still at most one sample)"""
    rng = np.random.default_rng(7300 + k)
    b = MAX_BAD
    groups = [[dict() for _ in range(n)] for n in (NA, NB, NC)]
    S = groups[0] + groups[1] + groups[2]
    names = {}

    def put(name, x, counts):
        """counts: one per sample, 0 = absent"""
        assert len(counts) == NA + NB + NC and x not in names.values()
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
    f = W2._fresh(rng, k, 12, taken)
    big = 32767
    # scarce: one sample holds it; a second one has it, but at max_bad
    put("scarce", f[0], [b + 1, 0, 0, b, 0, 0, 0, 0, 0])
    put("scarce_smallest", 0, [0, 0, 0, 0, 0, 0, 0, 77, 0])
    # in all
    put("in_all", f[1], [b + 1, 3, 3, 4, 5, 6, 7, 8, 9])
    put("in_all_largest", top, [3] * 9)
    # held by one group only and kept by both tests: every holder above every sample of the other groups (2 Umin = 0)
    put("only_a", f[2], [3, 4, 5, 0, 0, 0, 0, 0, 0])
    put("only_b", f[3], [0, 0, 0, 30, 40, 50, 0, 0, 0])
    put("only_c", f[4], [0, 0, 0, 0, 0, 0, 300, 400, 500])
    # chi-squared rejected: one holder in every group
    put("chi_rejected", lo_x, [5, 0, 0, 0, 9, 0, 0, 0, 7])
    # chi-squared kept (3 : 3 : 1), Mann-Whitney rejected: no pair of groups is cleanly apart
    put("mw_rejected", lo_y, [5, 50, 500, 6, 60, 600, 55, 0, 0])
    # group A, B, C: the group above both others, every pair with it cleanly apart
    put("group_a", hi_x, [100, 200, 300, 3, 0, 0, 0, 4, 0])
    put("group_b", f[5], [3, 0, 0, 100, 200, 300, 0, 0, 4])
    put("group_c", f[6], [0, 4, 0, 0, 0, 3, 100, 200, 300])
    # tied means of B and C (their samples have the same F_j) above A's: B's mean is not greater than C's, so the row goes to C ((A, B) is
    # cleanly apart: kept at either p_mw)
    put("tie", hi_y, [4, 0, 0, 8, 8, 8, 8, 8, 8])
    # a mean that truncates to 0: the two holders are the samples with F_j = 64000, v = 3 * 17333.3 / 64000 = 0.81, mean 0.54 (kept at p_mw = 0)
    put("mean_zero", f[7], [0, 3, 3, 0, 0, 0, 0, 0, 0])
    # ... and counts of 32767 in a row that is kept (at p_mw = 0)
    put("big_counts", f[8], [0, big, 20000, 0, 0, 0, 0, 0, 0])
    # presence is cut at max_bad, the gathered counts are not: no sample of A or B holds it, yet their counts of 1 and max_bad reach the row --
    # the means of A and B are not 0 and the row is not "unique left"
    put("low_counts", f[9], [1, b, 1, b, 1, b, 300, 300, 300])
    # the keys at the slice borders of S = 3 and 7: rows of group A, B and C in turn
    for i, x in enumerate(borders):
        c = [7 + i, 8 + i, 9 + i]
        put("border%d" % i, x, [0] * (3 * (i % 3)) + c + [0] * (6 - 3 * (i % 3)))
    # every sample is filled up to F_j = 4000 by one private k-mer (scarce, like every private k-mer), samples 1 and 2 to 64000 by two
    pad = W2._fresh(rng, k, 2 * len(S), taken)
    for j, t in enumerate(S):
        rest = (64000 if j in (1, 2) else 4000) - sum(t.values())
        assert b < rest <= 2 * big and (rest <= big or rest - big > b), (j, rest)
        t[pad[2 * j]] = min(rest, big)
        if rest > big:
            t[pad[2 * j + 1]] = rest - big
    if empty:
        groups["ABC".index(empty)].append({})
    names["borders"] = borders
    return groups[0], groups[1], groups[2], names


def random_cohort(k, na, nb, nc, n_kmers=300, base=5, seed=0, max_bad=MAX_BAD):
    """`base` distinct samples per group (fewer where the group is smaller), repeated to fill the groups: a k-mer leans to A, to B, to C, to
    none, or is rare; counts of 1, max_bad, max_bad + 1 and 32767 among them.  -> (A samples, B samples, C samples)"""
    rng = np.random.default_rng(9300 + 131 * k + 7 * na + 3 * nb + nc + seed)
    keys = W2._fresh(rng, k, n_kmers, set())
    counts = np.array([1, max_bad, max_bad + 1, 5, 17, 250, 4000, 32767])
    lean = rng.integers(0, 5, n_kmers)                      # 0 A, 1 B, 2 C, 3 none, 4 rare
    out = []
    for g, n in enumerate((na, nb, nc)):
        p = np.where(lean == g, 0.9, np.where(lean == 3, 0.6, np.where(lean == 4, 0.06, 0.15)))
        base_samples = []
        for _ in range(min(base, n)):
            has = rng.random(n_kmers) < p
            c = rng.choice(counts, n_kmers, p=[0.1, 0.1, 0.15, 0.2, 0.2, 0.15, 0.07, 0.03])
            c = np.where(lean == g, np.maximum(c, 5) * 3 % 32768, c)        # the group a k-mer leans to holds it with larger counts
            base_samples.append({keys[i]: int(max(c[i], 1)) for i in range(n_kmers) if has[i]})
        out.append([base_samples[j % len(base_samples)] for j in range(n)])
    return out[0], out[1], out[2]


def grouped_case(k):
    """kmers-grouped-counter: -> (kf samples, cd, uc, nonibd).  The -kf k-mers: some in no group, some in one group only, the keys on both
    sides of every slice border of S = 3 and 7, the ends of the key range; counts of max_bad = 1 that are a presence at max_bad = 0 only; a -kf
    k-mer listed in both -kf files; group k-mers that -kf does not ask for"""
    rng = np.random.default_rng(7700 + k)
    borders = sorted(set(border_keys(k, 3) + border_keys(k, 7)))
    top = WC.largest_canonical(k)
    taken = set(borders) | {0, top}
    f = W2._fresh(rng, k, 16, taken)
    asked = [0, top] + borders + f[:10]
    kf = [{x: 1 + i % 3 for i, x in enumerate(asked[::2] + [f[0]])}, {x: 5 for x in asked[1::2] + [f[0]]}]
    nowhere, cd_only, uc_only, ni_only = f[0:2], f[2:4], f[4:6], f[6:8]
    cd = [{}, {}, {}]
    uc = [{}, {}]
    ni = [{}, {}, {}, {}]
    for x in cd_only:
        cd[0][x] = 2; cd[2][x] = 1                      # (held once at max_bad = 1, twice at 0)
    for x in uc_only:
        uc[1][x] = 32767
    for x in ni_only:
        for t in ni:
            t[x] = 2
    for i, x in enumerate([0, top] + borders + f[8:10]):
        for g, grp in enumerate((cd, uc, ni)):
            for j, t in enumerate(grp):
                if (i + g + j) % 3:
                    t[x] = 1 + (i + j) % 3
    for j, t in enumerate(cd + uc + ni):                # k-mers that nobody asks for
        t[f[10 + j % 6]] = 9
    assert not any(x in t for x in nowhere for t in cd + uc + ni)
    return kf, cd, uc, ni


# (nA, nB, nC, p_chi2, p_mw) of every library run of tests/test_wstats3_gpu.py: tests/test_wstats3_cpu.py holds the margin guard over them.
# (12, 12, 12) and (3, 3, 3) at 0.05, 0.05 are the narrow tool's runs there.  p_chi2 = 0: the quantile is infinite and no k-mer survives the chi-squared test (m = 0 rows in every slice)
RANDOM_SHAPES = [(1, 1, 1), (11, 11, 10), (11, 11, 11), (24, 23, 23)]    # N = 3; 32: the last thread-per-row shape; 33: the first wave-per-row shape; 70: lanes loop twice
RANDOM_PS = [(0.05, 0.05), (0.05, 0.0), (0.0, 0.05)]
GPU_SHAPES = ([(na, nb, nc, P_CHI2, pm) for na, nb, nc in ((3, 3, 3), (4, 3, 3), (3, 4, 3), (3, 3, 4)) for pm in (P_MW, 0.0)] +
              [(12, 12, 12, 0.05, 0.05)] + [(na, nb, nc, pc, pm) for na, nb, nc in RANDOM_SHAPES for pc, pm in RANDOM_PS])
