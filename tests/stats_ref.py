"""Independent restatement of stats-kmers (src/tools/StatsKmersFinder.java:89-316, commons-math3 3.6.1 MannWhitneyUTest) and
kmers-samples-counter (src/tools/KmersSamplesCounter.java:69-140) in numpy, written from the Java; it shares no code with the library.

A sample is given as its .kmers.bin records: (keys uint64[n], counts int16[n]), duplicates allowed.  Outputs are (keys, values) in
ascending key order, values as the uint16 bit patterns the files hold."""
import math

import numpy as np

F32 = np.float32
MAX_COUNT = 32767


def records_from_bytes(raw):
    a = np.frombuffer(raw, dtype=np.dtype([("k", ">u8"), ("c", ">i2")]))
    return a["k"].astype(np.uint64), a["c"].astype(np.int16)


def records_to_bytes(keys, vals):
    a = np.empty(len(keys), dtype=np.dtype([("k", ">u8"), ("c", ">u2")]))
    a["k"] = keys
    a["c"] = np.asarray(vals).astype(np.int64) & 0xFFFF
    return a.tobytes()


def stat_txt(values):
    """the project's .stat.txt: distinct k-mers per value"""
    vals, cnt = np.unique(np.asarray(values, dtype=np.int64), return_counts=True)
    return "# k-mer frequency\tnumber of such k-mers\n" + "".join("%d\t%d\n" % (v, c) for v, c in zip(vals, cnt)) + "\n"


def present_keys(sample, b):
    """loadKmers([file], b) / loadBitShortaKmers: the keys with some record > b"""
    k, c = sample
    return np.unique(k[c.astype(np.int64) > b])


def load_freq(sample):
    """IOUtils.loadKmersFreq(file, 0): (unique keys, saturating sums of the records > 0, sum of those records)"""
    k, c = sample
    c = c.astype(np.int64)
    m = c > 0
    uk, inv = np.unique(k[m], return_inverse=True)
    s = np.zeros(len(uk), dtype=np.int64)
    np.add.at(s, inv, c[m])
    return uk, np.minimum(s, MAX_COUNT), int(c[m].sum())


# ---- chi-squared (StatsKmersFinder.chisq :300-316): float arithmetic, then double ----
def chisq_kk(n0a, n1a, n0b, n1b):
    """kk for arrays of counts (float32 operations in the Java order, then float64)"""
    with np.errstate(all="ignore"):
        c0, c1, p0, p1 = (np.asarray(x, dtype=F32) for x in (n0a, n1a, n0b, n1b))
        tmp = c0
        c0 = F32(100) * c0 / (c0 + c1)
        c1 = F32(100) * c1 / (tmp + c1)
        tmp = p0
        p0 = F32(100) * p0 / (p0 + p1)
        p1 = F32(100) * p1 / (tmp + p1)
        gr_1 = c0 + c1
        gr_2 = p0 + p1
        al = gr_1 + gr_2
        x1 = gr_1 / al * (p1 + c1)
        x2 = gr_1 / al * (p0 + c0)
        x3 = gr_2 / al * (p1 + c1)
        x4 = gr_2 / al * (p0 + c0)

        def term(a, x):
            d = np.abs(a - x).astype(np.float64) - 0.5
            return (d * d) / x.astype(np.float64)
        return ((term(p1, x1) + term(p0, x2)) + term(c1, x3)) + term(c0, x4)


def chi2_quantile(p_chi2):
    """ChiSquaredDistribution(1).inverseCumulativeProbability(1 - p): P(X > q) = erfc(sqrt(q / 2)), by bisection"""
    P = 1.0 - p_chi2
    if P >= 1.0:
        return math.inf
    if P <= 0.0:
        return 0.0
    tail = 1.0 - P
    lo, hi = 0.0, 1.0
    while math.erfc(math.sqrt(hi / 2)) > tail:
        hi *= 2
    for _ in range(300):
        mid = (lo + hi) / 2
        if mid <= lo or mid >= hi:
            break
        if math.erfc(math.sqrt(mid / 2)) > tail:
            lo = mid
        else:
            hi = mid
    return hi


# ---- Mann-Whitney (commons-math3 3.6.1) ----
def ranks_fixed_average(x):
    """NaturalRanking(NaNStrategy.FIXED, TiesStrategy.AVERAGE): NaN ranks stay NaN, the others are ranked among themselves"""
    x = np.asarray(x, dtype=np.float64)
    r = np.full(len(x), np.nan)
    ok = ~np.isnan(x)
    v = x[ok]
    order = np.argsort(v, kind="stable")
    rk = np.empty(len(v))
    i = 0
    while i < len(v):
        j = i
        while j + 1 < len(v) and v[order[j + 1]] == v[order[i]]:
            j += 1
        rk[order[i:j + 1]] = (i + 1 + j + 1) / 2.0
        i = j + 1
    r[ok] = rk
    return r


def mw_pvalue_from_umin(umin, n1, n2):
    prod = n1 * n2
    EU = prod / 2.0
    VarU = (prod * (n1 + n2 + 1)) / 12.0
    z = (umin - EU) / math.sqrt(VarU)
    if math.isnan(z):
        return math.nan
    cdf = (0.0 if z < 0 else 1.0) if abs(z) > 40 else 0.5 * math.erfc(-z / math.sqrt(2.0))
    return 2 * cdf


def mw_test(x, y):
    """mannWhitneyUTest(x, y) through ranks"""
    r = ranks_fixed_average(np.concatenate([x, y]))
    u1 = r[: len(x)].sum() - len(x) * (len(x) + 1) // 2
    u2 = len(x) * len(y) - u1
    umax = u1 if math.isnan(u1) else max(u1, u2)
    return mw_pvalue_from_umin(len(x) * len(y) - umax, len(x), len(y))


def mw_twice_u1(va, vb):
    """2 * U1 per row by pairs: 2 [a > b] + [a == b] (rows x nA, rows x nB)"""
    return (2 * (va[:, :, None] > vb[:, None, :]) + (va[:, :, None] == vb[:, None, :])).sum(axis=(1, 2))


def java_short_of_int(x):
    """(short)(int)x as the uint16 bit pattern"""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros(x.shape, dtype=np.int64)
    ok = ~np.isnan(x)
    out[ok] = np.trunc(np.clip(x[ok], -2147483648.0, 2147483647.0)).astype(np.int64)
    return (out & 0xFFFF).astype(np.uint16)


def stats_kmers(a_samples, b_samples, b=0, p_chi2=0.05, p_mw=0.05, F_override=None):
    """-> dict(chi=(keys, vals), A=(keys, vals), B=(keys, vals), counters=dict); F_override: the samples' F_j when the records given are
    a subset of each sample's"""
    na, nb = len(a_samples), len(b_samples)
    N = na + nb
    samples = list(a_samples) + list(b_samples)
    pres = [present_keys(s, b) for s in samples]
    union = np.unique(np.concatenate(pres)) if N else np.zeros(0, np.uint64)
    n1 = np.zeros((len(union), 2), dtype=np.int64)
    for j, p in enumerate(pres):
        n1[np.searchsorted(union, p), 0 if j < na else 1] += 1
    n1a, n1b = n1[:, 0], n1[:, 1]
    tot = n1a + n1b
    scarce = tot <= math.ceil(N * 0.05)
    inall = ~scarce & (tot == N)
    rest = ~scarce & ~inall
    unique = rest & ((n1a == 0) | (n1b == 0))
    q = chi2_quantile(p_chi2)
    kk = chisq_kk(na - n1a, n1a, nb - n1b, n1b)
    with np.errstate(invalid="ignore"):
        chi_ok = rest & (q < kk)
    surv = union[chi_ok]
    # pass 2
    C = np.zeros((len(surv), N), dtype=np.float64)
    F = np.zeros(N, dtype=np.int64)
    for j, s in enumerate(samples):
        uk, uc, F[j] = load_freq(s)
        pos = np.searchsorted(uk, surv)
        hit = pos < len(uk)
        hit[hit] = uk[pos[hit]] == surv[hit]
        C[hit, j] = uc[pos[hit]]
    if F_override is not None:
        F = np.asarray(F_override, dtype=np.int64)
    M = float(int(F.sum())) / N
    with np.errstate(all="ignore"):
        V = (C * M) / F.astype(np.float64)[None, :]
    va, vb = V[:, :na], V[:, na:]
    if p_mw > 0:
        u1x2 = mw_twice_u1(va, vb)
        p = np.array([mw_pvalue_from_umin(min(u, 2 * na * nb - u) / 2.0, na, nb) for u in u1x2])
        p[np.isnan(va).any(axis=1)] = np.nan
        with np.errstate(invalid="ignore"):
            keep = p < p_mw
    else:
        keep = np.ones(len(surv), dtype=bool)
    sa = np.zeros(len(surv))
    for j in range(na):
        sa = sa + va[:, j]
    sb = np.zeros(len(surv))
    for j in range(nb):
        sb = sb + vb[:, j]
    with np.errstate(invalid="ignore"):
        meanA, meanB = sa / na, sb / nb
        toA = keep & (meanA > meanB)
    toB = keep & ~toA
    ul = keep & ((meanA == 0) | (meanB == 0))
    ctr = dict(n=len(union), scarce=int(scarce.sum()), in_all=int(inall.sum()), unique=int(unique.sum()),
               chi2_rejected=int((rest & ~chi_ok).sum()), mw_rejected=int((~keep).sum()), group_a=int(toA.sum()), group_b=int(toB.sum()),
               unique_left=int(ul.sum()))
    return dict(chi=(surv, np.ones(len(surv), dtype=np.uint16)), A=(surv[toA], java_short_of_int(meanA[toA])),
                B=(surv[toB], java_short_of_int(meanB[toB])), counters=ctr, q=q, kk=kk[rest], p=(p if p_mw > 0 else None))


def kmers_samples_count(samples, b=1):
    """-> (keys, n) for every key with n > 0"""
    pres = [present_keys(s, b) for s in samples]
    if not pres:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint16)
    allk = np.concatenate(pres)
    keys, n = np.unique(allk, return_counts=True)
    return keys, n.astype(np.uint16)
