"""Independent restatement of stats-kmers-3 (src/tools/StatsKmers3GroupsFinder.java:92-377, commons-math3 MannWhitneyUTest) and
kmers-grouped-counter (src/tools/KmersGroupedSamplesCounter.java:82-190) in numpy, written from the Java; it shares no code with the
library.  Samples, outputs and the helpers for records are those of tests/stats_ref.py."""
import math

import numpy as np

from stats_ref import java_short_of_int, load_freq, mw_pvalue_from_umin, mw_twice_u1, present_keys, records_to_bytes  # noqa: F401

F32 = np.float32
COUNTERS = ("n", "scarce", "in_all", "unique", "chi2_rejected", "mw_rejected", "group_a", "group_b", "group_c", "unique_left")


# ---- chi-squared (StatsKmers3GroupsFinder.chisq :346-369): float arithmetic, then double ----
def chisq3_stat(n0a, n1a, n0b, n1b, n0c, n1c):
    """stat for arrays of counts (c = A, p = B, q = C; float32 operations in the Java order, then float64)"""
    with np.errstate(all="ignore"):
        c0, c1, p0, p1, q0, q1 = (np.asarray(x, dtype=F32) for x in (n0a, n1a, n0b, n1b, n0c, n1c))
        tmp = c0
        c0 = F32(100) * c0 / (c0 + c1)
        c1 = F32(100) * c1 / (tmp + c1)
        tmp = p0
        p0 = F32(100) * p0 / (p0 + p1)
        p1 = F32(100) * p1 / (tmp + p1)
        tmp = q0
        q0 = F32(100) * q0 / (q0 + q1)
        q1 = F32(100) * q1 / (tmp + q1)
        gr_1 = c0 + c1
        gr_2 = p0 + p1
        gr_3 = q0 + q1
        al = gr_1 + gr_2 + gr_3
        ones = p1 + c1 + q1
        zeros = p0 + c0 + q0
        x1 = gr_1 / al * ones
        x2 = gr_1 / al * zeros
        x3 = gr_2 / al * ones
        x4 = gr_2 / al * zeros
        x5 = gr_3 / al * ones
        x6 = gr_3 / al * zeros

        def term(a, x):
            d = np.abs(a - x).astype(np.float64) - 0.5
            return (d * d) / x.astype(np.float64)
        return ((((term(p1, x1) + term(p0, x2)) + term(c1, x3)) + term(c0, x4)) + term(q1, x5)) + term(q0, x6)


def chi2_2_quantile(p_chi2):
    """ChiSquaredDistribution(2).inverseCumulativeProbability(1 - p): P(X > q) = exp(-q / 2)"""
    if p_chi2 <= 0.0:
        return math.inf
    if p_chi2 >= 1.0:
        return 0.0
    return -2.0 * math.log(p_chi2)


def pair_pvalues(vx, vy):
    """mannWhitneyUTest(x, y) per row: NaN when x holds a NaN (its rank sum is NaN), a NaN of y ranks nowhere"""
    nx, ny = vx.shape[1], vy.shape[1]
    u2 = mw_twice_u1(vx, vy)
    by_u2 = np.array([mw_pvalue_from_umin(min(u, 2 * nx * ny - u) / 2.0, nx, ny) for u in range(2 * nx * ny + 1)], dtype=np.float64)
    p = by_u2[u2]
    p[np.isnan(vx).any(axis=1)] = np.nan
    return p


def _mean(v):
    s = np.zeros(v.shape[0])
    for j in range(v.shape[1]):
        s = s + v[:, j]
    with np.errstate(invalid="ignore"):
        return s / v.shape[1]


def decide_rows(V, na, nb, nc, p_mw):
    """rows of v_j -> (keep, group 0 / 1 / 2, value, unique-left, the three p-values or None) (:273-311)"""
    va, vb, vc = V[:, :na], V[:, na:na + nb], V[:, na + nb:]
    ps = None
    if p_mw > 0:
        ps = np.stack([pair_pvalues(va, vb), pair_pvalues(vb, vc), pair_pvalues(va, vc)], axis=1) if len(V) else np.zeros((0, 3))
        with np.errstate(invalid="ignore"):
            keep = (ps < p_mw).any(axis=1)
    else:
        keep = np.ones(len(V), dtype=bool)
    mA, mB, mC = _mean(va), _mean(vb), _mean(vc)
    with np.errstate(invalid="ignore"):
        toA = (mA > mB) & (mA > mC)
        toB = ~toA & (mB > mA) & (mB > mC)
        ul = ((mA + mB) == 0) | ((mA + mC) == 0) | ((mB + mC) == 0)
    grp = np.where(toA, 0, np.where(toB, 1, 2))
    val = java_short_of_int(np.where(toA, mA, np.where(toB, mB, mC)))
    return keep, grp, val, ul, ps


def stats_kmers3(a_samples, b_samples, c_samples, b=0, p_chi2=0.05, p_mw=0.05):
    """-> dict(chi, A, B, C: (keys, vals); counters; q; kk: the statistic of every k-mer that reached the test; p: the p-values)"""
    na, nb, nc = len(a_samples), len(b_samples), len(c_samples)
    N = na + nb + nc
    samples = list(a_samples) + list(b_samples) + list(c_samples)
    pres = [present_keys(s, b) for s in samples]
    union = np.unique(np.concatenate(pres))
    n1 = np.zeros((len(union), 3), dtype=np.int64)
    for j, p in enumerate(pres):
        n1[np.searchsorted(union, p), 0 if j < na else 1 if j < na + nb else 2] += 1
    n1a, n1b, n1c = n1[:, 0], n1[:, 1], n1[:, 2]
    tot = n1a + n1b + n1c
    scarce = tot <= math.ceil(N * 0.05)
    inall = ~scarce & (tot == N)
    rest = ~scarce & ~inall
    unique = rest & (((n1a + n1c) == 0) | ((n1b + n1a) == 0) | ((n1b + n1c) == 0))
    q = chi2_2_quantile(p_chi2)
    kk = chisq3_stat(na - n1a, n1a, nb - n1b, n1b, nc - n1c, n1c)
    with np.errstate(invalid="ignore"):
        chi_ok = rest & (q < kk)
    surv = union[chi_ok]
    C = np.zeros((len(surv), N), dtype=np.float64)
    F = np.zeros(N, dtype=np.int64)
    for j, s in enumerate(samples):
        uk, uc, F[j] = load_freq(s)
        pos = np.searchsorted(uk, surv)
        hit = pos < len(uk)
        hit[hit] = uk[pos[hit]] == surv[hit]
        C[hit, j] = uc[pos[hit]]
    M = float(int(F.sum())) / N
    with np.errstate(all="ignore"):
        V = (C * M) / F.astype(np.float64)[None, :]
    keep, grp, val, ul, ps = decide_rows(V, na, nb, nc, p_mw)
    sel = [keep & (grp == g) for g in range(3)]
    ctr = dict(n=len(union), scarce=int(scarce.sum()), in_all=int(inall.sum()), unique=int(unique.sum()),
               chi2_rejected=int((rest & ~chi_ok).sum()), mw_rejected=int((~keep).sum()), group_a=int(sel[0].sum()), group_b=int(sel[1].sum()),
               group_c=int(sel[2].sum()), unique_left=int((keep & ul).sum()))
    out = dict(chi=(surv, np.ones(len(surv), dtype=np.uint16)), counters=ctr, q=q, kk=kk[rest], p=ps)
    for g, name in enumerate("ABC"):
        out[name] = (surv[sel[g]], val[sel[g]])
    return out


def check_identities(c, n_chi):
    """the reference's two consistency checks (:173, :324)"""
    assert n_chi == c["n"] - c["in_all"] - c["scarce"] - c["chi2_rejected"], c
    assert c["group_a"] + c["group_b"] + c["group_c"] == c["n"] - c["in_all"] - c["scarce"] - c["chi2_rejected"] - c["mw_rejected"], c


# ---- kmers-grouped-counter ----
def kmers_grouped_count(kf_samples, cd, uc, nonibd, b=1):
    """-> (keys ascending, int64[n][3]): the k-mers of -kf with some record > 0, and per group the files that hold each with a record > b"""
    keys = np.unique(np.concatenate([present_keys(s, 0) for s in kf_samples])) if kf_samples else np.zeros(0, np.uint64)
    out = np.zeros((len(keys), 3), dtype=np.int64)
    for g, group in enumerate((cd, uc, nonibd)):
        for s in group:
            out[:, g] += np.isin(keys, present_keys(s, b))
    return keys, out


def kmer_text(key, k):
    """ShortKmer.toString: two bits a base, the first base in the highest bits, A G C T = 0 1 2 3"""
    return "".join("AGCT"[(int(key) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def groups_txt(keys, counts, k):
    return "Kmer\tcd_count\tuc_count\tnonibd_count\n" + "".join("%s\t%d\t%d\t%d\n" % (kmer_text(x, k), c[0], c[1], c[2]) for x, c in zip(keys, counts))
