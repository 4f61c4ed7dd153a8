"""Independent restatement of specific-kmers (src/tools/SpecificKmersFinder.java:65-245), specific-kmers-3
(src/tools/SpecificKmers3GroupsFinder.java:70-313) and unique-kmers (src/tools/UniqueKmersFinder.java:73-144) in numpy, written from the
Java and its loaders (IOUtils.loadKmers, Kmers2HMWorker.processKmer, BigLong2ShortHashMap.get / getWithZero / put / addAndBound); it shares
no code with the library.  Samples, outputs and the record helpers are those of tests/stats_ref.py; the statistics that the Java files
share word for word with the stats- tools (chisq, the Mann-Whitney p-value, the three-group choice) come from stats_ref / stats3_ref."""
import math

import numpy as np

import stats3_ref as R3
import stats_ref as R

COUNTERS = ("n", "unique", "scarce", "chi2_rejected", "mw_rejected", "unique_left", "group_a", "group_b")
COUNTERS3 = R3.COUNTERS
MAX_COUNT = 32767


def load_map(records, threshold):
    """IOUtils.loadKmers(files, threshold) of the concatenated records: a RECORD is added when its value is > threshold, values of one
    k-mer add up and stop at 32767 (addAndBound) -> (keys ascending, values)"""
    k, c = records
    c = np.asarray(c).astype(np.int64)
    m = c > threshold
    uk, inv = np.unique(np.asarray(k, dtype=np.uint64)[m], return_inverse=True)
    s = np.zeros(len(uk), dtype=np.int64)
    np.add.at(s, inv, c[m])
    return uk, np.minimum(s, MAX_COUNT)


def count_matrix(samples):
    """every sample loaded alone at threshold 0 -> (union keys ascending, int64 counts [n][N], 0 = absent)"""
    maps = [load_map(s, 0) for s in samples]
    union = np.unique(np.concatenate([m[0] for m in maps])) if maps else np.zeros(0, np.uint64)
    C = np.zeros((len(union), len(samples)), dtype=np.int64)
    for j, (uk, uc) in enumerate(maps):
        C[np.searchsorted(union, uk), j] = uc
    return union, C


def scarce_bound(N):
    return math.ceil(N * 0.05)


def mw_pvalues(ca, cb):
    """mannWhitneyUTest(groupA, groupB) per row of raw counts"""
    na, nb = ca.shape[1], cb.shape[1]
    u2 = R.mw_twice_u1(ca, cb)
    by_u2 = np.array([R.mw_pvalue_from_umin(min(u, 2 * na * nb - u) / 2.0, na, nb) for u in range(2 * na * nb + 1)])
    return by_u2[u2]


def _mean(c):
    s = np.zeros(c.shape[0])
    for j in range(c.shape[1]):
        s = s + c[:, j].astype(np.float64)
    return s / c.shape[1]


def specific_kmers(a_samples, b_samples, p_chi2=0.05, p_mw=0.05):
    """-> dict(A, B: (keys, vals); counters; q; kk: the statistic of every k-mer the test decides (not scarce, not in all); p: the
    p-values of the rows that reached Mann-Whitney, or None)"""
    na, nb = len(a_samples), len(b_samples)
    N = na + nb
    union, C = count_matrix(list(a_samples) + list(b_samples))
    pres = C > 0
    n1a, n1b = pres[:, :na].sum(axis=1), pres[:, na:].sum(axis=1)
    # entry.getValue() of the map the k-mer is met in first: the files are walked in order and a k-mer is zeroed everywhere once met
    first = C[np.arange(len(union)), pres.argmax(axis=1)] if len(union) else np.zeros(0, np.int64)
    unique = (n1a == 0) | (n1b == 0)                       # counted BEFORE the scarce cut (:151-158)
    scarce = first <= scarce_bound(N)
    in_all = (n1a + n1b) == N
    q = R.chi2_quantile(p_chi2)
    kk = R.chisq_kk(na - n1a, n1a, nb - n1b, n1b)
    with np.errstate(invalid="ignore"):
        chi_ok = in_all | (q < kk)                         # (:160-162: a k-mer of all files passes whatever kk is)
    reach = ~scarce & chi_ok
    ps = None
    rej = np.zeros(len(union), dtype=bool)
    if p_mw > 0:
        ps = mw_pvalues(C[:, :na], C[:, na:])
        rej = reach & (ps > p_mw)                          # (:166-170: p == pmw is kept)
        ps = ps[reach]
    kept = reach & ~rej
    mA, mB = _mean(C[:, :na]), _mean(C[:, na:])
    toA = kept & (mA > mB)
    toB = kept & ~toA                                      # (a tie goes to B)
    ctr = dict(n=len(union), unique=int(unique.sum()), scarce=int(scarce.sum()), chi2_rejected=int((~scarce & ~chi_ok).sum()),
               mw_rejected=int(rej.sum()), unique_left=int((kept & unique).sum()), group_a=int(toA.sum()), group_b=int(toB.sum()))
    return dict(A=(union[toA], R.java_short_of_int(mA[toA])), B=(union[toB], R.java_short_of_int(mB[toB])), counters=ctr, q=q,
                kk=kk[~scarce & ~in_all], p=ps)


def specific_kmers3(a_samples, b_samples, c_samples, p_chi2=0.05, p_mw=0.05):
    """-> dict(A, B, C: (keys, vals); counters named as stats-kmers-3's; q; kk; p; M)"""
    na, nb, nc = len(a_samples), len(b_samples), len(c_samples)
    N = na + nb + nc
    union, C = count_matrix(list(a_samples) + list(b_samples) + list(c_samples))
    pres = C > 0
    n1a, n1b, n1c = pres[:, :na].sum(axis=1), pres[:, na:na + nb].sum(axis=1), pres[:, na + nb:].sum(axis=1)
    tot = n1a + n1b + n1c                                  # hm_all: the number of maps that hold the k-mer (:103-112)
    scarce = tot <= scarce_bound(N)
    in_all = ~scarce & (tot == N)
    rest = ~scarce & ~in_all
    unique = rest & (((n1a + n1c) == 0) | ((n1b + n1a) == 0) | ((n1b + n1c) == 0))
    q = R.chi2_quantile(p_chi2)                            # ONE degree of freedom (:91)
    kk = R3.chisq3_stat(na - n1a, n1a, nb - n1b, n1b, nc - n1c, n1c)
    with np.errstate(invalid="ignore"):
        chi_ok = rest & (q < kk)
    F = C.sum(axis=0)                                      # n_kmers: the sum of the map's values (:104-113)
    M = int(F.sum()) // N                                  # a long (:147-151)
    Cs = C[chi_ok]
    with np.errstate(all="ignore"):
        V = np.where(Cs > 0, (Cs.astype(np.float64) * float(M)) / F.astype(np.float64)[None, :], 0.0)   # absent: 0 (:186-198)
    keep, grp, val, _, ps = R3.decide_rows(V, na, nb, nc, p_mw)
    surv = union[chi_ok]
    sel = [keep & (grp == g) for g in range(3)]
    ctr = dict(n=len(union), scarce=int(scarce.sum()), in_all=int(in_all.sum()), unique=int(unique.sum()), chi2_rejected=int((rest & ~chi_ok).sum()),
               mw_rejected=int((~keep).sum()), group_a=int(sel[0].sum()), group_b=int(sel[1].sum()), group_c=int(sel[2].sum()),
               unique_left=int((keep & unique[chi_ok]).sum()))     # isUniq, the presence test (:207, :248)
    out = dict(counters=ctr, q=q, kk=kk[rest], p=ps, M=M)
    for g, name in enumerate("ABC"):
        out[name] = (surv[sel[g]], val[sel[g]])
    return out


def unique_kmers(inputs, filters, b=1):
    """-> dict(hm: (keys, values) the pooled map with the zeroed k-mers at 0; out: the records printKmers writes; n: hm.size(); c)"""
    if inputs:
        pooled = (np.concatenate([np.asarray(s[0], np.uint64) for s in inputs]), np.concatenate([np.asarray(s[1], np.int64) for s in inputs]))
    else:
        pooled = (np.zeros(0, np.uint64), np.zeros(0, np.int64))
    keys, vals = load_map(pooled, b)
    vals = vals.copy()
    for f in filters:
        fk, fv = load_map(f, b)
        hit = np.isin(keys, fk[fv > b]) & (vals > b)
        vals[hit] = 0
    good = vals > b
    return dict(hm=(keys, vals), out=(keys[good], vals[good].astype(np.uint16)), n=len(keys), c=int(good.sum()))
