"""Reference of the wide (k = 32 ... 63) stats-kmers and sample counter: samples given as {(hi << 64) | lo: count} dicts.

stats-kmers depends on which k-mers are equal and on their order, not on their values, so the oracle is tests/stats_ref.py unchanged: every
distinct k-mer of the cohort is mapped to its rank (a uint64), stats_ref runs on the ranked tables, and the three lists are mapped back (the
route tests/wkps_ref.py takes through kps_ref).  The sample counter is written out on Python integers from the definition in
include/metafast_hip.h (mf_kmers_samples_count_wide_tables); it shares no code with the library."""
import numpy as np

import stats_ref as SR
import wide_files_ref as WF

MASK64 = (1 << 64) - 1
COUNTERS = ("n", "scarce", "in_all", "unique", "chi2_rejected", "mw_rejected", "group_a", "group_b", "unique_left")


def ranked(samples):
    """-> (the cohort's distinct k-mers ascending, the samples as stats_ref records (ranks uint64[n], counts int16[n]))"""
    keys = sorted(set().union(*samples)) if samples else []
    rank = {x: i for i, x in enumerate(keys)}
    recs = []
    for t in samples:
        xs = sorted(t)
        recs.append((np.array([rank[x] for x in xs], dtype=np.uint64), np.array([t[x] for x in xs], dtype=np.int16)))
    return keys, recs


def stats_kmers(a_samples, b_samples, b=0, p_chi2=0.05, p_mw=0.05):
    """-> dict(chi, A, B = (keys: ascending list of Python ints, values: uint16[n]), counters = dict, and stats_ref's q, kk, p)"""
    keys, recs = ranked(list(a_samples) + list(b_samples))
    r = SR.stats_kmers(recs[:len(a_samples)], recs[len(a_samples):], b=b, p_chi2=p_chi2, p_mw=p_mw)
    back = lambda kv: ([keys[int(i)] for i in kv[0]], np.asarray(kv[1], dtype=np.uint16))
    return dict(chi=back(r["chi"]), A=back(r["A"]), B=back(r["B"]), counters=r["counters"], q=r["q"], kk=r["kk"], p=r["p"])


def kmers_samples_count(samples, b=1):
    """-> (keys ascending, n uint16[len]) for every k-mer some sample holds with count > b"""
    if len(samples) > 32767:
        raise ValueError("more than 32767 samples")
    n = {}
    for t in samples:
        for x, c in t.items():
            if c > b:
                n[x] = n.get(x, 0) + 1
    keys = sorted(n)
    return keys, np.array([n[x] for x in keys], dtype=np.uint16)


def records(keys, vals):
    """wide .kmers.bin records of an ascending list: the values as the 16 bits they are"""
    v = np.asarray(vals, dtype=np.uint16).astype(np.int16)
    return WF.encode_kmers([x >> 64 for x in keys], [x & MASK64 for x in keys], v)
