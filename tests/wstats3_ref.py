"""Reference of the wide (k = 32 ... 63) stats-kmers-3 and kmers-grouped-counter: samples given as {(hi << 64) | lo: count} dicts.

stats-kmers-3 depends on which k-mers are equal and on their order, not on their values, so the oracle is tests/stats3_ref.py unchanged: every
distinct k-mer of the cohort is mapped to its rank (a uint64), stats3_ref runs on the ranked tables, and the four lists are mapped back (the
route tests/wstats_ref.py takes through stats_ref).  The grouped counter is written out on Python integers from the definition in
include/metafast_hip.h (mf_kmers_grouped_count_wide_tables); it shares no code with the library."""
import numpy as np

import stats3_ref as S3
from wstats_ref import MASK64, ranked, records  # noqa: F401

COUNTERS = S3.COUNTERS


def stats_kmers3(a_samples, b_samples, c_samples, b=0, p_chi2=0.05, p_mw=0.05):
    """-> dict(chi, A, B, C = (keys: ascending list of Python ints, values: uint16[n]), counters = dict, and stats3_ref's q, kk, p)"""
    na, nb = len(a_samples), len(b_samples)
    keys, recs = ranked(list(a_samples) + list(b_samples) + list(c_samples))
    r = S3.stats_kmers3(recs[:na], recs[na:na + nb], recs[na + nb:], b=b, p_chi2=p_chi2, p_mw=p_mw)
    back = lambda kv: ([keys[int(i)] for i in kv[0]], np.asarray(kv[1], dtype=np.uint16))
    return dict(chi=back(r["chi"]), A=back(r["A"]), B=back(r["B"]), C=back(r["C"]), counters=r["counters"], q=r["q"], kk=r["kk"], p=r["p"])


def kmers_grouped_count(kf_samples, cd, uc, nonibd, b=1):
    """-> (keys ascending: the k-mers some -kf sample lists with a count > 0, int64[n][3]: per group the samples that hold each with a count > b)"""
    for g in (cd, uc, nonibd):
        if len(g) > 1022:
            raise ValueError("more than 1022 samples in a group")
    keys = sorted({x for t in kf_samples for x, c in t.items() if c > 0})
    out = np.zeros((len(keys), 3), dtype=np.int64)
    for i, x in enumerate(keys):
        for g, group in enumerate((cd, uc, nonibd)):
            out[i, g] = sum(1 for t in group if t.get(x, 0) > b)
    return keys, out


def kmer_text(x, k):
    """the k bases, the first base in the highest bits, A G C T = 0 1 2 3"""
    return "".join("AGCT"[(x >> (2 * (k - 1 - i))) & 3] for i in range(k))


def groups_txt(keys, counts, k):
    return "Kmer\tcd_count\tuc_count\tnonibd_count\n" + "".join("%s\t%d\t%d\t%d\n" % (kmer_text(x, k), c[0], c[1], c[2]) for x, c in zip(keys, counts))
