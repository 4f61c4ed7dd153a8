"""Python-integer reference of the wide (k = 32 ... 63) kmers-per-sample: samples given as {(hi << 64) | lo: count} dicts, written from the
definition in include/metafast_hip.h (mf_kmers_per_sample_wide_tables; KmersPerSampleCounter.java:56-157 carried over to two-word k-mers).
Shares no code with the library or with tests/kps_ref.py.

    candidates   every k-mer some sample -- the first included -- holds with count > max_bad
    n(x)         the samples j >= 1 (count_first: j >= 0) that hold x with count > max_bad
    thresh       N * percent / 100 as a Java int computes it: the product wraps to 32 bits, the division truncates toward zero
    selected     n(x) >= thresh, ascending
    the text     "\\t" + the k bases per selected k-mer, newline; per file: its name without any ".kmers.bin", "\\t" + count per selected k-mer
"""
import os

import numpy as np

BASES = "AGCT"


def thresh(n_samples, percent):
    p = (n_samples * percent) & 0xFFFFFFFF
    if p >= 1 << 31:
        p -= 1 << 32
    return -((-p) // 100) if p < 0 else p // 100


def select(samples, percent=20, count_first=False, max_bad=0):
    """-> (keys: ascending list of Python ints, n: uint16[M], matrix: uint16[N][M])"""
    N = len(samples)
    n = {}
    for j, t in enumerate(samples):
        for x, c in t.items():
            if c > max_bad:
                n[x] = n.get(x, 0) + (1 if j > 0 or count_first else 0)
    th = thresh(N, percent)
    keys = sorted(x for x, v in n.items() if v >= th)
    col = {x: i for i, x in enumerate(keys)}
    mat = np.zeros((N, len(keys)), dtype=np.uint16)
    for j, t in enumerate(samples):
        for x, c in t.items():
            if c > max_bad and x in col:
                mat[j, col[x]] = c
    return keys, np.array([n[x] for x in keys], dtype=np.uint16), mat


def kmer_text(x, k):
    return "".join(BASES[(x >> (2 * (k - 1 - q))) & 3] for q in range(k))


def header_text(keys, k):
    return "".join("\t" + kmer_text(x, k) for x in keys).encode()


def row_text(row):
    return "".join("\t%d" % int(v) for v in row).encode()


def row_name(path):
    return os.path.basename(str(path)).replace(".kmers.bin", "")


def file_text(samples, names, k, percent=20, count_first=False):
    """the whole file of the file form (every load at 0) -> (keys, bytes)"""
    keys, _, mat = select(samples, percent, count_first, 0)
    out = header_text(keys, k) + b"\n"
    for j, nm in enumerate(names):
        out += row_name(nm).encode() + row_text(mat[j]) + b"\n"
    return keys, out
