"""kmers-per-sample restated from the reference (src/tools/KmersPerSampleCounter.java:56-157; the map: BigLong2ShortHashMap /
Long2ShortHashMap of the itmo assembler), in numpy and plain Python, sharing no code with the library.

A sample is a pair (keys, counts): the 10-byte records of its .kmers.bin file in file order, counts as Java shorts.

    loadKmers(file, 0)   :78, :140   the records with a value > 0; the values of a k-mer listed more than once are added, each add
                                     saturating at 32767
    the first file       :82-96      hm = filt_hm; hm.resetValues(): the first file's own map is the accumulator, zeroed BEFORE it is
                                     iterated -- no entry of it has a value > 0 any more, so file 0 brings its keys and no increments
    n(x)                 :93-95      + 1 for every later file that holds x
    thresh               :101        files * percent / 100 in Java int arithmetic (wrapping product, truncation toward zero)
    selected             :110        n(x) >= thresh
    the text             :128-153    "\\t" + k-mer per selected k-mer, newline; per file: its name with every ".kmers.bin" removed, "\\t" +
                                     getWithZero(k-mer) per selected k-mer, newline
Deviation stated by the project: the columns come in ascending key order, the reference's order is its hash map's."""
import os

import numpy as np

SHORT_MAX = 32767


def records_to_bytes(keys, counts):
    a = np.empty(len(keys), dtype=np.dtype([("k", ">u8"), ("c", ">i2")]))
    a["k"] = np.asarray(keys, dtype=np.uint64)
    a["c"] = np.asarray(counts, dtype=np.int64).astype(np.int16)
    return a.tobytes()


def load_kmers(sample, max_bad=0):
    """IOUtils.loadKmers(file, 0) -> (ascending distinct keys, their saturated sums); max_bad > 0: a resident table read at that
    threshold, i.e. the entries whose sum is > max_bad"""
    keys = np.asarray(sample[0], dtype=np.uint64)
    cnt = np.asarray(sample[1], dtype=np.int64)
    cnt = np.where(cnt > SHORT_MAX, cnt - 65536, cnt)            # (a value written as an unsigned 16-bit number is a Java short)
    keep = cnt > 0
    keys, cnt = keys[keep], cnt[keep]
    uk, inv = np.unique(keys, return_inverse=True)
    s = np.zeros(len(uk), dtype=np.int64)
    np.add.at(s, inv, cnt)
    s = np.minimum(s, SHORT_MAX)                                 # (positive addends: saturating add by add = the capped sum)
    keep = s > max_bad
    return uk[keep], s[keep]


def java_int(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def thresh_of(n_files, percent):
    p = java_int(n_files * percent)
    q = abs(p) // 100
    return q if p >= 0 else -q


def kmer_text(key, k):
    """ShortKmer.toString: two bits a base, the first base in the highest bits, A G C T = 0 1 2 3"""
    key = int(key)
    return "".join("AGCT"[(key >> (2 * (k - 1 - i))) & 3] for i in range(k))


def row_name(path):
    return os.path.basename(path).replace(".kmers.bin", "")


def select(samples, percent=20, count_first=False, max_bad=0):
    """-> (keys ascending uint64[M], n uint16[M], matrix uint16[N][M])"""
    loaded = [load_kmers(s, max_bad) for s in samples]
    N = len(loaded)
    union = np.unique(np.concatenate([k for k, _ in loaded])) if N else np.zeros(0, np.uint64)
    n = np.zeros(len(union), dtype=np.int64)
    for j, (k, _) in enumerate(loaded):
        if j == 0 and not count_first:
            continue
        n[np.searchsorted(union, k)] += 1
    sel = n >= thresh_of(N, percent)
    keys, ns = union[sel], n[sel]
    mat = np.zeros((N, len(keys)), dtype=np.uint16)
    for j, (k, c) in enumerate(loaded):
        if not len(keys):
            break
        at = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
        hit = keys[at] == k
        mat[j, at[hit]] = c[hit]
    return keys, ns.astype(np.uint16), mat


def header_text(keys, k):
    """a tab and kmer_text(x, k) for every key, in one numpy pass"""
    keys = np.asarray(keys, dtype=np.uint64)
    shifts = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    codes = ((keys[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.intp)
    cells = np.full((len(keys), k + 1), ord("\t"), dtype=np.uint8)
    cells[:, 1:] = np.frombuffer(b"AGCT", dtype=np.uint8)[codes]
    return cells.tobytes().decode()


def row_text(row):
    return "".join("\t%d" % v for v in row.tolist())


def kmers_per_sample(samples, names, k, percent=20, count_first=False, max_bad=0):
    """-> (keys, n, matrix, the file's bytes); names: the files' paths (or names), in argument order"""
    keys, ns, mat = select(samples, percent, count_first, max_bad)
    text = header_text(keys, k) + "\n" + "".join(row_name(nm) + row_text(mat[j]) + "\n" for j, nm in enumerate(names))
    return keys, ns, mat, text.encode()
