"""numpy restatement of the two file formats of the k = 32 ... 63 path (no reference format exists for k > 31) -- the checker of
metafast_amd/csrc/mf_wio.hip's encode / decode / validation kernels.

wide .kmers.bin      headerless; 18-byte big-endian records: int64 high word, int64 low word, int16 count; strictly ascending (hi, lo)
wide components.bin  int32 n; per component int32 size, int64 weight, size x (int64 hi, int64 lo); big-endian
"""
import numpy as np

REC = np.dtype([("hi", ">u8"), ("lo", ">u8"), ("cnt", ">i2")])
assert REC.itemsize == 18
MASK64 = (1 << 64) - 1


def encode_kmers(hi, lo, counts):
    r = np.empty(len(hi), dtype=REC)
    r["hi"], r["lo"], r["cnt"] = np.asarray(hi, dtype=np.uint64), np.asarray(lo, dtype=np.uint64), np.asarray(counts).astype(np.int16)
    return r.tobytes()


def decode_kmers(data):
    """-> (hi uint64[], lo uint64[], counts int16[]); ValueError when the size is no multiple of the record"""
    if len(data) % REC.itemsize:
        raise ValueError("size %d is not a multiple of the 18-byte record" % len(data))
    r = np.frombuffer(data, dtype=REC)
    return r["hi"].astype(np.uint64), r["lo"].astype(np.uint64), r["cnt"].astype(np.int16)


def revcomp(x, k):
    """reverse complement of a 2k-bit k-mer given as a Python int (A0 G1 C2 T3: complement = 3 - n)"""
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def first_bad_record(hi, lo, k):
    """the three validity rules, in the loader's order per record: None, or (record number, rule) with rule in
    'range' (key >= 4^k), 'canonical' (key > its reverse complement), 'order' (not strictly above its predecessor)"""
    prev = None
    for i, (h, l) in enumerate(zip(np.asarray(hi).tolist(), np.asarray(lo).tolist())):
        x = (int(h) << 64) | int(l)
        if x >> (2 * k):
            return i, "range"
        if x > revcomp(x, k):
            return i, "canonical"
        if prev is not None and not prev < x:
            return i, "order"
        prev = x
    return None


def encode_components(sizes, weights, hi, lo):
    """members grouped by component in (hi, lo), sizes[i] of them for component i"""
    out = [np.array([len(sizes)], dtype=">i4").tobytes()]
    at = 0
    for sz, w in zip(np.asarray(sizes).tolist(), np.asarray(weights).tolist()):
        out.append(np.array([sz], dtype=">i4").tobytes() + np.array([w], dtype=">i8").tobytes())
        m = np.empty((sz, 2), dtype=">u8")
        m[:, 0], m[:, 1] = hi[at:at + sz], lo[at:at + sz]
        out.append(m.tobytes())
        at += sz
    assert at == len(hi) == len(lo)
    return b"".join(out)


def decode_components(data):
    """-> (sizes, weights, hi, lo); ValueError on a file that does not add up"""
    if len(data) < 4:
        raise ValueError("no component count")
    n = int(np.frombuffer(data[:4], dtype=">i4")[0])
    at, sizes, weights, his, los = 4, [], [], [], []
    for _ in range(n):
        if at + 12 > len(data):
            raise ValueError("the file ends inside a header")
        sz = int(np.frombuffer(data[at:at + 4], dtype=">i4")[0])
        w = int(np.frombuffer(data[at + 4:at + 12], dtype=">i8")[0])
        at += 12
        if sz < 0 or at + 16 * sz > len(data):
            raise ValueError("a component larger than the file")
        m = np.frombuffer(data[at:at + 16 * sz], dtype=">u8").reshape(sz, 2)
        his.append(m[:, 0].astype(np.uint64)); los.append(m[:, 1].astype(np.uint64))
        sizes.append(sz); weights.append(w)
        at += 16 * sz
    if at != len(data):
        raise ValueError("bytes after the last component")
    cat = lambda v: np.concatenate(v) if v else np.empty(0, dtype=np.uint64)
    return np.array(sizes, dtype=np.uint64), np.array(weights, dtype=np.int64), cat(his), cat(los)


def stat_text(counts):
    """.stat.txt of a table with these counts (QuickQuantitativeStatistics.printToFile's text, as for k <= 31)"""
    h = np.bincount(np.asarray(counts, dtype=np.int64), minlength=1)
    return "# k-mer frequency\tnumber of such k-mers\n" + "".join("%d\t%d\n" % (v, c) for v, c in enumerate(h.tolist()) if c) + "\n"
