"""The eight de Bruijn neighbours of every k-mer of a table, and the minimizer partition of a k-mer, restated in plain numpy for the tests
of metafast_amd/csrc/mf_nbr.h.  Nothing here is shared with the kernels' way of getting there: a neighbour is built base by base, its
canonical form comes from a full reverse complement, and its place in the table from a sort and a binary search (the kernels hash the
interior (k-2)-mer the four neighbours of a side share, walk one probe sequence per side and get a neighbour's reverse complement by a
shift of the k-mer's own).  tests/test_nbr_ref_cpu.py pins this file with hand-worked cases.

A k-mer is a uint64 with two bits per base, A C G T = 0 1 2 3, the first base in the highest of its 2 k bits."""
import numpy as np

NONE = 0xFFFFFFFF
_U = np.uint64
_MASK32 = _U(0xFFFFFFFF)
MMER_MULT = 0x9E3779B1


def encode(s):
    v = 0
    for ch in s:
        v = (v << 2) | "ACGT".index(ch)
    return v


def decode(x, k):
    x = int(x)
    return "".join("ACGT"[(x >> (2 * (k - 1 - i))) & 3] for i in range(k))


def revcomp_plain(x, k):
    """reverse complement of k-mers (array or scalar), base by base: base i of the result is the complement of base k-1-i"""
    x = np.asarray(x, dtype=np.uint64)
    r = np.zeros_like(x)
    for i in range(k):
        r = (r << _U(2)) | (_U(3) - ((x >> _U(2 * i)) & _U(3)))
    return r


def revcomp(x, k):
    """the same on whole words (a table of 1e6 k-mers has 8e6 neighbours to turn round): complement every base, reverse the order of the
    32 two-bit groups of the word (pairs, nibbles, bytes), drop the 32 - k groups that were above the k-mer.  test_nbr_ref_cpu.py holds
    it against revcomp_plain for every k."""
    x = ~np.asarray(x, dtype=np.uint64)
    x = ((x >> _U(2)) & _U(0x3333333333333333)) | ((x & _U(0x3333333333333333)) << _U(2))
    x = ((x >> _U(4)) & _U(0x0F0F0F0F0F0F0F0F)) | ((x & _U(0x0F0F0F0F0F0F0F0F)) << _U(4))
    return x.byteswap() >> _U(64 - 2 * k)


def canonical(x, k):
    x = np.asarray(x, dtype=np.uint64)
    return np.minimum(x, revcomp(x, k))


def neighbour_kmers(keys, k):
    """-> uint64 [n, 8]: the neighbours as they are read off the k-mer (not canonical): slot 2 nuc = the k-mer without its first base
    and nuc appended on the right, slot 2 nuc + 1 = nuc prepended on the left of the k-mer without its last base"""
    keys = np.asarray(keys, dtype=np.uint64)
    mask = _U((1 << (2 * k)) - 1)
    out = np.empty((len(keys), 8), dtype=np.uint64)
    for nuc in range(4):
        out[:, 2 * nuc] = ((keys << _U(2)) | _U(nuc)) & mask
        out[:, 2 * nuc + 1] = (keys >> _U(2)) | _U(nuc << (2 * k - 2))
    return out


def neighbours(keys, k, with_strand=False, rows=None):
    """keys: the canonical k-mers of a table in table order (all different).  -> uint32 [n, 8]: the table position of each neighbour's
    canonical form, NONE where the table does not hold it.  A k-mer that is its own neighbour (poly-A) gets its own position; a
    palindromic neighbour is its own reverse complement and counts as itself.  with_strand: also bool [n, 8], True where the table
    holds the neighbour as its reverse complement (the neighbour as read off the k-mer is not canonical).  rows: the neighbours of
    keys[rows] only (looked up in the whole table)"""
    keys = np.asarray(keys, dtype=np.uint64)
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    assert len(sk) == 0 or np.all(sk[1:] > sk[:-1]), "the keys of a table are all different"
    y = neighbour_kmers(keys if rows is None else keys[rows], k)
    n = len(y)
    c = canonical(y.reshape(-1), k).reshape(n, 8)
    out = np.full((n, 8), NONE, dtype=np.uint32)
    if n:
        flat = c.reshape(-1)
        qo = np.argsort(flat)                               # (queries in ascending order: the binary searches walk the table once)
        pos = np.empty(flat.shape, dtype=np.int64)
        pos[qo] = np.searchsorted(sk, flat[qo])
        pos = pos.reshape(c.shape)
        hit = pos < len(sk)
        hit[hit] = sk[pos[hit]] == c[hit]
        out[hit] = order[pos[hit]].astype(np.uint32)
    return (out, c != y) if with_strand else out


def mmer_len(k):
    return 13 if k <= 25 else 15


def mmer_seed(M):
    return 0x00B9107F if M == 13 else 0x051E6720


def mmer_hash(canon, M):
    """the order of the canonical M-mers (mf_mmer_hash): (canon ^ seed) * 0x9E3779B1 in 32 bits"""
    canon = np.asarray(canon, dtype=np.uint64)
    return ((canon ^ _U(mmer_seed(M))) * _U(MMER_MULT)) & _MASK32


def remix32(h):
    h = np.asarray(h, dtype=np.uint64) & _MASK32
    h = h ^ (h >> _U(16))
    h = (h * _U(0x85EBCA6B)) & _MASK32
    h = h ^ (h >> _U(13))
    h = (h * _U(0xC2B2AE35)) & _MASK32
    return h ^ (h >> _U(16))


def part_hash(keys, k):
    """mf_skm_ph (mf_common.h): the smallest mmer_hash over the canonical forms of the k - M + 1 M-mers of a k-mer, mixed once more; a
    table with 2^b minimizer partitions keeps the k-mer in partition part_hash >> (32 - b).  -> uint64 array of 32-bit values"""
    keys = np.asarray(keys, dtype=np.uint64)
    M = mmer_len(k)
    mm = _U((1 << (2 * M)) - 1)
    best = np.full(keys.shape, 0xFFFFFFFF, dtype=np.uint64)
    for j in range(k - M + 1):                              # the M-mer that starts at base j
        f = (keys >> _U(2 * (k - M - j))) & mm
        best = np.minimum(best, mmer_hash(np.minimum(f, revcomp(f, M)), M))
    return remix32(best)


def low_mmers(M, count):
    """the `count` canonical M-mers with the smallest mmer_hash, ascending by hash: [(M-mer, hash)].  The multiplier is odd, so the hash is
    a bijection of the 32-bit words: walk the hash values up from 0, invert, keep what is an M-mer (fits 2 M bits) in canonical form.  A
    k-mer that holds such an M-mer (and none with a smaller hash) has it as its minimizer."""
    inv = pow(MMER_MULT, -1, 1 << 32)
    seed = mmer_seed(M)
    out = []
    h = 0
    while len(out) < count:
        c = ((h * inv) & 0xFFFFFFFF) ^ seed
        if c < (1 << (2 * M)) and c <= int(revcomp(c, M)):
            out.append((c, h))
        h += 1
    return out
