"""seq2comp restated on Python integers for any k <= 63 (tests/seq2comp_ref.py is the numpy restatement for k <= 31; no reference exists
for k > 31): one component per sequence, its members the distinct canonical k-mers ascending, size = their number, weight =
max(0, L - k + 1); a sequence shorter than k gives a component of size 0 and weight 0.  k-mers: A0 G1 C2 T3, the first base in the
most significant bits.  A component is (members as an ascending list of ints, size, weight), as in seq2comp_ref with lists for arrays.
Files: the wide components.bin of tests/wide_files_ref.py and the three-column components-stat.txt."""
import math

import numpy as np

import wide_files_ref as WF
from seq2comp_ref import NUC, rc_str, read_fasta, read_fastq, read_files, vec_txt  # noqa: F401

_CODE = {ch: i for i, ch in enumerate(NUC)}
_CODE.update({ch.lower(): i for i, ch in enumerate(NUC)})
MASK64 = (1 << 64) - 1


def occurrences(seq, k):
    """the canonical k-mer at every position, in order (list of ints, max(0, L - k + 1) of them)"""
    n = len(seq) - k + 1
    if n <= 0:
        return []
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    fw = rc = 0
    out = []
    for j, ch in enumerate(seq):
        c = _CODE[ch]
        fw = ((fw << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << top)
        if j >= k - 1:
            out.append(min(fw, rc))
    return out


def component(seq, k):
    occ = occurrences(seq, k)
    members = sorted(set(occ))
    return members, len(members), len(occ)


def components(seqs, k):
    return [component(s, k) for s in seqs]


def words(members):
    """-> (high words, low words) as uint64 arrays"""
    return (np.array([x >> 64 for x in members], dtype=np.uint64), np.array([x & MASK64 for x in members], dtype=np.uint64))


def arrays(comps):
    """what WideComps.export() gives: dict(sizes, weights, thr, offsets, hi, lo)"""
    sizes = np.array([c[1] for c in comps], dtype=np.uint64)
    off = np.zeros(len(comps) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(sizes, dtype=np.uint64)
    hi, lo = words([x for c in comps for x in c[0]])
    return dict(sizes=sizes, weights=np.array([c[2] for c in comps], dtype=np.int64), thr=np.zeros(len(comps), dtype=np.int32), offsets=off, hi=hi, lo=lo)


def components_bin(comps):
    a = arrays(comps)
    return WF.encode_components(a["sizes"], a["weights"], a["hi"], a["lo"])


def stat_txt(comps):
    return "# component.no\tcomponent.size\tcomponent.weight\n" + "".join(f"{i + 1}\t{c[1]}\t{c[2]}\n" for i, c in enumerate(comps))


def features(comps, sample, threshold=0):
    """seq2comp_ref.features on int members: a k-mer counts once per LISTING; -> (vec int64[], breadth float64[]; NaN for size 0)"""
    vec = np.zeros(len(comps), dtype=np.int64)
    br = np.zeros(len(comps), dtype=np.float64)
    for i, (members, size, _) in enumerate(comps):
        found = 0
        for x in members:
            v = sample.get(x, 0)
            if v > threshold:
                vec[i] += v
                found += 1
        br[i] = found / size if size else math.nan
    return vec, br


def kmers_bin(sample):
    """{k-mer: count} -> wide .kmers.bin bytes (ascending)"""
    keys = sorted(sample)
    hi, lo = words(keys)
    return WF.encode_kmers(hi, lo, [sample[x] for x in keys])


def encode(s):
    v = 0
    for ch in s:
        v = (v << 2) | _CODE[ch]
    return v


def decode(x, k):
    return "".join(NUC[(x >> (2 * (k - 1 - i))) & 3] for i in range(k))
