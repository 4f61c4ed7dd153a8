"""seq2comp restated in numpy / Python from src/tools/SequencesToComponents.java:61-103 and src/algo/ComponentFromSequence.java:24-30:
one component per sequence that survives the readers, its members the distinct canonical k-mers (ShortKmer.kmersOf, toLong() =
min(forward, reverse complement)), size = their number, weight = the k-mer occurrences max(0, L - k + 1) (the one-argument add of
SequenceComponent adds 1 per occurrence, duplicate or not); a sequence shorter than k gives a component of size 0 and weight 0.
k-mers: A0 G1 C2 T3, the first base in the most significant bits.  Members ascend here (the reference: first-occurrence order) and
components come in file order, then record order (the reference: as its thread pool finishes): the two stated deviations."""
import math
import struct

import numpy as np

NUC = "AGCT"
_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _ch in enumerate(NUC):
    _CODE[ord(_ch)] = _i
    _CODE[ord(_ch.lower())] = _i
_RC = str.maketrans("ACGT", "TGCA")


def rc_str(s):
    return s.translate(_RC)[::-1]


def encode(s):
    v = 0
    for ch in s:
        v = (v << 2) | NUC.index(ch)
    return v


def _codes(seq):
    b = np.frombuffer(seq.encode("ascii") if isinstance(seq, str) else bytes(seq), dtype=np.uint8)
    c = _CODE[b]
    assert not (c == 255).any(), "a sequence that survived the readers holds A, C, G and T only"
    return c.astype(np.uint64)


def occurrences(seq, k):
    """the canonical k-mer at every position, in order (uint64[max(0, L - k + 1)])"""
    c = _codes(seq)
    n = len(c) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint64)
    fw = np.zeros(n, dtype=np.uint64)
    rc = np.zeros(n, dtype=np.uint64)
    for j in range(k):
        w = c[j:j + n]
        fw = (fw << np.uint64(2)) | w
        rc = rc | ((np.uint64(3) - w) << np.uint64(2 * j))
    return np.minimum(fw, rc)


def component(seq, k):
    """-> (ascending distinct canonical k-mers uint64[], size, weight)"""
    occ = occurrences(seq, k)
    members = np.unique(occ)
    return members, len(members), len(occ)


def components(seqs, k):
    return [component(s, k) for s in seqs]


def components_bin(comps):
    """ConnectedComponent.saveComponents (src/structures/ConnectedComponent.java:80-93): int count; per component int size, long weight, the k-mers"""
    out = [struct.pack(">I", len(comps))]
    for members, size, weight in comps:
        out.append(struct.pack(">Iq", size, weight))
        out.append(np.asarray(members, dtype=">u8").tobytes())
    return b"".join(out)


def stat_txt(comps):
    """SequencesToComponents.java:84-91: three columns, numbered from 1"""
    return "# component.no\tcomponent.size\tcomponent.weight\n" + "".join(f"{i + 1}\t{c[1]}\t{c[2]}\n" for i, c in enumerate(comps))


def read_fasta(path):
    """the records FastaReader hands on: lines of a record joined, records with an N dropped (FastaReader.java:53-76)"""
    seqs, cur = [], None
    for ln in open(path).read().splitlines():
        if ln.startswith(">"):
            if cur is not None:
                seqs.append(cur)
            cur = ""
        elif cur is not None:
            cur += ln.strip()
    if cur is not None:
        seqs.append(cur)
    return [s.upper() for s in seqs if "N" not in s.upper()]


def read_fastq(path):
    """four-line records; a record with an N or a phred-0 base ('!') is dropped (FastaReaderFromXQSource.java:66-70)"""
    ln = open(path).read().splitlines()
    out = []
    for i in range(0, len(ln) - 3, 4):
        s, q = ln[i + 1].strip().upper(), ln[i + 3].strip()
        if "N" not in s and "!" not in q:
            out.append(s)
    return out


def read_files(paths):
    """-> (sequences of all files in order, sequences per file)"""
    seqs, per = [], []
    for p in paths:
        r = read_fastq(p) if str(p).endswith((".fq", ".fastq")) else read_fasta(p)
        seqs += r
        per.append(len(r))
    return seqs, per


def features(comps, sample, threshold=0):
    """FeaturesCalculatorMain.java:97-103, 192-203: the map holds every member once, buildAndPrintVector reads it once per LISTING -- a
    k-mer that several components list counts in each.  sample: {k-mer: count}.  -> (vec int64[], breadth float64[]; NaN for size 0)"""
    vec = np.zeros(len(comps), dtype=np.int64)
    br = np.zeros(len(comps), dtype=np.float64)
    for i, (members, size, _) in enumerate(comps):
        found = 0
        for x in members.tolist():
            v = sample.get(x, 0)
            if v > threshold:
                vec[i] += v
                found += 1
        br[i] = found / size if size else math.nan
    return vec, br


def vec_txt(vec):
    return "".join(f"{int(v)}\n" for v in vec)
