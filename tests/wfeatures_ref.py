"""features-calculator restated on Python ints and one dict, for any k <= 63: both inputs of the reference's tool (a k-mers table, reads) with
and without --selected.  Written from FeaturesCalculatorMain.java (:97-103 hm.put(kmer, 0); :117-131 the reads branch over
IOUtils.calculatePresenceForReads, 64-bit counts; :137-162 the k-mers branch; :186-206 buildAndPrintVector) and from the oracle's text
(oracle/mf_oracle_core.inc: build_vector, or_features_selected, or_features_reads_selected).

k-mers: A0 G1 C2 T3, the first base in the most significant bits, canonical = the smaller of a k-mer and its reverse complement.
A component is the list of its member k-mers as they are LISTED: a k-mer that two components list, or one lists twice, is read once per
listing.  sample / selected: {k-mer: value}.  -> (vec int64[], breadth float64[]); breadth = found / cnt, NaN when no listing takes part."""
import math
from decimal import Decimal

import numpy as np

_CODE = {"A": 0, "G": 1, "C": 2, "T": 3, "a": 0, "g": 1, "c": 2, "t": 3}
MASK64 = (1 << 64) - 1


def canonical_kmers(read, k):
    """the canonical k-mer at every position of a read, in order; a read shorter than k gives none"""
    if isinstance(read, (bytes, bytearray)):
        read = read.decode("ascii")
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    fw = rc = 0
    out = []
    for j, ch in enumerate(read):
        c = _CODE[ch]
        fw = ((fw << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << top)
        if j >= k - 1:
            out.append(min(fw, rc))
    return out


def _hm(comps):
    return {x: 0 for members in comps for x in members}


def build_vector(comps, hm, threshold=0, selected=None):
    vec = np.zeros(len(comps), dtype=np.int64)
    br = np.zeros(len(comps), dtype=np.float64)
    for i, members in enumerate(comps):
        total = cnt = found = 0
        for x in members:
            if selected is None or selected.get(x, 0) > 0:
                value = hm.get(x, 0)
                if value > threshold:
                    total += value
                    found += 1
                cnt += 1
        vec[i] = total
        br[i] = found / cnt if cnt else math.nan               # (Java: 0.0 / 0.0)
    return vec, br


def from_kmers(comps, sample, threshold=0, selected=None):
    hm = _hm(comps)
    for x, v in sample.items():                                 # every record of the .kmers.bin
        if x in hm:
            hm[x] += v
    return build_vector(comps, hm, threshold, selected)


def presence(comps, reads, k):
    """hm after the reads branch: occurrences of every member in the reads, unbounded"""
    hm = _hm(comps)
    for r in reads:
        for x in canonical_kmers(r, k):
            if x in hm:
                hm[x] += 1
    return hm


def from_reads(comps, reads, k, threshold=0, selected=None):
    return build_vector(comps, presence(comps, reads, k), threshold, selected)


def count(reads, k):
    """{canonical k-mer: occurrences} of the reads, capped at 32767 as a counted table is"""
    t = {}
    for r in reads:
        for x in canonical_kmers(r, k):
            t[x] = min(t.get(x, 0) + 1, 32767)
    return t


def encode(s):
    v = 0
    for ch in s:
        v = (v << 2) | _CODE[ch]
    return v


def revcomp_str(s):
    return s.translate(str.maketrans("ACGTacgt", "TGCAtgca"))[::-1]


def words(members):
    """-> (high words, low words) as uint64 arrays"""
    return (np.array([x >> 64 for x in members], dtype=np.uint64), np.array([x & MASK64 for x in members], dtype=np.uint64))


# ---- the tool's files ----
def java_double(d):
    """Double.toString for the values a breadth takes (0 <= d <= 1 or NaN): the shortest digits that round-trip, decimal notation
    from 1e-3 on, d.dddE-n below"""
    if math.isnan(d):
        return "NaN"
    if d == 0:
        return "0.0"
    if d >= 1e-3:
        return repr(float(d))
    _, digits, exp = Decimal(repr(float(d))).as_tuple()
    s = "".join(map(str, digits)).rstrip("0")
    return s[0] + "." + (s[1:] or "0") + "E" + str(len(digits) + exp - 1)


def vec_text(vec):
    return "".join("%d\n" % int(v) for v in vec)


def breadth_text(br):
    return "".join(java_double(float(b)) + "\n" for b in br)
