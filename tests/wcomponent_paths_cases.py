"""The inputs of tests/test_wcomponent_paths_gpu.py, built once per process: every builder gives (components, files, extra) -- components
as (members as ints, size, weight), numbered from 1; files as a list of lists of sequences, one list per call of add; extra is what the
case is about.  tests/test_wcomponent_paths_cpu.py asserts on these alone, with tests/wcomponent_paths_ref.py, what the GPU cases rely on."""
import functools

import numpy as np

import wseq2comp_ref as W
from wseq2comp_cases import KS, rnd  # noqa: F401

RUN = 32                               # CP_RUN: the positions one thread of k_cp_mark takes
RANDOM_PATHS = {32: 868, 33: 900, 47: 688, 63: 551}      # the paths the restatement finds in random_case(k) at min_len = k


def _comp(kmers, weight=None):
    members = sorted(set(kmers))
    return members, len(members), len(members) if weight is None else weight


@functools.lru_cache(maxsize=None)
def both_words(k):
    """T1: two neighbouring k-mers with the same low word (its last 33 bases are A) and another high word; T2: two with the same high
    word (its first k - 31 bases are A) and another low word.  Each of the four k-mers is a component of its own.  At k = 32 there is no high word: the pairs differ in the low word.  extra = the four k-mers."""
    rng = np.random.default_rng(5000 + k)
    t1 = ("C" + rnd(rng, k - 33) if k > 32 else "C") + "A" * (33 if k > 32 else 32)
    t2 = "A" * (k - 31) + rnd(rng, 30) + "CC"
    assert len(t1) == len(t2) == k + 1
    four = tuple(W.occurrences(t1, k) + W.occurrences(t2, k))
    comps = [_comp([x], 3) for x in four]
    n = lambda m: rnd(rng, m)
    files = [[n(20) + "T" + t1 + "T" + n(20), t1, n(7) + "G" + t2 + "G" + n(9), t2, t1[:k], t1[1:], W.rc_str(t2), (n(5) + "T" + t1 + "T" + n(5) + "G" + t2).lower()]]
    return comps, files, four


@functools.lru_cache(maxsize=None)
def strand(k):
    rng = np.random.default_rng(5100 + k)
    s1, s2 = rnd(rng, 150), rnd(rng, 90)
    comps = W.components([s1, s2], k)
    n = lambda m: rnd(rng, m)
    r1 = W.rc_str(s1)
    other = lambda b: "ACGT"[("ACGT".index(b) + 1) % 4]      # the filler's base next to the piece is not the sequence's own there: the path ends where it was cut
    files = [[r1, s1.lower(), W.rc_str(s2).lower(), n(29) + other(r1[4]) + r1[5:100] + other(r1[100]) + n(29), s2]]
    return comps, files, (s1, s2)


PLANS = ([(0, RUN - 1)], [(RUN, 2 * RUN - 1)], [(RUN - 1, RUN)], [(0, 0)], [(2 * RUN - 1, 2 * RUN - 1)], [(0, 0), (RUN - 1, RUN - 1), (RUN + 1, RUN + 1), (2 * RUN - 1, 2 * RUN - 1)],
         [(0, 2 * RUN - 1)], [(RUN - 12, RUN + 8)])


@functools.lru_cache(maxsize=None)
def borders(k):
    """sequences of 2 RUN = 64 positions, component i holds the positions PLANS[i] of sequence i; then the stretches of 0, 1, RUN - 1, RUN,
    RUN + 1 and 2 RUN positions of the sequence that lies in its component whole, a sequence shorter than k among them.  extra = PLANS"""
    rng = np.random.default_rng(5200 + k)
    seqs, comps = [], []
    for plan in PLANS:
        s = rnd(rng, 2 * RUN + k - 1)
        occ = W.occurrences(s, k)
        comps.append(_comp([x for a, b in plan for x in occ[a:b + 1]], 7 * len(plan)))
        seqs.append(s)
    whole = seqs[6]
    lens = [whole[:k - 1 + m] for m in (0, 1, RUN - 1, RUN, RUN + 1, 2 * RUN)]
    assert [len(s) for s in lens] == [k - 1, k, k + 30, k + 31, k + 32, k + 63]
    second = [lens[3], lens[0], lens[4], "", lens[1], lens[2], whole[-(k - 1):], lens[5], whole[-k:]]
    return comps, [seqs, second], PLANS


@functools.lru_cache(maxsize=None)
def shared(k):
    """seq2comp of a sequence given three times and two more that hold a stretch of it: that stretch's k-mers have five listings.
    extra = (the sequences the components are made of, the most listings of one k-mer)"""
    rng = np.random.default_rng(5300 + k)
    g = rnd(rng, 200)
    dom = g[40:150]
    n = lambda m: rnd(rng, m)
    seqs = [g, g, n(60) + dom + n(50), g, n(70) + dom]
    comps = W.components(seqs, k)
    files = [[g[10:190], n(30) + dom + n(30), W.rc_str(g)], [n(25) + dom[:100], g, n(100)]]
    count = {}
    for c in comps:
        for x in c[0]:
            count[x] = count.get(x, 0) + 1
    return comps, files, (seqs, max(count.values()))


@functools.lru_cache(maxsize=None)
def capped(k):
    """component 1 has six runs of at least 80 bases over three batches, component 2 is empty, component 3 has two.  extra = the same
    sequences as one batch"""
    rng = np.random.default_rng(5400 + k)
    gene, other = rnd(rng, 500), rnd(rng, 200)
    comps = [W.component(gene, k), W.component(rnd(rng, k - 1), k), W.component(other, k)]
    n = lambda m: rnd(rng, m)
    files = [[n(30) + gene[0:80] + n(30) + gene[100:190] + n(30)], [gene[200:300], n(40) + other[5:125]],
             [n(10) + gene[50:290] + n(10), gene[300:400] + n(20) + gene[0:100], other[60:190]]]
    return comps, files, [[s for f in files for s in f]]


@functools.lru_cache(maxsize=None)
def random_case(k):
    """about 200 components from random sequences of 40 .. 400 bases (some shorter than k: empty components), 300 queries spliced from
    pieces of them, their reverse complements and noise, in two batches.  extra = the sequences of the components"""
    rng = np.random.default_rng(5500 + k)
    genes = [rnd(rng, int(rng.integers(40, 401))) for _ in range(200)]
    queries = []
    for _ in range(300):
        want, s = int(rng.integers(30, 601)), ""
        while len(s) < want:
            kind = int(rng.integers(0, 4))
            if kind == 3:
                s += rnd(rng, int(rng.integers(3, 60)))
                continue
            g = genes[int(rng.integers(0, len(genes)))]
            a = int(rng.integers(0, max(1, len(g) - 20)))
            piece = g[a: a + int(rng.integers(20, 300))]
            s += W.rc_str(piece) if kind == 2 else piece
        queries.append(s[:want] if rng.random() < 0.8 else s[:want].lower())
    return W.components(genes, k), [queries[:170], queries[170:]], genes
