"""Crafted k-mer graphs for the sharded component cutter (metafast_amd/csrc/mf_cc.hip: k_dcc_*, mf_dcc_*, mf_cut_components_of_shard,
mf_cut_components_sharded), in plain numpy: no GPU, nothing of the library's.

A case is a list of DNA sequences with k, l, b1, b2.  The sequences go to the cutter as if they were the samples' unitigs: a rank counts
its shard of them (count_device_shard), the oracle counts all of them (Table.count_buffer sequence by sequence with min_len = l, which is
what Table.count_seqs does with unitigs of its own).  The value of a k-mer is the number of times it occurs in the sequences: a stretch
gets the value v by being listed v times.  Everything random comes from a fixed seed and is long enough that no k-mer occurs twice by
accident: `n_distinct` is the number of distinct k-mers the lengths promise, build() asserts it on table(), tests/test_dcc_cases_cpu.py
asserts it on the oracle's table, together with what every case is there for (the path it must reach).

table() and neighbours() restate the k-mer arithmetic (A, G, C, T = 0 .. 3, first base in the top bits, a k-mer stands for the smaller of
itself and its reverse complement) so that the tests can look at a case without the oracle: distinct k-mers, palindromes, and the
adjacency that tests/cc_ref.py's cut() takes -- a second reference on the same graph."""
import numpy as np

SWEEP_K = (20, 21, 22, 25, 26, 30, 31)          # 20: the smallest k with minimizer partitions; <= 25: 13-mer minimizers; even k: palindromes
BOTH_K = (31, 21)
NONE = 0xFFFFFFFF

_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"AGCT"):                # (the reference's DnaTools order: complement = 3 - code)
    _CODE[_c] = _i


# ---- k-mers in numpy ----

def revcomp(x, k):
    x = np.asarray(x, dtype=np.uint64)
    r = np.zeros_like(x)
    for j in range(k):
        r = (r << np.uint64(2)) | (np.uint64(3) - ((x >> np.uint64(2 * j)) & np.uint64(3)))
    return r


def kmers_of(seq, k):
    """-> (canonical k-mers of every position uint64[len - k + 1], palindrome there bool[])"""
    c = _CODE[np.frombuffer(seq.encode(), dtype=np.uint8)]
    assert c.max(initial=0) < 4, "ACGT only"
    c = c.astype(np.uint64)
    n = len(c) - k + 1
    if n <= 0:
        return np.empty(0, dtype=np.uint64), np.empty(0, dtype=bool)
    fw, rc = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    for j in range(k):
        fw = (fw << np.uint64(2)) | c[j:j + n]
        rc |= (np.uint64(3) - c[j:j + n]) << np.uint64(2 * j)
    return np.minimum(fw, rc), fw == rc


def table(seqs, k, l):
    """-> (keys uint64[] ascending, values int64[], palindrome bool[]) of the sequences of at least l bases"""
    parts = [kmers_of(s, k) for s in seqs if len(s) >= l]
    if not parts:
        return np.empty(0, dtype=np.uint64), np.empty(0, dtype=np.int64), np.empty(0, dtype=bool)
    km, pal = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    keys, first, vals = np.unique(km, return_index=True, return_counts=True)
    return keys, vals.astype(np.int64), pal[first]


def neighbours(keys, k):
    """-> uint32 [n, 8]: for every key the index of each of its eight possible neighbours (one base appended, one base prepended) in
    keys, NONE where the table does not hold it -- the graph tests/cc_ref.py cuts"""
    keys = np.asarray(keys, dtype=np.uint64)
    mask = np.uint64((1 << (2 * k)) - 1)
    nbr = np.full((len(keys), 8), NONE, dtype=np.uint32)
    if not len(keys):
        return nbr
    for nuc in range(4):
        right = ((keys << np.uint64(2)) | np.uint64(nuc)) & mask
        left = (keys >> np.uint64(2)) | (np.uint64(nuc) << np.uint64(2 * k - 2))
        for slot, y in ((2 * nuc, right), (2 * nuc + 1, left)):
            c = np.minimum(y, revcomp(y, k))
            at = np.minimum(np.searchsorted(keys, c), len(keys) - 1)
            hit = keys[at] == c
            nbr[hit, slot] = at[hit].astype(np.uint32)
    return nbr


def pack(seqs):
    """-> (bases uint8[], offsets uint64[n + 1]): the layout the C-ABI and the oracle take"""
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if seqs:
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return np.frombuffer("".join(seqs).encode(), dtype=np.uint8).copy(), off


# ---- the cases ----

class Case:
    def __init__(self, name, seqs, k, b1, b2, n_distinct=None, **want):
        self.name, self.seqs, self.k, self.l, self.b1, self.b2 = name, list(seqs), k, k, b1, b2      # l = k: a sequence of one k-mer counts
        self.n_distinct = n_distinct                        # None: the case has repeats on purpose
        self.want = want                                    # what the case was made for (asserted on the oracle by test_dcc_cases_cpu.py)
        assert all(len(s) >= self.l for s in self.seqs)

    def __repr__(self):
        return f"Case({self.name}, k={self.k}, b1={self.b1}, b2={self.b2}, {len(self.seqs)} sequences)"

    def table(self):
        return table(self.seqs, self.k, self.l)


def _rand(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n).tolist())


def _stretch(seq, first, n, k):
    """the bases of the k-mers first .. first + n - 1 of seq: listing them again adds 1 to the value of exactly these"""
    assert 0 <= first and first + n + k - 1 <= len(seq)
    return seq[first:first + n + k - 1]


def _checked(case):
    if case.n_distinct is not None:
        keys, _, _ = case.table()
        assert len(keys) == case.n_distinct, (case, len(keys), case.n_distinct)           # no k-mer twice by accident
    return case


def ties(k):
    """40 components of 60 k-mers of value 1: one (size, weight) forty times, in order of the smallest k-mer alone.  Two pairs that tie
    in size and weight with different values inside ((60, 80): 20 k-mers of value 2 at the front / in the middle; (60, 100): 40 of
    value 2 / 20 of value 3).  One component of 150 > b2 k-mers whose two stretches of 30 k-mers of value 2 tie at threshold 2."""
    rng = np.random.default_rng(1000 + k)
    n, b1, b2 = 60, 10, 100
    seqs = [_rand(rng, n + k - 1) for _ in range(40)]
    a, b, c, d = (_rand(rng, n + k - 1) for _ in range(4))
    seqs += [a, _stretch(a, 0, 20, k), b, _stretch(b, 20, 20, k)]
    seqs += [c, _stretch(c, 0, 40, k), d, _stretch(d, 40, 20, k), _stretch(d, 40, 20, k)]
    e = _rand(rng, 150 + k - 1)
    seqs += [e, _stretch(e, 10, 30, k), _stretch(e, 100, 30, k)]
    kept = [(60, 100, 1)] * 2 + [(60, 80, 1)] * 2 + [(60, 60, 1)] * 40 + [(30, 60, 2)] * 2
    return _checked(Case("ties", seqs, k, b1, b2, n_distinct=44 * n + 150, kept=kept))


BOUNDS = [(5, 40), (5, 5), (40, 5)]              # b1 < b2, b1 == b2, b2 < b1: cc_ref's handover, handover_b1_eq_b2, handover_b2_lt_b1
STRETCH = 5                                      # k-mers of value 2 in the middle of the component of b2 + 1


def bounds(k, b1, b2):
    """one component each of b1 - 1, b1, b1 + 1, b2 - 1, b2, b2 + 1 k-mers of value 1; the one of b2 + 1 has 5 k-mers of value 2 inside.
    Worked by hand (a component of size s is dropped if s < b1, else kept if s <= b2, else only its k-mers of value >= 2 go on):

      (5, 40):  sizes 4, 5, 6, 39, 40, 41: 4 is dropped; 5, 6, 39, 40 are kept at threshold 1; of the 41 (weight 46) the 5 of value 2 go on
                and are kept at threshold 2 (size 5, weight 10)
      (5, 5):   sizes 4, 5, 6, 4, 5, 6: the two 4s are dropped, the two 5s kept; both 6s are too large: one has nothing of value 2, of
                the other the 5 go on and are kept at threshold 2
      (40, 5):  sizes 39, 40, 41, 4, 5, 6: 39, 4, 5, 6 are dropped (the test against b1 comes first); 40 and 41 are too large and have
                nothing of value 2: nothing is kept at any threshold"""
    rng = np.random.default_rng(2000 + 100 * k + 7 * b1 + b2)
    sizes = [b1 - 1, b1, b1 + 1, b2 - 1, b2, b2 + 1]
    seqs = [_rand(rng, s + k - 1) for s in sizes]
    seqs.append(_stretch(seqs[-1], (b2 + 1 - STRETCH) // 2, STRETCH, k))
    kept = {(5, 40): [(40, 40, 1), (39, 39, 1), (6, 6, 1), (5, 5, 1), (5, 10, 2)],
            (5, 5): [(5, 5, 1), (5, 5, 1), (5, 10, 2)],
            (40, 5): []}[b1, b2]
    return _checked(Case(f"bounds_{b1}_{b2}", seqs, k, b1, b2, n_distinct=sum(sizes), kept=kept, sizes=sizes))


def singletons(k, b2, n=200):
    """n sequences of exactly k bases: n components of one k-mer, b1 = 1; all tie, the order is the k-mers' own.  n = 3: over 8 ranks
    most ranks own nothing from the first level on"""
    rng = np.random.default_rng(3000 + k)
    seqs = [_rand(rng, k) for _ in range(n)]
    return _checked(Case(f"singletons_{n}_b2_{b2}", seqs, k, 1, b2, n_distinct=n, kept=[(1, 1, 1)] * n))


def long_path(k, whole):
    """one path of 30000 - k + 1 k-mers of value 2 (29 970 at k = 31), no cycle: one component that changes rank at every change of the
    minimizer.  whole: b2 above its size, it is kept as it is.  Else b2 below: too large at threshold 1, all of it goes on (value 2),
    too large at threshold 2, nothing goes on: no component, three levels"""
    rng = np.random.default_rng(4000 + k)
    s = _rand(rng, 30000)
    n = 30000 - k + 1
    b1, b2 = (1000, 40000) if whole else (1000, 10000)
    return _checked(Case("long_path_" + ("whole" if whole else "none"), [s, s], k, b1, b2, n_distinct=n, kept=[(n, 2 * n, 1)] if whole else [], levels=1 if whole else 3))


def ladder(k):
    """a backbone of 6000 bases whose inner stretches [500 (v - 1), 6000 - 500 (v - 1)) are listed again for v = 2 .. 6: the values step
    1, 2, .. 6 towards the middle, 6000 - 1000 (v - 1) - k + 1 k-mers have a value >= v.  b2 = 1200 lies between the 1970 (k = 31) of
    value >= 5 and the 970 of value 6: the large component is cut again at thresholds 1 .. 5 and kept at 6.  Islands (a stretch of the
    flank listed once or twice more) fall off on the way: two of 30 k-mers and one of 25 at threshold 2, 45 at 3, 40 at 4 (beside 10:
    fewer than b1, dropped), 60 at 5; a sequence of its own of 50 k-mers is kept at threshold 1."""
    rng = np.random.default_rng(5000 + k)
    L, b1, b2 = 6000, 20, 1200
    B = _rand(rng, L)
    seqs = [B] + [B[500 * (v - 1):L - 500 * (v - 1)] for v in range(2, 7)]
    islands = [(100, 30, 1), (5800, 30, 1), (300, 25, 2), (700, 45, 1), (1200, 10, 1), (1300, 40, 1), (1700, 60, 1)]     # (first k-mer, k-mers, times listed)
    for first, n, times in islands:
        seqs += [_stretch(B, first, n, k)] * times
    seqs.append(_rand(rng, 50 + k - 1))
    core = L - 5000 - k + 1
    kept = [(50, 50, 1), (30, 60, 2), (30, 60, 2), (25, 75, 2), (45, 135, 3), (40, 160, 4), (60, 300, 5), (core, 6 * core, 6)]
    return _checked(Case("ladder", seqs, k, b1, b2, n_distinct=L - k + 1 + 50, kept=sorted(kept, key=lambda c: (c[2], -c[1], -c[0])), levels=6,
                         dropped=_stretch(B, 1200, 10, k)))


def low_complexity(k):
    """runs of one base, of a period of 2 and of 4, and a cycle, each between random flanks of 40 bases: a k-mer that is its own
    neighbour (AAA..), k-mers that are their own reverse complement at even k (ATAT.., ACGTACGT.., AATTAATT..), a k-mer whose
    neighbour is its reverse complement (ATATA.. at odd k), values up to 90 - k + 1.  No hand-worked expectation: the oracle's"""
    rng = np.random.default_rng(6000 + k)
    cyc = _rand(rng, 76)
    cores = ["A" * 90, "AT" * 45, "ACGT" * 25, "AATT" * 25, cyc * 3]
    seqs = [_rand(rng, 40) + c + _rand(rng, 40) for c in cores]
    return Case("low_complexity", seqs, k, 1, 60)


SWEEP = {"ties": ties, "ladder": ladder, "low_complexity": low_complexity}              # the cases of the k sweep
OTHER = {f"bounds_{b1}_{b2}": (lambda k, b1=b1, b2=b2: bounds(k, b1, b2)) for b1, b2 in BOUNDS}      # the cases that run at k = 31 and k = 21 only
OTHER.update({"singletons_200_b2_1": lambda k: singletons(k, 1), "singletons_200_b2_10": lambda k: singletons(k, 10),
              "long_path_whole": lambda k: long_path(k, True), "long_path_none": lambda k: long_path(k, False)})
FEW = {"singletons_3_b2_1": lambda k: singletons(k, 1, n=3)}                                # three k-mers for a world of 8
CASES = {**SWEEP, **OTHER, **FEW}


def by_name(name, k):
    case = CASES[name](k)
    assert case.name == name
    return case
