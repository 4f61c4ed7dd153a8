"""The unitig builder (metafast_amd/csrc/mf_unitig.hip) restated in plain Python for its tests: U1 (the info byte, ridx / lidx, pal) on top
of tests/nbr_ref.py, the layout of a table with made-up minimizer partitions, what the host of mf_ut_build must see on such a table (its
trace), and the crafted tables of tests/test_unitig_gpu.py.  The EXPECTED UNITIGS never come from here: they are the oracle's
(oracle.build_unitigs / wide_build_unitigs on the same (k-mer, count) pairs), which knows nothing of flags, nodes or jump words.
tests/test_ut_ref_cpu.py pins this file and asserts, case by case, the arithmetic that makes a case reach the path it was made for.

A k-mer is a Python int with two bits per base, the first base in the highest of its 2 k bits, complement = 3 - code (the library prints
code c as "AGCT"[c]; nothing here prints).  A node is 2 * index + strand (strand 1: the reverse complement of the canonical k-mer); a
palindromic k-mer (even k) has its strand-0 node only.

The constants of mf_unitig.hip this file mirrors, each once:"""
import functools

import numpy as np

import nbr_ref as NR

CHUNKS = (32, 128, 512, 4096)   # mf_unitig.hip: chunk_of() in mf_ut_build, "round == 0 ? 32 : round == 1 ? 128 : round == 2 ? 512 : UT_WALK_CHUNK" (4096)
J_MAXN = 1024                   # mf_unitig.hip: #define UT_J_MAXN 1024 (oriented nodes of a partition k_ut_contract takes into LDS: 512 k-mers)
J_ROUNDS = 11                   # mf_unitig.hip: k_ut_contract, "for (int round = 0; round < 11; round++)"
SEG = 192                       # mf_unitig.hip: #define UT_SEG 192u
PLAIN_MIN_N = 1 << 16           # mf_unitig.hip: "rounds_j = n >= (1u << 16) ? ..." (k_ut_jump_double runs from this many k-mers on)
CODE_NONE, CODE_MANY = 4, 5     # mf_unitig.hip: UT_CODE_NONE / UT_CODE_MANY
NONE = 0xFFFFFFFF               # mf_unitig.hip: UT_NONE
MAX_COUNT = 32767               # include/metafast_hip.h: MF_MAX_COUNT
TRACE_FIELDS = ("n_starts", "walk_rounds", "doubled", "entries", "double_rounds", "longest", "candidates", "paths", "seg_slots")     # mf_unitig.h: mf_ut_trace


# ---------------------------------------------------------------------------------------------------------------------------------
# k-mers
# ---------------------------------------------------------------------------------------------------------------------------------
def rc_plain(x, k):
    """reverse complement of one k-mer (any k), base by base"""
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def _rc_many(xs, k):
    """the same for a list of ints of up to 126 bits, on whole words (held against rc_plain in test_ut_ref_cpu.py)"""
    m64 = (1 << 64) - 1
    lo = np.array([x & m64 for x in xs], dtype=np.uint64)
    hi = np.array([x >> 64 for x in xs], dtype=np.uint64)
    rlo, rhi = NR.revcomp(lo, 32).tolist(), NR.revcomp(hi, 32).tolist()
    sh = 128 - 2 * k
    return [((a << 64) | b) >> sh for a, b in zip(rlo, rhi)]


def seq_kmers(seq, k):
    """seq: base codes -> (oriented k-mers as read, their canonical forms), lists of ints, by rolling both strands"""
    seq = [int(c) for c in seq]
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    fw = rc = 0
    out, can = [], []
    for i, c in enumerate(seq):
        fw = ((fw << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << top)
        if i >= k - 1:
            out.append(fw)
            can.append(min(fw, rc))
    return out, can


def revcomp_seq(seq):
    return (3 - np.asarray(seq, dtype=np.uint8))[::-1]


def split_words(keys):
    """list of ints -> (low words, high words) uint64"""
    m64 = (1 << 64) - 1
    return np.array([x & m64 for x in keys], dtype=np.uint64), np.array([x >> 64 for x in keys], dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------------
# U1
# ---------------------------------------------------------------------------------------------------------------------------------
def _neighbours_wide(keys, k):
    """nbr_ref.neighbours(..., with_strand=True) for k-mers of any width: a neighbour is built from the k-mer by a shift, its canonical form from a full
    reverse complement, its place from a dictionary"""
    keys = [int(x) for x in keys]
    n = len(keys)
    where = {x: i for i, x in enumerate(keys)}
    assert len(where) == n, "the keys of a table are all different"
    mask, top = (1 << (2 * k)) - 1, 2 * k - 2
    nbr = np.full((n, 8), NONE, dtype=np.uint32)
    strand = np.zeros((n, 8), dtype=bool)
    for nuc in range(4):
        for side in (0, 1):
            ys = [((x << 2) | nuc) & mask for x in keys] if side == 0 else [(x >> 2) | (nuc << top) for x in keys]
            for i, (y, r) in enumerate(zip(ys, _rc_many(ys, k))):
                j = where.get(min(y, r))
                if j is not None:
                    nbr[i, 2 * nuc + side] = j
                strand[i, 2 * nuc + side] = r < y
    return nbr, strand


def flags(keys, k):
    """HashMapOperations.getRightNucleotide / getLeftNucleotide for every canonical k-mer of a table (keys in table order), as k_ut_flags leaves
    them: -> (info uint8[n], ridx uint32[n], lidx uint32[n], pal uint8[n]).  info = rcode | lcode << 3 | ror << 6 | lor << 7; a code is the
    only present nucleotide of its side, 4 where there is none, 5 where there are several; ridx / ror (lidx / lor) are the table position and
    the strand (1: the table holds the reverse complement) of the FIRST present neighbour of the side, NONE / 0 where there is none"""
    if k <= 31:
        karr = np.asarray(keys, dtype=np.uint64)
        nbr, strand = NR.neighbours(karr, k, with_strand=True)
        pal = (NR.revcomp(karr, k) == karr).astype(np.uint8)
    else:
        nbr, strand = _neighbours_wide(keys, k)
        pal = np.array([int(r == x) for x, r in zip(keys, _rc_many([int(x) for x in keys], k))], dtype=np.uint8)
    n = len(nbr)
    rows = np.arange(n)
    out = []
    for side in (0, 1):
        present = nbr[:, side::2] != NONE
        cnt = present.sum(axis=1)
        first = present.argmax(axis=1)
        code = np.where(cnt == 0, CODE_NONE, np.where(cnt == 1, first, CODE_MANY)).astype(np.uint8)
        idx = np.where(cnt > 0, nbr[rows, 2 * first + side], NONE).astype(np.uint32)
        orient = np.where(cnt > 0, strand[rows, 2 * first + side], False).astype(np.uint8)
        out.append((code, idx, orient))
    (rcode, ridx, ror), (lcode, lidx, lor) = out
    info = (rcode | (lcode << 3) | (ror << 6) | (lor << 7)).astype(np.uint8)
    return info, ridx, lidx, pal


# ---------------------------------------------------------------------------------------------------------------------------------
# U2: links between oriented nodes
# ---------------------------------------------------------------------------------------------------------------------------------
def links(info, ridx, lidx, pal):
    """-> (succ: list, node -> node or None; starts: sorted list of nodes without an incoming link).  A link f -> g exists iff the right
    neighbour of f is unique, it is g, and the left neighbour of g is unique (task.run :52-69)"""
    info, ridx, lidx = [int(x) for x in info], [int(x) for x in ridx], [int(x) for x in lidx]
    pal = [int(x) for x in pal] if pal is not None else [0] * len(info)
    n = len(info)

    def node(i, s):
        return 2 * i + (0 if pal[i] else s)

    def r_unique(f):
        b = info[f >> 1]
        return ((b >> 3) if f & 1 else b) & 7 < 4

    def l_unique(f):
        b = info[f >> 1]
        return (b if f & 1 else (b >> 3)) & 7 < 4

    def right(f):
        i, b = f >> 1, info[f >> 1]
        return node(lidx[i], ((b >> 7) & 1) ^ 1) if f & 1 else node(ridx[i], (b >> 6) & 1)

    succ = [None] * (2 * n)
    has_in = [False] * (2 * n)
    exists = [not (f & 1 and pal[f >> 1]) for f in range(2 * n)]
    for f in range(2 * n):
        if exists[f] and r_unique(f):
            g = right(f)
            if l_unique(g):
                succ[f] = g
                assert not has_in[g], "two links into one node"
                has_in[g] = True
    starts = [f for f in range(2 * n) if exists[f] and not has_in[f]]
    return succ, starts, right, r_unique


# ---------------------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------------------
def layout(keys, assignment, part_bits=None):
    """keys (any order), assignment[i] = the partition of keys[i] (or None: a table without partitions, the order as given).  -> (order: the
    positions of `keys` in table order -- partitions ascending, inside a partition the order given --, part_bits, offsets uint64[2^part_bits + 1]
    or None).  Partitions nobody is assigned to are empty."""
    if assignment is None:
        return np.arange(len(keys)), 0, None
    a = np.asarray(assignment, dtype=np.int64)
    assert len(a) == len(keys) and (len(a) == 0 or a.min() >= 0)
    top = int(a.max()) + 1 if len(a) else 1
    bits = max(1, (top - 1).bit_length())
    if part_bits is not None:
        assert part_bits >= bits
        bits = part_bits
    order = np.argsort(a, kind="stable")
    off = np.zeros((1 << bits) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.bincount(a, minlength=1 << bits))
    return order, bits, off


# ---------------------------------------------------------------------------------------------------------------------------------
# what mf_ut_build must see: jump words, walks, doubling, emission, segments
# ---------------------------------------------------------------------------------------------------------------------------------
def jump_words(succ, n, off, plain_rounds):
    """per node (target, hops, end) by the words' DEFINITION (k_ut_contract's comment): with partitions of at most J_MAXN nodes the chain is
    followed while it stays inside the node's partition -- end: it stops there, target = its last node; else target = the first node
    outside --, a larger partition and a table without partitions give one hop per word; without partitions and from PLAIN_MIN_N k-mers
    on, plain_rounds times word := word followed by its target's word.  A chain that closes inside its partition has no such word: None."""
    nn = 2 * n
    words = [None] * nn
    if off is not None:
        sizes = np.diff(off.astype(np.int64))
        part = np.repeat(np.arange(len(sizes)), sizes).tolist()
        small = (2 * sizes <= J_MAXN).tolist()
        for f in range(nn):
            p = part[f >> 1]
            e, h, m = f, 0, 2 * int(sizes[p])
            if small[p]:
                while succ[e] is not None and part[succ[e] >> 1] == p and h <= m:
                    e, h = succ[e], h + 1
                if h > m:
                    continue                                # a cycle closed inside the partition (a chain has fewer hops than the partition nodes)
            words[f] = (e, h, True) if succ[e] is None else (succ[e], h + 1, False)
        return words
    for f in range(nn):
        words[f] = (f, 0, True) if succ[f] is None else (succ[f], 1, False)
    if n >= PLAIN_MIN_N:
        for _ in range(max(0, min(int(plain_rounds), 8))):
            words = [w if w[2] else (words[w[0]][0], w[1] + words[w[0]][1], words[w[0]][2]) for w in words]
    return words


def predict(info, ridx, lidx, pal, keys, k, off, min_len, double_after=4, plain_rounds=3):
    """-> dict: the fields of mf_ut_trace (double_rounds as an interval, see below) plus, per start, the jump words its walk reads, the
    longest word, and per written path its nodes and its segments under the cutter that runs (and the slots that stay empty).

    double_rounds: the rounds of k_utd_double run IN PLACE, so a word spans AT LEAST twice as much after every round (more where a thread
    reads a word another thread has already doubled in this round).  The host looks after every third round whether every unfinished walk
    reads its end in one word: surely once 8^t >= the entry steps such a walk still has to go, perhaps earlier; then it goes on to
    need + 1 rounds, 2^need >= longest hops + 2.  Hence lo = max(3, need + 1), hi = max(3 t_sure, need + 1)."""
    n = len(info)
    succ, starts, right, r_unique = links(info, ridx, lidx, pal)
    words = jump_words(succ, n, off, plain_rounds)
    pal = [0] * n if pal is None else [int(x) for x in pal]
    keys = [int(x) for x in keys]
    walks = []                                              # per start: (start, end node, hops, words read)
    for s in starts:
        f, d, nw = s, 0, 0
        while True:
            t, h, end = words[f]
            f, d, nw = t, d + h, nw + 1
            if end:
                break
        walks.append((s, f, d, nw))
    nwords = [w[3] for w in walks]
    rounds, cum, doubled = (1 if starts else 0), CHUNKS[0], False
    while starts and max(nwords) > cum:
        if rounds >= double_after:
            doubled = True
            break
        cum += CHUNKS[min(rounds, 3)]
        rounds += 1
    res = dict(n_starts=len(starts), walk_rounds=rounds, doubled=int(doubled), entries=0, double_rounds=(0, 0), longest=0,
               words=sorted(nwords), longest_word=max([w[1] for w in words if w is not None], default=0),
               unsettled=sum(w is None for w in words), pal_starts=sum(pal[s >> 1] for s in starts))
    entries = set()
    if doubled:
        assert res["unsettled"] == 0, "the entry count of a cycle closed inside a partition is not defined by the words"
        entries = {w[0] for w in words if not w[2]}
        longest = max(w[2] for w in walks)
        need = 1
        while need < 32 and (1 << need) < longest + 2:
            need += 1
        togo = max(nw - cum for nw in nwords if nw > cum)
        t_sure = 1
        while 8 ** t_sure < togo:
            t_sure += 1
        res.update(entries=len(entries), longest=longest + 1, double_rounds=(max(3, need + 1), max(3 * t_sure, need + 1)))
    # U4: the emission rule
    cands, eqmin = [], {}
    for s, f, d, nw in walks:
        if d + k < min_len:
            continue
        ei = (right(f) >> 1) if r_unique(f) else (f >> 1)
        st, en = keys[s >> 1], keys[ei]
        if st > en:
            continue
        eq = st == en
        if eq:
            eqmin[s >> 1] = min(eqmin.get(s >> 1, s), s)
        cands.append((s, d, eq, bool(pal[s >> 1]) and not eq))
    res["candidates"] = sum(2 if tw else 1 for _, _, _, tw in cands)
    res["twice"] = sum(1 for _, _, _, tw in cands if tw)
    paths = []
    for s, d, eq, tw in cands:
        if eq and eqmin[s >> 1] != s:
            continue
        paths += [(s, d + 1)] * (2 if tw else 1)
    res["paths"] = len(paths)
    res["seg_slots"] = sum(nodes // SEG + 1 for _, nodes in paths)     # k_ut_seg_bound: nodes / 192 + 1
    segs = []
    for s, nodes in paths:
        if doubled:                                         # k_utd_cuts: the first entry in every stretch of SEG nodes, and the start
            slots, f, d = {0}, s, 0
            while succ[f] is not None:
                f, d = succ[f], d + 1
                if f in entries:
                    slots.add(d // SEG)
            segs.append(len(slots))
        else:                                               # k_ut_segments: a cut at the first word end SEG nodes or more after the last cut
            f, d, last, cuts = s, 0, 0, 0
            while not words[f][2]:
                t, h, _ = words[f]
                f, d = t, d + h
                if d - last >= SEG:
                    cuts, last = cuts + 1, d
            segs.append(cuts + 1)
    res["path_nodes"] = [nodes for _, nodes in paths]
    res["path_nodes_sorted"] = sorted(res["path_nodes"])
    res["segments"] = segs
    res["segments_sorted"] = sorted(segs)
    res["sizes"] = [] if off is None else np.diff(off.astype(np.int64)).tolist()
    res["empty_slots"] = res["seg_slots"] - sum(segs)
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# the crafted tables
# ---------------------------------------------------------------------------------------------------------------------------------
class Case:
    """keys: canonical k-mers in table order; counts; off / part_bits: the partitions (None / 0: none); settings: the
    (ut_double_after, ut_plain_rounds) pairs it runs under; want: what test_ut_ref_cpu.py asserts of predict() per setting"""

    def __init__(self, name, k, keys, counts, part_bits=0, off=None, min_len=None, settings=((4, 3),), want=None, nseq=None):
        self.name, self.k, self.keys, self.counts = name, k, [int(x) for x in keys], np.asarray(counts, dtype=np.uint16)
        self.part_bits, self.off, self.min_len = part_bits, off, k if min_len is None else min_len
        self.settings, self.want, self.nseq = tuple(settings), want or {}, nseq
        assert len(set(self.keys)) == len(self.keys) == len(self.counts)

    @functools.cached_property
    def flags(self):
        return flags(self.keys, self.k)

    def pal(self):
        return self.flags[3] if self.k % 2 == 0 else None

    @functools.lru_cache(maxsize=None)
    def predict(self, double_after=4, plain_rounds=3):
        info, ridx, lidx, _ = self.flags
        return predict(info, ridx, lidx, self.pal(), self.keys, self.k, self.off, self.min_len, double_after, plain_rounds)

    def oracle_unitigs(self, oracle):
        """-> (the oracle's sequences, its census)"""
        if self.k <= 31:
            t = oracle.Table()
            for x, c in zip(self.keys, self.counts.tolist()):
                t.add(x, c)
            return oracle.build_unitigs(t, self.k, 0, self.min_len).all(), oracle.unitig_census()
        t = oracle.WTable()
        for x, c in zip(self.keys, self.counts.tolist()):
            t.add(x, c)
        return oracle.wide_build_unitigs(t, self.k, 0, self.min_len).all(), oracle.wide_unitig_census()


class _Builder:
    """collects sequences: every k-mer of a sequence gets the partition its `assign` names (a function of the k-mer's position along the
    sequence, or a list), the order inside a partition is the order of arrival unless `order` says otherwise"""

    def __init__(self, k, seed, parts=True):
        self.k, self.rng, self.parts = k, np.random.default_rng(seed), parts
        self.keys, self.part, self.cnt, self.where = [], [], [], {}
        self.next_part = 0

    def new_parts(self, count):
        p = self.next_part
        self.next_part += count
        return p

    def random_seq(self, nodes):
        return self.rng.integers(0, 4, size=nodes + self.k - 1, dtype=np.uint8)

    def add(self, seq, assign=None, counts=None, order="asc"):
        """-> the positions (in arrival order) of the sequence's canonical k-mers, one per node, a k-mer met before keeps its place"""
        _, can = seq_kmers(seq, self.k)
        idx = list(range(len(can)))
        if order == "desc":
            idx.reverse()
        elif order == "perm":
            idx = self.rng.permutation(len(can)).tolist()
        for j in idx:
            x = can[j]
            if x in self.where:
                continue
            self.where[x] = len(self.keys)
            self.keys.append(x)
            self.part.append(0 if assign is None else int(assign(j) if callable(assign) else assign[j]))
            self.cnt.append(int(self.rng.integers(2, 60)) if counts is None else int(counts[j]))
        return [self.where[x] for x in can]

    def alternate(self, nodes, per=800):
        """an assignment that puts consecutive k-mers into different partitions (every jump word is one hop), at most per / 2 k-mers each"""
        base = self.new_parts(2 * ((nodes + per - 1) // per))
        return lambda j: base + 2 * (j // per) + (j & 1)

    def blocks(self, nodes, size):
        """... `size` consecutive k-mers per partition"""
        base = self.new_parts((nodes + size - 1) // size)
        return lambda j: base + j // size

    def case(self, name, **kw):
        order, bits, off = layout(self.keys, self.part if self.parts else None)
        keys = [self.keys[i] for i in order]
        cnt = [self.cnt[i] for i in order]
        return Case(name, self.k, keys, cnt, part_bits=bits, off=off, **kw)


def self_rc_seq(rng, length):
    """a sequence equal to its own reverse complement (even length)"""
    assert length % 2 == 0
    h = rng.integers(0, 4, size=length // 2, dtype=np.uint8)
    return np.concatenate([h, revcomp_seq(h)])


def case_border(order):
    """a. one whole path in a partition of exactly 512 k-mers (1024 nodes: pointer jumping in LDS, one word of 511 hops per strand) and one in a
    partition of 513 (one hop per word), laid out ascending along the path, descending or permuted"""
    b = _Builder(21, 200)
    for nodes in (512, 513):
        p = b.new_parts(1)
        b.add(b.random_seq(nodes), assign=lambda j, p=p: p, order=order)
    return b.case(f"border_512_513_{order}", nseq=2, want={(4, 3): dict(sizes=[512, 513], words=[1, 1, 513, 513], longest_word=511, walk_rounds=3, doubled=0)})


def case_longest_chain(split):
    """b. a sequence of 1023 + k bases equal to its reverse complement, k odd: 512 canonical k-mers, ONE chain of 1024 nodes through both
    strands of each; in one partition that is 1023 hops in one word; start and end are the two strands of one k-mer (the equal case)"""
    k = 21
    b = _Builder(k, 101)
    seq = self_rc_seq(b.rng, 1023 + k)
    if split:                                               # the k-mers of the first and of the last quarter of the chain / of its middle half
        b.add(seq, assign=lambda j: int(256 <= j < 768))
        want = dict(sizes=[256, 256], words=[3], longest_word=512, walk_rounds=1, doubled=0, candidates=1, paths=1, path_nodes=[1024])
    else:
        b.add(seq, assign=lambda j: 0, order="perm")
        want = dict(sizes=[512, 0], words=[1], longest_word=1023, walk_rounds=1, doubled=0, candidates=1, paths=1, path_nodes=[1024])
    return b.case("longest_chain_" + ("split" if split else "one_word"), nseq=1, want={(4, 3): want})


def _cycle_seq(b, c):
    s = b.rng.integers(0, 4, size=c, dtype=np.uint8)
    return np.resize(s, c + b.k - 1)


def case_cycle_inside():
    """c. an isolated cycle of 150 k-mers closed inside a partition that also holds a path of 200: the cycle's chains never settle (300 nodes,
    their words say nothing), nobody walks them, the path is one word"""
    b = _Builder(21, 102)
    b.add(_cycle_seq(b, 150), assign=lambda j: 0)
    b.add(b.random_seq(200), assign=lambda j: 0)
    b.add(b.random_seq(40), assign=lambda j: 1)
    return b.case("cycle_inside_a_partition", nseq=2, want={(4, 3): dict(sizes=[350, 40], words=[1, 1, 1, 1], unsettled=300, doubled=0, paths=2)})


def case_cycle_across():
    """c. an isolated cycle of 100 k-mers alternating between two partitions in a table where a path of 100 words starts the doubling
    (ut_double_after = 1): the cycle's 200 nodes are entries for ever, no path's"""
    b = _Builder(21, 103)
    b.add(_cycle_seq(b, 100), assign=b.alternate(100))
    b.add(b.random_seq(100), assign=b.alternate(100))
    return b.case("cycle_across_partitions", nseq=1, settings=((1, 3), (4, 3)),
                  want={(1, 3): dict(words=[100, 100], doubled=1, entries=200 + 2 * 99, paths=1), (4, 3): dict(doubled=0, walk_rounds=2, paths=1)})


WALK_WORDS = (1, 2, 32, 33, 160, 161, 672, 673, 4768)


def case_walk_rounds(extra):
    """d. paths whose walks read exactly 1, 2, 32, 33, 160, 161, 672, 673 and 4768 words (every k-mer in another partition than the next): the
    borders of the chunked rounds; with `extra` one of 4769, which the fourth round leaves unfinished"""
    b = _Builder(23, 104)
    lens = WALK_WORDS + ((4769,) if extra else ())
    for nodes in lens:
        b.add(b.random_seq(nodes), assign=b.alternate(nodes))
    words = sorted(list(lens) * 2)
    ent = sum(2 * (n - 1) for n in lens)
    want = {(1, 3): dict(words=words, walk_rounds=1, doubled=1, entries=ent),
            (4, 3): dict(words=words, walk_rounds=4, doubled=int(extra), entries=ent if extra else 0),
            (64, 3): dict(words=words, walk_rounds=5 if extra else 4, doubled=0, entries=0)}
    return b.case("walk_rounds" + ("_4769" if extra else ""), nseq=len(lens), settings=((1, 3), (4, 3), (64, 3)), want=want)


SEG_NODES = (1, 191, 192, 193, 384, 385, 1000)


def case_segments(variant):
    """e. paths of 1, 191, 192, 193, 384, 385 and 1000 nodes: `hop` every word one hop, `p100` partitions of 100 k-mers along the path (a cut
    can fall on every 100th node only: segments of 200), `p512` of 512 (words of 511 hops: the doubled cutter's slots 1 and 2 of the 1000-node
    path stay empty); one more path of 40 one-hop words, so that ut_double_after = 1 brings the doubled cutter"""
    b = _Builder(21, 105 + len(variant))
    for nodes in SEG_NODES:
        assign = b.alternate(nodes) if variant == "hop" else b.blocks(nodes, 100 if variant == "p100" else 512)
        b.add(b.random_seq(nodes), assign=assign)
    b.add(b.random_seq(40), assign=b.alternate(40))
    nodes = sorted(SEG_NODES + (40,))
    walk = {"hop": [1, 1, 1, 2, 2, 3, 6], "p100": [1, 1, 1, 1, 2, 2, 5], "p512": [1, 1, 1, 1, 1, 1, 2]}[variant]
    dbl = {"hop": [1, 1, 1, 2, 2, 3, 6], "p100": [1, 1, 1, 1, 2, 2, 5], "p512": [1, 1, 1, 1, 1, 1, 2]}[variant]
    want = {(4, 3): dict(doubled=0, path_nodes_sorted=nodes, segments_sorted=sorted(walk + [1])),
            (1, 3): dict(doubled=1, path_nodes_sorted=nodes, segments_sorted=sorted(dbl + [1]))}
    return b.case("segments_" + variant, nseq=len(SEG_NODES) + 1, settings=((4, 3), (1, 3)), want=want)


def case_alignment():
    """f. 320 paths of 1 .. 40 nodes in a table without partitions: the offsets of the paths and of their first hop take every residue mod 8
    (the aligned 8-byte stores of k_ut_walk2 at path borders), under both cutters"""
    b = _Builder(21, 109, parts=False)
    for i in range(320):
        b.add(b.random_seq(1 + i % 40))
    return b.case("store_alignment", nseq=320, settings=((4, 3), (1, 3)), want={(4, 3): dict(doubled=0, paths=320), (1, 3): dict(doubled=1, paths=320)})


def case_weights():
    """g. one path of 1000 one-hop nodes with the counts MF_MAX_COUNT and 1 in different segments (sum, min and max meet by atomics) and one of
    1000 nodes, all MF_MAX_COUNT (the largest sum)"""
    b = _Builder(21, 110)
    cnt = b.rng.integers(2, 60, size=1000)
    cnt[[5, 700]] = MAX_COUNT
    cnt[300] = 1
    b.add(b.random_seq(1000), assign=b.alternate(1000), counts=cnt)
    b.add(b.random_seq(1000), assign=b.blocks(1000, 100), counts=[MAX_COUNT] * 1000)
    return b.case("weights", nseq=2, settings=((4, 3), (1, 3)), want={(4, 3): dict(doubled=0, segments_sorted=[5, 6]), (1, 3): dict(doubled=1, segments_sorted=[5, 6])})


def _twice_case(k, seed):
    """h. A path of 420 nodes the reference prints from BOTH ends: either walk stops ON the k-mer beyond the path (that one has two left
    neighbours: the path's end and a tip), and canon(start) <= canon(that k-mer) holds both ways.  main = 9 bases + stem + 9 bases, a tip
    joining the k-mer after the stem, a tip leaving the k-mer before it; seeds are tried until the rule says twice"""
    for s in range(seed, seed + 200):
        b = _Builder(k, s)
        r = lambda m: b.rng.integers(0, 4, size=m, dtype=np.uint8)
        main = r(9 + 420 + k - 1 + 9)
        A, B = main[9:9 + k], main[9 + 419:9 + 419 + k]
        tip_r = np.concatenate([r(8), [(B[0] + 1) & 3], B[1:], main[9 + 419 + k:9 + 419 + k + 1]])
        tip_l = np.concatenate([main[8:9], A[:-1], [(A[-1] + 1) & 3], r(8)])
        b.add(main, assign=b.blocks(len(main) - k + 1, 150))
        for t in (tip_r, tip_l):
            b.add(t, assign=b.blocks(len(t) - k + 1, 150))
        b.add(b.random_seq(100), assign=b.alternate(100))  # (brings the doubled cutter under ut_double_after = 1)
        c = b.case(f"printed_twice_k{k}", settings=((4, 3), (1, 3)))
        if c.predict(4, 3)["path_nodes"].count(420) == 2:
            c.want = {(4, 3): dict(doubled=0), (1, 3): dict(doubled=1)}
            return c
    raise AssertionError("no seed gives a path printed twice")


def case_twice(k):
    return _twice_case(k, 1000 + k)


def case_palindromic_start(k):
    """h. A palindromic start k-mer P (even k) -- the `twice` of k_ut_ends, the second copy of k_utd_cuts.  P's right neighbours are the reverse
    complements of its left neighbours, so P has a unique right neighbour x exactly when it has a unique left one, rc(x); the link P -> x needs
    L(x) unique, and P is a start only if R(rc(x)) is NOT unique -- which is the same statement about the same k-mer.  A palindromic start
    therefore ALWAYS heads a path of exactly one node: the path `a palindromic start k-mer, more than 400 nodes` does not exist.  What exists
    is built here: P with one right neighbour x that has a second left neighbour (P is a start, printed twice: the walk stops on x, and
    canon(P) <= canon(x) where the seed is chosen so), next to a path of 420 nodes THROUGH a palindrome (printed once, 839 nodes)
    and a path of 100 one-hop words for the doubled cutter"""
    for s in range(2000 + k, 2200 + k):
        b = _Builder(k, s)
        h = b.rng.integers(0, 4, size=k // 2, dtype=np.uint8)
        pal = np.concatenate([h, revcomp_seq(h)])
        x_tail = b.rng.integers(0, 4, size=30, dtype=np.uint8)
        other = np.concatenate([b.rng.integers(0, 4, size=12, dtype=np.uint8), pal[1:], x_tail])
        other[11] = (pal[0] + 1) & 3                        # a second left neighbour of x = pal[1:] + x_tail[0]
        b.add(np.concatenate([pal, x_tail]), assign=b.blocks(31, 150))
        b.add(other, assign=b.blocks(len(other) - k + 1, 150))
        h2 = b.rng.integers(0, 4, size=k // 2, dtype=np.uint8)
        ext = b.rng.integers(0, 4, size=419, dtype=np.uint8)
        through = np.concatenate([revcomp_seq(ext), h2, revcomp_seq(h2), ext])
        b.add(through, assign=b.blocks(len(through) - k + 1, 150))
        b.add(b.random_seq(100), assign=b.alternate(100))
        c = b.case(f"palindromic_start_k{k}", settings=((4, 3), (1, 3)))
        p = c.predict(4, 3)
        if p["twice"] == 1 and 839 in p["path_nodes"]:
            _, can = seq_kmers(pal, k)
            c.pal_kmer = can[0]
            c.want = {(4, 3): dict(doubled=0), (1, 3): dict(doubled=1)}
            return c
    raise AssertionError("no seed gives a palindromic start printed twice")


def case_wide(k, big):
    """i. 2k-bit k-mers (two words), no partitions.  Small: below 2^16 k-mers, one hop per word.  Big: about 70 000 k-mers with a path of 5500
    nodes, under ut_plain_rounds 0 / 3 / 8 (a word spans 1 / 8 / 256 steps: 5500 / 688 / 22 words -- with 0 the walks outlast the fourth round
    and the doubling starts)"""
    b = _Builder(k, 120 + k + big, parts=False)
    if not big:
        for nodes in (1, 2, 191, 192, 193, 385, 1000, 37):
            b.add(b.random_seq(nodes))
        b.add(_cycle_seq(b, 100))
        return b.case(f"wide_k{k}_small", nseq=8, settings=((4, 3), (1, 3)), want={(4, 3): dict(doubled=0, paths=8, walk_rounds=4), (1, 3): dict(doubled=1, paths=8)})
    lens = [5500] + [1000] * 64 + [100] * 5
    for nodes in lens:
        b.add(b.random_seq(nodes))
    b.add(_cycle_seq(b, 100))
    w = lambda r: sorted(2 * [-(-n // (1 << r)) for n in lens])
    want = {(4, 0): dict(doubled=1, words=w(0), walk_rounds=4), (4, 3): dict(doubled=0, words=w(3), walk_rounds=4), (4, 8): dict(doubled=0, words=w(8), walk_rounds=1)}
    return b.case(f"wide_k{k}_big", nseq=len(lens), settings=((4, 0), (4, 3), (4, 8)), want=want)


CASES = {}
for _o in ("asc", "desc", "perm"):
    CASES[f"a_border_{_o}"] = functools.partial(case_border, _o)
CASES["b_longest_chain_one_word"] = functools.partial(case_longest_chain, False)
CASES["b_longest_chain_split"] = functools.partial(case_longest_chain, True)
CASES["c_cycle_inside"] = case_cycle_inside
CASES["c_cycle_across"] = case_cycle_across
CASES["d_walk_rounds"] = functools.partial(case_walk_rounds, False)
CASES["d_walk_rounds_4769"] = functools.partial(case_walk_rounds, True)
for _v in ("hop", "p100", "p512"):
    CASES[f"e_segments_{_v}"] = functools.partial(case_segments, _v)
CASES["f_store_alignment"] = case_alignment
CASES["g_weights"] = case_weights
for _k in (22, 26):
    CASES[f"h_printed_twice_k{_k}"] = functools.partial(case_twice, _k)
    CASES[f"h_palindromic_start_k{_k}"] = functools.partial(case_palindromic_start, _k)
for _k in (33, 47, 63):
    CASES[f"i_wide_k{_k}_small"] = functools.partial(case_wide, _k, False)
    CASES[f"i_wide_k{_k}_big"] = functools.partial(case_wide, _k, True)

_built = {}


def get_case(name):
    """built once per process, never changed"""
    if name not in _built:
        _built[name] = CASES[name]()
    return _built[name]


def random_assignments(n, seed):
    """j. four partition assignments of a table of n k-mers: none, one partition, random sizes with empty partitions and one above 512, every
    k-mer alone"""
    rng = np.random.default_rng(seed)
    nparts = 256
    p = rng.random(nparts) ** 3
    p[rng.choice(nparts, size=40, replace=False)] = 0       # empty ones
    p[7] = p.sum() * 0.05                                   # one with a twentieth of the table
    a = rng.choice(nparts, size=n, p=p / p.sum())
    return {"none": None, "one": np.zeros(n, dtype=np.int64), "random": a, "alone": np.arange(n, dtype=np.int64)}
