"""comp2graph restated in Python: Comp2Graph.java (buildComponent, initStructures, mergePaths, mergeNodes) and GFAWriter.java
(generateOutput, printLabel, printEdge, normalizeDna), statement by statement, one component at a time.  The reference keeps the k-mers of
a component in a HashMap<String, Short> and numbers the nodes in its iteration order; here that order is a parameter, a permutation of
the distinct normalised k-mers.  canon() is the form in which two GFA texts are equal when they differ in names and line order only.
Also the values of ComponentsToGraph.java:85-102 and the builders of the test cases.

A k-mer is an int with two bits per base, A0 G1 C2 T3 (DnaTools.java:31); normalizeDna orders STRINGS (A < C < G < T), the library's
canonical form orders the codes, so the two pick different strands now and then -- both name the same k-mer."""
import collections
import random

import numpy as np

import comp2seq_ref as CR

MAX_COUNT = 32767


def normalize(s):
    """GFAWriter.normalizeDna"""
    rc = CR.rc_str(s)
    return s if s < rc else rc


class _Node:
    """algo/SingleNode.java"""

    def __init__(self, sequence, ident):
        self.sequence, self.id = sequence, ident
        self.rc = None
        self.neighbors = []
        self.deleted = False


def component_values(members, k, values=None):
    """Comp2Graph.buildComponent -> {normalised k-mer string: value}, in the order of first insertion.  values: {canonical k-mer: value}
    (all_kmers; a k-mer it does not hold is worth 0) or None (every k-mer 1).  A member is looked up by its canonical form: the
    reference looks up the member as listed, and the files it reads list canonical k-mers."""
    sub = {}
    for x in members:
        v = 1 if values is None else values.get(CR.canon(int(x), k), 0)
        sub[normalize(CR.decode(int(x), k))] = v
    return sub


def component_gfa(members, k, comp_id, values=None, order=None):
    """Comp2Graph.run for one component -> its GFA text.  order: the iteration order of `subgraph` (a list holding every distinct
    normalised k-mer once); None: insertion order.  Raises AssertionError where the reference's checkLabels does."""
    subgraph = component_values(members, k, values)
    keys = list(subgraph) if order is None else list(order)
    assert sorted(keys) == sorted(subgraph)
    # initStructures
    nodes = []
    for seq in keys:
        a, b = _Node(seq, len(nodes)), _Node(CR.rc_str(seq), len(nodes))
        a.rc, b.rc = b, a
        nodes += [a, b]
    by_kmer = {}
    for nd in nodes:
        by_kmer.setdefault(nd.sequence[:k - 1], []).append(nd)
    for nd in nodes:
        last = nd.sequence[1:]
        if last in by_kmer:
            nd.rc.neighbors.extend(by_kmer[last])

    def merge_labels(a, b):
        if a[len(a) - (k - 1):] != b[:k - 1]:
            raise AssertionError("Labels should be merged, but can not: " + a + " and " + b)
        return a + b[k - 1:]

    # mergePaths
    for _ in range(4 * len(nodes) + 4):
        acted = False
        for nd in nodes:
            if not nd.deleted and len(nd.neighbors) == 1:
                other = nd.neighbors[0]
                if len(other.neighbors) != 1:
                    continue
                first_plus, second_minus = nd, other                      # mergeNodes
                first_minus, second_plus = first_plus.rc, second_minus.rc
                new_seq = merge_labels(second_plus.sequence, first_plus.sequence)
                new_rc = merge_labels(first_minus.sequence, second_minus.sequence)
                second_plus.sequence, first_minus.sequence = new_seq, new_rc
                second_plus.rc, first_minus.rc = first_minus, second_plus
                first_plus.deleted = second_minus.deleted = True
                acted = True
        if not acted:
            break
    else:
        raise AssertionError("mergePaths does not end")

    # GFAWriter.generateOutput
    def node_id(nd):
        return f"{min(nd.rc.id, nd.id) + 1}_i{comp_id}"

    out = []
    for nd in nodes:
        if not nd.deleted and nd.sequence <= nd.rc.sequence:
            s = nd.sequence
            cov = sum(subgraph[normalize(s[i:i + k])] for i in range(len(s) - k + 1))
            cov += subgraph[normalize(s[len(s) - k:])] * (k - 1)
            out.append(f"S\t{node_id(nd)}\t{s}\tLN:i:{len(s)}\tKC:i:{cov}\n")
    for a in nodes:
        if not a.deleted:
            for b in a.neighbors:
                if not b.deleted:
                    out.append(f"L\t{node_id(a)}\t{'+' if a.sequence >= a.rc.sequence else '-'}\t{node_id(b)}\t"
                               f"{'+' if b.sequence <= b.rc.sequence else '-'}\t{k - 1}M\n")
    return "".join(out)


def gfa(comps, k, values=None, orders=None):
    """ComponentsToGraph.runImpl: the components' texts in file order"""
    return "".join(component_gfa(m, k, i, values, None if orders is None else orders[i]) for i, m in enumerate(comps))


def permuted_orders(comps, k, seed):
    rnd = random.Random(seed)
    out = []
    for m in comps:
        keys = list(component_values(m, k))
        rnd.shuffle(keys)
        out.append(keys)
    return out


def sample_values(tables, coverage):
    """ComponentsToGraph.java:85-102 over {canonical k-mer: count} per file (counts > 0): coverage -- IOUtils.loadKmers(files, 0), counts
    added and bounded at Short.MAX_VALUE; else the number of files that hold the k-mer"""
    out = {}
    for t in tables:
        for x, c in t.items():
            if c > 0:
                out[x] = min(out.get(x, 0) + (c if coverage else 1), MAX_COUNT)
    return out


# ---- the canonical form ----
def parse(text):
    """-> {component: ([(name, seq, LN, KC)], [(from, sign, to, sign, overlap)])}; raises ValueError on a malformed line, a name that
    is not <n>_i<c>, a link into another component or to a name without S line, or an S line after an L line of its component"""
    comps = collections.OrderedDict()
    if text and not text.endswith("\n"):
        raise ValueError("the text does not end with a newline")
    for ln in text.split("\n")[:-1]:
        f = ln.split("\t")
        if f[0] == "S" and len(f) == 5 and f[3].startswith("LN:i:") and f[4].startswith("KC:i:"):
            n, c = f[1].split("_i")
            segs, links = comps.setdefault(int(c), ([], []))
            if links:
                raise ValueError("S line after an L line of its component: " + ln)
            segs.append((f[1], f[2], int(f[3][5:]), int(f[4][5:])))
        elif f[0] == "L" and len(f) == 6 and f[2] in "+-" and f[4] in "+-":
            c = int(f[1].split("_i")[1])
            if int(f[3].split("_i")[1]) != c or c not in comps:
                raise ValueError("a link out of its component: " + ln)
            comps[c][1].append((f[1], f[2], f[3], f[4], f[5]))
        else:
            raise ValueError("not a line of this GFA: " + ln)
    for c, (segs, links) in comps.items():
        names = {s[0] for s in segs}
        for l in links:
            if l[0] not in names or l[2] not in names:
                raise ValueError(f"component {c}: link {l} names no segment")
    return comps


def canon(text):
    """{component: (sorted multiset of (min(seq, rc), LN, KC), sorted multiset of links with names replaced by printed sequences)}"""
    out = {}
    for c, (segs, links) in parse(text).items():
        seq_of = {s[0]: s[1] for s in segs}
        out[c] = (sorted((min(s[1], CR.rc_str(s[1])), s[2], s[3]) for s in segs),
                  sorted((seq_of[l[0]], l[1], seq_of[l[2]], l[3], l[4]) for l in links))
    return out


def parity(comps, k, values=None, seeds=range(8)):
    """per component: True when the restatement gives one canonical form under every seeded iteration order and never raises"""
    ok = []
    for i, m in enumerate(comps):
        forms = []
        try:
            for s in seeds:
                forms.append(canon(component_gfa(m, k, i, values, permuted_orders([m], k, s)[0])))
        except AssertionError:
            ok.append(False)
            continue
        ok.append(all(f == forms[0] for f in forms))
    return ok


def check_rules(text, k, n_comps):
    """the tool's own rules on any output: names dense from 1 per component, printed strand <= its reverse complement, LN = length, L
    lines sorted by (from, from sign, to, to sign) with '+' first, components in file order, S before L"""
    comps = parse(text)
    assert list(comps) == sorted(comps) and all(0 <= c < n_comps for c in comps), list(comps)
    for c, (segs, links) in comps.items():
        nums = []
        for name, seq, ln, kc in segs:
            assert seq <= CR.rc_str(seq), (c, name)
            assert ln == len(seq) and ln >= k, (c, name)
            n = int(name.split("_i")[0])
            if seq == CR.rc_str(seq):
                assert nums.count(n) <= 1                                # (the two S lines of a palindromic k-mer)
            else:
                assert n not in nums, (c, name)
            nums.append(n)
        assert sorted(set(nums)) == list(range(1, len(set(nums)) + 1)), (c, nums)
        assert nums == sorted(nums), (c, nums)
        keys = [(int(l[0].split("_i")[0]), "+-".index(l[1]), int(l[2].split("_i")[0]), "+-".index(l[3])) for l in links]
        assert keys == sorted(keys), c
        assert all(l[4] == f"{k - 1}M" for l in links)
    return comps


# ---- the cases: name -> (k, components as lists of k-mers, family) ; family: "plain", "cycle", "hairpin" ----
def _distinct(seq, k):
    km = CR.kmers_of(seq, k)
    return len(set(km)) == len(km)


def _search(rng, n_bases, k, ok):
    for _ in range(100000):
        s = CR._rand_seq(rng, n_bases)
        if _distinct(s, k) and ok(s):
            return s
    raise AssertionError("no such sequence")


def _no_pal(s, k):
    return all(s[i:i + k] != CR.rc_str(s[i:i + k]) for i in range(len(s) - k + 1))


def crafted():
    k = 5
    rng = np.random.default_rng(55)
    cases = {}
    plain = lambda s: _no_pal(s, k)
    cases["one"] = (k, [CR.kmers_of(_search(rng, 5, k, plain), k)], "plain")
    cases["path2"] = (k, [CR.kmers_of(_search(rng, 6, k, plain), k)], "plain")
    cases["path3"] = (k, [CR.kmers_of(_search(rng, 7, k, plain), k)], "plain")

    def rc_smaller(s):          # the walk starts on the smaller canonical k-mer (so it reads s), the printed strand is rc(s)
        km = CR.kmers_of(s, k)
        return plain(s) and CR.rc_str(s) < s and km[0] < km[-1] and CR.encode(s[:k]) == km[0]
    cases["rc_printed"] = (k, [CR.kmers_of(_search(rng, 9, k, rc_smaller), k)], "plain")
    cases["fork"] = (k, [CR.kmers_of("AACCGA", k) + CR.kmers_of("AACCGT", k)[1:]], "plain")
    cases["bubble"] = (k, [sorted(set(CR.kmers_of(BUBBLE[0], k) + CR.kmers_of(BUBBLE[1], k)))], "plain")
    p = CR.kmers_of(_search(rng, 10, k, plain), k)
    mask = (1 << (2 * k)) - 1
    rcs = lambda x: CR.encode(CR.rc_str(CR.decode(x, k)))
    cases["dups_noncanonical"] = (k, [[p[0], rcs(p[1]), p[1], p[2], p[2], rcs(p[3]), p[4], p[5], p[5] & mask]], "plain")
    a = _search(rng, 5, k, plain)
    cases["shared"] = (k, [CR.kmers_of("AC" + a + "TC", k) if _distinct("AC" + a + "TC", k) else CR.kmers_of(a, k),
                           CR.kmers_of("GA" + a + "CA", k) if _distinct("GA" + a + "CA", k) else CR.kmers_of(a, k)], "plain")
    cases["empty_between"] = (k, [CR.kmers_of(_search(rng, 7, k, plain), k), [], CR.kmers_of(_search(rng, 8, k, plain), k)], "plain")
    r31 = np.random.default_rng(31)
    trunk = CR._simple_path(r31, 6, 31)
    cases["k31"] = (31, [sorted(set(CR.kmers_of(trunk + "A" + CR._rand_seq(r31, 5), 31) + CR.kmers_of(trunk + "C" + CR._rand_seq(r31, 5), 31))),
                         CR.kmers_of(CR._simple_path(r31, 40, 31), 31)], "plain")
    cases["k4_palindrome"] = (4, [CR.kmers_of("GGACGTCA", 4)], "plain")                 # ACGT is its own reverse complement
    def circular(s):            # the 7 k-mers of a circular sequence of 7 bases, and 2 bases that lead into it
        c = (s[2:] * 2)[:7 + k - 1]
        return plain(s[:2] + c) and _distinct(s[:2] + c, k)
    s9 = _search(rng, 9, k, circular)
    cyc = (s9[2:] * 2)[:7 + k - 1]
    global CYCLE
    CYCLE = s9[2:]                                           # the circular sequence of the "cycle" case
    cases["cycle"] = (k, [CR.kmers_of(cyc, k)], "cycle")
    cases["cycle_tail"] = (k, [CR.kmers_of(s9[:2] + cyc, k)], "plain")
    # two paths in one component: A starts (as walked, from its end with the smaller canonical k-mer) on the reverse complement strand
    # of its start k-mer, B on the canonical strand, and canonical(A) < canonical(B) < oriented(A) in the 2-bit code: the names go by
    # (canonical start k-mer, strand), so A is 1 and B is 2 -- by the oriented k-mer it would be the other way round
    def walk(s):
        km = CR.kmers_of(s, k)
        return s if km[0] < km[-1] else CR.rc_str(s)
    global STRAND1
    for _ in range(100000):
        sa, sb = walk(_search(rng, 7, k, plain)), walk(_search(rng, 7, k, plain))
        ca, oa, cb, ob = CR.kmers_of(sa, k)[0], CR.encode(sa[:k]), CR.kmers_of(sb, k)[0], CR.encode(sb[:k])
        members = CR.kmers_of(sa, k) + CR.kmers_of(sb, k)
        if oa != ca and ob == cb and ca < cb < oa and len(set(members)) == 6:
            segs, links = parse(component_gfa(members, k, 0))[0]
            if len(segs) == 2 and not links:
                STRAND1 = (normalize(sa), normalize(sb))
                cases["strand1_start"] = (k, [members], "plain")
                break
    assert "strand1_start" in cases
    # a hairpin: ACATG is followed by its own reverse complement CATGT (a b c ~c ~b); two k-mers lead up to it
    cases["hairpin"] = (k, [CR.kmers_of("GGACATG", k)], "hairpin")
    return cases


CYCLE = None
STRAND1 = None                                               # the printed sequences of "strand1_start" in name order
BUBBLE = ("AAACCAGTGAA", "AAACCCGTGAA")       # AAACC, two branches of five k-mers, GTGAA; no 4-mer of them is its own reverse complement


def generated(O, L, n_reads=20000, seed=3, k=21, b1=190, b2=200):
    """reads of the benchmark's generator, counted and cut with small bounds by the CPU reference implementation (O) -> (k, components,
    [{canonical k-mer: count} of two samples: the halves of the reads])"""
    bases, off = L.synth_reads_host(seed, 0, 0, n_reads, 150, 40000)
    t = O.Table().count_buffer(bases, off, k)
    comps = [[int(x) for x in c[3]] for c in O.cut_components(t, k, b1, b2).all()]
    half = n_reads // 2
    samples = []
    for lo, hi in ((0, half), (half, n_reads)):
        st = O.Table().count_buffer(bases[lo * 150:hi * 150], off[lo:hi + 1] - off[lo], k)
        keys, vals = st.export(0)
        samples.append({int(x): int(v) for x, v in zip(keys, vals)})
    return k, comps, samples
