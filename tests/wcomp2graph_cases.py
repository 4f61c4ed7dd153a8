"""The cases of comp2graph on wide components (32 <= k <= 63; tests/test_wcomp2graph_cpu.py, tests/test_wcomp2graph_gpu.py).  Members are
Python ints, ascending inside a component as the wide loader demands; they are written with wcomp2seq_ref.write_components, sample files
with wide_files_ref.encode_kmers (wcomp2seq_ref.kmers_bin).  tests/comp2graph_ref.py, the restatement of Comp2Graph.java / GFAWriter.java
on strings and Python ints, holds for any k as it stands and is the reference here too.

crafted() -> {name: (k, components, family)}; family "plain": compared with comp2graph_ref.gfa; "cycle", "hairpin": the stated rule."""
import numpy as np

import comp2graph_ref as G
import comp2seq_ref as R
import wcomp2seq_ref as W

# ---- the two hand-worked cases at k = 33 (A0 G1 C2 T3; names by canonical start k-mer) ----
# a path of three 33-mers: 35 bases.  Its reverse complement starts with AC.., the sequence itself with AG..: the reverse complement is printed
PATH3 = "AGCATTGACCGTAGGCTTACGATCCGATTAGCAGT"
PATH3_TEXT = "S\t1_i0\tACTGCTAATCGGATCGTAAGCCTACGGTCAATGCT\tLN:i:35\tKC:i:35\n"
# a fork: the trunk 33-mer and its two successors, trunk[1:] + A and trunk[1:] + C.
#   trunk  ACGG..CCA   reverse complement TGGA..: below it in both orders -- canonical and printed as written; A (0) first: segment 1
#   + A    CGGA..CAA   reverse complement TTGG..: below it in both orders -- canonical and printed as written
#   + C    CGGA..CAC   reverse complement GTGG..: string order C < G, printed as written; code order G (1) < C (2), canonical GTGG..
# The names go by the canonical k-mer in code order: GTGG.. (+ C) is segment 2, CGGA.. (+ A) segment 3.
FORK_TRUNK = "ACGGATTCAGCATTGACCTTAGGCATCGATCCA"
FORK_A = FORK_TRUNK[1:] + "A"
FORK_C = FORK_TRUNK[1:] + "C"
FORK_TEXT = ("S\t1_i0\t" + FORK_TRUNK + "\tLN:i:33\tKC:i:33\n" "S\t2_i0\t" + FORK_C + "\tLN:i:33\tKC:i:33\n" "S\t3_i0\t" + FORK_A + "\tLN:i:33\tKC:i:33\n"
             "L\t1_i0\t+\t2_i0\t+\t32M\n" "L\t1_i0\t+\t3_i0\t+\t32M\n" "L\t2_i0\t-\t1_i0\t-\t32M\n" "L\t3_i0\t-\t1_i0\t-\t32M\n")

CYCLE = {}            # k -> the circular sequence of the "cycle" case
HAIRPIN = {}          # k -> the walked sequence of the hairpin case


def sorted_comps(comps):
    return [sorted(int(x) for x in m) for m in comps]


def _no_pal(s, k):
    return all(s[i:i + k] != R.rc_str(s[i:i + k]) for i in range(len(s) - k + 1))


def fork(k):
    """a trunk k-mer with two successors: three segments of one k-mer, four links"""
    rng = np.random.default_rng(400 + k)
    while True:
        t = R._rand_seq(rng, k)
        km = R.kmers_of(t + "A", k) + R.kmers_of(t + "C", k)[1:]
        if len(set(km)) == 3 and _no_pal(t + "A", k) and _no_pal(t + "C", k):
            return k, [km]


def rc_printed(k):
    """the walk starts on the smaller canonical k-mer, on its canonical strand, and reads s; the printed strand is rc(s)"""
    rng = np.random.default_rng(900 + k)
    while True:
        s = R._simple_path(rng, 5, k)
        km = R.kmers_of(s, k)
        if _no_pal(s, k) and R.rc_str(s) < s and km[0] < km[-1] and R.encode(s[:k]) == km[0]:
            return k, [km]


def one_word_apart(same_component):
    """k = 63: k-mers that agree in their low word (the last 32 bases) and differ in the high word, and the mirror image; paths that run
    into the shared stretch and out of it (as tests/test_wcomp2seq_gpu.py lays them out)"""
    k = 63
    rng = np.random.default_rng(6363)
    tail, head = R._rand_seq(rng, 31) + "A", "A" + R._rand_seq(rng, 31)
    lo_same = [R.encode("A" + R._rand_seq(rng, 30) + tail) for _ in range(3)]
    hi_same = [R.encode(head + R._rand_seq(rng, 30) + "A") for _ in range(3)]
    assert len({x & W.MASK64 for x in lo_same}) == 1 and len({x >> 64 for x in lo_same}) == 3
    assert len({x >> 64 for x in hi_same}) == 1 and len({x & W.MASK64 for x in hi_same}) == 3
    assert all(R.canon(x, k) == x for x in lo_same + hi_same)
    t32, h32 = R._rand_seq(rng, 32), R._rand_seq(rng, 32)
    into = [R.kmers_of(R._rand_seq(rng, 33) + t32, k) for _ in range(2)]
    out_of = [R.kmers_of(h32 + R._rand_seq(rng, 33), k) for _ in range(2)]
    groups = [[x] for x in lo_same] + [[x] for x in hi_same] + into + out_of
    assert len({x for g in groups for x in g}) == sum(len(g) for g in groups)
    return k, ([sum(groups, [])] if same_component else groups)


def palindromes(k):
    """even k: a palindromic k-mer inside a path, one as a whole component, one at the start of a path"""
    assert k % 2 == 0
    rng = np.random.default_rng(k)
    h = R._rand_seq(rng, k // 2)
    p = h + R.rc_str(h)
    assert R.encode(p) == R.encode(R.rc_str(p))
    h2 = R._rand_seq(rng, k // 2)
    p2 = h2 + R.rc_str(h2)
    return k, [sorted(set(m)) for m in (R.kmers_of(R._rand_seq(rng, 6) + p + R._rand_seq(rng, 6), k), [R.encode(p)], R.kmers_of(p2 + R._rand_seq(rng, 7), k))]


def cycle(k, tail):
    """the 15 k-mers of a circular sequence of 15 bases; tail: two bases that lead into it"""
    rng = np.random.default_rng(1500 + k)
    while True:
        s = R._rand_seq(rng, 17)
        circ = s[2:]
        walk = (circ * (k // 15 + 2))[:15 + k - 1]
        if len(set(R.kmers_of(s[:2] + walk, k))) == 17 and _no_pal(s[:2] + walk, k):
            break
    CYCLE[k] = circ
    return k, [R.kmers_of((s[:2] if tail else "") + walk, k)]


def hairpin(k):
    """k odd: b + w with w = h + rc(h), k - 1 bases that are their own reverse complement -- the k-mer is followed by its own reverse
    complement, w + complement(b); two k-mers lead up to it.  The walk starts with T and w with A: the reverse complement is printed"""
    assert k % 2 == 1
    rng = np.random.default_rng(7700 + k)
    while True:
        h = "A" + R._rand_seq(rng, (k - 1) // 2 - 1)
        s = "T" + R._rand_seq(rng, 2) + h + R.rc_str(h)
        km = R.kmers_of(s, k)
        if len(set(km)) == 3 and km[0] < km[-1]:
            break
    assert len(s) == k + 2 and s[3:] == R.rc_str(s[3:]) and R.rc_str(s) < s
    HAIRPIN[k] = s
    return k, [km]


def x_and_rcx(k):
    """a path of nine k-mers one of which is listed as x and as rc(x): one row, drawn once"""
    rng = np.random.default_rng(31 + k)
    path = R.kmers_of(R._simple_path(rng, 9, k), k)
    both = path + [R.encode(R.rc_str(R.decode(path[3], k)))]
    assert len(set(both)) == 10
    return k, [both]


def bubble(k):
    """left k-mer, two branches of k k-mers that differ in one base, right k-mer: four segments, eight links"""
    rng = np.random.default_rng(8800 + k)
    while True:
        left, right = R._rand_seq(rng, k), R._rand_seq(rng, k)
        a, b = left + "A" + right, left + "C" + right
        km = sorted(set(R.kmers_of(a, k) + R.kmers_of(b, k)))
        if len(km) == 2 * k + 2 and _no_pal(a, k) and _no_pal(b, k):
            return k, [km]


def crafted():
    cases = {}
    for k in (32, 33, 47, 62, 63):
        cases[f"1_fork_k{k}"] = (*fork(k), "plain")
    cases["2_path3_k33"] = (33, [R.kmers_of(PATH3, 33)], "plain")
    cases["2_fork_literal_k33"] = (33, [[R.encode(FORK_TRUNK), R.encode(FORK_A), R.encode(FORK_C)]], "plain")
    cases["3_rc_printed_k63"] = (*rc_printed(63), "plain")
    cases["4_one_word_apart_same_component"] = (*one_word_apart(True), "plain")
    cases["4_one_word_apart_different_components"] = (*one_word_apart(False), "plain")
    cases["5_palindromes_k32"] = (*palindromes(32), "plain")
    cases["5_palindromes_k62"] = (*palindromes(62), "plain")
    cases["6_cycle_k33"] = (*cycle(33, False), "cycle")
    cases["6_cycle_tail_k33"] = (*cycle(33, True), "plain")
    cases["6_hairpin_k33"] = (*hairpin(33), "hairpin")
    cases["6_hairpin_k63"] = (*hairpin(63), "hairpin")
    cases["7_shared_k33"] = (*R.case_shared(33), "plain")
    k, adj = R.case_adjacent(33)
    cases["7_empty_between_k33"] = (k, [adj[0], [], adj[2]], "plain")
    cases["7_no_components"] = (33, [], "plain")
    cases["7_x_and_rcx_k63"] = (*x_and_rcx(63), "plain")
    cases["9_bubble_k63"] = (*bubble(63), "plain")
    return {n: (k, sorted_comps(c), f) for n, (k, c, f) in cases.items()}


def cover(text, comps, k):
    """every canonical member k-mer lies on exactly one segment exactly once: the k-mers of the S lines (a palindrome's second line not
    counted) are the component's canonical members as a multiset.  Needs no reference."""
    parsed = G.parse(text)
    for c, members in enumerate(comps):
        want = sorted({R.canon(int(x), k) for x in members})
        got, seen = [], set()
        for name, seq, _, _ in parsed.get(c, ([], []))[0]:
            if name in seen:
                assert seq == R.rc_str(seq) and len(seq) == k, (c, name)      # (the second S line of a palindromic k-mer)
                continue
            seen.add(name)
            got += R.kmers_of(seq, k)
        assert sorted(got) == want, c
    assert all(c < len(comps) for c in parsed)


def generated(O, L, n_reads=20000, seed=3, k=33, b1=190, b2=200):
    """comp2graph_ref.generated at a wide k: reads of the benchmark's generator, counted and cut with small bounds by the 128-bit CPU
    reference implementation (O) -> (k, components, [{canonical k-mer: count} of two samples: the halves of the reads])"""
    bases, off = L.synth_reads_host(seed, 0, 0, n_reads, 150, 40000)
    t = O.WTable().count_buffer(bases, off, k)
    comps = [sorted(O.w128_to_ints(c[3])) for c in O.wide_cut_components(t, k, b1, b2).all()]
    half = n_reads // 2
    samples = []
    for lo, hi in ((0, half), (half, n_reads)):
        st = O.WTable().count_buffer(bases[lo * 150:hi * 150], off[lo:hi + 1] - off[lo], k)
        keys, vals = st.export(0)
        samples.append({int(x): int(v) for x, v in zip(O.w128_to_ints(keys), vals.tolist())})
    return k, comps, samples
