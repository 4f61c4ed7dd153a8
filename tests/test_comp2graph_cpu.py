"""tests/comp2graph_ref.py, the yardstick of tests/test_comp2graph_gpu.py, without a GPU: the restatement of Comp2Graph.java and
GFAWriter.java pinned on hand-written GFA, and WHERE it is a yardstick at all -- the cases on which its canonical form does not depend
on the iteration order of the reference's hash map (8 seeded permutations)."""
import pytest

import comp2graph_ref as G
import comp2seq_ref as CR

CASES = G.crafted()

# the fork AACCG -> ACCGA | ACCGT, k-mers in this order: nodes 1, 3, 5 (a node and its reverse complement share an id)
FORK = ("S\t1_i0\tAACCG\tLN:i:5\tKC:i:5\n" "S\t3_i0\tACCGA\tLN:i:5\tKC:i:5\n" "S\t5_i0\tACCGT\tLN:i:5\tKC:i:5\n"
        "L\t1_i0\t+\t3_i0\t+\t4M\n" "L\t1_i0\t+\t5_i0\t+\t4M\n" "L\t3_i0\t-\t1_i0\t-\t4M\n" "L\t5_i0\t-\t1_i0\t-\t4M\n")
# the bubble AAACC -> AACCAGTGA | AACCCGTGA -> GTGAA: four segments, every adjacency from both sides
BUBBLE_S = [("AAACC", 5, 5), ("AACCAGTGA", 9, 9), ("AACCCGTGA", 9, 9), ("GTGAA", 5, 5)]
BUBBLE_L = [("AAACC", "+", "AACCAGTGA", "+"), ("AAACC", "+", "AACCCGTGA", "+"), ("AACCAGTGA", "-", "AAACC", "-"), ("AACCCGTGA", "-", "AAACC", "-"),
            ("AACCAGTGA", "+", "GTGAA", "+"), ("AACCCGTGA", "+", "GTGAA", "+"), ("GTGAA", "-", "AACCAGTGA", "-"), ("GTGAA", "-", "AACCCGTGA", "-")]


def test_string_order_is_not_the_order_of_the_codes():
    """normalizeDna compares strings (A < C < G < T), the library's canonical form the 2-bit codes (A < G < C < T): ACCGT / ACGGT"""
    assert G.normalize("ACGGT") == "ACCGT" and CR.decode(CR.canon(CR.encode("ACCGT"), 5), 5) == "ACGGT"


def test_fork_by_hand():
    k, comps, _ = CASES["fork"]
    assert [G.normalize(CR.decode(x, k)) for x in comps[0]] == ["AACCG", "ACCGA", "ACCGT"]
    assert G.gfa(comps, k) == FORK
    # values: AACCG 3, ACCGA 0 (no file holds it), ACCGT 7: KC = value x (1 + (k - 1))
    vals = {CR.canon(CR.encode("AACCG"), k): 3, CR.canon(CR.encode("ACCGT"), k): 7}
    assert [s[3] for s in G.parse(G.gfa(comps, k, vals))[0][0]] == [15, 0, 35]


def test_bubble_by_hand():
    k, comps, _ = CASES["bubble"]
    form = G.canon(G.gfa(comps, k))
    assert form == {0: (sorted(BUBBLE_S), sorted(l + ("4M",) for l in BUBBLE_L))}


def test_a_palindromic_kmer_is_printed_twice_and_linked_twice():
    k, comps, _ = CASES["k4_palindrome"]
    segs, links = G.parse(G.gfa(comps, k))[0]
    assert [s[1] for s in segs].count("ACGT") == 2 and len(segs) == 5
    assert len(links) == 8 and len(set(links)) == 6


@pytest.mark.parametrize("name", list(CASES))
def test_where_the_restatement_is_a_yardstick(name):
    k, comps, family = CASES[name]
    par = G.parity(comps, k)
    if family == "plain":
        assert all(par), name
    elif family == "hairpin":
        assert not all(par)                                  # mergeNodes(x, x): what comes out depends on who is asked first
    else:
        assert G.gfa(comps, k) == ""                         # an isolated cycle merges itself away: the reference draws nothing


def test_canon_ignores_names_and_order_and_sees_everything_else():
    k, comps, _ = CASES["bubble"]
    a, b = G.gfa(comps, k), G.gfa(comps, k, orders=G.permuted_orders(comps, k, 1))
    assert a != b and G.canon(a) == G.canon(b)
    assert G.canon(a.replace("KC:i:9", "KC:i:8", 1)) != G.canon(a)
    lines = a.splitlines(keepends=True)
    with pytest.raises(ValueError, match="S line after an L line"):
        G.canon("".join(lines[:2] + lines[4:5] + lines[2:4] + lines[5:]))
    G.check_rules("", k, 1)


def test_sample_values():
    t = [{1: 2, 2: 1}, {1: 40000 - 2, 3: 5}, {1: 1}]
    assert G.sample_values(t, False) == {1: 3, 2: 1, 3: 1}
    assert G.sample_values(t, True) == {1: 32767, 2: 1, 3: 5}


def test_generated_components_are_parity_cases(oracle):
    from metafast_amd import lib as L
    k, comps, samples = G.generated(oracle, L)
    assert 100 <= len(comps) <= 1000
    par = G.parity(comps, k, G.sample_values(samples, False))
    assert par.count(False) <= len(comps) // 100, par.count(False)
