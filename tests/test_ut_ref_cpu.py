"""tests/ut_ref.py pinned without a GPU: flags() against hand-worked k-mers and, through a sequential walk, against the oracle's unitigs;
every crafted case of tests/test_unitig_gpu.py against the arithmetic that makes it reach its path (a case that silently stops exercising
its border fails here), and against the oracle (the sequences the case was made of come out, as often as it says)."""
from collections import Counter

import numpy as np
import pytest

import nbr_ref as NR
import ut_ref as R
from util import canon_seq, genome_reads

E = NR.encode                   # "ACGT" -> 0 1 2 3: complement = 3 - code, as in the library (which PRINTS the codes as "AGCT")


def test_rc_on_words_is_rc_base_by_base():
    rng = np.random.default_rng(1)
    for k in (1, 5, 31, 32, 33, 47, 63):
        xs = [int(rng.integers(0, 1 << 62)) << 64 | int(rng.integers(0, 1 << 62)) for _ in range(50)]
        xs = [x & ((1 << (2 * k)) - 1) for x in xs] + [0, (1 << (2 * k)) - 1]
        assert R._rc_many(xs, k) == [R.rc_plain(x, k) for x in xs]
    assert R.rc_plain(E("AAACG"), 5) == E("CGTTT")


def test_flags_branch_and_dead_end():
    """AAACG has the right neighbours AACGA and AACGC (MANY; the first present one, A, gives ridx / ror) and no left one (NONE); both of them
    have AAACG as their only left neighbour and nothing on their right"""
    keys = [E("AAACG"), E("AACGA"), E("AACGC")]
    info, ridx, lidx, pal = R.flags(keys, 5)
    assert info.tolist() == [5 | (4 << 3), 4 | (0 << 3), 4 | (0 << 3)]
    assert ridx.tolist() == [1, R.NONE, R.NONE] and lidx.tolist() == [R.NONE, 0, 0] and pal.tolist() == [0, 0, 0]


def test_flags_neighbour_on_the_other_strand():
    """the left neighbour T of AAATG is TAAAT, held as ATTTA (lor = 1); seen from ATTTA, its left neighbour C, CATTT, is held as AAATG"""
    keys = [E("AAATG"), E("ATTTA")]
    info, ridx, lidx, pal = R.flags(keys, 5)
    assert info.tolist() == [4 | (3 << 3) | (1 << 7), 4 | (1 << 3) | (1 << 7)]
    assert lidx.tolist() == [1, 0] and ridx.tolist() == [R.NONE, R.NONE]


def test_flags_palindrome_and_self_loop():
    """ACGT is its own reverse complement: its right neighbour A (CGTA) and its left neighbour T (TACG, held as CGTA) are one k-mer.  AAAAA is
    its own right and left neighbour"""
    info, ridx, lidx, pal = R.flags([E("ACGT"), E("CGTA")], 4)
    assert info.tolist() == [0 | (3 << 3) | (1 << 7), 4 | (0 << 3)] and pal.tolist() == [1, 0]
    assert ridx.tolist() == [1, R.NONE] and lidx.tolist() == [1, 0]
    info, ridx, lidx, pal = R.flags([E("AAAAA")], 5)
    assert info.tolist() == [0] and ridx.tolist() == [0] and lidx.tolist() == [0]
    wide = R.flags([0], 40)                                 # the same k-mer of 40 bases, by the two-word path
    assert wide[0].tolist() == [0] and wide[1].tolist() == [0] and wide[2].tolist() == [0] and wide[3].tolist() == [0]


def _walk_unitigs(keys, counts, k, min_len):
    """the reference's walk on top of flags(): from every start along the links; the emission rule of processSequence"""
    info, ridx, lidx, pal = R.flags(keys, k)
    succ, starts, right, r_unique = R.links(info, ridx, lidx, pal if k % 2 == 0 else None)
    oriented = lambda f: R.rc_plain(keys[f >> 1], k) if f & 1 else keys[f >> 1]
    out, used = [], set()
    for s in starts:
        x = oriented(s)
        seq, w, f = ["AGCT"[(x >> (2 * (k - 1 - i))) & 3] for i in range(k)], [int(counts[s >> 1])], s
        while succ[f] is not None:
            f = succ[f]
            seq.append("AGCT"[oriented(f) & 3])
            w.append(int(counts[f >> 1]))
        en = keys[right(f) >> 1] if r_unique(f) else keys[f >> 1]
        st = keys[s >> 1]
        if len(seq) < min_len or st > en or (st == en and st in used):
            continue
        if st == en:
            used.add(st)
        twice = k % 2 == 0 and pal[s >> 1] and st != en     # {kmerF, kmerF.rc()} of a palindrome: the same walk twice
        out += [("".join(seq), sum(w) // len(w), min(w), max(w))] * (2 if twice else 1)
    return out


@pytest.mark.parametrize("k", [21, 22, 31, 47])
def test_flags_walked_sequentially_give_the_oracles_unitigs(oracle, k):
    bases, off = genome_reads(np.random.default_rng(50 + k), 3000, 1500, 80, err=0.01)
    if k <= 31:
        keys, vals = oracle.Table().count_buffer(bases, off, k).export(0)
        g = oracle.Table()
        for x, v in zip(keys.tolist(), vals.tolist()):
            g.add(x, v)
        want = oracle.build_unitigs(g, k, 0, 30).all()
        keys = keys.tolist()
    else:
        t = oracle.WTable().count_buffer(bases, off, k)
        keys, vals = t.export(0)
        want = oracle.wide_build_unitigs(t.good(0), k, 0, 30).all()
        keys = oracle.w128_to_ints(keys)
    got = _walk_unitigs(keys, vals.tolist(), k, 30)
    norm = lambda seqs: sorted((canon_seq(s), a, mn, mx) for s, a, mn, mx in seqs)
    assert len(want) > 20 and norm(got) == norm(want)
    info = R.flags(keys, k)[0]
    assert (info & 7 == R.CODE_MANY).any() and (info & 7 == R.CODE_NONE).any() and (info >> 6).any()


def test_layout_keeps_empty_partitions_and_the_order_inside():
    order, bits, off = R.layout([10, 11, 12, 13, 14], [5, 0, 5, 2, 0])
    assert order.tolist() == [1, 4, 3, 0, 2] and bits == 3 and off.tolist() == [0, 2, 2, 3, 3, 3, 5, 5, 5]
    assert R.layout([1, 2], None)[1:] == (0, None)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_crafted_case_reaches_its_path(oracle, name):
    c = R.get_case(name)
    seqs, census = c.oracle_unitigs(oracle)
    assert set(c.want) == set(c.settings), name
    for st in c.settings:
        p = c.predict(*st)
        for f, v in c.want[st].items():
            assert p[f] == v, (name, st, f, p[f], v)
        assert p["paths"] == len(seqs) == census[2] and p["n_starts"] + p["pal_starts"] == census[0], (name, st, census)      # (the reference walks a palindromic start twice)
        assert sorted(p["path_nodes"]) == sorted(len(s[0]) - c.k + 1 for s in seqs)
        assert all(s <= nodes // R.SEG + 1 for s, nodes in zip(p["segments"], p["path_nodes"]))        # the bound of k_ut_seg_bound, both cutters
        lo, hi = p["double_rounds"]
        assert lo <= hi <= 40 and (lo > 0) == bool(p["doubled"])
    if c.nseq is not None:                                  # the sequences the case was made of, each once, nothing else
        assert len(seqs) == c.nseq and len({canon_seq(s[0]) for s in seqs}) == c.nseq
    assert max(c.counts) <= R.MAX_COUNT and min(c.counts) >= 1 and len(c.keys) <= 71000


def test_partition_border_and_longest_chain():
    for o in ("asc", "desc", "perm"):
        c = R.get_case(f"a_border_{o}")
        sizes = np.diff(c.off.astype(np.int64)).tolist()
        assert sizes == [512, 513] and 2 * sizes[0] == R.J_MAXN < 2 * sizes[1]
    one = R.get_case("b_longest_chain_one_word")
    p = one.predict()
    assert p["longest_word"] == R.J_MAXN - 1 < 2 ** R.J_ROUNDS and len(one.keys) == 512 and one.k % 2 == 1
    assert p["candidates"] == p["paths"] == 1 and p["n_starts"] == 1      # start and end: the two strands of one k-mer


def test_walk_round_borders():
    cum = np.cumsum(R.CHUNKS).tolist()
    assert cum == [32, 160, 672, 4768]
    assert sorted(set(R.WALK_WORDS)) == sorted({1, 2} | set(cum) | {c + 1 for c in cum[:-1]})
    assert max(R.get_case("d_walk_rounds").predict()["words"]) == cum[-1]
    assert max(R.get_case("d_walk_rounds_4769").predict()["words"]) == cum[-1] + 1


def test_segment_cases_leave_slots_empty():
    for v in ("hop", "p100", "p512"):
        c = R.get_case(f"e_segments_{v}")
        for st in c.settings:
            p = c.predict(*st)
            assert p["seg_slots"] == sum(n // R.SEG + 1 for n in R.SEG_NODES + (40,))
            assert p["empty_slots"] == p["seg_slots"] - sum(p["segments"]) > 0
    p = R.get_case("e_segments_p512").predict(1, 3)
    i = p["path_nodes"].index(1000)
    assert p["segments"][i] == 2 and 1000 // R.SEG + 1 == 6   # the 1000-node path under the doubled cutter: slots 0 and 2 of 6 (entry at node 512)
    p = R.get_case("e_segments_p100").predict(4, 3)
    assert p["segments"][p["path_nodes"].index(1000)] == 5     # cuts every 200 nodes


def test_store_alignment_case_takes_every_residue():
    c = R.get_case("f_store_alignment")
    p = c.predict()
    lens = sorted(p["path_nodes"])
    assert lens[0] == 1 and lens[-1] == 40 and len(lens) == 320
    # (the residues of the OFFSETS depend on the order the paths are written in: asserted on the output itself in test_unitig_gpu.py)
    assert {(n + c.k - 1) % 8 for n in lens} == set(range(8))


@pytest.mark.parametrize("k", [22, 26])
def test_printed_twice(oracle, k):
    c = R.get_case(f"h_printed_twice_k{k}")
    seqs, census = c.oracle_unitigs(oracle)
    twice = [s for s, n in Counter(canon_seq(s[0]) for s in seqs).items() if n == 2]
    assert [len(s) for s in twice if len(s) > 400 + k - 1] == [420 + k - 1] and census[2] == len(seqs)      # (short tips may come twice too)
    c = R.get_case(f"h_palindromic_start_k{k}")
    seqs, census = c.oracle_unitigs(oracle)
    cnt = Counter(canon_seq(s[0]) for s in seqs)
    twice = [s for s, n in cnt.items() if n == 2]
    assert len(twice) == 1 and len(twice[0]) == k and twice[0] == twice[0][::-1].translate(str.maketrans("ACGT", "TGCA"))
    assert c.predict()["twice"] == 1
    through = [s for s in cnt if len(s) == 839 + k - 1]    # the path THROUGH a palindrome: 839 nodes of 420 k-mers, once
    assert len(through) == 1 and cnt[through[0]] == 1
    # a palindromic start never heads a longer path (ut_ref.case_palindromic_start): over all starts of both cases
    info, ridx, lidx, pal = c.flags
    succ, starts, _, _ = R.links(info, ridx, lidx, pal)
    assert all(succ[s] is None for s in starts if pal[s >> 1]) and any(pal[s >> 1] for s in starts)


def test_random_assignments():
    a = R.random_assignments(60000, 5)
    sizes = np.bincount(a["random"], minlength=256)
    assert (sizes == 0).sum() >= 40 and sizes.max() > 512 and (sizes > 0).sum() > 100 and a["none"] is None
    assert len(set(a["alone"].tolist())) == 60000 and set(a["one"].tolist()) == {0}
