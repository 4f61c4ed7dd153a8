"""tests/cc_ref.py, the plain restatement of the component cutter's steps C2 .. C5 that tests/test_cc_gpu.py holds the kernels against:
hand-worked graphs, the pinned oracle on a read-derived table, and -- for every crafted graph of the GPU tests -- the arithmetic that
makes it reach the path it is there for (a case that no longer does fails here, on the CPU)."""
import numpy as np
import pytest

import cc_ref as R
import nbr_ref


def _plain(comps):
    return [(s, w, t, m.tolist()) for s, w, t, m in comps]


def test_two_components_around_the_bounds():
    """0 - 1 - 2 and 3 - 4 - 5 - 6, values 1 .. 7"""
    nbr = R.from_edges(7, [0, 1, 3, 4, 5], [1, 2, 4, 5, 6])
    vals = [1, 2, 3, 4, 5, 6, 7]
    assert _plain(R.cut(nbr, vals, 3, 4)) == [(4, 22, 1, [3, 4, 5, 6]), (3, 6, 1, [0, 1, 2])]
    assert _plain(R.cut(nbr, vals, 4, 4)) == [(4, 22, 1, [3, 4, 5, 6])]
    assert _plain(R.cut(nbr, vals, 1, 2)) == [(2, 5, 2, [1, 2]), (2, 13, 6, [5, 6])]
    # b2 = 3: the four are oversize while all of them reach the threshold (levels 1 .. 4), at level 5 vertex 3 (value 4) is gone
    levels = []
    assert _plain(R.cut(nbr, vals, 3, 3, levels=levels)) == [(3, 6, 1, [0, 1, 2]), (3, 18, 5, [4, 5, 6])]
    assert [(lv["thr"], lv["alive"], lv["nkept"], lv["nkm"], lv["nbig"], lv["na"]) for lv in levels] == [
        (1, 7, 1, 3, 1, 4), (2, 4, 0, 0, 1, 4), (3, 4, 0, 0, 1, 4), (4, 4, 0, 0, 1, 3), (5, 3, 1, 3, 0, 0)]
    assert _plain(R.cut(nbr, vals, 4, 3)) == []              # b2 < b1: nothing can be kept


def test_three_levels_and_a_bridge_of_value_one():
    """a path of seven, values 3 3 2 1 2 3 3: the middle vertex holds the two halves together at level 1 only"""
    nbr = R.path_graph(7)
    vals = [3, 3, 2, 1, 2, 3, 3]
    levels = []
    assert _plain(R.cut(nbr, vals, 1, 2, levels=levels)) == [(2, 6, 3, [0, 1]), (2, 6, 3, [5, 6])]
    assert [(lv["alive"], lv["nbig"], lv["na"]) for lv in levels] == [(7, 1, 6), (6, 2, 4), (4, 0, 0)]
    assert _plain(R.cut(nbr, vals, 1, 3)) == [(3, 8, 2, [0, 1, 2]), (3, 8, 2, [4, 5, 6])]
    assert _plain(R.cut(nbr, vals, 1, 7)) == [(7, 17, 1, [0, 1, 2, 3, 4, 5, 6])]
    # with keys: members are keys, ascending, and the tie between the two halves goes to the smaller key
    keys = [70, 60, 50, 40, 30, 20, 10]
    assert _plain(R.cut(nbr, vals, 1, 2, keys=keys)) == [(2, 6, 3, [10, 20]), (2, 6, 3, [60, 70])]


def test_an_oversize_component_that_dies_out():
    """a ring of six, all of value 1, b2 = 5: oversize at level 1, nobody reaches level 2, which runs on nothing"""
    v = np.arange(6)
    nbr = R.from_edges(6, v, (v + 1) % 6)
    levels = []
    assert R.cut(nbr, np.ones(6), 1, 5, levels=levels) == []
    assert [(lv["thr"], lv["alive"], lv["nbig"], lv["na"]) for lv in levels] == [(1, 6, 1, 0), (2, 0, 0, 0)]


def test_self_loop_and_doubled_edge():
    """0 - 0, 0 - 1 twice, 2 - 3; 4 and 5 alone"""
    nbr = R.from_edges(6, [0, 0, 0, 2], [0, 1, 1, 3])
    assert nbr[0].tolist() == [0, 1, 1] + [R.NONE] * 5 and nbr[1].tolist() == [0, 0] + [R.NONE] * 6
    assert R.is_symmetric(nbr) and R.degrees(nbr).tolist() == [3, 2, 1, 1, 0, 0]
    assert _plain(R.cut(nbr, [1, 2, 3, 4, 5, 6], 1, 10)) == [(2, 7, 1, [2, 3]), (1, 6, 1, [5]), (1, 5, 1, [4]), (2, 3, 1, [0, 1])]
    assert _plain(R.cut(nbr, [1, 2, 3, 4, 5, 6], 2, 2)) == [(2, 7, 1, [2, 3]), (2, 3, 1, [0, 1])]
    assert not R.is_symmetric(np.array([[1] + [R.NONE] * 7, [R.NONE] * 8], dtype=np.uint32))
    with pytest.raises(AssertionError):
        R.from_edges(10, [0] * 9, range(1, 10))


@pytest.fixture(scope="module")
def cutter_tables(oracle):
    """the oracle's cutter table of three samples of one genome (as tests/test_round4_gpu.py builds it), per k"""
    from util import branchy_reads
    out = {}
    for k in (21, 31):
        cutter = oracle.Table()
        for rs in (107, 117, 127):
            bases, offsets = branchy_reads(rs, genome_seed=7, n=6000)
            keys, vals = oracle.Table().count_buffer(bases, offsets, k).export(1)
            g = oracle.Table()
            for kk, vv in zip(keys.tolist(), vals.tolist()):
                g.add(kk, vv)
            cutter.count_seqs(oracle.build_unitigs(g, k, 1, 100), k, 100)
        out[k] = cutter
    return out


@pytest.mark.parametrize("k", [21, 31])
@pytest.mark.parametrize("b1,b2", [(100, 1000), (1, 50)])
def test_tie_to_the_oracle(oracle, cutter_tables, k, b1, b2):
    cutter = cutter_tables[k]
    keys, vals = cutter.export()
    want = oracle.cut_components(cutter, k, b1, b2).all()
    levels = []
    got = R.cut(nbr_ref.neighbours(keys, k), vals, b1, b2, keys=keys, levels=levels)
    assert len(levels) >= 3
    if b2 == 1000:                                          # (the table's unitigs are 70 k-mers and longer: b2 = 50 keeps none of them, at any level)
        assert len(want) >= 2 and max(c[2] for c in want) >= 2
    assert [c[:3] for c in got] == [tuple(c[:3]) for c in want]
    for g, w in zip(got, want):
        assert np.array_equal(g[3], np.asarray(w[3], dtype=np.uint64))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_crafted_case_reaches_its_path(name):
    R.check_case(R.CASES[name]())


@pytest.mark.parametrize("seed,n,mean_degree", R.RANDOM)
def test_random_case_reaches_its_paths(seed, n, mean_degree):
    case = R.random_case(seed, n, mean_degree)
    assert R.degrees(case.nbr).max() <= 8 and abs(R.degrees(case.nbr).mean() - mean_degree) < 0.1
    R.check_case(case)
