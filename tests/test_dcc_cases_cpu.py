"""The crafted cases of the sharded cutter (tests/dcc_cases.py) on the oracle alone: every case reaches the path it was made for, before
a GPU sees it.  These are conditions on the INPUTS: a seed or a length that misses one is changed in dcc_cases.py, the condition stays.

Every case also goes through tests/cc_ref.py's cut() on the adjacency dcc_cases.neighbours() builds in numpy: a second reference, written
independently of the oracle's breadth-first search, that must tell the same components -- and the number of threshold levels, which the
oracle does not report."""
import numpy as np
import pytest

import cc_ref
import dcc_cases as D
from dcc_util import _oracle_of_sequences


def _cut(oracle, case):
    """-> (oracle's table keys, values, components)"""
    table, comps = _oracle_of_sequences(oracle, case.seqs, case.k, case.l, case.b1, case.b2)
    keys, vals = table.export()
    return keys, vals, comps


def _swt(comps):
    return [(s, w, t) for s, w, t, _ in comps]


def _check_common(oracle, case):
    """the numpy table is the oracle's; no k-mer twice by accident; the oracle's components in the oracle's order of ties"""
    keys, vals, comps = _cut(oracle, case)
    nk, nv, _ = case.table()
    assert np.array_equal(keys, nk) and np.array_equal(vals.astype(np.int64), nv), case
    if case.n_distinct is not None:
        assert len(keys) == case.n_distinct, (case, len(keys))
    if "kept" in case.want:
        assert _swt(comps) == case.want["kept"], case                  # the expectation written next to the case
    order = [(t, -w, -s, int(km[0])) for s, w, t, km in comps]
    assert order == sorted(order), case
    assert all(len(km) == s and np.all(km[1:] > km[:-1]) for s, _, _, km in comps), case
    return keys, vals, comps


def _second_reference(case, keys, vals, comps):
    """-> the levels cc_ref.cut ran"""
    nbr = D.neighbours(keys, case.k)
    v, slot = np.nonzero(nbr != D.NONE)
    edges = np.unique(v.astype(np.int64) * len(keys) + nbr[v, slot])
    assert np.array_equal(edges, np.unique(nbr[v, slot].astype(np.int64) * len(keys) + v)), case         # u among v's eight <=> v among u's
    levels = []
    ref = cc_ref.cut(nbr, vals, case.b1, case.b2, keys=keys, levels=levels)
    assert _swt(ref) == _swt(comps), case
    assert all(np.array_equal(a[3], b[3]) for a, b in zip(ref, comps)), case
    if "levels" in case.want:
        assert len(levels) == case.want["levels"], (case, levels)
    return levels


@pytest.mark.parametrize("k", D.SWEEP_K)
def test_ties(oracle, k):
    case = D.by_name("ties", k)
    keys, vals, comps = _check_common(oracle, case)
    same = [km for s, w, t, km in comps if (s, w, t) == (60, 60, 1)]
    assert len(same) >= 40                                              # one (size, weight) forty times ...
    firsts = [int(km[0]) for km in same]
    assert firsts == sorted(firsts) and len(set(firsts)) == len(firsts)              # ... in ascending order of the smallest k-mer
    for swt in ((60, 100, 1), (60, 80, 1), (30, 60, 2)):                # the pairs: equal in size and weight, different inside
        pair = [km for s, w, t, km in comps if (s, w, t) == swt]
        assert len(pair) == 2 and int(pair[0][0]) < int(pair[1][0])
        pv = [vals[np.searchsorted(keys, km)].tolist() for km in pair]
        assert (pv[0] != pv[1]) == (swt != (30, 60, 2))
    _second_reference(case, keys, vals, comps)


@pytest.mark.parametrize("k", D.BOTH_K)
@pytest.mark.parametrize("b1,b2", D.BOUNDS)
def test_bounds(oracle, k, b1, b2):
    case = D.bounds(k, b1, b2)
    keys, vals, comps = _check_common(oracle, case)
    assert case.want["sizes"] == [b1 - 1, b1, b1 + 1, b2 - 1, b2, b2 + 1]
    level1 = sorted(s for s, _, t, _ in comps if t == 1)
    assert level1 == sorted(s for s in case.want["sizes"] if b1 <= s <= b2)           # which of the six sizes are kept
    assert [(s, w) for s, w, t, _ in comps if t == 2] == ([(D.STRETCH, 2 * D.STRETCH)] if b1 <= b2 else [])
    assert all(t <= 2 for _, _, t, _ in comps)
    _second_reference(case, keys, vals, comps)


@pytest.mark.parametrize("k", D.BOTH_K)
def test_singletons(oracle, k):
    for case in (D.singletons(k, 1), D.singletons(k, 10), D.by_name("singletons_3_b2_1", k)):
        keys, vals, comps = _check_common(oracle, case)
        assert len(comps) == len(case.seqs) == len(keys) and all(len(s) == k for s in case.seqs)
        assert [int(km[0]) for _, _, _, km in comps] == keys.tolist()   # every k-mer a component, in the k-mers' order
        assert np.all(D.neighbours(keys, k) == D.NONE)                  # no two of them are neighbours
        _second_reference(case, keys, vals, comps)


@pytest.mark.parametrize("k", D.BOTH_K)
def test_long_path(oracle, k):
    n = 30000 - k + 1
    assert k != 31 or n == 29970
    whole = D.long_path(k, True)
    keys, vals, comps = _check_common(oracle, whole)
    assert len(keys) == n and np.all(vals == 2) and _swt(comps) == [(n, 2 * n, 1)]
    deg = (D.neighbours(keys, k) != D.NONE).sum(axis=1)
    assert sorted(np.unique(deg, return_counts=True)[1].tolist()) == [2, n - 2]     # a path: two ends, no branch, no cycle
    assert len(_second_reference(whole, keys, vals, comps)) == 1
    none = D.long_path(k, False)
    assert none.seqs == whole.seqs and n > none.b2
    keys, vals, comps = _check_common(oracle, none)
    assert comps == []
    levels = _second_reference(none, keys, vals, comps)
    assert [(lv["alive"], lv["nbig"]) for lv in levels] == [(n, 1), (n, 1), (0, 0)]


@pytest.mark.parametrize("k", D.SWEEP_K)
def test_ladder(oracle, k):
    case = D.ladder(k)
    keys, vals, comps = _check_common(oracle, case)
    assert sorted(set(vals.tolist())) == [1, 2, 3, 4, 5, 6]
    assert len({t for _, _, t, _ in comps}) >= 5                        # kept at five thresholds at least
    levels = _second_reference(case, keys, vals, comps)
    assert len(levels) == 6 and all(lv["nbig"] == 1 for lv in levels[:5]) and levels[5]["nbig"] == 0      # cut again five times
    assert all(lv["nkept"] >= 1 for lv in levels)                       # something is kept at every level ...
    small = D.kmers_of(case.want["dropped"], k)[0]                      # ... and the island of fewer than b1 k-mers falls away at its own
    assert len(small) < case.b1 and np.all(vals[np.searchsorted(keys, small)] == 4) and not np.isin(small, np.concatenate([c[3] for c in comps])).any()


@pytest.mark.parametrize("k", D.SWEEP_K)
def test_low_complexity(oracle, k):
    case = D.low_complexity(k)
    keys, vals, comps = _check_common(oracle, case)
    _, _, pal = case.table()
    assert bool(pal.any()) == (k % 2 == 0)                              # k-mers that are their own reverse complement: at even k only
    if k % 2 == 0:
        at = D.kmers_of("AT" * k, k)[0][0]
        assert pal[np.searchsorted(keys, at)] and keys[np.searchsorted(keys, at)] == at
    nbr = D.neighbours(keys, k)
    loops = np.flatnonzero((nbr == np.arange(len(keys), dtype=np.uint32)[:, None]).any(axis=1))
    assert keys[0] == 0 and 0 in loops                                  # AAA..: its own neighbour
    if k % 2:
        ata = D.kmers_of("AT" * k, k)[0]
        assert ata[0] == ata[1] and int(np.searchsorted(keys, ata[0])) in loops      # ATATA.. and TATAT..: ONE k-mer, the neighbour is its reverse complement
    assert int(vals[0]) >= 90 - k + 1                                  # (a flank may begin or end with an A)
    assert len(comps) >= 5 and max(t for _, _, t, _ in comps) >= 3
    _second_reference(case, keys, vals, comps)
