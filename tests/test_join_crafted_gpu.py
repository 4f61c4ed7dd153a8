"""The eleven cohort tools that stand on the join core's union table (mf_join.h, mf_join.hip), in their table forms, on one adversarial cohort
(tests/join_cases.py: crafted_pool -- per third of the hash space 100 keys of home cap - 1, whose cluster runs over the end of the table, a
stair of merging clusters and keys of home 0; the border keys of 3 and of 7 slices; keys 0 and 2^62 - 1), each against its own restatement in
tests/*_ref.py, unchanged, with option stats_slices at 1, 3 and 7: the results equal the restatement and are identical across the three.

Ghosts -- keys of no table, homes at the head of, inside and in front of the clusters -- go wherever a tool probes with keys that are not in its
table: the filter samples of unique-kmers and unique-kmers-multi, the input sample of kmers-multiple-filters, the k-mer list of
kmers-grouped-counter.

Before each tool the capacity the plan gives for that tool's own `total` (mf_debug_join_plan) is asserted to be join_ref.cap_of's and at most
2^20 slots: the families' homes are then as designed, and a later change of the plan fails here instead of silently emptying the test."""
import numpy as np
import pytest

import color_ref as CR
import join_cases as JC
import join_ref as J
import kmersets_ref as KS
import kps_ref as KP
import specific_ref as SP
import stats3_ref as R3
import stats_ref as R
from test_join_slots_gpu import plan
from test_specific_gpu import _margins

pytestmark = pytest.mark.gpu

SLICES = (1, 3, 7)
P_CHI2, P_MW = 0.3, 0.05
_want = {}


def _tab(ctx, sample):
    return ctx.table_from_host(np.asarray(sample[0], np.uint64), np.asarray(sample[1]).astype(np.uint16), 31)


def _rec(t):
    return R.records_to_bytes(*t.export(-1))


def _once(name, make):
    """a tool's restatement, computed once and left unchanged"""
    if name not in _want:
        _want[name] = make()
    return _want[name]


class Cohort:
    def __init__(self, ctx):
        self.s = JC.crafted_cohort()
        self.t = [_tab(ctx, x) for x in self.s]
        self.g = [JC.with_ghosts(self.s[j], seed=20 + j) for j in range(JC.CRAFTED_N)]         # sample j and the ghosts
        self.tg = [_tab(ctx, x) for x in self.g]
        self.kps = JC.crafted_cohort(seed=3, kps=True)
        self.tkps = [_tab(ctx, x) for x in self.kps]
        assert all(len(t) == len(x[0]) <= 620 for t, x in zip(self.t + self.tg + self.tkps, self.s + self.g + self.kps))


# name -> (total of the plan, got, want); every `got` and `want` is a list of bytes, numbers and dicts
def _stats(ctx, c):
    b = 1
    chi, ga, gb, ctr = ctx.stats_kmers(c.t[:3], c.t[3:], p_chi2=P_CHI2, p_mw=P_MW, max_bad=b)
    w = _once("stats", lambda: R.stats_kmers(c.s[:3], c.s[3:], b=b, p_chi2=P_CHI2, p_mw=P_MW))
    _margins(w, P_MW)
    return [_rec(chi), _rec(ga), _rec(gb), ctr], [R.records_to_bytes(*w[n]) for n in ("chi", "A", "B")] + [w["counters"]]


def _stats3(ctx, c):
    chi, ga, gb, gc, ctr = ctx.stats_kmers3(c.t[:2], c.t[2:4], c.t[4:], p_chi2=P_CHI2, p_mw=P_MW, max_bad=0)
    w = _once("stats3", lambda: R3.stats_kmers3(c.s[:2], c.s[2:4], c.s[4:], b=0, p_chi2=P_CHI2, p_mw=P_MW))
    _margins(w, P_MW)
    return [_rec(chi), _rec(ga), _rec(gb), _rec(gc), ctr], [R.records_to_bytes(*w[n]) for n in ("chi", "A", "B", "C")] + [w["counters"]]


def _specific(ctx, c):
    ga, gb, ctr = ctx.specific_kmers(c.t[:3], c.t[3:], p_chi2=P_CHI2, p_mw=P_MW)
    w = _once("specific", lambda: SP.specific_kmers(c.s[:3], c.s[3:], p_chi2=P_CHI2, p_mw=P_MW))
    _margins(w, P_MW)
    return [_rec(ga), _rec(gb), ctr], [R.records_to_bytes(*w[n]) for n in ("A", "B")] + [w["counters"]]


def _specific3(ctx, c):
    ga, gb, gc, ctr = ctx.specific_kmers3(c.t[:2], c.t[2:4], c.t[4:], p_chi2=P_CHI2, p_mw=P_MW)
    w = _once("specific3", lambda: SP.specific_kmers3(c.s[:2], c.s[2:4], c.s[4:], p_chi2=P_CHI2, p_mw=P_MW))
    _margins(w, P_MW)
    return [_rec(ga), _rec(gb), _rec(gc), ctr], [R.records_to_bytes(*w[n]) for n in ("A", "B", "C")] + [w["counters"]]


def _samples_counter(ctx, c):
    w = _once("nsamples", lambda: R.kmers_samples_count(c.s, 2))
    return [_rec(ctx.kmers_samples_count(c.t, 2))], [R.records_to_bytes(*w)]


def _grouped(ctx, c):
    gk, gc = ctx.kmers_grouped_count(c.tg[0], c.t[1:3], c.t[3:5], c.t[5:], max_bad=1)
    wk, wc = _once("grouped", lambda: R3.kmers_grouped_count([c.g[0]], c.s[1:3], c.s[3:5], c.s[5:], b=1))
    assert (wc.sum(axis=1) == 0).sum() >= len(JC.crafted_pool()["ghosts"])                    # the ghosts are in the list and in no group
    return [gk.tobytes(), gc.tobytes()], [wk.tobytes(), wc.astype(gc.dtype).tobytes()]


def _unique(ctx, c):
    t, n = ctx.unique_kmers(c.t[:4], c.tg[4:], max_bad=1)
    w = _once("unique", lambda: SP.unique_kmers(c.s[:4], c.g[4:], b=1))
    assert 0 < w["c"] < w["n"]
    return [_rec(t), n], [R.records_to_bytes(*w["out"]), w["n"]]


def _unique_multi(ctx, c):
    outs, n_union, counts = ctx.unique_kmers_multi(c.t[:4], c.tg[4:], 1, 1, 4)
    w = _once("ukm", lambda: KS.unique_kmers_multi(c.s[:4], c.g[4:], 1, 1, 4))
    assert 0 < w["counts"][0] < w["n_union"]
    return [[_rec(t) for t in outs], n_union, counts], [[R.records_to_bytes(wk, wv) for _, wk, wv in w["files"]], w["n_union"], w["counts"]]


def _filters(ctx, c):
    kept, triples, counts, found, nkept = ctx.kmers_multiple_filters(c.tg[0], c.t[1], c.t[2], c.t[3], 1)
    w = _once("kmf", lambda: KS.kmers_multiple_filters(c.g[0], [c.s[1]], [c.s[2]], [c.s[3]], 1))
    assert 0 < len(w["kept"][0]) < w["found"]
    return ([_rec(kept), triples.tolist(), counts.astype(np.int64).tolist(), found, nkept],
            [R.records_to_bytes(*w["kept"]), np.asarray(w["triples"]).tolist(), np.asarray(w["counts"]).astype(np.int64).tolist(), w["found"], len(w["kept"][0])])


def _color(ctx, c, val):
    classes = [0, 1, 2, 0, 1, 2]
    gk, gv = ctx.kmers_color(c.t, classes, 1, val).export()
    wk, wv = _once(("color", val), lambda: CR.kmers_color(c.s, classes, 1, val))
    return [CR.ctable_to_bytes(gk, gv)], [CR.ctable_to_bytes(wk, wv)]


def _per_sample(ctx, c):
    """percent 80 of 6 samples: thresh 4 of the five samples behind the first -- the columns are the 300 `last` keys, so the column index
    (1024 slots) holds one cluster of 300 that starts in its last slot"""
    wk, wn, wm = _once("kps", lambda: KP.select(c.kps, 80, False, 0))
    assert sorted(int(k) for k in wk) == sorted(JC.crafted_pool()["last"]) and J.index_cap_of(len(wk)) == 1024
    assert {J.home(int(k), J.index_cap_of(len(wk))) for k in wk} == {1023}
    r = ctx.kmers_per_sample(c.tkps, percent=80, max_bad=0, count_first=False)
    gk, gn, gm = r.export()
    text = [r.header_text(31)] + [r.row_text(j) for j in range(JC.CRAFTED_N)]
    r.close()
    return ([gk.tobytes(), gn.tobytes(), gm.tobytes(), text],
            [wk.tobytes(), wn.astype(gn.dtype).tobytes(), wm.astype(gm.dtype).tobytes(), [KP.header_text(wk, 31).encode()] + [KP.row_text(wm[j]).encode() for j in range(JC.CRAFTED_N)]])


def _n(tabs):
    return sum(len(t) for t in tabs)


# (tool, its `total` as the C entry point computes it, the run)
TOOLS = (("stats-kmers", lambda c: _n(c.t), _stats), ("stats-kmers-3", lambda c: _n(c.t), _stats3), ("specific-kmers", lambda c: _n(c.t), _specific),
         ("specific-kmers-3", lambda c: _n(c.t), _specific3), ("kmers-samples-counter", lambda c: _n(c.t), _samples_counter),
         ("kmers-grouped-counter", lambda c: _n(c.t[1:]), _grouped),                           # the groups' entries, not the k-mer list's
         ("unique-kmers", lambda c: _n(c.t[:4]), _unique), ("unique-kmers-multi", lambda c: _n(c.t[:4]), _unique_multi),      # the inputs', not the filters'
         ("kmers-multiple-filters", lambda c: _n(c.t[1:4]), _filters),                         # the three filter tables', not the input's
         ("kmers-color", lambda c: _n(c.t), lambda ctx, c: _color(ctx, c, False)), ("kmers-color -val", lambda c: _n(c.t), lambda ctx, c: _color(ctx, c, True)),
         ("kmers-per-sample", lambda c: _n(c.tkps), _per_sample))

_cohort = {}


@pytest.mark.parametrize("tool", [t[0] for t in TOOLS])
def test_tool_on_the_crafted_cohort(gpu_ctx, tool):
    if "c" not in _cohort:
        _cohort["c"] = Cohort(gpu_ctx)
    c = _cohort["c"]
    _, total, run = next(t for t in TOOLS if t[0] == tool)
    first = None
    try:
        for S in SLICES:
            gpu_ctx.set_option("stats_slices", S)
            gS, cap = plan(gpu_ctx, total(c))
            assert (gS, cap) == (S, J.cap_of(total(c), S)) and 2048 <= cap <= 1 << JC.LOW, (tool, S, cap)
            got, want = run(gpu_ctx, c)
            assert got == want, (tool, S)
            first = first or got
            assert got == first, (tool, S)
    finally:
        gpu_ctx.set_option("stats_slices", 0)
