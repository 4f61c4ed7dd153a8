"""Steps C2 .. C5 of the component cutter (metafast_amd/csrc/mf_cc.hip, mf_cc_build: tile union-find, edge list, per-vertex fallback,
compression, the LDS tables of the statistics, sparse levels, classification, members, the hand-over between threshold levels) on crafted
graphs, component by component against tests/cc_ref.py.

mf_debug_components (mf_cc.hip; bound here with ctypes, not part of the C-ABI) runs mf_cc_build on an adjacency given as vertex ids and
returns the ordinary components plus a trace of the threshold levels: dense or on a list, vertices visited, the two counters of the edge
list, components kept / oversize, survivors, whether a list of them was asked for and whether it stood.  Every case

    * compares sizes, weights, thresholds, order and members with cc_ref.cut, element by element,
    * asserts from the trace that the path it was made for ran (tests/test_cc_ref_cpu.py asserts the arithmetic behind it on the CPU),
    * does both under cc_compress = 0 / 1 and cc_sparse = 0 / 1: four runs, four times the reference's answer.

With b2 < b1 k_cc_classify drops a component of b2 < size < b1 while k_cc_members lets its vertices of a high value live on; they can
never be kept (nothing is, with b2 < b1), but they are counted among the survivors: there the trace's na / visited may exceed the
reference's, everything else is held as usual."""
import ctypes as C

import numpy as np
import pytest

import cc_ref as R

pytestmark = pytest.mark.gpu

FIELDS = ("thr", "sparse", "visited", "ecount0", "ecount1", "nkept", "nkm", "nbig", "na", "want_list", "list_stands")
SETTINGS = [(c, s) for c in (0, 1) for s in (0, 1)]         # (cc_compress, cc_sparse)


def debug_components(ctx, nbr, vals, b1, b2, keys=None, trace_cap=64, n=None):
    """-> (Comps.export() of the hook's components, [dict per threshold level])"""
    from metafast_amd import lib as L
    fn = L.lib().mf_debug_components
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64, C.POINTER(C.c_int)]
    nbr = np.ascontiguousarray(nbr, dtype=np.uint32)
    vals = np.ascontiguousarray(vals, dtype=np.uint16)
    keys = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint64)
    n = len(vals) if n is None else n
    trace = np.zeros((trace_cap, len(FIELDS)), dtype=np.uint64)
    h, nl = C.c_void_p(), C.c_int(-1)
    L._check(fn(ctx.h, n, nbr.ctypes.data if nbr.size else None, vals.ctypes.data if vals.size else None, None if keys is None else keys.ctypes.data,
                b1, b2, C.byref(h), trace.ctypes.data, trace_cap, C.byref(nl)))
    comps = L.Comps(ctx, h)
    try:
        out = comps.export()
    finally:
        comps.close()
    debug_components.levels = nl.value                      # (all that ran; the trace holds the first trace_cap of them)
    return out, [dict(zip(FIELDS, map(int, row))) for row in trace[:min(nl.value, trace_cap)]]


def same_components(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for j, name in enumerate(("size", "weight", "thr")):
        g, w = np.array([c[j] for c in got], dtype=np.int64), np.array([c[j] for c in want], dtype=np.int64)
        bad = np.flatnonzero(g != w)
        assert not len(bad), (what, name, "first at component", int(bad[0]), int(g[bad[0]]), int(w[bad[0]]), len(bad))
    if got:                                                 # (sizes agree: the member lists line up)
        g, w = np.concatenate([c[3] for c in got]), np.concatenate([c[3] for c in want])
        assert g.dtype == w.dtype == np.uint64 and all(len(c[3]) == c[0] for c in got)
        bad = np.flatnonzero(g != w)
        assert not len(bad), (what, "members: first at", int(bad[0]), int(g[bad[0]]), int(w[bad[0]]), len(bad))


def check_trace(trace, case, sparse_opt, what):
    want = R.expected_trace(case, sparse_opt)
    exact = case.b1 <= case.b2                              # (else: see the module's docstring)
    assert len(trace) == len(want), (what, trace, want)
    for t, w in zip(trace, want):
        for f in ("thr", "sparse", "nkept", "nkm", "nbig", "want_list", "list_stands"):
            assert t[f] == w[f], (what, f, t, w)
        for f in ("na", "visited", "ecount0"):
            assert t[f] == w[f] if exact else t[f] >= w[f], (what, f, t, w)
        assert (t["ecount1"] >= 1) == w["incomplete"] or not exact, (what, t, w)
        if t["sparse"]:
            assert t["ecount0"] == t["ecount1"] == 0, (what, t)
    for a, b in zip(trace, trace[1:]):                      # the hand-over as the trace itself tells it
        assert b["sparse"] == (a["sparse"] or a["list_stands"]), (what, a, b)
        assert b["visited"] == (a["na"] if b["sparse"] else case.n), (what, a, b)
        assert a["nbig"] > 0
    if trace:
        assert trace[-1]["nbig"] == 0
    return want


def run_case(ctx, case, keys=None):
    """the four settings against the reference -> {setting: trace}"""
    want = case.ref()[0] if keys is None else R.cut(case.nbr, case.vals, case.b1, case.b2, keys=keys)
    traces = {}
    try:
        for compress, sparse in SETTINGS:
            ctx.set_option("cc_compress", compress)
            ctx.set_option("cc_sparse", sparse)
            what = f"cc_compress = {compress}, cc_sparse = {sparse}"
            got, trace = debug_components(ctx, case.nbr, case.vals, case.b1, case.b2, keys=keys)
            same_components(got, want, what)
            check_trace(trace, case, sparse, what)
            traces[compress, sparse] = trace
    finally:
        ctx.set_option("cc_compress", 1)
        ctx.set_option("cc_sparse", 1)
    return traces


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_crafted_graph(gpu_ctx, name):
    case = R.CASES[name]()
    R.check_case(case)
    want = case.want
    traces = run_case(gpu_ctx, case)
    for (compress, sparse), trace in traces.items():
        what = (name, compress, sparse, trace)
        if sparse and "pattern" in want:
            assert "".join("DS"[t["sparse"]] for t in trace) == want["pattern"], what
        if not sparse:
            assert all(t["sparse"] == 0 and t["want_list"] == 0 and t["visited"] == case.n for t in trace), what
        if case.n:                                          # level 1: the edge list
            t = trace[0]
            assert (t["ecount0"] > R.ecap(case.n)) == want["glob"], what
            assert (t["ecount1"] >= 1) == (want["lds"] or want["glob"]), what
            if "ecount0" in want:
                assert t["ecount0"] == want["ecount0"], what
        else:
            assert trace == [], what
        if want.get("m0") and sparse:
            assert trace[-1]["sparse"] == 1 and trace[-1]["visited"] == 0 and trace[-2]["nbig"] >= 1 and trace[-2]["na"] == 0, what
        if "lists" in want and sparse:
            # dense with more survivors than the list holds, dense with a list that stands, two levels on a list (the second from the
            # other of the two buffers), a level on nothing
            assert [(t["sparse"], t["want_list"], t["list_stands"]) for t in trace] == [(0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 1), (1, 0, 0)], what
            assert trace[0]["na"] > R.lcap(case.n) >= trace[1]["na"] and trace[2]["visited"] == trace[1]["na"] and trace[3]["visited"] == trace[2]["na"] > 0, what
        if "wave_roots" in want and want["wave_roots"][0] == 2 and sparse:
            assert trace[1]["sparse"] == 1 and trace[1]["nkept"] == want["ncomp"], what


@pytest.mark.parametrize("seed,n,mean_degree", R.RANDOM)
def test_random_graph(gpu_ctx, seed, n, mean_degree):
    case = R.random_case(seed, n, mean_degree)
    R.check_case(case)
    comps, levels = case.ref()
    assert len(levels) >= 3
    assert {case.b1, case.b2} <= {c[0] for c in comps}
    traces = run_case(gpu_ctx, case)
    for (compress, sparse), trace in traces.items():
        assert len(trace) >= 3
        big = mean_degree > 2                               # a giant component: both lists overflow at level 1
        assert (trace[0]["ecount0"] > R.ecap(n)) == big and (trace[0]["ecount1"] >= 1) == big, (seed, n, trace[0])
        if sparse:
            assert any(t["sparse"] for t in trace), (seed, n, trace)


def test_keys_break_ties_and_are_the_members(gpu_ctx):
    """with keys: the members are keys (descending in the vertex id here), components that tie in weight and size go by their smallest key"""
    case = R.CASES["wave_tails_8_sparse"]()
    keys = (np.uint64(1) << np.uint64(61)) - np.arange(case.n, dtype=np.uint64) * np.uint64(3)
    run_case(gpu_ctx, case, keys=keys)


def test_arguments_are_checked(gpu_ctx):
    from metafast_amd import lib as L
    nbr, vals = R.path_graph(4), np.ones(4, dtype=np.uint16)
    bad = nbr.copy()
    bad[3, 7] = 4
    with pytest.raises(L.MetafastError, match="neighbour 7 of vertex 3"):
        debug_components(gpu_ctx, bad, vals, 1, 4)
    for v in (0, R.MAX_COUNT + 1):
        with pytest.raises(L.MetafastError, match="value"):
            debug_components(gpu_ctx, nbr, np.array([1, 1, v, 1], dtype=np.uint16), 1, 4)
    with pytest.raises(L.MetafastError, match="62 bits"):
        debug_components(gpu_ctx, nbr, vals, 1, 4, keys=np.array([1, 2, 3, 1 << 62], dtype=np.uint64))
    with pytest.raises(L.MetafastError, match="vertices"):
        debug_components(gpu_ctx, nbr, vals, 1, 4, n=0xFFFFFFFF)
    got, trace = debug_components(gpu_ctx, nbr, [R.MAX_COUNT] * 4, 1, 4)
    assert [(c[0], c[1], c[2], c[3].tolist()) for c in got] == [(4, 4 * R.MAX_COUNT, 1, [0, 1, 2, 3])] and len(trace) == 1
    got, trace = debug_components(gpu_ctx, R.path_graph(3000), np.ones(3000), 1, 1, trace_cap=1)        # (two levels ran, room for one)
    assert got == [] and len(trace) == 1 and debug_components.levels == 2


@pytest.mark.parametrize("k", [31, 22])
def test_both_front_ends_on_a_counted_table(gpu_ctx, k):
    """the adjacency of a counted table (mf_debug_neighbours) fed to the hook with the table's keys = mf_cut_components_device on that
    table; fed without keys (ids for k-mers, as the 128-bit front end has it) = the same after ids -> keys and the ties put in key order"""
    from test_nbr_gpu import debug_neighbours
    from util import branchy_reads, gpu_count
    parts = [branchy_reads(rs, genome_seed=7, n=2000) for rs in (107, 117, 127)]
    bases = np.concatenate([b for b, _ in parts])
    offsets = np.arange(3 * 2000 + 1, dtype=np.uint64) * np.uint64(150)
    t = gpu_count(gpu_ctx, bases, offsets, k)
    tkeys, nbr, _, _ = debug_neighbours(gpu_ctx, t, 0)
    vals = t.lookup(tkeys).astype(np.uint16)
    assert R.is_symmetric(nbr) and vals.min() >= 1
    b1, b2 = 20, 400
    want = gpu_ctx.cut_components(t, b1, b2).export()
    assert len(want) >= 10 and max(c[2] for c in want) >= 3
    levels = []
    ref = R.cut(nbr, vals, b1, b2, keys=tkeys, levels=levels)
    same_components(want, ref, "mf_cut_components_device against the reference")
    got, trace = debug_components(gpu_ctx, nbr, vals, b1, b2, keys=tkeys)
    same_components(got, want, "with keys")
    assert [(t_["thr"], t_["nkept"], t_["nkm"], t_["nbig"], t_["na"]) for t_ in trace] == [(lv["thr"], lv["nkept"], lv["nkm"], lv["nbig"], lv["na"]) for lv in levels]
    ids, _ = debug_components(gpu_ctx, nbr, vals, b1, b2)
    mapped = [(s, w, th, np.sort(tkeys[m.astype(np.int64)])) for s, w, th, m in ids]
    mapped.sort(key=lambda c: (c[2], -c[1], -c[0], int(c[3][0])))
    same_components(mapped, want, "without keys")
