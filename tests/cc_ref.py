"""Steps C2 .. C5 of the component cutter (metafast_amd/csrc/mf_cc.hip, mf_cc_build) restated in plain numpy / Python for the tests, and
the crafted graphs those tests run on.

cut() follows ComponentsBuilder as oracle/mf_oracle_core.inc reads it (bfs, or_cut_components): level thr = 1, 2, ... takes the graph
induced on the vertices still alive; a component smaller than b1 is dropped, one of at most b2 vertices is kept (thr, size, weight = the
sum of its values, members), of a larger one the vertices with value >= thr + 1 stay alive and all others die; the loop ends with the
first level that had no component larger than b2.  The components of a level come from ONE sequential union-find over the list of edges
(no tiles, no atomics, no lists of survivors: nothing of the kernels' way of getting there).  tests/test_cc_ref_cpu.py pins this file
with hand-worked cases and ties it to the oracle.

A graph is nbr uint32 [n, 8]: the ids of a vertex's neighbours in any of its eight slots, NONE elsewhere; symmetric -- u is among the
eight of v as often as v is among the eight of u."""
import numpy as np

NONE = 0xFFFFFFFF
TILE = 1024                 # CC_TILE
LEDGE = 2048                # CC_LEDGE
MAX_COUNT = 32767           # MF_MAX_COUNT


def ecap(n):
    """room of the cutter's global edge list"""
    return n // 2 + 1024


def lcap(n):
    """survivors a dense level can list for the next one"""
    return max(n // 3, 1)


# ---- the reference ----

def labels(nbr, alive):
    """-> int64 [n]: for every alive vertex the smallest vertex id of its component in the graph induced on the alive vertices, -1 for
    the others.  Sequential union-find with path halving over the edges (v, u), u < v, both ends alive."""
    nbr = np.asarray(nbr, dtype=np.uint32).reshape(-1, 8)
    n = len(nbr)
    alive = np.asarray(alive, dtype=bool)
    src = np.repeat(np.arange(n, dtype=np.int64), 8)
    dst = nbr.reshape(-1).astype(np.int64)
    ok = dst != NONE
    ok[ok] = (dst[ok] < src[ok]) & alive[src[ok]] & alive[dst[ok]]
    parent = list(range(n))
    for a, b in zip(src[ok].tolist(), dst[ok].tolist()):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a < b:
            parent[b] = a
        elif b < a:
            parent[a] = b
    p = np.array(parent, dtype=np.int64)
    while True:                                             # every vertex to its root
        q = p[p]
        if np.array_equal(q, p):
            break
        p = q
    p[~alive] = -1
    return p


def cut(nbr, vals, b1, b2, keys=None, levels=None, masks=False):
    """-> the components as Comps.export() gives them: [(size, weight, thr, members uint64[] ascending)], ordered by thr ascending, weight
    descending, size descending, smallest member ascending.  A member is keys[v], or v itself without keys.  levels (a list): one dict
    per threshold level is appended -- thr, alive (vertices the level started with), nkept, nkm, nbig, na (vertices that go on), and with masks also mask: bool [n], the
    vertices the level started with."""
    nbr = np.asarray(nbr, dtype=np.uint32).reshape(-1, 8)
    n = len(nbr)
    vals = np.asarray(vals).astype(np.int64)
    assert len(vals) == n
    ids = np.arange(n, dtype=np.uint64) if keys is None else np.asarray(keys, dtype=np.uint64)
    assert len(ids) == n
    alive = np.ones(n, dtype=bool)
    out = []
    thr = 1
    while n:
        lab = labels(nbr, alive)
        idx = np.flatnonzero(alive)
        _, inv, sizes = np.unique(lab[idx], return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        weights = np.zeros(len(sizes), dtype=np.int64)
        np.add.at(weights, inv, vals[idx])
        dropped = sizes < b1
        kept = ~dropped & (sizes <= b2)
        big = ~dropped & ~kept
        order = np.lexsort((ids[idx], inv))                 # by component, members ascending
        starts = np.concatenate([[0], np.cumsum(sizes)])
        members = ids[idx][order]
        for c in np.flatnonzero(kept).tolist():
            out.append((int(sizes[c]), int(weights[c]), thr, members[starts[c]:starts[c + 1]].copy()))
        stay = big[inv] & (vals[idx] >= thr + 1)
        if levels is not None:
            levels.append(dict(thr=thr, alive=len(idx), nkept=int(kept.sum()), nkm=int(sizes[kept].sum()), nbig=int(big.sum()), na=int(stay.sum())))
            if masks:
                levels[-1]["mask"] = alive
        if not big.any():
            break
        alive = np.zeros(n, dtype=bool)
        alive[idx[stay]] = True
        thr += 1
    out.sort(key=lambda c: (c[2], -c[1], -c[0], int(c[3][0])))
    return out


def component_sizes(nbr, alive=None):
    """sizes of the components of the graph induced on the alive vertices (all of them by default), ascending"""
    nbr = np.asarray(nbr, dtype=np.uint32).reshape(-1, 8)
    alive = np.ones(len(nbr), dtype=bool) if alive is None else alive
    lab = labels(nbr, alive)
    return np.sort(np.unique(lab[lab >= 0], return_counts=True)[1])


# ---- what a graph offers the kernels' paths (for the tests' conditions; the only place here that knows of tiles) ----

def is_symmetric(nbr):
    nbr = np.asarray(nbr, dtype=np.uint32).reshape(-1, 8)
    n = len(nbr)
    src = np.repeat(np.arange(n, dtype=np.int64), 8)
    dst = nbr.reshape(-1).astype(np.int64)
    ok = dst != NONE
    if np.any(dst[ok] >= n):
        return False
    fwd = np.sort(src[ok] * n + dst[ok])
    back = np.sort(dst[ok] * n + src[ok])
    return bool(np.array_equal(fwd, back))


def degrees(nbr):
    return (np.asarray(nbr, dtype=np.uint32).reshape(-1, 8) != NONE).sum(axis=1)


def edges_to_smaller_tiles(nbr, alive=None):
    """-> int64 [tiles]: per tile of 1024 consecutive vertices, the slots of its alive vertices that hold a vertex of a smaller tile (what
    k_cc_hook_tile collects: the other end's being alive is looked at later, a doubled edge counts twice)"""
    nbr = np.asarray(nbr, dtype=np.uint32).reshape(-1, 8)
    n = len(nbr)
    alive = np.ones(n, dtype=bool) if alive is None else np.asarray(alive, dtype=bool)
    v = np.arange(n, dtype=np.int64)[:, None]
    u = nbr.astype(np.int64)
    out = (u != NONE) & (u < (v // TILE) * TILE) & alive[:, None]
    return np.bincount((v // TILE).reshape(-1).repeat(8)[out.reshape(-1)], minlength=(n + TILE - 1) // TILE)


def edge_list_counters(nbr, alive=None):
    """-> (ecount[0] as k_cc_hook_tile leaves it, a tile overflowed its LDS list, the global list overflowed)"""
    per = edges_to_smaller_tiles(nbr, alive)
    listed = int(np.minimum(per, LEDGE).sum())
    return listed, bool((per > LEDGE).any()), listed > ecap(len(np.asarray(nbr).reshape(-1, 8)))


def distinct_parents_after_tile(nbr, tile):
    """the distinct roots of a tile's vertices when only the edges inside the tile are joined (the parent values k_cc_hook_tile leaves)"""
    nbr = np.asarray(nbr, dtype=np.uint32).reshape(-1, 8)
    lo, hi = tile * TILE, min((tile + 1) * TILE, len(nbr))
    sub = nbr[lo:hi].astype(np.int64)
    inside = (sub != NONE) & (sub >= lo) & (sub < hi)
    local = np.where(inside, sub - lo, NONE).astype(np.uint32)
    return len(np.unique(labels(local, np.ones(hi - lo, dtype=bool))))


def roots_per_wave(nbr, alive):
    """the vertices `alive` in ascending order, 64 to a wave: the smallest number of different components in a full wave"""
    lab = labels(nbr, alive)
    lab = lab[lab >= 0]
    full = len(lab) // 64
    assert full >= 1
    return min(len(np.unique(lab[i * 64:(i + 1) * 64])) for i in range(full))


# ---- generators ----

def from_edges(n, u, v, rng=None):
    """nbr [n, 8] of the undirected edges u[i] - v[i] (a pair given twice takes two slots at either end, u == v one slot); the slots are
    filled from the left, or at random places with rng.  More than eight slots at a vertex: AssertionError"""
    u = np.asarray(u, dtype=np.int64).reshape(-1)
    v = np.asarray(v, dtype=np.int64).reshape(-1)
    assert len(u) == len(v) and (len(u) == 0 or (min(u.min(), v.min()) >= 0 and max(u.max(), v.max()) < n))
    loop = u == v
    src = np.concatenate([u, v[~loop]])
    dst = np.concatenate([v, u[~loop]])
    order = np.argsort(src, kind="stable")
    src, dst = src[order], dst[order]
    first = np.searchsorted(src, src, side="left")
    slot = np.arange(len(src)) - first
    assert len(slot) == 0 or slot.max() < 8, "a vertex with more than eight neighbours"
    nbr = np.full((n, 8), NONE, dtype=np.uint32)
    nbr[src, slot] = dst.astype(np.uint32)
    if rng is not None and n:
        perm = np.argsort(rng.random((n, 8)), axis=1)
        nbr = np.take_along_axis(nbr, perm, axis=1)
    return nbr


def stride_graph(n, stride, lo=None, hi=None):
    """edges v - (v - stride) for v in [max(lo, stride), hi)"""
    v = np.arange(max(stride, stride if lo is None else lo), n if hi is None else hi, dtype=np.int64)
    return from_edges(n, v, v - stride)


def path_graph(n):
    return stride_graph(n, 1) if n else np.zeros((0, 8), dtype=np.uint32)


def lds_overflow_graph():
    """n = 4096: every vertex of tile 3 is joined to v - 1024, v - 2048 and v - 3072: 3072 edges to smaller tiles from one tile, 1024
    components of four"""
    v = np.arange(3 * TILE, 4 * TILE, dtype=np.int64)
    return from_edges(4 * TILE, np.concatenate([v, v, v]), np.concatenate([v - TILE, v - 2 * TILE, v - 3 * TILE]))


def permuted_path(n, pieces=None, mult=1025):
    """a path whose i-th vertex is (i * mult) mod n (consecutive vertices of the path lie in different tiles for n = 65536, mult = 1025).
    pieces: the path is cut into pieces of these lengths, in this order from its start (they must add up to n).
    -> (nbr, position -> vertex)"""
    pos = (np.arange(n, dtype=np.int64) * mult) % n
    assert len(np.unique(pos)) == n
    joined = np.ones(max(n - 1, 0), dtype=bool)             # joined[i]: path vertex i - path vertex i + 1
    if pieces is not None:
        assert sum(pieces) == n
        ends = np.cumsum(pieces)[:-1]
        joined[ends - 1] = False
    i = np.flatnonzero(joined)
    return from_edges(n, pos[i], pos[i + 1]), pos


def staggered_values(n, stride, run=2, period=8):
    """for stride_graph(n, stride) made oversize: value 2 where (v // stride) % period < run, else 1 -- at level 2 every chain falls into
    pieces of `run` vertices, `stride` pieces side by side in the order of the vertices; one vertex in period / run survives"""
    v = np.arange(n)
    return np.where((v // stride) % period < run, 2, 1).astype(np.uint16)


def handover_graph(b1, b2, n=12 * TILE, sizes=None):
    """One path v - v + 1 over n vertices whose values make the threshold loop take every hand-over between its levels (b2 < 1500):

        core      1500 vertices of value 4
        region 3  1500 vertices: value 3, with islands of value 4 between single vertices of value 3
        region 2  3000 vertices: value 2, with islands of value 3 between single vertices of value 2
        region 1  the rest: value 1, with islands of value 2 between single vertices of value 1

    level 1 is one component; at level t = 2, 3, 4 the core and the regions >= t still hang together (oversize) while the islands of
    region t - 1 stand alone; at level 4 the core is oversize and none of it has value 5: level 5 starts with nothing.  The islands take
    the sizes `sizes` in turn (default b1 - 1, b1, b2, between the two); every third island of the regions 1 and 2 has one vertex of a value
    one higher (no vertex has value 5).  -> (nbr, vals)"""
    if sizes is None:
        sizes = [s for s in (b1 - 1, b1, b2, (b1 + b2) // 2) if s >= 1]
    vals = []

    def region(length, base, count, spikes=True):
        seg = np.full(length, base, dtype=np.int64)
        at, made = 1, 0
        while made < count:
            s = sizes[made % len(sizes)]
            assert at + s + 1 <= length
            seg[at:at + s] = base + 1
            if spikes and made % 3 == 0:
                seg[at + s // 2] = base + 2
            at += s + 1
            made += 1
        return seg
    vals.append(np.full(1500, 4, dtype=np.int64))
    vals.append(region(1500, 3, 12, spikes=False))
    vals.append(region(3000, 2, 12))
    vals.append(region(n - 6000, 1, 24))
    return path_graph(n), np.concatenate(vals).astype(np.uint16)


def random_graph(seed, n, mean_degree):
    """n * mean_degree / 2 random pairs on randomly permuted ids; the edges that would be a ninth at one of their ends are left out.
    Values 1 + the number of successes in a row at 0.85, at most 12.  -> (nbr, vals)"""
    rng = np.random.default_rng(seed)
    m = int(n * mean_degree / 2)
    u = rng.integers(0, n, size=m)
    v = rng.integers(0, n, size=m)
    keep = u != v
    u, v = u[keep], v[keep]
    while True:
        src = np.concatenate([u, v])
        order = np.argsort(src, kind="stable")
        rank = np.empty(len(src), dtype=np.int64)
        s = src[order]
        rank[order] = np.arange(len(s)) - np.searchsorted(s, s, side="left")
        over = (rank[:len(u)] >= 8) | (rank[len(u):] >= 8)
        if not over.any():
            break
        u, v = u[~over], v[~over]
    perm = rng.permutation(n)
    vals = np.minimum(rng.geometric(0.15, size=n), 12).astype(np.uint16)
    return from_edges(n, perm[u], perm[v], rng), vals


def pick_bounds(nbr):
    """b1, b2 from the sizes of the graph's own components: b1 the second smallest size that occurs, b2 the size six tenths of the way up
    the list of the different sizes (some component is larger)"""
    sizes = np.unique(component_sizes(nbr))
    assert len(sizes) >= 4
    return int(sizes[1]), int(sizes[min(int(0.6 * len(sizes)), len(sizes) - 2)])


# ---- the crafted cases of tests/test_cc_gpu.py (tests/test_cc_ref_cpu.py checks on the CPU that each one meets its condition) ----

class Case:
    """a graph, its bounds, and what it is there to reach.  want: pattern -- a letter per threshold level with the survivor lists on, D a
    dense level and S one on the list; lds / glob -- level 1 overflows a tile's LDS edge list / the global edge list; m0 -- the last level
    starts with no vertex at all; plus the case's own figures (checked by check_case)"""
    def __init__(self, nbr, vals, b1, b2, **want):
        self.nbr, self.vals, self.b1, self.b2, self.want = nbr, np.asarray(vals, dtype=np.uint16), b1, b2, want
        self.n = len(nbr)
        self._ref = None

    def ref(self):
        """(components, levels) of the reference, computed once"""
        if self._ref is None:
            levels = []
            self._ref = (cut(self.nbr, self.vals, self.b1, self.b2, levels=levels, masks=True), levels)
        return self._ref


def _vals(n, period):
    return (1 + np.arange(n) % period).astype(np.uint16)


def _pieces(b1, b2, n):
    cycle = [b1 - 1, b1, b2, b2 + 1]
    out = cycle * (n // sum(cycle))
    return out + [n - sum(out)]


CASES = {}
for _n in (0, 1, 1023, 1024, 1025, 2049):
    CASES[f"path_kept_{_n}"] = lambda n=_n: Case(path_graph(n), _vals(n, 5), 1, max(n, 1), pattern="D" if n else "", lds=False, glob=False, ncomp=1 if n else 0)
    CASES[f"path_dies_{_n}"] = lambda n=_n: Case(path_graph(n), np.ones(n), 1, 1, pattern="DS" if n > 1 else "D" if n else "", lds=False, glob=False,
                                                 m0=n > 1, ncomp=1 if n == 1 else 0)
CASES["lds_overflow"] = lambda: Case(lds_overflow_graph(), _vals(4096, 7), 4, 4, pattern="D", lds=True, glob=False, ncomp=1024, ecount0=2048)
CASES["global_overflow_8192"] = lambda: Case(stride_graph(8192, 1024), _vals(8192, 7), 1, 8, pattern="D", lds=False, glob=True, ncomp=1024, ecount0=7168)
CASES["list_complete_3072"] = lambda: Case(stride_graph(3072, 1024), _vals(3072, 7), 1, 8, pattern="D", lds=False, glob=False, ncomp=1024, ecount0=2048)
CASES["roots_1024_kept"] = lambda: Case(stride_graph(2048, 1024), _vals(2048, 7), 2, 2, pattern="D", lds=False, glob=False, ncomp=1024, parents=(1, 1024))
CASES["roots_1024_dropped"] = lambda: Case(stride_graph(2048, 1024), _vals(2048, 7), 3, 3, pattern="D", lds=False, glob=False, ncomp=0, parents=(1, 1024))
CASES["deep_forest"] = lambda: Case(permuted_path(65536)[0], _vals(65536, 7), 1, 65536, pattern="D", lds=False, glob=True, ncomp=1)
CASES["deep_forest_pieces"] = lambda: Case(permuted_path(65536, _pieces(100, 1000, 65536))[0], _vals(65536, 3), 100, 1000, lds=False, glob=True,
                                            level1_sizes=(100, 1000), ncomp=2 * (65536 // 2201))
for _s in (8, 16):
    CASES[f"wave_tails_{_s}"] = lambda s=_s: Case(stride_graph(4096, s), _vals(4096, 5), 4096 // s, 4096 // s, pattern="D", lds=False, glob=False, ncomp=s,
                                                  wave_roots=(1, s))
    CASES[f"wave_tails_{_s}_sparse"] = lambda s=_s: Case(stride_graph(4096, s), staggered_values(4096, s), 2, 2, pattern="DS", lds=False, glob=False, ncomp=512,
                                                         wave_roots=(2, 32))
CASES["handover"] = lambda: Case(*handover_graph(5, 40), 5, 40, pattern="DDSSS", lds=False, glob=False, m0=True, lists="0111")
CASES["handover_b1_eq_b2"] = lambda: Case(*handover_graph(5, 5), 5, 5, pattern="DDSSS", lds=False, glob=False, m0=True, lists="0111")
CASES["handover_b2_lt_b1"] = lambda: Case(*handover_graph(40, 5, sizes=[5, 17, 39, 40, 45]), 40, 5, pattern="DDSSS", lds=False, glob=False, m0=True, lists="0111",
                                          ncomp=0)

RANDOM = [(seed, n, (1.0, 3.0)[seed & 1]) for n in (20_000, 200_003) for seed in range(6)]


def random_case(seed, n, mean_degree):
    nbr, vals = random_graph(seed, n, mean_degree)
    b1, b2 = pick_bounds(nbr)
    return Case(nbr, vals, b1, b2, lds=mean_degree > 2, glob=mean_degree > 2, min_levels=3, sizes_occur=(b1, b2))


def level_mask(levels, i, n):
    return levels[i]["mask"] if i < len(levels) else np.zeros(n, dtype=bool)


def expected_trace(case, sparse_opt):
    """what the cutter's trace must read for this case, from the reference's levels and the rule the threshold loop hands its levels
    over by: [dict] with the fields of the trace that are certain (ecount1 as a bool: the list was incomplete)"""
    _, levels = case.ref()
    n = case.n
    out, sparse = [], False
    for lv in levels:
        want_list = bool(lv["nbig"]) and bool(sparse_opt)
        stands = want_list and (sparse or lv["na"] <= lcap(n))
        e = dict(thr=lv["thr"], sparse=int(sparse), visited=lv["alive"] if sparse else n, nkept=lv["nkept"], nkm=lv["nkm"], nbig=lv["nbig"], na=lv["na"],
                 want_list=int(want_list), list_stands=int(stands))
        if sparse:
            e.update(ecount0=0, incomplete=False)
        else:
            listed, lds, glob = edge_list_counters(case.nbr, lv["mask"])
            e.update(ecount0=listed, incomplete=lds or glob)
        out.append(e)
        sparse = sparse or stands
    return out


def check_case(case):
    """the arithmetic that makes a case reach its path, from the graph and the reference alone"""
    nbr, n, want = case.nbr, case.n, case.want
    assert nbr.shape == (n, 8) and nbr.dtype == np.uint32
    assert is_symmetric(nbr)
    assert n == 0 or (1 <= case.vals.min() and case.vals.max() <= MAX_COUNT)
    comps, levels = case.ref()
    trace = expected_trace(case, 1)
    if "pattern" in want:
        assert "".join("DS"[e["sparse"]] for e in trace) == want["pattern"]
    if n:
        per = edges_to_smaller_tiles(nbr)
        listed, lds, glob = edge_list_counters(nbr)
        assert lds == want["lds"] == bool(per.max() > LEDGE), per.max()
        assert glob == want["glob"] == (listed > ecap(n)), (listed, ecap(n))
        if "ecount0" in want:
            assert listed == want["ecount0"]
    if want.get("m0"):
        assert trace[-1]["sparse"] and trace[-1]["visited"] == 0 and trace[-2]["nbig"] > 0 and trace[-2]["na"] == 0
    if "ncomp" in want:
        assert len(comps) == want["ncomp"]
    if "parents" in want:
        tile, count = want["parents"]
        assert distinct_parents_after_tile(nbr, tile) == count
    if "wave_roots" in want:
        level, count = want["wave_roots"]
        assert roots_per_wave(nbr, levels[level - 1]["mask"]) >= count > 6 - 2 * (level == 1)       # k_cc_members groups 4 rounds, k_ccs_stats 6
        if level == 2:
            assert trace[1]["sparse"] and levels[0]["na"] <= lcap(n)
    if "lists" in want:                                      # the list of level i + 1 stood: 0 = asked for and too short
        assert [e["want_list"] for e in trace[:4]] == [1, 1, 1, 1] and "".join(str(e["list_stands"]) for e in trace[:4]) == want["lists"]
        assert levels[0]["na"] > lcap(n) >= levels[1]["na"]
        if case.b1 <= case.b2:                               # (components are kept on a list as well)
            assert levels[2]["nkept"] and levels[3]["nkept"]
    if "level1_sizes" in want:
        b1, b2 = want["level1_sizes"]
        sizes = component_sizes(nbr)
        for s in (b1 - 1, b1, b2, b2 + 1):
            assert (sizes == s).sum() >= 1
        assert {c[0] for c in comps if c[2] == 1} == {b1, b2}
    if "min_levels" in want:
        assert len(levels) >= want["min_levels"], len(levels)
    if "sizes_occur" in want:
        got = {c[0] for c in comps}
        assert set(want["sizes_occur"]) <= got and max(component_sizes(nbr)) > case.b2
