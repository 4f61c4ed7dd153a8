"""The neighbour look-up of the k = 32 ... 63 tables neighbour by neighbour: k_windex_build, w_side_walk / w_neighbours behind k_w_cc_adjacency and
k_w_ut_flags, mf_windex_find behind k_w_lookup (metafast_amd/csrc/mf_wgraph.hip, mf_wide.h) on tables made up on the host, bit for bit against
tests/ut_ref.py (_neighbours_wide, flags) and a dictionary.

mf_debug_wide_neighbours (the end of mf_wgraph.hip; bound here with ctypes, not part of the C-ABI) takes distinct canonical ascending k-mers and
look-up queries, builds the index with mf_windex_build, launches the production kernels unchanged and hands back the adjacency, the U1 arrays, the
look-up values and the index itself.  The tables are tests/wnbr_ref.py's, and tests/test_wnbr_ref_cpu.py asserts what each is made for:

    fan          all sixteen a + I + b in one cluster with one tag; 0 .. 4 neighbours on a side; both strands on one side; keys equal in their low word
    palindromes  (even k) a palindromic vertex, a palindromic neighbour (once, strand bit 0), a palindromic interior (sixteen strings, ten k-mers)
    loops        the hairpin a + w, w = rc(w) (odd k); code 0 k times; the windows of (AC)^n, (AT)^n, (ACGT)^n, (AATT)^n
    collision    two interiors with one tag and one home slot, every second sibling behind each
    seam         (k = 47, 62, 63) two such interiors that also share their last 31 bases: keys equal in low word, tag and home slot, the fan of one absent
    wrap1024     a fan whose cluster runs over the end of the index to slot 0; wrap2048: the same among 513 keys, 2048 slots
    empty        no k-mer: no index, every query -1
    broad        the ~5 000 k-mers of fifty reads: the crafted cases did not over-fit the hook

For every table: the adjacency, the flags, the look-ups (every key, siblings with an absent end base, keys equal to a present one in one word, keys
whose home slot is empty, random ones -- also through the public mf_wtable_lookup on a table loaded from a wide k-mers file), and the invariants of the
returned index against the numpy port of its hash.  The order inside a cluster is left free: it depends on which atomicCAS wins.  For the small
tables also components and unitigs through the public entry points against the 128-bit oracle, which ties the hook's kernels to what production
launches."""
import ctypes as C

import numpy as np
import pytest

import ut_ref as UR
import wide_files_ref as WF
import wnbr_ref as W
from util import canon_seq

pytestmark = pytest.mark.gpu

ALL = [(name, k) for k in W.KS for name in W.case_names(k)]
SMALL = [(name, k) for name, k in ALL if name not in ("broad", "empty")]


def debug_wide_neighbours(ctx, k, hi, lo, cnt, q_hi=None, q_lo=None, slots_room=None):
    """-> dict(nbr [n, 8], info, ridx, lidx, pal [n], values [m], cap, slots [cap])"""
    from metafast_amd import lib as L
    fn = L.lib().mf_debug_wide_neighbours
    fn.restype = C.c_int
    vp, u64 = C.c_void_p, C.c_uint64
    fn.argtypes = [vp, C.c_int, u64, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp, u64]
    hi, lo = np.ascontiguousarray(hi, dtype=np.uint64), np.ascontiguousarray(lo, dtype=np.uint64)
    cnt = np.ascontiguousarray(cnt, dtype=np.uint16)
    n = len(hi)
    m = 0 if q_hi is None else len(q_hi)
    if m:
        q_hi, q_lo = np.ascontiguousarray(q_hi, dtype=np.uint64), np.ascontiguousarray(q_lo, dtype=np.uint64)
    room = W.cap_of(n) if slots_room is None else slots_room
    nbr = np.full((n, 8), 0xDEADBEEF, dtype=np.uint32)
    info, pal = np.full(n, 0xEE, dtype=np.uint8), np.full(n, 0xEE, dtype=np.uint8)
    ridx, lidx = np.full(n, 0xDEADBEEF, dtype=np.uint32), np.full(n, 0xDEADBEEF, dtype=np.uint32)
    values = np.full(m, -7, dtype=np.int32)
    slots = np.zeros(max(room, 1), dtype=np.uint64)
    cap = u64(12345)
    p = lambda a, on: a.ctypes.data if on else None
    L._check(fn(ctx.h, k, n, p(hi, n), p(lo, n), p(cnt, n), m, p(q_hi, m) if m else None, p(q_lo, m) if m else None, p(nbr, n), p(info, n), p(ridx, n),
                p(lidx, n), p(pal, n), p(values, m), C.byref(cap), p(slots, n), room))
    return dict(nbr=nbr, info=info, ridx=ridx, lidx=lidx, pal=pal, values=values, cap=cap.value, slots=slots[:cap.value])


_runs = {}


def run(ctx, name, k):
    """per table, once: the hook with the queries of wnbr_ref.queries"""
    if (name, k) not in _runs:
        t = W.get_case(name, k)
        q, want, kinds = W.queries(t)
        qhi, qlo = W.split(q)
        out = debug_wide_neighbours(ctx, k, t.hi, t.lo, t.counts, qhi, qlo)
        out.update(t=t, q=q, want=want, kinds=kinds)
        _runs[name, k] = out
    return _runs[name, k]


def explain(t, got, want):
    """the first wrong neighbours: case, k, the vertex as bases, the slot as (nucleotide, side), got / wanted"""
    bad = np.argwhere(got != want)
    lines = ["case %s, k = %d: %d wrong neighbours of %d" % (t.name, t.k, len(bad), got.size)]
    for v, s in bad[:12].tolist():
        lines.append("vertex %d %s, slot %d (%s, %s): got %#x, wanted %#x" % (v, W.bases(t.keys[v], t.k), s, W.NUC[s >> 1], "left" if s & 1 else "right", got[v, s], want[v, s]))
    return "\n".join(lines)


def explain_flags(t, what, got, want):
    bad = np.flatnonzero(got != want)
    lines = ["case %s, k = %d: %d wrong %s of %d" % (t.name, t.k, len(bad), what, len(got))]
    for v in bad[:12].tolist():
        lines.append("vertex %d %s: got %#x, wanted %#x" % (v, W.bases(t.keys[v], t.k), got[v], want[v]))
    return "\n".join(lines)


@pytest.mark.parametrize("name,k", ALL)
def test_adjacency_neighbour_by_neighbour(gpu_ctx, name, k):
    r = run(gpu_ctx, name, k)
    t = r["t"]
    want = t.neighbours[0]
    assert r["nbr"].shape == want.shape
    assert np.array_equal(r["nbr"], want), explain(t, r["nbr"], want)


@pytest.mark.parametrize("name,k", ALL)
def test_flags_of_every_vertex(gpu_ctx, name, k):
    """k_w_ut_flags: the info byte (codes and strand bits of both sides), the first neighbour of either side, the palindrome flag (0 everywhere for
    an odd k)"""
    r = run(gpu_ctx, name, k)
    t = r["t"]
    for what, want in zip(("info", "ridx", "lidx", "pal"), t.flags):
        assert np.array_equal(r[what], want), explain_flags(t, what, r[what], want)
    if k % 2:
        assert not r["pal"].any(), "case %s, k = %d: a palindrome at an odd k" % (name, k)


def _explain_lookup(t, q, kinds, got, want):
    bad = np.flatnonzero(got != want)
    lines = ["case %s, k = %d: %d wrong look-ups of %d" % (t.name, t.k, len(bad), len(got))]
    for i in bad[:12].tolist():
        lines.append("query %d %s (%s; hi %#x lo %#x): got %d, wanted %d" % (i, W.bases(q[i], t.k), kinds[i], q[i] >> 64, q[i] & W.M64, got[i], want[i]))
    return "\n".join(lines)


@pytest.mark.parametrize("name,k", ALL)
def test_lookup_present_absent_and_across_the_seam(gpu_ctx, name, k):
    r = run(gpu_ctx, name, k)
    assert np.array_equal(r["values"], r["want"]), _explain_lookup(r["t"], r["q"], r["kinds"], r["values"], r["want"])


@pytest.mark.parametrize("name,k", [(n, k) for n, k in ALL if n != "empty"])
def test_lookup_of_keys_whose_home_slot_is_empty(gpu_ctx, name, k):
    """the probe that ends at once; m = 0 on the way (the first call of this test asks nothing)"""
    r = run(gpu_ctx, name, k)
    t = r["t"]
    rng = np.random.default_rng(9000 + k)
    cand = W.random_canonical(rng, k, 400, avoid=t.keys)
    home, _ = W.home_tag(W.hash_of_keys(cand, k), r["cap"])
    q = [x for x, h in zip(cand, home.tolist()) if r["slots"][h] == W.EMPTY]
    assert len(q) >= 100                                    # (load <= 0.5)
    again = debug_wide_neighbours(gpu_ctx, k, t.hi, t.lo, t.counts)
    assert len(again["values"]) == 0 and np.array_equal(again["nbr"], r["nbr"]) and again["cap"] == r["cap"]
    assert np.array_equal(again["slots"] == W.EMPTY, r["slots"] == W.EMPTY)       # (which slots are taken does not depend on who came first)
    qhi, qlo = W.split(q)
    got = debug_wide_neighbours(gpu_ctx, k, t.hi, t.lo, t.counts, qhi, qlo)["values"]
    assert (got == -1).all(), _explain_lookup(t, q, ["empty home"] * len(q), got, np.full(len(q), -1))


@pytest.mark.parametrize("name,k", ALL)
def test_index_invariants(gpu_ctx, name, k):
    """every table position once, under the tag of the ported hash, reachable from its home slot without crossing an empty slot; as many slots taken as
    there are keys; the smallest power of two >= max(1024, 2 n) slots"""
    r = run(gpu_ctx, name, k)
    t = r["t"]
    n, cap, slots = len(t), r["cap"], r["slots"]
    assert cap == W.cap_of(n) and len(slots) == cap, (name, k, cap)
    if n == 0:
        return
    assert cap >= max(1024, 2 * n) and cap & (cap - 1) == 0 and (cap == 1024 or cap // 2 < 2 * n)
    taken = np.flatnonzero(slots != W.EMPTY)
    assert len(taken) == n, "case %s, k = %d: %d slots taken, %d keys" % (name, k, len(taken), n)
    pos = (slots[taken] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    tag = (slots[taken] >> np.uint64(32)).astype(np.int64)
    assert np.array_equal(np.sort(pos), np.arange(n)), "case %s, k = %d: the positions in the index are not 0 .. n - 1, each once" % (name, k)
    home, want_tag = W.home_tag(t.hashes, cap)
    bad = np.flatnonzero(tag != want_tag[pos])
    assert not len(bad), "case %s, k = %d: key %s at slot %d has tag %#x, wanted %#x" % (name, k, W.bases(t.keys[pos[bad[0]]], k), taken[bad[0]], tag[bad[0]], want_tag[pos[bad[0]]])
    empty = slots == W.EMPTY
    for s, p in zip(taken.tolist(), pos.tolist()):
        h = int(home[p])
        between = empty[h:s] if h <= s else np.concatenate([empty[h:], empty[:s]])
        assert not between.any(), "case %s, k = %d: key %s (home slot %d) sits at slot %d behind an empty slot" % (name, k, W.bases(t.keys[p], k), h, s)
    if name.startswith("wrap"):                             # 5. the fan's cluster runs over the end
        fk = [t.where[W.canon(x, k)] for x in W.fan(t.note["interior"], k).values()]
        at = {int(p): int(s) for s, p in zip(taken, pos)}
        h = int(home[fk[0]])
        mine = sorted(at[p] for p in fk)
        assert h >= cap - 3 and sum(s < h for s in mine) >= 13, (name, k, h, mine)      # (at most three of the sixteen fit in front of the end)
    if name == "collision":                                 # 4. both fans in one cluster under one tag
        w1, w2 = t.note["interiors"]
        assert len(set(int(want_tag[i]) for i, x in enumerate(t.keys) if min(W.interior(x, k), UR.rc_plain(W.interior(x, k), k - 2)) in (w1, w2))) == 1


def _wide_table(ctx, t, tmp_path):
    p = tmp_path / ("%s_%d.kmers.bin" % (t.name, t.k))
    p.write_bytes(WF.encode_kmers(t.hi, t.lo, t.counts))
    return ctx.load_kmers_wide([str(p)], t.k)


@pytest.mark.parametrize("name,k", [(n, k) for n, k in ALL if n != "empty"])
def test_public_lookup_on_a_table_loaded_from_a_file(gpu_ctx, tmp_path, name, k):
    """the same queries through mf_wtable_lookup: the table's own index (mf_wtable_ensure_index) under the same kernel"""
    r = run(gpu_ctx, name, k)
    t = r["t"]
    wt = _wide_table(gpu_ctx, t, tmp_path)
    hi, lo, cnt = wt.export()
    assert np.array_equal(hi, t.hi) and np.array_equal(lo, t.lo) and np.array_equal(cnt, t.counts)
    got = wt.lookup(r["q"])
    assert np.array_equal(got, r["want"]), _explain_lookup(t, r["q"], r["kinds"], got, r["want"])


def _norm_seqs(seqs):
    return sorted((canon_seq(s), a, mn, mx) for s, a, mn, mx in seqs)


@pytest.mark.parametrize("name,k", SMALL)
def test_components_and_unitigs_of_the_same_tables(gpu_ctx, oracle, tmp_path, name, k):
    """cut_components_wide and build_unitigs_wide on a table of exactly these k-mers against the 128-bit oracle on the same (k-mer, count) pairs"""
    t = W.get_case(name, k)
    wt = _wide_table(gpu_ctx, t, tmp_path)
    ot = oracle.WTable()
    for x, c in zip(t.keys, t.counts.tolist()):
        ot.add(x, c)
    want = _norm_seqs(oracle.wide_build_unitigs(ot, k, 0, k).all())
    got = _norm_seqs(gpu_ctx.build_unitigs_wide(wt, 0, k).export())
    assert len(want) > 0 and got == want, (name, k)
    levels, largest = set(), 0
    for b1, b2 in ((1, 100000), (2, 8)):
        wc = oracle.wide_cut_components(ot, k, b1, b2).all()
        gc = gpu_ctx.cut_components_wide(wt, b1, b2).export()
        assert [(int(a), int(w), int(th)) for a, w, th in zip(gc["sizes"], gc["weights"], gc["thr"])] == [(a, w, th) for a, w, th, _ in wc], (name, k, b1, b2)
        at = 0
        for n, _, th, km in wc:
            assert np.array_equal(gc["hi"][at:at + n], km["hi"]) and np.array_equal(gc["lo"][at:at + n], km["lo"]), (name, k, b1, b2)
            at += n
            levels.add(th)
            largest = max(largest, n)
        assert at == len(gc["hi"]) and len(wc) >= 1
    assert largest <= 8 or len(levels) >= 2, "a component above the small bound must be split at a higher threshold"


def test_the_hook_refuses_what_is_no_table(gpu_ctx):
    """everything is checked on the host before a launch"""
    from metafast_amd import lib as L
    k = 47
    t = W.get_case("fan", k)
    hi, lo, cnt = t.hi.copy(), t.lo.copy(), t.counts.copy()

    def refused(match, k=k, hi=hi, lo=lo, cnt=cnt, **kw):
        with pytest.raises(L.MetafastError, match=match):
            debug_wide_neighbours(gpu_ctx, k, hi, lo, cnt, **kw)

    refused(r"k = 31", k=31)
    refused(r"k = 64", k=64)
    refused("not above", hi=hi[::-1].copy(), lo=lo[::-1].copy())
    refused("not above", hi=np.concatenate([hi[:1], hi]), lo=np.concatenate([lo[:1], lo]), cnt=np.concatenate([cnt[:1], cnt]))
    rc = UR.rc_plain(t.keys[3], k)
    assert rc > t.keys[3]
    keys = sorted(t.keys[:3] + t.keys[4:] + [rc])
    nhi, nlo = W.split(keys)
    refused("not canonical", hi=nhi, lo=nlo)
    big = hi.copy(); big[-1] |= np.uint64(1 << (2 * k - 64))
    refused("does not fit", hi=big)
    zero = cnt.copy(); zero[5] = 0
    refused("count 0", cnt=zero)
    over = cnt.copy(); over[5] = 32768
    refused("count 32768", cnt=over)
    refused("room for 512 index slots", slots_room=512)
