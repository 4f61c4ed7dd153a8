"""features-calculator for k = 32 ... 63 on the GPU (mf_wfeatures.hip) against tests/wfeatures_ref.py, exactly: vec equal, breadth bit-equal,
NaN at the same places.  Components come from files the test writes (mf_wcomps_load), from seq2comp_wide and from the device cutter; the
shapes are the smallest where the kernels can go wrong -- reads around the border of a run of positions, both words of a k-mer, listings
that repeat (the insert-or-find index), counts above 32767.  What the reference itself computes is pinned in tests/test_wfeatures_cpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import wfeatures_ref as R
import wide_files_ref as WF
from util import pack_reads, to_device

pytestmark = pytest.mark.gpu

KS = (32, 33, 40, 63)
THRS = (-1, 0, 1, 3)


def _rnd(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _dev(reads):
    """reads in HBM with NO slack behind the last base: the last read ends exactly at n_bases and at the buffer's end"""
    import torch
    bases, off = pack_reads(reads)
    tb = torch.from_numpy(bases.copy()).cuda() if len(bases) else torch.zeros(1, dtype=torch.uint8, device="cuda")
    to = torch.from_numpy(off.view(np.int64).copy()).cuda()
    return tb, to, len(reads), int(off[-1])


def _reads_features(ctx, comps, reads, thr=0, selected=None):
    tb, to, n, nb = _dev(reads)
    return ctx.features_reads_wide(comps, tb.data_ptr(), to.data_ptr(), n, nb, thr, selected)


def _members(seq, k):
    return sorted(set(R.canonical_kmers(seq, k)))


def _load_comps(ctx, tmp_path, comps, k, name="components.bin"):
    hi, lo = R.words([x for m in comps for x in m])
    p = tmp_path / name
    p.write_bytes(WF.encode_components([len(m) for m in comps], [len(m) for m in comps], hi, lo))
    return ctx.load_components_wide(str(p), k)


def _load_table(ctx, tmp_path, table, k, name):
    keys = sorted(table)
    hi, lo = R.words(keys)
    p = tmp_path / name
    p.write_bytes(WF.encode_kmers(hi, lo, [table[x] for x in keys]))
    return ctx.load_kmers_wide([str(p)], k)


def _same(got, exp):
    assert got[0].dtype == np.int64 and np.array_equal(got[0], exp[0])
    assert np.array_equal(np.isnan(got[1]), np.isnan(exp[1]))
    assert got[1][~np.isnan(got[1])].tobytes() == exp[1][~np.isnan(exp[1])].tobytes()


def _fw(read, k):
    """the k-mers of a read as they stand (not canonical)"""
    return {R.encode(read[i:i + k]) for i in range(len(read) - k + 1)}


def _edge_case(k, seed=5):
    """-> (components as member lists, reads): two components that share a stretch, an empty one, a one-member one, a palindrome (even k),
    a member that occurs only as its reverse complement; reads of k - 1 ... k + 33 bases, some reverse-complemented, some lower case"""
    rng = np.random.default_rng(seed + k)
    g = _rnd(rng, 420)
    run = R_RUN[0]
    comps = [_members(g[0:200], k), _members(g[100:290], k), [], _members(g[300:300 + k], k)]
    only_rc = g[330:330 + k]
    comps.append(_members(only_rc, k))
    reads = [g[290:310 + k]]
    for i, n in enumerate(sorted({k - 1, k, k + 1, k + 31, k + 32, k + 33, k + run - 1, k + run, k + run + 1, 2 * run + k, 150})):
        for st in (0, 97, 118):
            r = g[st:st + n]
            reads.append(r.lower() if (i + st) % 3 == 0 else (R.revcomp_str(r) if (i + st) % 3 == 1 else r))
    # only_rc is in the reads as the reverse complement of its canonical text, never as that text itself
    reads.append(R.revcomp_str(g[325:340 + k]) if R.encode(only_rc) == comps[4][0] else g[325:340 + k])
    assert all(WF.revcomp(comps[4][0], k) in _fw(r, k) and comps[4][0] not in _fw(r, k) for r in reads[-1:]) or WF.revcomp(comps[4][0], k) == comps[4][0]
    if k % 2 == 0:
        h = _rnd(rng, k // 2)
        pal = h + R.revcomp_str(h)
        comps.append(_members(pal, k))
        assert len(comps[-1]) == 1 and WF.revcomp(comps[-1][0], k) == comps[-1][0]
        reads += [pal, "AC" + pal + "GT"]
    reads.append(g[200:200 + k + 1])                             # the last read ends the buffer
    return comps, reads


R_RUN = []


@pytest.fixture(scope="module", autouse=True)
def _run_length(gpu_ctx):
    R_RUN.append(gpu_ctx.stat("wf_run"))
    assert R_RUN[0] >= 32
    yield
    R_RUN.clear()


@pytest.mark.parametrize("k", KS)
def test_edges(gpu_ctx, tmp_path, k):
    comps, reads = _edge_case(k)
    hm = R.presence(comps, reads, k)
    assert set(comps[0]) & set(comps[1]) and hm[comps[4][0]] >= 1 and hm[comps[3][0]] >= 1
    if k == 32:
        assert all(x >> 64 == 0 for m in comps for x in m)
    else:
        assert any(x >> 64 for m in comps for x in m)
    c = _load_comps(gpu_ctx, tmp_path, comps, k)
    twice = _load_comps(gpu_ctx, tmp_path, comps + comps, k, "twice.bin")      # one component file given twice: every k-mer is listed twice
    for thr in (-1, 0, 1):
        exp = R.from_reads(comps, reads, k, thr)
        assert np.isnan(exp[1][2]) and (thr != 0 or exp[0].sum() > 0)
        got = _reads_features(gpu_ctx, c, reads, thr)
        _same(got, exp)
        _same(_reads_features(gpu_ctx, c, reads, thr), got)                     # a second call gives the same
        _same(_reads_features(gpu_ctx, twice, reads, thr), R.from_reads(comps + comps, reads, k, thr))
    # no reads; reads that are all shorter than k
    zero = (np.zeros(len(comps), dtype=np.int64), np.array([0.0 / len(m) if m else np.nan for m in comps]))
    _same(gpu_ctx.features_reads_wide(c, 0, 0, 0, 0, 0), zero)
    _same(_reads_features(gpu_ctx, c, ["ACGT" * 7, "A" * (k - 1)], 0), zero)
    # no components: nothing to do
    none = _load_comps(gpu_ctx, tmp_path, [], k, "none.bin")
    got = _reads_features(gpu_ctx, none, reads, 0)
    assert len(got[0]) == 0 and len(got[1]) == 0
    assert len(gpu_ctx.features_wide(none, _load_table(gpu_ctx, tmp_path, {comps[0][0]: 1}, k, "one.kmers.bin"))[0]) == 0


def test_listings_that_repeat(gpu_ctx, tmp_path):
    """seq2comp_wide of 300 identical sequences, two sequences with a common stretch and one given twice: every member is listed up to 302
    times, and the insert-or-find index sees all listings of a k-mer at once"""
    k = 40
    rng = np.random.default_rng(77)
    g = _rnd(rng, 300)
    seqs = [g[0:100]] * 300 + [g[50:200], g[150:300], g[50:200], "ACGT"]
    fa = tmp_path / "s.fa"
    fa.write_text("".join(f">s{i}\n{s}\n" for i, s in enumerate(seqs)))
    cb = tmp_path / "components.bin"
    assert gpu_ctx.seq2comp_wide([str(fa)], k, str(cb))[0] == len(seqs)
    c = gpu_ctx.load_components_wide(str(cb), k)
    comps = [_members(s, k) for s in seqs]
    assert c.stats() == (len(seqs), sum(len(m) for m in comps))
    reads = [g[0:130], R.revcomp_str(g[40:260]), g[60:60 + k], g[0:100].lower(), g[170:300]]
    sel = {x: 2 for x in comps[0][::2]}
    sel.update({x: 1 for x in comps[301][::3]})
    st = _load_table(gpu_ctx, tmp_path, sel, k, "sel.kmers.bin")
    for thr in (0, 1):
        for s_dev, s_py in ((None, None), (st, sel)):
            exp = R.from_reads(comps, reads, k, thr, s_py)
            got = _reads_features(gpu_ctx, c, reads, thr, s_dev)
            _same(got, exp)
            _same(_reads_features(gpu_ctx, c, reads, thr, s_dev), got)
    assert np.isnan(R.from_reads(comps, reads, k, 0, sel)[1][-1]) and R.from_reads(comps, reads, k, 0)[0][0] == R.from_reads(comps, reads, k, 0)[0][299] > 0


@pytest.mark.parametrize("k", [33, 63])
def test_no_saturation(gpu_ctx, tmp_path, k):
    rng = np.random.default_rng(k)
    read = _rnd(rng, k + 1)
    m = R.canonical_kmers(read, k)
    assert len(set(m)) == 2
    comps = [[m[0]], [m[1]]]
    c = _load_comps(gpu_ctx, tmp_path, comps, k)
    n = 40000
    bases = np.tile(np.frombuffer(read.encode(), dtype=np.uint8), n)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(k + 1)
    tb, to = to_device(bases, off)
    vec, br = gpu_ctx.features_reads_wide(c, tb.data_ptr(), to.data_ptr(), n, int(off[-1]), 0)
    assert vec.tolist() == [40000, 40000] and br.tolist() == [1.0, 1.0]
    t = gpu_ctx.count_wide_table(tb.data_ptr(), to.data_ptr(), n, int(off[-1]), k)
    vec, br = gpu_ctx.features_wide(c, t, 0)
    assert vec.tolist() == [32767, 32767] and br.tolist() == [1.0, 1.0]


def _property_case(k):
    rng = np.random.default_rng(1000 + k)
    g = _rnd(rng, 3000)
    reads = []
    for _ in range(2000):
        n = int(rng.integers(100, 151)); st = int(rng.integers(0, len(g) - n + 1))
        r = g[st:st + n]
        reads.append(R.revcomp_str(r) if rng.integers(0, 2) else r)
    junk = _rnd(rng, 400)
    comps = [_members(g[0:500], k), _members(g[400:900], k), _members(junk, k), [], _members(g[2000:2600] , k), _members(g[2950:], k)]
    return g, reads, comps


@pytest.mark.parametrize("k", [33, 63])
def test_reads_equal_count_then_features(gpu_ctx, oracle, tmp_path, k):
    """where no count saturates the new route and the old one (count_wide + features_wide) are the same function"""
    g, reads, comps = _property_case(k)
    bases, off = pack_reads(reads)
    _, _, cnt, _ = oracle.count_wide(bases, off, k)
    assert 1 < cnt.max() <= 32767
    c = _load_comps(gpu_ctx, tmp_path, comps, k)
    tb, to = to_device(bases, off)
    n, nb = len(reads), int(off[-1])
    table = gpu_ctx.count_wide_table(tb.data_ptr(), to.data_ptr(), n, nb, k)
    flat = [x for m in comps for x in m]
    sel = {x: 1 + i % 5 for i, x in enumerate(flat[::4])}
    sel.update({x: 3 for x in _members(_rnd(np.random.default_rng(k), 60 + k), k)[:5]})      # k-mers outside every component
    st = _load_table(gpu_ctx, tmp_path, sel, k, "sel.kmers.bin")
    exp0 = R.from_reads(comps, reads, k, 0)
    assert exp0[0][0] > 0 and exp0[0][2] == 0 and np.isnan(exp0[1][3])
    for thr in THRS:
        for s_dev, s_py in ((None, None), (st, sel)):
            a = gpu_ctx.features_reads_wide(c, tb.data_ptr(), to.data_ptr(), n, nb, thr, s_dev)
            b = gpu_ctx.features_wide(c, table, thr, s_dev)
            _same(a, b)
            if thr in (0, 3):
                _same(a, R.from_reads(comps, reads, k, thr, s_py))


def test_selected_tables(gpu_ctx, tmp_path):
    k = 33
    comps, reads = _edge_case(k)
    c = _load_comps(gpu_ctx, tmp_path, comps, k)
    sample = R.count(reads, k)
    t = _load_table(gpu_ctx, tmp_path, sample, k, "x.kmers.bin")
    rng = np.random.default_rng(9)
    outside = {x: 7 for x in _members(_rnd(rng, 200), k)}
    assert not set(outside) & {x for m in comps for x in m}
    some = dict(outside)
    some.update({x: 1 for x in comps[0][::2]}); some.update({comps[4][0]: 32767})
    for name, sel in (("some", some), ("outside", outside)):
        st = _load_table(gpu_ctx, tmp_path, sel, k, name + ".kmers.bin")
        for thr in (-1, 0, 2):
            exp = R.from_reads(comps, reads, k, thr, sel)
            _same(_reads_features(gpu_ctx, c, reads, thr, st), exp)
            _same(gpu_ctx.features_wide(c, t, thr, st), R.from_kmers(comps, sample, thr, sel))
            if name == "outside":
                assert np.isnan(exp[1]).all() and not exp[0].any()
            else:
                assert not np.isnan(exp[1][0]) and np.isnan(exp[1][1]) == (not set(comps[0][::2]) & set(comps[1]))
    # the k-mers branch without a selection is what it was
    _same(gpu_ctx.features_wide(c, t, 0), R.from_kmers(comps, sample, 0))


@pytest.mark.parametrize("k", [33, 63])
def test_against_the_oracle_on_device_cut_components(gpu_ctx, oracle, tmp_path, k):
    from util import genome_reads
    rng = np.random.default_rng(100 + k)
    bases, off = genome_reads(rng, 1200, 120, 90, err=0.004)
    otable = oracle.WTable().count_buffer(bases, off, k, 0)
    ocomps = oracle.wide_cut_components(otable.good(1), k, 5, 300)
    assert len(ocomps) >= 2
    tb, to = to_device(bases, off)
    n, nb = len(off) - 1, int(off[-1])
    cutter, _ = gpu_ctx.count_wide_above(tb.data_ptr(), to.data_ptr(), n, nb, k, 1)
    c = gpu_ctx.cut_components_wide(cutter, 5, 300)
    ex = c.export()
    want = ocomps.all()
    assert ex["sizes"].tolist() == [w[0] for w in want]
    assert np.array_equal(ex["hi"], np.concatenate([w[3]["hi"] for w in want])) and np.array_equal(ex["lo"], np.concatenate([w[3]["lo"] for w in want]))
    flat = [x for w in want for x in oracle.w128_to_ints(w[3])]
    sel = oracle.WTable()
    for i, x in enumerate(flat[::3]):
        sel.add(x, 1 + i % 3)
    keys, vals = sel.export()
    (tmp_path / "sel.kmers.bin").write_bytes(WF.encode_kmers(keys["hi"], keys["lo"], vals))
    st = gpu_ctx.load_kmers_wide([str(tmp_path / "sel.kmers.bin")], k)
    for thr in THRS:
        for s_or in (None, sel):
            nc = len(ocomps)
            vec = np.zeros(nc, dtype=np.int64); br = np.zeros(nc, dtype=np.float64)
            b = np.ascontiguousarray(bases, dtype=np.uint8); o = np.ascontiguousarray(off, dtype=np.uint64)
            assert oracle.lib().orw_features_reads_selected(ocomps.h, b.ctypes.data, o.ctypes.data, n, k, thr, s_or.h if s_or is not None else None,
                                                            vec.ctypes.data, br.ctypes.data) == 0
            _same(gpu_ctx.features_reads_wide(c, tb.data_ptr(), to.data_ptr(), n, nb, thr, st if s_or is not None else None), (vec, br))


def test_file_forms(gpu_ctx, tmp_path):
    k = 40
    comps, reads = _edge_case(k)
    _load_comps(gpu_ctx, tmp_path, comps, k)
    cb = str(tmp_path / "components.bin")
    fa, fq = tmp_path / "a.fa", tmp_path / "b.fq"
    half = len(reads) // 2
    fa.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(reads[:half])))
    fq.write_text("".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(reads[half:])))
    sel = {x: 1 for x in comps[1][::2]}
    st = _load_table(gpu_ctx, tmp_path, sel, k, "sel.kmers.bin")
    sample = R.count(reads, k)
    _load_table(gpu_ctx, tmp_path, sample, k, "x.kmers.bin")
    for name, s_dev, s_py in (("plain", None, None), ("sel", st, sel)):
        v, b = str(tmp_path / (name + ".vec")), str(tmp_path / (name + ".breadth"))
        gpu_ctx.features_reads_wide_files(cb, [str(fa), str(fq)], k, 1, v, b, selected=s_dev)
        exp = R.from_reads(comps, reads, k, 1, s_py)
        assert open(v).read() == R.vec_text(exp[0]) and open(b).read() == R.breadth_text(exp[1]) and "NaN" in open(b).read()
        gpu_ctx.features_wide_files(cb, str(tmp_path / "x.kmers.bin"), k, 1, v, b, selected=s_dev)
        exp = R.from_kmers(comps, sample, 1, s_py)
        assert open(v).read() == R.vec_text(exp[0]) and open(b).read() == R.breadth_text(exp[1])
    # no files: the library with no reads
    v, b = str(tmp_path / "empty.vec"), str(tmp_path / "empty.breadth")
    gpu_ctx.features_reads_wide_files(cb, [], k, 0, v, b)
    assert open(v).read() == "0\n" * len(comps) and open(b).read() == "".join("0.0\n" if m else "NaN\n" for m in comps)


def test_refusals(gpu_ctx, tmp_path):
    import torch
    from metafast_amd import lib as L
    k = 33
    comps, reads = _edge_case(k)
    c = _load_comps(gpu_ctx, tmp_path, comps, k)
    cb = str(tmp_path / "components.bin")
    tb, to, n, nb = _dev(reads)
    sample = _load_table(gpu_ctx, tmp_path, R.count(reads, k), k, "x.kmers.bin")
    # a table of another k, as sample and as selection: by the entry point's name
    pb, po = to_device(*pack_reads(reads))
    t35 = gpu_ctx.count_wide_table(pb.data_ptr(), po.data_ptr(), n, nb, 35)
    with pytest.raises(L.MetafastError, match="mf_features_reads_wide_device_selected: components of 33-mers, selected k-mers of 35-mers"):
        gpu_ctx.features_reads_wide(c, tb.data_ptr(), to.data_ptr(), n, nb, 0, t35)
    with pytest.raises(L.MetafastError, match="mf_features_wide_device_selected: components of 33-mers, selected k-mers of 35-mers"):
        gpu_ctx.features_wide(c, sample, 0, t35)
    with pytest.raises(L.MetafastError, match="mf_features_wide_device_selected: components of 33-mers, sample of 35-mers"):
        gpu_ctx.features_wide(c, t35, 0, sample)
    with pytest.raises(L.MetafastError, match="mf_features_wide_device: components of 33-mers, sample of 35-mers"):
        gpu_ctx.features_wide(c, t35, 0)
    with pytest.raises(L.MetafastError, match="mf_features_reads_wide_selected: components of 33-mers, selected k-mers of 35-mers"):
        gpu_ctx.features_reads_wide_files(cb, [], k, 0, str(tmp_path / "no.vec"), str(tmp_path / "no.breadth"), selected=t35)
    # NULL arguments
    lib, last = L.lib(), lambda: L.lib().mf_last_error().decode()
    vec = np.zeros(len(comps), dtype=np.int64)
    P = C.c_void_p
    assert lib.mf_features_reads_wide_device(gpu_ctx.h, None, P(tb.data_ptr()), P(to.data_ptr()), n, nb, 0, vec.ctypes.data, None) != 0
    assert "mf_features_reads_wide_device: NULL argument" in last()
    assert lib.mf_features_reads_wide_device(gpu_ctx.h, c.h, P(tb.data_ptr()), None, n, nb, 0, vec.ctypes.data, None) != 0
    assert "mf_features_reads_wide_device: NULL argument" in last()
    assert lib.mf_features_reads_wide_device_selected(gpu_ctx.h, c.h, P(tb.data_ptr()), P(to.data_ptr()), n, nb, None, 0, None, None) != 0
    assert "mf_features_reads_wide_device_selected: NULL argument" in last()
    assert lib.mf_features_wide_device_selected(gpu_ctx.h, c.h, None, None, 0, vec.ctypes.data, None) != 0
    assert "mf_features_wide_device_selected: NULL argument" in last()
    assert lib.mf_features_wide_selected(gpu_ctx.h, cb.encode(), None, k, 0, None, None, None) != 0 and "mf_features_wide_selected: NULL argument" in last()
    assert lib.mf_features_reads_wide(gpu_ctx.h, None, None, 0, k, 0, None, None) != 0 and "mf_features_reads_wide: NULL argument" in last()
    assert lib.mf_features_reads_wide_selected(gpu_ctx.h, cb.encode(), None, 1, k, 0, None, None, None) != 0 and "mf_features_reads_wide_selected: NULL argument" in last()
    # breadth may be NULL: vec alone
    assert lib.mf_features_reads_wide_device(gpu_ctx.h, c.h, P(tb.data_ptr()), P(to.data_ptr()), n, nb, 0, vec.ctypes.data, None) == 0
    assert np.array_equal(vec, R.from_reads(comps, reads, k, 0)[0])
    # a handle of another context
    other = L.Context(0, stream=torch.cuda.current_stream())
    try:
        oc = _load_comps(other, tmp_path, comps, k, "other.bin")
        with pytest.raises(L.MetafastError, match="mf_features_reads_wide_device: a handle belongs to another context"):
            gpu_ctx.features_reads_wide(oc, tb.data_ptr(), to.data_ptr(), n, nb, 0)
        with pytest.raises(L.MetafastError, match="mf_features_wide_device_selected: a handle belongs to another context"):
            ot = _load_table(other, tmp_path, {comps[0][0]: 1}, k, "o.kmers.bin")
            try:
                other.features_wide(oc, ot, 0, sample)
            finally:
                ot.close()
        oc.close()
    finally:
        other.close()
    # k outside 32 ... 63: the file forms name the narrow entry point; a components file that does not load; nothing is written
    out = [str(tmp_path / "no.vec"), str(tmp_path / "no.breadth")]
    fa = tmp_path / "a.fa"
    fa.write_text(">r\n" + reads[-2] + "\n")
    for kk in (31, 64):
        with pytest.raises(L.MetafastError, match=r"mf_features_reads_wide: 32 <= k <= 63 \(k <= 31: mf_features_reads\)"):
            gpu_ctx.features_reads_wide_files(cb, [str(fa)], kk, 0, *out)
        with pytest.raises(L.MetafastError, match=r"mf_features_wide_selected: 32 <= k <= 63 \(k <= 31: mf_features\)"):
            gpu_ctx.features_wide_files(cb, str(tmp_path / "x.kmers.bin"), kk, 0, *out, selected=sample)
    with pytest.raises(L.MetafastError, match="nothing.bin"):
        gpu_ctx.features_reads_wide_files(str(tmp_path / "nothing.bin"), [str(fa)], k, 0, *out)
    (tmp_path / "short.bin").write_bytes(open(cb, "rb").read()[:-8])
    with pytest.raises(L.MetafastError, match="short.bin"):
        gpu_ctx.features_reads_wide_files(str(tmp_path / "short.bin"), [str(fa)], k, 0, *out)
    _load_comps(gpu_ctx, tmp_path, [], k, "none.bin")
    with pytest.raises(L.MetafastError, match="No components were found"):
        gpu_ctx.features_reads_wide_files(str(tmp_path / "none.bin"), [str(fa)], k, 0, *out)
    with pytest.raises(L.MetafastError, match="missing.fa"):
        gpu_ctx.features_reads_wide_files(cb, [str(tmp_path / "missing.fa")], k, 0, *out)
    assert not os.path.exists(out[0]) and not os.path.exists(out[1])
    # offsets that do not fit the bases
    with pytest.raises(L.MetafastError, match="mf_features_reads_wide_device: the offsets end at"):
        gpu_ctx.features_reads_wide(c, tb.data_ptr(), to.data_ptr(), n, nb + 1, 0)
    back = torch.tensor([0, 150, 80, 230], dtype=torch.int64).cuda()
    with pytest.raises(L.MetafastError, match="mf_features_reads_wide_device: offsets that go backwards"):
        gpu_ctx.features_reads_wide(c, tb.data_ptr(), back.data_ptr(), 3, 230, 0)
