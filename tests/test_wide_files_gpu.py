"""NO-REFERENCE EXTENSION, files of the k = 32 ... 63 path (metafast_amd/csrc/mf_wio.hip; formats: DESIGN 4.4): wide .kmers.bin / .stat.txt /
components.bin written and loaded on the GPU against the 128-bit build of the pinned oracle and the numpy restatement of the formats
(tests/wide_files_ref.py, itself pinned by literal bytes in tests/test_wide_files_cpu.py).  Reads of a few thousand bases."""
import os

import numpy as np
import pytest

import wide_files_ref as R
from util import genome_reads, pack_reads, to_device

pytestmark = pytest.mark.gpu

KS = [32, 33, 47, 63]
_CACHE = {}


def _reads():
    """60 reads of 100 bases from a genome of 1500 with errors (counts 1 .. ~8) + a poly-A read (key 0 at every k)"""
    if "reads" not in _CACHE:
        rng = np.random.default_rng(3263)
        bs, off = genome_reads(rng, 1500, 60, 100, err=0.01)
        reads = [bytes(bs[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)] + [b"A" * 100]
        _CACHE["reads"] = pack_reads(reads)
    return _CACHE["reads"]


def _want(oracle, k):
    """the oracle's uncut table of the reads: (hi, lo, counts int32), ascending -- computed once per k"""
    if k not in _CACHE:
        b, o = _reads()
        keys, vals = oracle.WTable().count_buffer(b, o, k).export()
        _CACHE[k] = (keys["hi"].astype(np.uint64), keys["lo"].astype(np.uint64), vals.copy())
        for a in _CACHE[k]:
            a.setflags(write=False)
    return _CACHE[k]


def _fasta(tmp_path):
    b, o = _reads()
    p = tmp_path / "reads.fa"
    with open(p, "wb") as f:
        for i in range(len(o) - 1):
            f.write(b">r%d\n" % i + bytes(b[int(o[i]):int(o[i + 1])]) + b"\n")
    return str(p)


def _same(table, hi, lo, cnt):
    ghi, glo, gc = table.export()
    return np.array_equal(ghi, hi) and np.array_equal(glo, lo) and np.array_equal(gc.astype(np.int32), np.asarray(cnt).astype(np.int32))


@pytest.mark.parametrize("k", KS)
def test_reads_to_files_and_back(gpu_ctx, oracle, tmp_path, k):
    """count_reads_wide -> write_kmers (cut b = 1) -> load: the oracle's table; the bytes are the numpy encoder's; .stat.txt is the histogram
    of the UNCUT table; a table in the order of its counting units (record path) and an ascending one (sort path) give identical bytes"""
    hi, lo, cnt = _want(oracle, k)
    assert hi[0] == 0 and lo[0] == 0 and cnt[0] == 101 - k                      # poly-A: key 0
    keep = cnt > 1
    assert 0 < keep.sum() < len(cnt)
    fa = _fasta(tmp_path)
    files = {}
    try:
        for name, opts in (("lazy", {"wide_skm": 1, "wide_skm_min": 1}), ("sorted", {"wide_skm": 0})):
            for o, v in opts.items():
                gpu_ctx.set_option(o, v)
            t = gpu_ctx.count_reads_wide([fa], k)
            assert t.stats()[0] == len(cnt)
            kb, st = str(tmp_path / (name + ".kmers.bin")), str(tmp_path / (name + ".stat.txt"))
            assert t.write_kmers(1, kb, st) == keep.sum()
            files[name] = (open(kb, "rb").read(), open(st).read())
            assert _same(t, hi, lo, cnt)                                        # (the table itself is still whole, now ascending)
    finally:
        gpu_ctx.set_option("wide_skm", 1); gpu_ctx.set_option("wide_skm_min", 1 << 20)
    assert files["lazy"][0] == files["sorted"][0] == R.encode_kmers(hi[keep], lo[keep], cnt[keep])
    assert files["lazy"][1] == files["sorted"][1] == R.stat_text(cnt)
    back = gpu_ctx.load_kmers_wide([str(tmp_path / "lazy.kmers.bin")], k, 0)
    assert _same(back, hi[keep], lo[keep], cnt[keep])
    # the threshold is applied on load; a cut table has no histogram to write
    assert _same(gpu_ctx.load_kmers_wide([str(tmp_path / "lazy.kmers.bin")], k, 2), hi[cnt > 2], lo[cnt > 2], cnt[cnt > 2])
    from metafast_amd import lib as L
    with pytest.raises(L.MetafastError, match="histogram"):
        back.filter(3).write_kmers(3, str(tmp_path / "x.kmers.bin"), str(tmp_path / "x.stat.txt"))


@pytest.mark.parametrize("n,slab", [(0, 0), (1, 0), (255, 0), (256, 0), (257, 0), (257, 100), (700, 256)])
def test_record_counts_around_a_workgroup_and_across_slabs(gpu_ctx, oracle, tmp_path, n, slab):
    """0, 1, 255, 256, 257 records (a workgroup encodes 256) and files that cross a shortened slab, at k = 63 and 33"""
    for k in (63, 33):
        hi, lo, cnt = _want(oracle, k)
        assert len(hi) >= n
        # (counts up to 32767 on the way: the format's largest)
        c = cnt.copy(); c[: n // 2] = 32767 - np.arange(n // 2)
        src = str(tmp_path / ("src%d.kmers.bin" % k))
        data = R.encode_kmers(hi[:n], lo[:n], c[:n])
        open(src, "wb").write(data)
        t = gpu_ctx.load_kmers_wide([src], k, 0)
        assert t.stats()[0] == n and _same(t, hi[:n], lo[:n], c[:n])
        out, st = str(tmp_path / ("out%d.kmers.bin" % k)), str(tmp_path / ("out%d.stat.txt" % k))
        try:
            if slab:
                gpu_ctx.set_option("wide_write_slab", slab)
            assert t.write_kmers(0, out, st) == n
        finally:
            gpu_ctx.set_option("wide_write_slab", 1 << 25)
        assert open(out, "rb").read() == data
        assert open(st).read() == R.stat_text(c[:n])


def test_several_files_give_the_saturating_sum(gpu_ctx, oracle, tmp_path):
    for k in (32, 47):
        hi, lo, cnt = _want(oracle, k)
        assert len(hi) >= 500
        parts = [(0, 300), (100, 400), (200, 500)]
        want = {}
        files = []
        for j, (a, b) in enumerate(parts):
            c = (np.arange(a, b) % 7 + 1 + j).astype(np.int32)
            if j < 2:
                c[150 - a] = 20000                                                # k-mer 150 is in the first two files: 20000 + 20000 -> 32767
            if j == 2:
                c[250 - a] = 32767                                                # k-mer 250: 32767 + small counts
            f = str(tmp_path / ("p%d_%d.kmers.bin" % (k, j)))
            open(f, "wb").write(R.encode_kmers(hi[a:b], lo[a:b], c))
            files.append(f)
            for i, v in zip(range(a, b), c.tolist()):
                want.setdefault(i, []).append(v)
        for thr in (0, 2):
            exp = {i: min(32767, sum(v for v in vs if v > thr)) for i, vs in want.items() if any(v > thr for v in vs)}
            idx = np.array(sorted(exp), dtype=np.int64)
            t = gpu_ctx.load_kmers_wide(files, k, thr)
            assert _same(t, hi[idx], lo[idx], np.array([exp[i] for i in idx.tolist()]))
            assert exp[150] == 32767 and exp[250] == 32767
        # a table loaded from several files goes to the unitig builder as it is (one ascending piece)
        t = gpu_ctx.load_kmers_wide(files, k, 0)
        assert len(t.pieces()) == 1
        gpu_ctx.build_unitigs_wide(t, 0, k)


def test_malformed_files_are_refused_by_name(gpu_ctx, oracle, tmp_path):
    from metafast_amd import lib as L
    k = 40
    b, o = _reads()
    keys, vals = oracle.WTable().count_buffer(b, o, k).export()
    hi, lo, cnt = keys["hi"].astype(np.uint64), keys["lo"].astype(np.uint64), vals
    assert len(hi) > 520
    good = str(tmp_path / "good.kmers.bin")
    open(good, "wb").write(R.encode_kmers(hi, lo, cnt))

    def refused(name, data, what):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        with pytest.raises(L.MetafastError) as e:
            gpu_ctx.load_kmers_wide([p], k, 0)
        assert name in str(e.value) and what in str(e.value), str(e.value)
        with pytest.raises(L.MetafastError):                                      # ... also as one of several files
            gpu_ctx.load_kmers_wide([good, p], k, 0)

    whole = R.encode_kmers(hi, lo, cnt)
    refused("short.kmers.bin", whole[:-1], "multiple of the 18-byte record")
    refused("ten.kmers.bin", b"\0" * 10, "multiple of the 18-byte record")
    # a descending pair exactly at a 256-record boundary (records 255 | 256 and 511 | 512 belong to different workgroups)
    for at in (256, 512):
        order = np.arange(len(hi)); order[[at - 1, at]] = [at, at - 1]
        assert R.first_bad_record(hi[order], lo[order], k) == (at, "order")
        refused("desc%d.kmers.bin" % at, R.encode_kmers(hi[order], lo[order], cnt[order]), "record %d: the k-mer is not above its predecessor" % at)
    dup = np.arange(len(hi)); dup[256] = 255
    refused("dup.kmers.bin", R.encode_kmers(hi[dup], lo[dup], cnt[dup]), "record 256: the k-mer is not above its predecessor")
    # not canonical: record 300 replaced by its reverse complement
    x = R.revcomp((int(hi[300]) << 64) | int(lo[300]), k)
    h2, l2 = hi.copy(), lo.copy(); h2[300], l2[300] = x >> 64, x & R.MASK64
    assert R.first_bad_record(h2, l2, k) == (300, "canonical")
    refused("rc.kmers.bin", R.encode_kmers(h2, l2, cnt), "record 300: the k-mer is above its reverse complement")
    # key >= 4^k: bit 2k set in the last record (still ascending)
    h3 = hi.copy(); h3[-1] |= np.uint64(1 << (2 * k - 64))
    assert R.first_bad_record(h3, lo, k) == (len(hi) - 1, "range")
    refused("range.kmers.bin", R.encode_kmers(h3, lo, cnt), "record %d: the k-mer is not below 4^k" % (len(hi) - 1))
    # a k <= 31 file of 10-byte records whose size happens to divide by 18
    ten = np.zeros(9 * 20, dtype=np.dtype([("key", ">u8"), ("cnt", ">i2")]))
    ten["key"] = np.arange(1, len(ten) + 1) * 0x0123456789ABCD; ten["cnt"] = 5
    h10, l10, _ = R.decode_kmers(ten.tobytes())
    bad = R.first_bad_record(h10, l10, k)
    assert bad is not None
    refused("k31.kmers.bin", ten.tobytes(), "record %d:" % bad[0])
    # a count that is not positive
    c4 = cnt.copy(); c4[7] = 0
    refused("zero.kmers.bin", R.encode_kmers(hi, lo, c4), "record 7: the count is not positive")
    # and the good file still loads
    assert _same(gpu_ctx.load_kmers_wide([good], k, 0), hi, lo, cnt)


def _component_case(oracle, k):
    """a genome read at uneven depth + one read of exactly k bases: components at two threshold levels or more, one of them a single k-mer"""
    rng = np.random.default_rng(77 + k)
    al = np.frombuffer(b"ACGT", dtype=np.uint8)
    g = bytes(al[rng.integers(0, 4, 2500)])
    reads = [g[s:s + 120] for s in range(0, 2500 - 120, 40)] + [g[s:s + 120] for s in range(400, 1400, 30)] + [bytes(al[rng.integers(0, 4, k)])]
    b, o = pack_reads(reads)
    wt = oracle.WTable().count_buffer(b, o, k)
    return b, o, wt


@pytest.mark.parametrize("k", [33, 63])
def test_components_file_round_trip_and_features(gpu_ctx, oracle, tmp_path, k):
    from metafast_amd import lib as L
    b, o, wt = _component_case(oracle, k)
    want = oracle.wide_cut_components(wt, k, 1, 600).all()
    assert len({t for _, _, t, _ in want}) >= 2 and any(n == 1 for n, _, _, _ in want), [(n, t) for n, _, t, _ in want]
    db, do = to_device(b, o)
    table = gpu_ctx.count_wide_table(db.data_ptr(), do.data_ptr(), len(o) - 1, len(b), k)
    comps = gpu_ctx.cut_components_wide(table, 1, 600)
    e = comps.export()
    assert [(int(a), int(w), int(t)) for a, w, t in zip(e["sizes"], e["weights"], e["thr"])] == [(n, w, t) for n, w, t, _ in want]
    cb, cs = str(tmp_path / "components.bin"), str(tmp_path / "components-stat.txt")
    comps.write(cb, cs)
    assert open(cb, "rb").read() == R.encode_components(e["sizes"], e["weights"], e["hi"], e["lo"])
    assert open(cs).read() == "# component.no\tcomponent.size\tcomponent.weight\tusedFreqThreshold\n" + "".join(
        "%d\t%d\t%d\t%d\n" % (i + 1, n, w, t) for i, (n, w, t, _) in enumerate(want))
    back = gpu_ctx.load_components_wide(cb, k)
    eb = back.export()
    for f in ("sizes", "weights", "offsets", "hi", "lo"):
        assert np.array_equal(eb[f], e[f]), f
    # features through the files == features on the resident objects
    kb = str(tmp_path / "s.kmers.bin")
    table.write_kmers(1, kb)
    sample = gpu_ctx.load_kmers_wide([kb], k, -1)
    for thr in (0, 2):
        vec, br = gpu_ctx.features_wide(comps, sample, thr)
        vp, bp = str(tmp_path / "s.vec"), str(tmp_path / "s.breadth")
        gpu_ctx.features_wide_files(cb, kb, k, thr, vp, bp)
        assert [int(x) for x in open(vp).read().split()] == vec.tolist()
        assert [float(x) for x in open(bp).read().split()] == br.tolist()
        assert vec.sum() > 0
    # malformed components files: a member out of order inside a component, a member >= 4^k, a file cut short, a k <= 31 layout
    big = int(np.argmax(e["sizes"])); at = int(e["offsets"][big])
    h2, l2 = e["hi"].copy(), e["lo"].copy()
    h2[[at, at + 1]] = h2[[at + 1, at]]; l2[[at, at + 1]] = l2[[at + 1, at]]
    h3 = e["hi"].copy(); h3[at] |= np.uint64(1 << (2 * k - 64))
    data = open(cb, "rb").read()
    for name, blob, what in (("swap.bin", R.encode_components(e["sizes"], e["weights"], h2, l2), "member %d: the k-mer is not above its predecessor" % (at + 1)),
                             ("range.bin", R.encode_components(e["sizes"], e["weights"], h3, e["lo"]), "member %d: the k-mer is not below 4^k" % at),
                             ("cut.bin", data[:-8], "more than the file holds"),
                             ("more.bin", data + b"\0" * 4, "after the last component")):
        p = str(tmp_path / name)
        open(p, "wb").write(blob)
        with pytest.raises(L.MetafastError) as err:
            gpu_ctx.load_components_wide(p, k)
        assert name in str(err.value) and what in str(err.value), str(err.value)
