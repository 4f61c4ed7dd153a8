"""seq2comp on the GPU (mf_seq2comp.hip) against tests/seq2comp_ref.py, exactly: sizes, weights, offsets and k-mers of mf_comps_export.
Every case runs with option s2c_lds at its default (short sequences build their sets in LDS) and at 0 (every sequence through the
sort path).  Then the files form, the features calls over components that share k-mers (three routes), and the command line."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import comp2seq_ref as CR
import seq2comp_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metafast.sh")
GOLD = os.path.join(ROOT, "tests", "golden", "seq2comp")
FA = os.path.join(GOLD, "catalogue.fa")


def _rnd(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


def _upload(seqs):
    import torch
    bases = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    tb = torch.zeros(len(bases) + 64, dtype=torch.uint8, device="cuda")
    if len(bases):
        tb[: len(bases)] = torch.from_numpy(bases.copy())
    to = torch.from_numpy(off.view(np.int64).copy()).cuda()
    return tb, to, len(seqs), int(off[-1])


def _export(c):
    """-> sizes, weights, thr, offsets, k-mers as mf_comps_export gives them"""
    from metafast_amd import lib as L
    n, nk = c.stats()
    sizes, w, thr = np.zeros(n, np.uint64), np.zeros(n, np.int64), np.ones(n, np.int32)
    off, km = np.zeros(n + 1, np.uint64), np.zeros(nk, np.uint64)
    L._check(L.lib().mf_comps_export(c.h, sizes.ctypes.data, w.ctypes.data, thr.ctypes.data, off.ctypes.data, km.ctypes.data))
    return sizes, w, thr, off, km


def _expected(seqs, k):
    comps = R.components(seqs, k)
    sizes = np.array([c[1] for c in comps], dtype=np.uint64)
    off = np.zeros(len(comps) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(sizes, dtype=np.uint64)
    km = np.concatenate([c[0] for c in comps]) if comps else np.zeros(0, np.uint64)
    return sizes, np.array([c[2] for c in comps], dtype=np.int64), off, km.astype(np.uint64)


def _build(ctx, seqs, k, lds, batch=None):
    tb, to, n, nb = _upload(seqs)
    ctx.set_option("s2c_lds", lds)
    if batch:
        ctx.set_option("s2c_batch_pairs", batch)
    try:
        return ctx.comps_from_sequences(tb.data_ptr(), to.data_ptr(), n, nb, k)
    finally:
        ctx.set_option("s2c_lds", 1)
        ctx.set_option("s2c_batch_pairs", 1 << 28)


def _check(ctx, seqs, k, lds, exp, batch=None):
    c = _build(ctx, seqs, k, lds, batch)
    sizes, w, thr, off, km = _export(c)
    es, ew, eo, ek = exp
    assert c.stats() == (len(seqs), len(ek))
    assert np.array_equal(sizes, es)
    assert np.array_equal(w, ew)
    assert not thr.any()
    assert np.array_equal(off, eo)
    assert np.array_equal(km, ek)
    return c


@functools.lru_cache(maxsize=None)
def _edges(k):
    rng = np.random.default_rng(1000 + k)
    s, twice, w = _rnd(rng, 100), _rnd(rng, 120), _rnd(rng, (k + 1) // 2)
    pal = w + R.rc_str(w)                                  # an even-length palindrome: of length k where k is even
    assert R.rc_str(pal) == pal and len(pal) in (k, k + 1)
    seqs = ["", _rnd(rng, k - 1), _rnd(rng, k), _rnd(rng, k + 1), "A" * (k + 5), "T" * 50, ("ACG" * 167)[:500], s + R.rc_str(s), twice, twice,
            _rnd(rng, 7) + pal + _rnd(rng, 9), pal, _rnd(rng, 300).lower()]
    return seqs, _expected(seqs, k)


@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("k", [5, 16, 21, 31])
def test_edges(gpu_ctx, k, lds):
    seqs, exp = _edges(k)
    assert exp[0][0] == 0 and exp[0][1] == 0 and exp[1][0] == 0 and exp[0][4] == 1 and exp[1][4] == 6          # empty components stay; the homopolymer
    _check(gpu_ctx, seqs, k, lds, exp)


@functools.lru_cache(maxsize=None)
def _boundary(T):
    k = 21
    rng = np.random.default_rng(4096)
    unit50, unit1000 = _rnd(rng, 50), _rnd(rng, 1000)
    seqs = []
    for n in (T // 4 - 1, T // 4, T // 4 + 1, T - 1, T, T + 1, 2 * T):      # occurrences: the wave / workgroup / sort classes, on both sides
        seqs.append(_rnd(rng, n + k - 1))
        seqs.append((unit50 * (n // 50 + 2))[: n + k - 1])
    seqs.append(_rnd(rng, 300000))
    seqs.append(unit1000 * 300)
    return k, seqs, _expected(seqs, k)


@pytest.mark.parametrize("lds", [1, 0])
def test_class_boundary(gpu_ctx, lds):
    T = gpu_ctx.stat("s2c_lds_max")
    k, seqs, exp = _boundary(T)
    assert [int(x) for x in exp[1][6:14:2]] == [T - 1, T, T + 1, 2 * T]
    assert exp[0][7] == 50 and exp[0][-1] == 1000                             # few distinct k-mers, many occurrences
    _check(gpu_ctx, seqs, k, lds, exp)


def test_sort_path_in_batches(gpu_ctx):
    """the sort path with a small batch: whole sequences together while they fit, a longer one alone"""
    T = gpu_ctx.stat("s2c_lds_max")
    k, seqs, exp = _boundary(T)
    before = gpu_ctx.stat("s2c_sort_batches")
    _check(gpu_ctx, seqs, k, 0, exp, batch=3 * T)
    assert gpu_ctx.stat("s2c_sort_batches") - before >= 6
    before = gpu_ctx.stat("s2c_sort_batches")
    _check(gpu_ctx, seqs, k, 1, exp, batch=3 * T)                             # only the sequences above T are sorted: T + 1, 2 T and the 300 000s
    assert 3 <= gpu_ctx.stat("s2c_sort_batches") - before <= 6


@functools.lru_cache(maxsize=None)
def _many():
    k = 31
    rng = np.random.default_rng(20000)
    lens = rng.integers(31, 401, 20000)
    for at in (0, 10000, 19999):
        lens[at] = 6000 + at % 7
    pool = _rnd(rng, int(lens.sum()))
    ends = np.cumsum(lens)
    seqs = [pool[int(e - n): int(e)] for e, n in zip(ends, lens)]
    return k, seqs, _expected(seqs, k)


@pytest.mark.parametrize("lds", [1, 0])
def test_many_short(gpu_ctx, lds):
    k, seqs, exp = _many()
    _check(gpu_ctx, seqs, k, lds, exp)


@pytest.mark.parametrize("lds", [1, 0])
def test_invariant_against_the_counter(gpu_ctx, ref_files, lds):
    import torch
    k = 31
    bases, off = gpu_ctx.load_reads([ref_files[0]])
    tb = torch.zeros(len(bases) + 64, dtype=torch.uint8, device="cuda")
    tb[: len(bases)] = torch.from_numpy(bases)
    to = torch.from_numpy(off.view(np.int64).copy()).cuda()
    t = gpu_ctx.count_device(tb.data_ptr(), to.data_ptr(), len(off) - 1, int(off[-1]), k, 0)
    keys, _ = t.export()
    gpu_ctx.set_option("s2c_lds", lds)
    try:
        c = gpu_ctx.comps_from_sequences(tb.data_ptr(), to.data_ptr(), len(off) - 1, int(off[-1]), k)
    finally:
        gpu_ctx.set_option("s2c_lds", 1)
    sizes, w, _, offs, km = _export(c)
    assert len(sizes) == len(off) - 1
    assert np.array_equal(np.unique(km), keys)
    assert int(w.sum()) == t.occurrences()
    assert int(offs[-1]) == int(sizes.sum()) == len(km)


def _three_files(tmp_path):
    """the fixture, a second FASTA that repeats two of its records (and adds one that is shorter than k), a FASTQ"""
    recs = R.read_fasta(FA)
    fb, fq = tmp_path / "again.fa", tmp_path / "reads.fq"
    fb.write_text(f">gene_1_again\n{recs[0]}\n>short\nACGTACGT\n>gene_4_again\n{recs[10]}\n")
    rng = np.random.default_rng(7)
    q = [recs[0][20:140], _rnd(rng, 80), _rnd(rng, 25)]
    fq.write_text("".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(q)))
    return [FA, str(fb), str(fq)]


@pytest.mark.parametrize("lds", [1, 0])
def test_files(gpu_ctx, tmp_path, lds):
    k = 21
    files = _three_files(tmp_path)
    seqs, per = R.read_files(files)
    assert per == [12, 3, 3]
    comps = R.components(seqs, k)
    cb, st = tmp_path / "components.bin", tmp_path / "components-stat.txt"
    gpu_ctx.set_option("s2c_lds", lds)
    try:
        n, got_per = gpu_ctx.seq2comp(files, k, str(cb), str(st))
        n1, per1 = gpu_ctx.seq2comp(files[:1], k, str(tmp_path / "one.bin"), str(tmp_path / "one.txt"))
    finally:
        gpu_ctx.set_option("s2c_lds", 1)
    assert (n, got_per) == (18, per) and (n1, per1) == (12, [12])             # the record with an N is absent
    assert cb.read_bytes() == R.components_bin(comps)
    assert st.read_text() == R.stat_txt(comps)
    assert (tmp_path / "one.bin").read_bytes() == open(os.path.join(GOLD, "catalogue.k21.components.bin"), "rb").read()
    assert (tmp_path / "one.txt").read_text() == open(os.path.join(GOLD, "catalogue.k21.components-stat.txt")).read()
    loaded = gpu_ctx.load_components(str(cb))
    sizes, w, _, off, km = _export(loaded)
    es, ew, eo, ek = _expected(seqs, k)
    assert np.array_equal(sizes, es) and np.array_equal(w, ew) and np.array_equal(off, eo) and np.array_equal(km, ek)


def _sample_of(comps, rng):
    """a sample that holds about a third of the members (counts 1 .. 9) and some k-mers of its own: fewer entries than the member list"""
    members = np.unique(np.concatenate([c[0] for c in comps]))
    take = members[rng.random(len(members)) < 0.33]
    sample = {int(x): int(v) for x, v in zip(take, rng.integers(1, 10, len(take)))}
    for x in rng.integers(0, 1 << 42, 40):
        sample.setdefault(int(x), 5)
    return sample


def _same(got, exp):
    vec, br = got
    evec, ebr = exp
    assert np.array_equal(vec, evec)
    assert np.array_equal(np.isnan(br), np.isnan(ebr))
    assert np.array_equal(br[~np.isnan(br)], ebr[~np.isnan(ebr)])


def test_features_with_shared_members(gpu_ctx, tmp_path):
    """components that share k-mers (gene_1 and gene_2's common stretch, gene_1 / gene_4 given again, the same record twice): a k-mer
    counts in EVERY component that lists it -- through the index over the components (sample without an index, fewer entries than
    members), through the sample's index, and from reads"""
    k = 21
    files = _three_files(tmp_path)
    seqs, _ = R.read_files(files)
    comps = R.components(seqs, k)
    n_members = sum(c[1] for c in comps)
    assert n_members > len(np.unique(np.concatenate([c[0] for c in comps])))    # members are shared
    assert comps[1][1] == 0 and comps[13][1] == 0                               # empty components: breadth NaN, vector 0
    rng = np.random.default_rng(11)
    sample = _sample_of(comps, rng)
    assert len(sample) < n_members
    exp = R.features(comps, sample)
    assert math.isnan(exp[1][1]) and exp[0][1] == 0 and exp[0][0] > 0 and exp[0][0] == exp[0][12]
    keys = np.array(sorted(sample), dtype=np.uint64)
    cnts = np.array([sample[int(x)] for x in keys], dtype=np.uint16)
    cb = tmp_path / "components.bin"
    gpu_ctx.seq2comp(files, k, str(cb))
    for c in (_build(gpu_ctx, seqs, k, 1), gpu_ctx.load_components(str(cb))):
        t = gpu_ctx.table_from_host(keys, cnts, k)
        _same(gpu_ctx.features(c, t), exp)                                       # no index on the sample: the components are probed
        _same(gpu_ctx.features(c, t, threshold=4), R.features(comps, sample, 4))
        assert np.array_equal(t.lookup(keys[:5]), cnts[:5].astype(np.int32))     # builds the sample's index
        _same(gpu_ctx.features(c, t), exp)
    # reads: every sample k-mer as many times as its count, the k-mers apart (a read per occurrence)
    reads = [CR.decode(x, k) for x in keys.tolist() for _ in range(sample[int(x)])]
    tb, to, n, nb = _upload(reads)
    for c in (_build(gpu_ctx, seqs, k, 0), gpu_ctx.load_components(str(cb))):
        _same(gpu_ctx.features_reads(c, tb.data_ptr(), to.data_ptr(), n, nb, k), exp)
        _same(gpu_ctx.features_reads(c, tb.data_ptr(), to.data_ptr(), n, nb, k, threshold=4), R.features(comps, sample, 4))


def test_empty_components_through_the_other_tools(gpu_ctx, tmp_path):
    """a component of size 0 survives write, load, export, comp2seq and comp2graph"""
    k = 21
    seqs = R.read_fasta(FA)
    c = _build(gpu_ctx, seqs, k, 1)
    cb = tmp_path / "c.bin"
    c.write(str(cb))
    assert cb.read_bytes() == open(os.path.join(GOLD, "catalogue.k21.components.bin"), "rb").read()
    for comps in (c, gpu_ctx.load_components(str(cb))):
        got = comps.export()
        assert [g[0] for g in got] == [x[1] for x in R.components(seqs, k)] and got[1][0] == 0 and len(got[1][3]) == 0
        s, comp_of = gpu_ctx.comps_unitigs(comps, split=True, k=k)
        assert 1 not in set(comp_of.tolist()) and 11 not in set(comp_of.tolist()) and 0 in set(comp_of.tolist())
        text, stats = gpu_ctx.comps_graph(comps, k=k)
        assert "_i1\t" not in text and "_i11\t" not in text and "1_i0\t" in text and "1_i10\t" in text and stats["segments"] >= 10


def _run(*args):
    return subprocess.run([EXE, *[str(a) for a in args], "--device", "0"], capture_output=True, text=True, timeout=300)


def test_cli(tmp_path):
    k = 21
    files = _three_files(tmp_path)
    seqs, per = R.read_files(files)
    comps = R.components(seqs, k)
    w = tmp_path / "w"
    r = _run("-t", "seq2comp", "-k", k, "-i", files[0], files[1], "-w", w)
    assert r.returncode == 0, r.stderr
    two = comps[: per[0] + per[1]]
    assert (w / "components.bin").read_bytes() == R.components_bin(two)
    assert (w / "components-stat.txt").read_text() == R.stat_txt(two)
    assert (w / "SUCCESS").exists() and (w / "in.properties").exists() and (w / "out.properties").exists()
    log = (w / "log").read_text()
    for line in ("Loading file catalogue.fa...", "12 components added", "Loading file again.fa...", "3 components added", "Total 15 components were found",
                 f"Components saved to {w}/components.bin"):
        assert line in log, line
    # a sample's .kmers.bin -> features-calculator on these components
    rng = np.random.default_rng(5)
    sample = _sample_of(two, rng)
    ka = tmp_path / "a.kmers.bin"
    ka.write_bytes(CR.kmers_bin(sample))
    w2 = tmp_path / "w2"
    r = _run("-t", "features-calculator", "-k", k, "-cm", w / "components.bin", "-ka", ka, "-w", w2)
    assert r.returncode == 0, r.stderr
    vec, br = R.features(two, sample)
    assert (w2 / "vectors" / "a.vec").read_text() == R.vec_txt(vec)
    lines = (w2 / "vectors" / "a.breadth").read_text().splitlines()
    empty = [i for i, c in enumerate(two) if c[1] == 0]
    assert empty == [1, 11, 13]                                               # shorter than k: the .breadth line is NaN, the .vec line 0
    assert all(lines[i] == "NaN" and int(vec[i]) == 0 for i in empty)
    assert [float(x) for i, x in enumerate(lines) if i not in empty] == [float(b) for i, b in enumerate(br) if i not in empty]
    # --components-file, -c finds the finished run, k = 32 and a missing file are errors
    r = _run("-t", "seq2comp", "-k", k, "-i", files[2], "-w", tmp_path / "w3", "--components-file", tmp_path / "elsewhere.bin")
    assert r.returncode == 0 and (tmp_path / "elsewhere.bin").read_bytes() == R.components_bin(comps[per[0] + per[1]:])
    r = _run("-t", "seq2comp", "-k", k, "-i", files[0], files[1], "-w", w, "-c")
    assert r.returncode == 0 and "SUCCESS file found" in r.stdout + r.stderr + (w / "log").read_text()
    r = _run("-t", "seq2comp", "-k", 32, "-i", files[0], "-w", tmp_path / "w4")
    assert r.returncode == 1 and "no more than 31" in r.stderr
    r = _run("-t", "seq2comp", "-k", k, "-i", tmp_path / "nothing.fa", "-w", tmp_path / "w5")
    assert r.returncode == 1 and "nothing.fa" in r.stderr
    r = _run("-ts")
    assert "seq2comp\t\tTransforms sequences to components" in r.stdout
