"""seq2comp for k = 32 ... 63 on the GPU (mf_wseq2comp.hip) against tests/wseq2comp_ref.py, exactly: sizes, weights, thr, offsets, high and
low words of WideComps.export().  Every case runs with option s2c_lds at 1 (short sequences are sorted in LDS) and at 0 (every sequence
through the pair sorts).  export() does not sort: that it equals the reference, whose members ascend, IS the check of the invariant
"ascending in (hi, lo) inside every component on the device" -- the one a hash-set build would break.  Then the file form, the way into
features_wide and comp2seq_wide, the command line and the refusals.  What the cases hold is asserted in tests/test_wseq2comp_cpu.py."""
import glob
import os
import subprocess

import numpy as np
import pytest

import seq2comp_ref as N
import wseq2comp_cases as CASES
import wseq2comp_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metafast.sh")
FA = os.path.join(ROOT, "tests", "golden", "seq2comp", "catalogue.fa")


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


def _build(ctx, seqs, k, lds, batch=None):
    tb, to, n, nb = _upload(seqs)
    ctx.set_option("s2c_lds", lds)
    if batch:
        ctx.set_option("s2c_batch_pairs", batch)
    try:
        return ctx.wcomps_from_sequences(tb.data_ptr(), to.data_ptr(), n, nb, k)
    finally:
        ctx.set_option("s2c_lds", 1)
        ctx.set_option("s2c_batch_pairs", 1 << 28)


def _same_arrays(got, exp):
    for name in ("sizes", "weights", "thr", "offsets", "hi", "lo"):
        assert got[name].dtype == exp[name].dtype and np.array_equal(got[name], exp[name]), name


def _check(ctx, seqs, k, lds, comps, batch=None):
    c = _build(ctx, seqs, k, lds, batch)
    exp = R.arrays(comps)
    assert c.stats() == (len(seqs), len(exp["hi"]))
    _same_arrays(c.export(), exp)
    return c


@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("k", CASES.KS)
def test_edges(gpu_ctx, k, lds):
    seqs, comps = CASES.edges(k)
    _check(gpu_ctx, seqs, k, lds, comps)


@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("k", CASES.KS)
def test_both_words(gpu_ctx, k, lds):
    """k-mers that agree in one word and differ in the other: a compare or a head flag that reads one word fails here"""
    seqs, comps, _ = CASES.both_words(k)
    _check(gpu_ctx, seqs, k, lds, comps)


@pytest.mark.parametrize("lds", [1, 0])
def test_class_borders(gpu_ctx, lds):
    T = gpu_ctx.stat("ws2c_lds_max")
    assert T == CASES.lds_max_in_source()
    k, seqs, comps = CASES.borders(T)
    _check(gpu_ctx, seqs, k, lds, comps)


def test_sort_path_in_batches(gpu_ctx):
    """the sort path with a small batch: whole sequences together while they fit, a longer one alone (the bounds of the k <= 31 test)"""
    T = gpu_ctx.stat("ws2c_lds_max")
    k, seqs, comps = CASES.borders(T)
    before = gpu_ctx.stat("s2c_sort_batches")
    _check(gpu_ctx, seqs, k, 0, comps, batch=3 * T)
    assert gpu_ctx.stat("s2c_sort_batches") - before >= 6
    before = gpu_ctx.stat("s2c_sort_batches")
    _check(gpu_ctx, seqs, k, 1, comps, batch=3 * T)                             # only the sequences above T are sorted
    assert 3 <= gpu_ctx.stat("s2c_sort_batches") - before <= 6


@pytest.mark.parametrize("lds", [1, 0])
def test_many_short(gpu_ctx, lds):
    """four sequences to a workgroup, grid-stride, teams that skip the sequences of the other class and the empty ones"""
    k, seqs, comps = CASES.many()
    _check(gpu_ctx, seqs, k, lds, comps)


def _three_files(tmp_path):
    """the fixture, a second FASTA that repeats two of its records (and adds one that is shorter than k), a FASTQ
    (the construction of tests/test_seq2comp_gpu.py)"""
    recs = N.read_fasta(FA)
    fb, fq = tmp_path / "again.fa", tmp_path / "reads.fq"
    fb.write_text(f">gene_1_again\n{recs[0]}\n>short\nACGTACGT\n>gene_4_again\n{recs[10]}\n")
    rng = np.random.default_rng(7)
    q = [recs[0][20:140], CASES.rnd(rng, 80), CASES.rnd(rng, 25)]
    fq.write_text("".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(q)))
    return [FA, str(fb), str(fq)]


@pytest.mark.parametrize("lds", [1, 0])
def test_files(gpu_ctx, tmp_path, lds):
    k = 33
    files = _three_files(tmp_path)
    seqs, per = R.read_files(files)
    assert per == [12, 3, 3]
    comps = R.components(seqs, k)
    assert sum(1 for c in comps if c[1] == 0) >= 3                             # empty components survive write and load
    cb, st = tmp_path / "components.bin", tmp_path / "components-stat.txt"
    gpu_ctx.set_option("s2c_lds", lds)
    try:
        n, got_per = gpu_ctx.seq2comp_wide(files, k, str(cb), str(st))
    finally:
        gpu_ctx.set_option("s2c_lds", 1)
    assert (n, got_per) == (18, per)
    assert cb.read_bytes() == R.components_bin(comps)
    assert st.read_text() == R.stat_txt(comps)
    _same_arrays(gpu_ctx.load_components_wide(str(cb), k).export(), R.arrays(comps))
    n0, per0 = gpu_ctx.seq2comp_wide([], k, str(tmp_path / "none.bin"))
    assert (n0, per0) == (0, []) and (tmp_path / "none.bin").read_bytes() == R.components_bin([])


def _same_features(got, exp):
    (vec, br), (evec, ebr) = got, exp
    assert np.array_equal(vec, evec)
    assert np.array_equal(np.isnan(br), np.isnan(ebr))
    assert np.array_equal(br[~np.isnan(br)], ebr[~np.isnan(ebr)])


def test_into_features(gpu_ctx, tmp_path):
    """components that share k-mers and empty ones, from the device call and from the file: a shared k-mer is credited to every component
    that lists it, an empty component has breadth NaN"""
    k = 33
    files = _three_files(tmp_path)
    seqs, _ = R.read_files(files)
    comps = R.components(seqs, k)
    assert sum(c[1] for c in comps) > len({x for c in comps for x in c[0]})    # members are shared
    sample = CASES.sample_of(comps, k, np.random.default_rng(11))
    ka = tmp_path / "a.kmers.bin"
    ka.write_bytes(R.kmers_bin(sample))
    cb = tmp_path / "components.bin"
    gpu_ctx.seq2comp_wide(files, k, str(cb))
    t = gpu_ctx.load_kmers_wide([str(ka)], k)
    for thr in (0, 4):
        exp = R.features(comps, sample, thr)
        assert np.isnan(exp[1]).sum() >= 3 and exp[0].sum() > 0
        for c in (_build(gpu_ctx, seqs, k, 1), _build(gpu_ctx, seqs, k, 0), gpu_ctx.load_components_wide(str(cb), k)):
            _same_features(gpu_ctx.features_wide(c, t, threshold=thr), exp)


def _contigs(path):
    """the records of a FASTA file, the lines of a record joined"""
    return ["".join(rec.split("\n")[1:]) for rec in open(path).read().split(">")[1:]]


def test_roundtrip_through_comp2seq(gpu_ctx, tmp_path):
    """sequences -> seq2comp_wide -> comp2seq_wide --split: every component gives back its sequence (or the reverse complement) as one contig"""
    k, seqs, comps = CASES.roundtrip()
    fa = tmp_path / "r.fa"
    fa.write_text("".join(f">s{i}\n{s}\n" for i, s in enumerate(seqs)))
    cb = tmp_path / "components.bin"
    assert gpu_ctx.seq2comp_wide([str(fa)], k, str(cb)) == (len(seqs), [len(seqs)])
    assert cb.read_bytes() == R.components_bin(comps)
    out = tmp_path / "c2s"
    os.makedirs(out)
    nf, ns = gpu_ctx.comp2seq_wide(str(cb), k, str(out), split=True)
    assert (nf, ns) == (len(seqs), len(seqs))
    for i, s in enumerate(seqs):
        got = _contigs(out / "seq-builder-many" / "sequences" / f"component_{i + 1}.seq.fasta")
        assert len(got) == 1 and got[0] in (s, R.rc_str(s)), i


def _run(*args):
    return subprocess.run([EXE, *[str(a) for a in args], "--device", "0"], capture_output=True, text=True, timeout=300)


def test_cli(gpu_ctx, tmp_path):
    k = 33
    files = _three_files(tmp_path)
    seqs, per = R.read_files(files)
    comps = R.components(seqs, k)
    lib_cb, lib_st = tmp_path / "lib.bin", tmp_path / "lib.txt"
    gpu_ctx.seq2comp_wide(files, k, str(lib_cb), str(lib_st))
    w = tmp_path / "w"
    r = _run("--wide-kmers", "-t", "seq2comp", "-k", k, "-i", *files, "-w", w)
    assert r.returncode == 0, r.stderr
    assert (w / "components.bin").read_bytes() == lib_cb.read_bytes() == R.components_bin(comps)
    assert (w / "components-stat.txt").read_text() == lib_st.read_text() == R.stat_txt(comps)
    assert (w / "SUCCESS").exists() and "wide-kmers" in (w / "in.properties").read_text() and (w / "out.properties").exists()
    log = (w / "log").read_text()
    for line in ("Loading file catalogue.fa...", "12 components added", "Loading file again.fa...", "3 components added", "Total 18 components were found",
                 f"Components saved to {w}/components.bin"):
        assert line in log, line
    # a sample counted from reads -> features-calculator on these components -> the library's files
    reads = tmp_path / "a.fa"
    reads.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate([seqs[0], seqs[0][40:], seqs[10][:120], CASES.rnd(np.random.default_rng(3), 100)])))
    w2 = tmp_path / "w2"
    r = _run("-t", "kmer-counter", "--wide-kmers", "-k", k, "-b", 0, "-i", reads, "-w", w2)
    assert r.returncode == 0, r.stderr
    ka = glob.glob(str(w2 / "kmers" / "*.kmers.bin"))
    assert len(ka) == 1
    w3 = tmp_path / "w3"
    r = _run("-t", "features-calculator", "--wide-kmers", "-k", k, "-cm", w / "components.bin", "-ka", ka[0], "-w", w3)
    assert r.returncode == 0, r.stderr
    gpu_ctx.features_wide_files(str(lib_cb), ka[0], k, 0, str(tmp_path / "lib.vec"), str(tmp_path / "lib.breadth"))
    assert (w3 / "vectors" / "a.vec").read_bytes() == (tmp_path / "lib.vec").read_bytes()
    assert (w3 / "vectors" / "a.breadth").read_bytes() == (tmp_path / "lib.breadth").read_bytes()
    vec = [int(x) for x in (w3 / "vectors" / "a.vec").read_text().split()]
    lines = (w3 / "vectors" / "a.breadth").read_text().splitlines()
    assert vec[0] >= (150 - k + 1) + (110 - k + 1) and vec[12] == vec[0] and vec[10] >= 120 - k + 1      # gene_1 again: its k-mers count in both components
    assert [i for i, c in enumerate(comps) if c[1] == 0] == [i for i, ln in enumerate(lines) if ln == "NaN"] != []
    # view lists the members
    r = _run("-t", "view", "--wide-kmers", "-k", k, "-cf", w / "components.bin", "-o", tmp_path / "view.txt", "-w", tmp_path / "w4")
    assert r.returncode == 0, r.stderr
    text = (tmp_path / "view.txt").read_text().split("\n")
    assert text[0] == "18 components:"
    listed = [R.encode(ln) for ln in text[1:] if ln and not ln.startswith("Component ")]
    assert listed == [x for c in comps for x in c[0]]
    # -c finds the finished run; without the flag k = 33 is the reference's error
    r = _run("--wide-kmers", "-t", "seq2comp", "-k", k, "-i", *files, "-w", w, "-c")
    assert r.returncode == 0 and "SUCCESS file found" in r.stdout + r.stderr + (w / "log").read_text()
    r = _run("-t", "seq2comp", "-k", k, "-i", files[0], "-w", tmp_path / "w5")
    assert r.returncode == 1 and "no more than 31" in r.stderr


def test_refusals(gpu_ctx, tmp_path):
    from metafast_amd import lib as L
    seqs = ["ACGT" * 20, "TTGCA" * 30]
    tb, to, n, nb = _upload(seqs)
    out = tmp_path / "no.bin"
    for k in (31, 64):
        with pytest.raises(L.MetafastError, match="32 <= k <= 63.*mf_comps_from_sequences_device"):
            gpu_ctx.wcomps_from_sequences(tb.data_ptr(), to.data_ptr(), n, nb, k)
        with pytest.raises(L.MetafastError, match="32 <= k <= 63.*mf_seq2comp"):
            gpu_ctx.seq2comp_wide([FA], k, str(out), str(tmp_path / "no.txt"))
    with pytest.raises(L.MetafastError, match="n_bases"):
        gpu_ctx.wcomps_from_sequences(tb.data_ptr(), to.data_ptr(), n, nb + 1, 33)
    import torch
    back = torch.tensor([0, 150, 80, 230], dtype=torch.int64).cuda()
    with pytest.raises(L.MetafastError, match="offsets that go backwards"):
        gpu_ctx.wcomps_from_sequences(tb.data_ptr(), back.data_ptr(), 3, 230, 33)
    with pytest.raises(L.MetafastError, match="NULL argument"):
        gpu_ctx.wcomps_from_sequences(0, to.data_ptr(), n, nb, 33)
    with pytest.raises(L.MetafastError, match="NULL argument"):
        gpu_ctx.wcomps_from_sequences(tb.data_ptr(), 0, n, nb, 33)
    import ctypes
    last = lambda: L.lib().mf_last_error().decode()
    assert L.lib().mf_wcomps_from_sequences_device(gpu_ctx.h, ctypes.c_void_p(tb.data_ptr()), ctypes.c_void_p(to.data_ptr()), n, nb, 33, None) != 0
    assert "NULL argument" in last()
    assert L.lib().mf_seq2comp_wide(gpu_ctx.h, None, 0, 33, None, None, None, None) != 0 and "NULL argument" in last()
    with pytest.raises(L.MetafastError, match="nothing.fa"):
        gpu_ctx.seq2comp_wide([str(tmp_path / "nothing.fa")], 33, str(out))
    assert not out.exists() and not (tmp_path / "no.txt").exists()
    assert len(gpu_ctx.wcomps_from_sequences(0, 0, 0, 0, 33)) == 0               # no sequences: no components, and no error
