"""component-paths for k = 32 ... 63 on the GPU (mf_wcomppaths.hip; the marking kernel of mf_cp.h on 128-bit keys) against
tests/wcomponent_paths_ref.py, exactly: the bytes of every file, the counts, the components whose count reached the cap.  The cases are
those of tests/wcomponent_paths_cases.py; what they hold is asserted in tests/test_wcomponent_paths_cpu.py.  Then the file form and the
command line."""
import os
import subprocess

import numpy as np
import pytest

import seq2comp_ref as N
import wcomponent_paths_cases as CASES
import wcomponent_paths_ref as R
import wseq2comp_ref as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metafast.sh")
CATALOGUE = os.path.join(ROOT, "tests", "golden", "seq2comp", "catalogue.fa")
CONTIGS = os.path.join(ROOT, "tests", "golden", "component_paths", "contigs.fa")
NARROW_CB = os.path.join(ROOT, "tests", "golden", "component_paths", "genes.k21.components.bin")


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


def _load(ctx, comps, k, tmp_path, name="c.bin"):
    """components of the restatement's shape -> WideComps, through a wide components.bin"""
    p = tmp_path / name
    p.write_bytes(W.components_bin(comps))
    return ctx.load_components_wide(str(p), k)


def _device(ctx, c, files, selection=None, min_len=50, max_paths=R.MAX_PATHS_COUNT):
    """-> ({file name: bytes}, numbers of the components whose count reached the cap, Paths)"""
    p = ctx.paths_wide(c, selection=selection, min_len=min_len, max_paths=max_paths)
    for seqs in files:
        tb, to, n, nb = _upload(seqs)
        p.add(tb.data_ptr(), to.data_ptr(), n, nb)
    p.finish()
    no, cnt, nb, cap = p.slots()
    out = p.files()
    assert [len(out[f"component-{int(x)}.seq.fasta"]) for x in no] == [int(x) for x in nb]
    assert [out[f"component-{int(x)}.seq.fasta"].count(b">") for x in no] == [int(x) for x in cnt]
    return out, [int(x) for x, r in zip(no, cap) if r], p


def _same(got, exp):
    assert list(got[0]) == list(exp[0])                     # (the files in slot order)
    for name in exp[0]:
        assert got[0][name] == exp[0][name], name
    assert sorted(got[1]) == sorted(set(exp[1]))


@pytest.mark.parametrize("k", CASES.KS)
def test_both_words_decide(gpu_ctx, tmp_path, k):
    """k-mers that agree in one word and differ in the other, each a component: a sequence that walks from one into the other breaks
    the run exactly there.  A find or a head flag that compares one word joins them"""
    comps, files, _ = CASES.both_words(k)
    c = _load(gpu_ctx, comps, k, tmp_path)
    runs = R.find_runs(comps, k, files)
    for kw in ({"min_len": k}, {"min_len": k + 1}, {"min_len": k, "selection": [2, 1]}, {"min_len": k, "selection": [4]}):
        got = _device(gpu_ctx, c, files, **kw)
        _same(got, R.component_paths(comps, k, files, runs=runs, **kw))
        assert got[2].max_listings() == 1


@pytest.mark.parametrize("k", CASES.KS)
def test_strand(gpu_ctx, tmp_path, k):
    comps, files, _ = CASES.strand(k)
    c = _load(gpu_ctx, comps, k, tmp_path)
    for min_len in (k, 50, 96, 151):
        _same(_device(gpu_ctx, c, files, min_len=min_len), R.component_paths(comps, k, files, min_len=min_len))


@pytest.mark.parametrize("k", CASES.KS)
def test_thread_borders(gpu_ctx, tmp_path, k):
    assert gpu_ctx.stat("cp_run") == CASES.RUN
    comps, files, _ = CASES.borders(k)
    c = _load(gpu_ctx, comps, k, tmp_path)
    for fl in (files[:1], files[1:], files):
        runs = R.find_runs(comps, k, fl)
        for min_len in (k, k + 1, 50):
            _same(_device(gpu_ctx, c, fl, min_len=min_len), R.component_paths(comps, k, fl, runs=runs, min_len=min_len))


@pytest.mark.parametrize("k", CASES.KS)
def test_shared_members(gpu_ctx, k):
    comps, files, (seqs, listings) = CASES.shared(k)
    tb, to, n, nb = _upload(seqs)
    c = gpu_ctx.wcomps_from_sequences(tb.data_ptr(), to.data_ptr(), n, nb, k)
    runs = R.find_runs(comps, k, files)
    for kw in ({"min_len": k}, {"min_len": 100}, {"min_len": k, "selection": [5, 2, 3]}, {"min_len": k, "max_paths": 2}):
        got = _device(gpu_ctx, c, files, **kw)
        _same(got, R.component_paths(comps, k, files, runs=runs, **kw))
        assert got[2].max_listings() == (3 if "selection" in kw else listings)
    got = _device(gpu_ctx, c, files, min_len=k, selection=[3])
    assert got[2].max_listings() == 1


@pytest.mark.parametrize("k", CASES.KS)
def test_selection_and_cap(gpu_ctx, tmp_path, k):
    from metafast_amd import lib as L
    comps, files, once = CASES.capped(k)
    c = _load(gpu_ctx, comps, k, tmp_path)
    runs = R.find_runs(comps, k, files)
    got = _device(gpu_ctx, c, files, selection=[3, 1, 3], min_len=80)
    _same(got, R.component_paths(comps, k, files, selection=[3, 1, 3], min_len=80, runs=runs))
    assert list(got[0]) == ["component-3.seq.fasta", "component-1.seq.fasta"]
    for bad, what in (([0], "no component 0"), ([1, 4], "no component 4")):
        with pytest.raises(L.MetafastError, match=what):
            gpu_ctx.paths_wide(c, selection=bad)
    assert _device(gpu_ctx, c, files, min_len=k)[0]["component-2.seq.fasta"] == b""       # an empty component: an empty file
    for cap in (2, 5, 6, 7, 10 ** 6):                       # component 1 keeps 6: below, at and above
        got = _device(gpu_ctx, c, files, min_len=80, max_paths=cap)
        exp = R.component_paths(comps, k, files, min_len=80, max_paths=cap, runs=runs)
        _same(got, exp)
        assert got[1] == exp[1] == {2: [1, 3], 5: [1], 6: [1], 7: [], 10 ** 6: []}[cap]
        assert _device(gpu_ctx, c, once, min_len=80, max_paths=cap)[:2] == got[:2]        # one add or three: the same bytes


@pytest.mark.parametrize("k", CASES.KS)
def test_random(gpu_ctx, k):
    """200 components, 300 queries; the restatement finds CASES.RANDOM_PATHS[k] paths at min_len = k (868, 900, 688, 551)"""
    comps, files, genes = CASES.random_case(k)
    tb, to, n, nb = _upload(genes)
    c = gpu_ctx.wcomps_from_sequences(tb.data_ptr(), to.data_ptr(), n, nb, k)
    runs = R.find_runs(comps, k, files)
    pick = [int(x) for x in np.random.default_rng(17 + k).choice(np.arange(1, 201), 13, replace=False)]
    for min_len, sel in ((k, None), (50, None), (k, pick)):
        exp = R.component_paths(comps, k, files, selection=sel, min_len=min_len, runs=runs)
        _same(_device(gpu_ctx, c, files, selection=sel, min_len=min_len), exp)
        if min_len == k and sel is None:
            assert sum(t.count(b">") for t in exp[0].values()) == CASES.RANDOM_PATHS[k]


# ---- files and the command line ----
def _read_dir(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_files(gpu_ctx, tmp_path):
    from metafast_amd import lib as L
    k = 33
    cat, contigs = N.read_fasta(CATALOGUE), N.read_fasta(CONTIGS)
    comps = W.components(cat, k)
    cb = tmp_path / "components.bin"
    assert gpu_ctx.seq2comp_wide([CATALOGUE], k, str(cb))[0] == len(cat) == 12
    for files, seqs, sel, min_len in (([CONTIGS], [contigs], None, 50), ([CATALOGUE], [cat], None, k), ([CONTIGS, CATALOGUE], [contigs, cat], [3, 1, 3], k)):
        exp = R.component_paths(comps, k, seqs, selection=sel, min_len=min_len)[0]
        out = tmp_path / f"paths_{len(files)}_{min_len}"
        nc, npaths = gpu_ctx.component_paths_wide(str(cb), k, files, str(out), selection=sel, min_len=min_len)
        assert nc == 12 and npaths == sum(v.count(b">") for v in exp.values())
        assert (npaths > 0) == (CATALOGUE in files)         # (the contigs are of other genes: twelve empty files)
        assert _read_dir(out) == exp
        if files == [CATALOGUE]:                            # every component of at least one k-mer holds its own sequence whole
            for i, s in enumerate(cat):
                text = exp[f"component-{i + 1}.seq.fasta"].decode()
                assert text == "" if len(s) < k else s.upper() in "".join(text.split(">")[1].split("\n")[1:])
    # refusals: nothing is written
    bad = tmp_path / "bad"
    for kw, what in ((dict(k=31), "32 <= k <= 63"), (dict(k=64), "32 <= k <= 63"), (dict(selection=[0]), "no component 0"), (dict(selection=[13]), "no component 13"),
                     (dict(files=[str(tmp_path / "no.fa")]), "no.fa")):
        args = dict(components_bin=str(cb), k=k, files=[CONTIGS], out_dir=str(bad))
        args.update(kw)
        with pytest.raises(L.MetafastError, match=what):
            gpu_ctx.component_paths_wide(**args)
    with pytest.raises(L.MetafastError):                    # a k <= 31 components.bin given as wide: mf_wcomps_load's refusal
        gpu_ctx.component_paths_wide(NARROW_CB, k, [CONTIGS], str(bad))
    with pytest.raises(L.MetafastError):
        gpu_ctx.component_paths_wide(str(tmp_path / "no.bin"), k, [CONTIGS], str(bad))
    assert not bad.exists()
    c = gpu_ctx.load_components_wide(str(cb), k)
    p = gpu_ctx.paths_wide(c)
    with pytest.raises(L.MetafastError, match="not finished"):
        p.text()
    p.finish()
    assert p.files() == {f"component-{i}.seq.fasta": b"" for i in range(1, 13)}


def _run(*args):
    return subprocess.run([EXE, *[str(a) for a in args], "--device", "0"], capture_output=True, text=True, timeout=300)


def test_cli(gpu_ctx, tmp_path):
    cat, contigs = N.read_fasta(CATALOGUE), N.read_fasta(CONTIGS)
    for k in (33, 63):
        comps = W.components(cat, k)
        cb = tmp_path / f"components.{k}.bin"
        gpu_ctx.seq2comp_wide([CATALOGUE], k, str(cb))
        w = tmp_path / f"w{k}"
        r = _run("-t", "component-paths", "--wide-kmers", "-k", k, "-cf", cb, "--seq", CONTIGS, CATALOGUE, "-a", "-w", w)
        assert r.returncode == 0, r.stderr
        exp = R.component_paths(comps, k, [contigs, cat])[0]
        assert _read_dir(w / "paths") == exp and sum(len(v) > 0 for v in exp.values()) >= 4
        log = (w / "log").read_text()
        for line in (f"12 components loaded from {cb}", "Loading file contigs.fa...", "Loading file catalogue.fa...", f"Paths for 12 component(s) were saved in directory {w}/paths"):
            assert line in log, line
        assert (w / "SUCCESS").exists() and "Too many paths" not in log
    k, cb = 33, tmp_path / "components.33.bin"
    comps = W.components(cat, k)
    o = tmp_path / "elsewhere"
    r = _run("-t", "component-paths", "--wide-kmers", "-k", k, "-cf", cb, "--seq", CONTIGS, CATALOGUE, "-cm", 3, 1, 3, "-l", k, "-o", o, "-w", tmp_path / "w2")
    assert r.returncode == 0, r.stderr
    assert _read_dir(o) == R.component_paths(comps, k, [contigs, cat], selection=[3, 1, 3], min_len=k)[0] and sorted(os.listdir(o)) == ["component-1.seq.fasta", "component-3.seq.fasta"]
    assert "Paths for 2 component(s)" in (tmp_path / "w2" / "log").read_text()
    # refusals: a k <= 31 components.bin as wide, a missing file, no -a / -cm, a number out of range; without the flag the reference's message
    r = _run("-t", "component-paths", "--wide-kmers", "-k", k, "-cf", NARROW_CB, "--seq", CONTIGS, "-a", "-w", tmp_path / "w3")
    assert r.returncode == 1 and not (tmp_path / "w3" / "SUCCESS").exists() and not (tmp_path / "w3" / "paths").exists()
    r = _run("-t", "component-paths", "--wide-kmers", "-k", k, "-cf", cb, "--seq", tmp_path / "nothing.fa", "-a", "-w", tmp_path / "w4")
    assert r.returncode == 1 and "nothing.fa" in r.stderr
    r = _run("-t", "component-paths", "--wide-kmers", "-k", k, "-cf", tmp_path / "nothing.bin", "--seq", CONTIGS, "-a", "-w", tmp_path / "w5")
    assert r.returncode == 1 and "nothing.bin" in r.stderr
    r = _run("-t", "component-paths", "--wide-kmers", "-k", k, "-cf", cb, "--seq", CONTIGS, "-w", tmp_path / "w6")
    assert r.returncode == 1 and "No components to process!!! Do you forget to set --all-components or --components n1,n2,...?" in r.stderr
    r = _run("-t", "component-paths", "--wide-kmers", "-k", k, "-cf", cb, "--seq", CONTIGS, "-cm", 2, 13, "-w", tmp_path / "w7")
    assert r.returncode == 1 and "no component 13" in r.stderr
    r = _run("-t", "component-paths", "-k", k, "-cf", cb, "--seq", CONTIGS, "-a", "-w", tmp_path / "w8")
    assert r.returncode == 1 and "no more than 31" in r.stderr
