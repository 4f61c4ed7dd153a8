"""component-paths on the GPU (mf_comppaths.hip) against tests/component_paths_ref.py, byte for byte: every file of every case.  The device
form (create / add / finish), the kernel's own tiling, components that share k-mers, a randomised cohort, the cap across batches, the
file form and the command line."""
import functools
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import component_paths_ref as R
import seq2comp_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metafast.sh")
GOLD = os.path.join(ROOT, "tests", "golden", "component_paths")
FA = os.path.join(GOLD, "contigs.fa")
CB = os.path.join(GOLD, "genes.k21.components.bin")


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


def _load(ctx, comps, tmp_path, name="c.bin"):
    """components of the restatement's shape -> an mf_comps, through a components.bin (it does not know its k)"""
    p = tmp_path / name
    p.write_bytes(S.components_bin(comps))
    return ctx.load_components(str(p))


def _device(ctx, c, k, files, selection=None, min_len=50, max_paths=R.MAX_PATHS_COUNT):
    """-> ({file name: bytes}, numbers of the components whose count reached the cap, Paths)"""
    p = ctx.paths(c, selection=selection, min_len=min_len, max_paths=max_paths, k=k)
    for seqs in files:
        tb, to, n, nb = _upload(seqs)
        p.add(tb.data_ptr(), to.data_ptr(), n, nb)
    p.finish()
    no, cnt, nb, cap = p.slots()
    out = p.files()
    assert [len(out[f"component-{int(x)}.seq.fasta"]) for x in no] == [int(x) for x in nb]
    assert [out[f"component-{int(x)}.seq.fasta"].count(b">") for x in no] == [int(x) for x in cnt]
    assert p.text(0) == out[f"component-{int(no[0])}.seq.fasta"] if len(no) else True
    return out, [int(x) for x, r in zip(no, cap) if r], p


def _same(got, exp):
    assert sorted(got[0]) == sorted(exp[0])
    for name in exp[0]:
        assert got[0][name] == exp[0][name], name
    assert sorted(got[1]) == sorted(set(exp[1]))


# ---- the hand cases of test_component_paths_cpu.py, at every k ----
@functools.lru_cache(maxsize=None)
def _edge(k):
    rng = np.random.default_rng(900 + k)
    gene, other, left, right, mid = _rnd(rng, 150), _rnd(rng, 90), _rnd(rng, 40), _rnd(rng, 40), _rnd(rng, 3 * k)
    a, b = left + mid, mid + right                          # two components that share the stretch `mid`
    two = _rnd(rng, k + 1)                                  # two k-mers: weight 5 / size 2 -> 3, weight 3 / size 2 -> 2
    w = _rnd(rng, (k + 1) // 2)
    pal = w + S.rc_str(w)                                   # an even-length palindrome: of length k where k is even
    t = S.component(two, k)
    assert t[1] == 2
    comps = [S.component(gene, k), S.component(_rnd(rng, k - 1), k), (t[0], 2, 5), (t[0], 2, 3), S.component(a, k), S.component(b, k),
             S.component(_rnd(rng, 30) + pal + _rnd(rng, 30), k), S.component(other, k)]
    f = lambda n: _rnd(rng, n)
    fl = lambda n, g: f(n - 1) + "ACGT"[("ACGT".index(g) + 1) % 4]        # filler whose last / first base is not the gene's own there: the path
    fr = lambda n, g: "ACGT"[("ACGT".index(g) + 2) % 4] + f(n - 1)        # ends where it was planted
    f1 = [gene + f(40), f(40) + gene, gene, fl(30, gene[9]) + gene[10:80] + fr(30, gene[80]), f(30) + gene[0:71] + fr(30, gene[71]), fl(9, gene[4]) + gene[5:145],
          two + f(25), f(k - 1), "",
          f(12) + pal + f(12), pal, (f(25) + gene[20:100] + f(25)).lower(), f(30) + left + mid + right + f(30), mid, f(33) + gene[:60], gene[40:] + f(33),
          fl(64, gene[63]) + gene[64:64 + k] + fr(64, gene[64 + k])]
    # ties of equal length across two files, two records, two positions
    f2 = [f(20) + other[0:50] + f(20) + other[30:80] + f(20), other[40:90], S.rc_str(other)[0:50] + f(5) + gene[100:150]]
    f3 = [other[10:60] + f(31) + other[20:70], f(50), gene[3:53] + f(2) + gene[60:110] + f(2) + gene[97:147]]
    return comps, [f1, f2, f3]


@pytest.mark.parametrize("k", [5, 16, 21, 31])
def test_edges(gpu_ctx, tmp_path, k):
    comps, files = _edge(k)
    c = _load(gpu_ctx, comps, tmp_path)
    runs = R.find_runs_plain(comps, k, files)
    for kw in ({"min_len": k}, {"min_len": 50}, {"min_len": 70}, {"min_len": 71}, {"min_len": 0}, {"min_len": 150}, {"min_len": 151},
               {"min_len": k, "selection": [3, 1, 3]}, {"min_len": k, "selection": [8]}, {"min_len": 50, "max_paths": 3}, {"min_len": k, "max_paths": 5}):
        exp = R.component_paths(comps, k, files, runs=runs, **kw)
        got = _device(gpu_ctx, c, k, files, **kw)
        _same(got, exp)
    exp = R.component_paths(comps, k, files, runs=runs, min_len=k)[0]
    assert exp["component-2.seq.fasta"] == b"" and b"av_weight=3 " in exp["component-3.seq.fasta"] and b"av_weight=2 " in exp["component-4.seq.fasta"]
    if k > 5:                                               # (at k = 5 the filler matches by chance and the lengths are others)
        text = exp["component-1.seq.fasta"].decode()
        assert ">1 length=150 " in text and all(f" length={n} " in text for n in (70, 71, 140, k))
        assert exp["component-5.seq.fasta"].startswith(f">1 length={40 + 3 * k} ".encode())


# ---- the boundaries of k_cp_mark's own tiling ----
@functools.lru_cache(maxsize=None)
def _tiling(run, block):
    k = 21
    rng = np.random.default_rng(8192)
    npos = 3 * block + 17
    plans = [[(0, run - 1), (run + 1, block - 1), (block + 1, 2 * block + 5)],
             [(run - 1, run), (block - 1, block), (2 * block - 1, 2 * block)],
             [(run, run + 1), (block, block + 1), (2 * block, 2 * block + 1)],
             [(7, 2 * block + 50)],                         # longer than two workgroups' positions
             [(0, npos - 1)],                               # the whole sequence
             [(run - 1, run - 1), (run + 1, run + 1), (block - 1, block - 1), (block + 1, block + 1), (3 * block - 1, npos - 1)]]
    seqs, comps = [], []
    for plan in plans:
        s = _rnd(rng, npos + k - 1)
        occ = S.occurrences(s, k)
        members = np.unique(np.concatenate([occ[a:b + 1] for a, b in plan]))
        seqs.append(s)
        comps.append((members, len(members), 3 * len(members) // 2))
    whole = seqs[4]
    around = []                                             # every sequence between one that ends and one that starts inside component 5
    for s in seqs:
        around += [_rnd(rng, 30) + whole[100:200], s, whole[300:400] + _rnd(rng, 30)]
    return k, comps, [seqs], [around], plans


def test_tile_boundaries(gpu_ctx, tmp_path):
    run, block = gpu_ctx.stat("cp_run"), gpu_ctx.stat("cp_block")
    assert block % run == 0 and block // run in (64, 128, 256, 512, 1024)
    k, comps, plain, around, plans = _tiling(run, block)
    c = _load(gpu_ctx, comps, tmp_path)
    for files in (plain, around, plain + around):
        runs = R.find_runs(comps, k, files)
        if files is plain:                                  # the plan is what the restatement finds
            for i, plan in enumerate(plans):
                assert [(f, cur - 1) for _, f, cur in runs[i]] == plan
        for min_len in (k, k + 1, 50):
            _same(_device(gpu_ctx, c, k, files, min_len=min_len), R.component_paths(comps, k, files, runs=runs, min_len=min_len))


# ---- components that share members ----
@functools.lru_cache(maxsize=None)
def _shared():
    k = 21
    rng = np.random.default_rng(77)
    G = _rnd(rng, 2000)
    seqs = [G[8 * i: 8 * i + 500] for i in range(55)] + [G[0:500], _rnd(rng, 400), G[1200:1900]]       # overlapping windows, one twice, one apart
    q = [G[100:700], _rnd(rng, 50) + G[300:420] + _rnd(rng, 40) + G[900:1100] + _rnd(rng, 30), S.rc_str(G[200:1000]), G, G[430:470],
         _rnd(rng, 300), S.rc_str(G[1150:1300]) + _rnd(rng, 20) + G[0:60]]
    comps = S.components(seqs, k)
    listings = max(sum(int(x) in set(c[0].tolist()) for c in comps) for x in S.occurrences(G[440:461], k).tolist())
    return k, seqs, comps, [q[:4], q[4:]], listings


def test_shared_members(gpu_ctx):
    k, seqs, comps, files, listings = _shared()
    assert listings >= 50
    tb, to, n, nb = _upload(seqs)
    c = gpu_ctx.comps_from_sequences(tb.data_ptr(), to.data_ptr(), n, nb, k)
    runs = R.find_runs(comps, k, files)
    for kw in ({"min_len": k}, {"min_len": 50}, {"min_len": 50, "selection": [56, 1, 30, 58, 57]}, {"min_len": k, "max_paths": 2}):
        got = _device(gpu_ctx, c, k, files, **kw)
        _same(got, R.component_paths(comps, k, files, runs=runs, **kw))
        if "selection" not in kw:
            assert got[2].max_listings() == listings        # one k-mer, that many listings: the index hands out all of them
            assert got[0]["component-1.seq.fasta"] == got[0]["component-56.seq.fasta"] != b""      # the same sequence twice
    # a disjoint control: no k-mer is listed twice
    ctl = [_rnd(np.random.default_rng(3 + i), 300) for i in range(5)]
    tb, to, n, nb = _upload(ctl)
    c2 = gpu_ctx.comps_from_sequences(tb.data_ptr(), to.data_ptr(), n, nb, k)
    got = _device(gpu_ctx, c2, k, [ctl], min_len=k)
    assert got[2].max_listings() == 1
    _same(got, R.component_paths(S.components(ctl, k), k, [ctl], min_len=k))


# ---- randomised ----
@functools.lru_cache(maxsize=None)
def _cohort():
    rng = np.random.default_rng(2026)
    genes = [_rnd(rng, int(rng.integers(2000, 5001))) for _ in range(300)]
    queries = []
    for _ in range(2000):
        want, s = int(rng.integers(100, 3001)), ""
        while len(s) < want:
            kind = int(rng.integers(0, 4))
            if kind == 3:
                s += _rnd(rng, int(rng.integers(5, 120)))
                continue
            g = genes[int(rng.integers(0, len(genes)))]
            a = int(rng.integers(0, len(g) - 30))
            piece = g[a: a + int(rng.integers(25, 900))]
            s += S.rc_str(piece) if kind == 2 else piece
        queries.append(s[:want])
    return genes, [queries[:1100], queries[1100:]]


@functools.lru_cache(maxsize=None)
def _cohort_runs(k):
    genes, files = _cohort()
    comps = S.components(genes, k)
    return comps, R.find_runs(comps, k, files)


@pytest.mark.parametrize("k", [21, 31])
def test_random(gpu_ctx, k):
    genes, files = _cohort()
    comps, runs = _cohort_runs(k)
    tb, to, n, nb = _upload(genes)
    c = gpu_ctx.comps_from_sequences(tb.data_ptr(), to.data_ptr(), n, nb, k)
    pick = [int(x) for x in np.random.default_rng(17 + k).choice(np.arange(1, 301), 17, replace=False)]
    for min_len in (k, 50):
        for sel in (None, pick):
            exp = R.component_paths(comps, k, files, selection=sel, min_len=min_len, runs=runs)
            got = _device(gpu_ctx, c, k, files, selection=sel, min_len=min_len)
            _same(got, exp)
            assert len(exp[0]) == (300 if sel is None else 17) and sum(len(v) > 0 for v in exp[0].values()) >= len(exp[0]) * 9 // 10


# ---- the cap across batches ----
def test_cap_across_batches(gpu_ctx, tmp_path):
    k = 21
    rng = np.random.default_rng(44)
    gene = _rnd(rng, 400)
    comps = [S.component(gene, k), S.component(_rnd(rng, 100), k)]
    f = lambda n: _rnd(rng, n)
    files = [[f(30) + gene[0:60] + f(30) + gene[100:170] + f(30)], [gene[200:280], f(40)], [f(10) + gene[50:250] + f(10), gene[300:390] + f(20) + gene[0:100]]]
    c = _load(gpu_ctx, comps, tmp_path)
    runs = R.find_runs_plain(comps, k, files)
    assert len(runs[0]) == 6
    exp = R.component_paths(comps, k, files, runs=runs, min_len=50, max_paths=4)
    assert exp[1] == [1] and exp[0]["component-1.seq.fasta"].count(b">") == 4 and b"length=200" in exp[0]["component-1.seq.fasta"]
    got = _device(gpu_ctx, c, k, files, min_len=50, max_paths=4)
    _same(got, exp)
    assert got[1] == [1]                                    # the count-reached flag
    for cap in (3, 6, 7, 10 ** 6):                          # 3: the 200-base path is dropped although it is the longest; 6: reached, nothing dropped
        _same(_device(gpu_ctx, c, k, files, min_len=50, max_paths=cap), R.component_paths(comps, k, files, runs=runs, min_len=50, max_paths=cap))
    assert _device(gpu_ctx, c, k, files, min_len=50, max_paths=7)[0] == _device(gpu_ctx, c, k, files, min_len=50)[0]


# ---- files and the command line ----
def _three_files(tmp_path):
    """the fixture, a .gz copy of it, and a FASTQ with a phred-0 record"""
    gz = tmp_path / "again.fa.gz"
    with open(FA, "rb") as src, gzip.open(gz, "wb") as dst:
        shutil.copyfileobj(src, dst)
    seqs = S.read_fasta(FA)
    fq = tmp_path / "reads.fq"
    recs = [("r1", seqs[0][5:140], "I" * 135), ("r2", seqs[1], "I" * 50 + "!" + "I" * 59), ("r3", S.rc_str(seqs[2]), "5" * 140), ("r4", seqs[1][3:100].lower(), "I" * 97)]
    fq.write_text("".join(f"@{n}\n{s}\n+\n{q}\n" for n, s, q in recs))
    return [FA, str(gz), str(fq)], [seqs, seqs, S.read_fastq(str(fq))]


def _read_dir(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_files(gpu_ctx, tmp_path):
    k = 21
    paths, files = _three_files(tmp_path)
    assert len(files[2]) == 3                               # the phred-0 record is not there
    comps = S.components(files[0][:4], k)
    out = tmp_path / "paths"
    assert gpu_ctx.component_paths(CB, k, [FA], str(out)) == (4, 17)
    assert _read_dir(out) == _read_dir(os.path.join(GOLD, "paths"))
    for sel, min_len in ((None, 50), ([2, 3, 2], k), ([4], 50)):
        exp = R.component_paths(comps, k, files, selection=sel, min_len=min_len)[0]
        out = tmp_path / f"paths_{min_len}_{len(sel or [])}"
        nc, npaths = gpu_ctx.component_paths(CB, k, paths, str(out), selection=sel, min_len=min_len)
        assert nc == 4 and npaths == sum(v.count(b">") for v in exp.values())
        assert _read_dir(out) == exp
    from metafast_amd import lib as L
    for bad, what in ((dict(k=32), "k must be"), (dict(selection=[0]), "no component 0"), (dict(selection=[1, 5]), "no component 5"), (dict(files=[str(tmp_path / "no.fa")]), "no.fa")):
        kw = dict(components_bin=CB, k=k, files=[FA], out_dir=str(tmp_path / "bad"))
        kw.update(bad)
        with pytest.raises(L.MetafastError, match=what):
            gpu_ctx.component_paths(**kw)
    with pytest.raises(L.MetafastError):
        gpu_ctx.component_paths(str(tmp_path / "no.bin"), k, [FA], str(tmp_path / "bad"))


def test_errors_of_the_device_form(gpu_ctx):
    from metafast_amd import lib as L
    c = gpu_ctx.load_components(CB)
    with pytest.raises(L.MetafastError, match="no more than 31"):
        gpu_ctx.paths(c, k=32)
    with pytest.raises(L.MetafastError, match="know their k"):
        gpu_ctx.paths(gpu_ctx.load_components(CB))
    with pytest.raises(L.MetafastError, match="no component 0"):
        gpu_ctx.paths(c, selection=[1, 0], k=21)
    p = gpu_ctx.paths(c, k=21)
    with pytest.raises(L.MetafastError, match="not finished"):
        p.text()
    p.finish()
    assert p.files() == {f"component-{i}.seq.fasta": b"" for i in (1, 2, 3, 4)}
    with pytest.raises(L.MetafastError, match="finished"):
        p.add(1, 1, 1, 1)


def _run(*args):
    return subprocess.run([EXE, *[str(a) for a in args], "--device", "0"], capture_output=True, text=True, timeout=300)


def test_cli(tmp_path):
    k = 21
    paths, files = _three_files(tmp_path)
    comps = S.components(files[0][:4], k)
    w = tmp_path / "w"
    r = _run("-t", "component-paths", "-k", k, "-cf", CB, "--seq", paths[0], paths[1], paths[2], "-a", "-w", w)
    assert r.returncode == 0, r.stderr
    assert _read_dir(w / "paths") == R.component_paths(comps, k, files)[0]
    assert (w / "SUCCESS").exists() and (w / "in.properties").exists() and (w / "out.properties").exists()
    log = (w / "log").read_text()
    for line in (f"4 components loaded from {CB}", "Loading file contigs.fa...", "Loading file again.fa.gz...", "Loading file reads.fq...",
                 f"Paths for 4 component(s) were saved in directory {w}/paths"):
        assert line in log, line
    assert "Too many paths" not in log
    o = tmp_path / "elsewhere"
    r = _run("-t", "component-paths", "-k", k, "--components-file", CB, "--seq", paths[0], "-cm", 3, 1, 3, "-l", k, "-o", o, "-w", tmp_path / "w2")
    assert r.returncode == 0, r.stderr
    assert _read_dir(o) == R.component_paths(comps, k, files[:1], selection=[3, 1, 3], min_len=k)[0] and sorted(os.listdir(o)) == ["component-1.seq.fasta", "component-3.seq.fasta"]
    assert "Paths for 2 component(s)" in (tmp_path / "w2" / "log").read_text() and (tmp_path / "w2" / "SUCCESS").exists()
    # no selection, a number out of range, a missing file, k = 32
    r = _run("-t", "component-paths", "-k", k, "-cf", CB, "--seq", paths[0], "-w", tmp_path / "w3")
    assert r.returncode == 1 and "No components to process!!! Do you forget to set --all-components or --components n1,n2,...?" in r.stderr and not (tmp_path / "w3" / "SUCCESS").exists()
    r = _run("-t", "component-paths", "-k", k, "-cf", CB, "--seq", paths[0], "-cm", 2, 5, "-w", tmp_path / "w4")
    assert r.returncode == 1 and "no component 5" in r.stderr
    r = _run("-t", "component-paths", "-k", k, "-cf", CB, "--seq", paths[0], "-cm", 0, "-w", tmp_path / "w5")
    assert r.returncode == 1 and "no component 0" in r.stderr.lower()
    r = _run("-t", "component-paths", "-k", k, "-cf", CB, "--seq", tmp_path / "nothing.fa", "-a", "-w", tmp_path / "w6")
    assert r.returncode == 1 and "nothing.fa" in r.stderr
    r = _run("-t", "component-paths", "-k", k, "-cf", tmp_path / "nothing.bin", "--seq", paths[0], "-a", "-w", tmp_path / "w7")
    assert r.returncode == 1 and "nothing.bin" in r.stderr
    r = _run("-t", "component-paths", "-k", 32, "-cf", CB, "--seq", paths[0], "-a", "-w", tmp_path / "w8")
    assert r.returncode == 1 and "no more than 31" in r.stderr
    r = _run("-ts")
    assert "component-paths\t\tExtracts paths in the components" in r.stdout
    # seq2comp -> component-paths on the same sequences with -l k: a non-empty component's first path holds at least its own sequence
    w9, w10 = tmp_path / "w9", tmp_path / "w10"
    r = _run("-t", "seq2comp", "-k", k, "-i", FA, "-w", w9)
    assert r.returncode == 0, r.stderr
    r = _run("-t", "component-paths", "-k", k, "-cf", w9 / "components.bin", "--seq", FA, "-a", "-l", k, "-w", w10)
    assert r.returncode == 0, r.stderr
    got = _read_dir(w10 / "paths")
    seqs = files[0]
    assert got == R.component_paths(S.components(seqs, k), k, [seqs], min_len=k)[0] and len(got) == 12
    for i, s in enumerate(seqs):
        text = got[f"component-{i + 1}.seq.fasta"].decode()
        if len(s) < k:
            assert text == ""
            continue
        first = "".join(text.split(">")[1].split("\n")[1:])
        assert s.upper() in first
