"""NO-REFERENCE EXTENSION: looking at what `metafast.sh --wide-kmers` left behind -- comp2seq, view and bin2fasta on the wide
components.bin of a matrix-builder run at k = 33 and 63, against the reference built from oracle.run_pipeline_wide's components
(tests/wcomp2seq_ref.py); comp2seq's definition executed with the three single tools; -c on a wide comp2seq workDir."""
import glob
import os
import subprocess

import numpy as np
import pytest

import comp2seq_ref as R
import wcomp2seq_ref as W
from util import pack_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metafast.sh")
NAMES = ("a", "b", "c")
B, L_, B1, B2 = 1, 60, 20, 400
DIRS = ("kmers_fasta", "kmer-counter-many/kmers", "kmer-counter-many/stats", "seq-builder-many/sequences")
_CACHE = {}


def _samples():
    """three samples of ONE genome (3000 bases, 150 reads of 100 bases each, 0.5 % errors) at different depths along it
    (the recipe of tests/test_wide_cli_gpu.py)"""
    if "s" not in _CACHE:
        rng = np.random.default_rng(6340)
        al = np.frombuffer(b"ACGT", dtype=np.uint8)
        g = al[rng.integers(0, 4, 3000)]
        comp = np.zeros(256, dtype=np.uint8)
        for x, y in zip(b"ACGT", b"TGCA"):
            comp[x] = y
        out = []
        for s in range(3):
            lo, hi = (0, 3000 - 100) if s == 0 else ((0, 1800) if s == 1 else (1000, 2900))
            reads = []
            for st in rng.integers(lo, hi, 150):
                r = g[st:st + 100].copy()
                m = rng.random(100) < 0.005
                r[m] = al[rng.integers(0, 4, int(m.sum()))]
                reads.append(bytes(comp[r[::-1]] if rng.integers(0, 2) else r))
            out.append(pack_reads(reads))
        _CACHE["s"] = out
    return _CACHE["s"]


def _files(tmp_path):
    fs = []
    for name, (b, o) in zip(NAMES, _samples()):
        p = tmp_path / (name + ".fa")
        if not p.exists():
            with open(p, "wb") as f:
                for i in range(len(o) - 1):
                    f.write(b">r%d\n" % i + bytes(b[int(o[i]):int(o[i + 1])]) + b"\n")
        fs.append(str(p))
    return fs


def _want_comps(oracle, k):
    """the oracle's components as lists of Python-int members (ascending)"""
    if k not in _CACHE:
        want = oracle.run_pipeline_wide(_samples(), k, b=B, l=L_, b1=B1, b2=B2)
        _CACHE[k] = [[(int(h) << 64) | int(l) for h, l in zip(km["hi"].tolist(), km["lo"].tolist())] for _, _, _, km in want["comps"].all()]
    return _CACHE[k]


def _run(args, cwd, ok=True):
    r = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=300, cwd=cwd)
    if ok:
        assert r.returncode == 0, r.stderr[-3000:]
    return r


def _tree(wd):
    out = {}
    for d in DIRS:
        for p in glob.glob(os.path.join(str(wd), d, "*")):
            out[os.path.relpath(p, str(wd))] = open(p, "rb").read()
    return out


@pytest.mark.parametrize("k", [33, 63])
def test_the_builders_components_inspected(oracle, tmp_path, k):
    wd = tmp_path / "wd"
    _run(["--wide-kmers", "-k", k, "-b", B, "-l", L_, "-b1", B1, "-b2", B2, "-i", *_files(tmp_path), "-w", wd], tmp_path)
    cf = wd / "component-cutter" / "components.bin"
    comps = _want_comps(oracle, k)
    assert len(comps) >= 3
    # comp2seq --split on the run's own components.bin: every file against the reference
    c2s = tmp_path / "c2s"
    r = _run(["-t", "comp2seq", "--wide-kmers", "-k", k, "-cf", cf, "--split", "-w", c2s], tmp_path)
    assert "%d components loaded from" % len(comps) in r.stderr.replace("'", "") and "sequences found" in r.stderr
    want = W.expected_files(oracle, comps, k, split=True)
    got = _tree(c2s)
    assert sorted(got) == sorted(want) and len(want) == 4 * len(comps)
    for rel in want:
        assert got[rel] == want[rel], rel
    assert (c2s / "SUCCESS").exists()
    props = open(c2s / "in.properties").read()
    assert "wide-kmers" in props
    outp = open(c2s / "out.properties").read()
    assert "output-files" in outp and "component_%d.seq.fasta" % len(comps) in outp
    # view -cf lists exactly those members
    _run(["-t", "view", "--wide-kmers", "-k", k, "-cf", cf, "-o", tmp_path / "view.txt", "-w", tmp_path / "wview"], tmp_path)
    lines = open(tmp_path / "view.txt").read().split("\n")
    assert lines[0] == "%d components:" % len(comps)
    listed, cur = [], None
    for ln in lines[1:]:
        if ln.startswith("Component "):
            cur = []
            listed.append(cur)
            assert ln.startswith("Component %d, size = %d kmers, weight = " % (len(listed), len(comps[len(listed) - 1])))
        elif ln:
            cur.append(R.encode(ln))
            assert len(ln) == k
    assert listed == comps
    # the definition, executed: bin2fasta --split, kmer-counter-many -b 0, seq-builder-many -b 0 -l k on the first three components
    chain = tmp_path / "chain"
    _run(["-t", "bin2fasta", "--wide-kmers", "-k", k, "-cf", cf, "--split", "-o", chain / "fa" / "p", "-w", chain / "bin2fasta"], tmp_path)
    fastas = [chain / "fa" / ("p_%d.fasta" % i) for i in (1, 2, 3)]
    for i, f in enumerate(fastas):
        assert open(f, "rb").read() == got["kmers_fasta/component_%d.fasta" % (i + 1)]
    _run(["-t", "kmer-counter-many", "--wide-kmers", "-k", k, "-b", 0, "-i", *fastas, "-w", chain / "kmer-counter-many"], tmp_path)
    kbins = [chain / "kmer-counter-many" / "kmers" / ("p_%d.kmers.bin" % i) for i in (1, 2, 3)]
    _run(["-t", "seq-builder-many", "--wide-kmers", "-k", k, "-b", 0, "-l", k, "-i", *kbins, "-w", chain / "seq-builder-many"], tmp_path)
    for i in (1, 2, 3):
        assert open(kbins[i - 1], "rb").read() == got["kmer-counter-many/kmers/component_%d.kmers.bin" % i], i
        assert open(chain / "kmer-counter-many" / "stats" / ("p_%d.stat.txt" % i), "rb").read() == got["kmer-counter-many/stats/component_%d.stat.txt" % i], i
        assert open(chain / "seq-builder-many" / "sequences" / ("p_%d.seq.fasta" % i), "rb").read() == got["seq-builder-many/sequences/component_%d.seq.fasta" % i], i
    if k == 33:
        # -c on the finished workDir re-uses the step; without SUCCESS it runs again, wide-kmers read back from in.properties
        r = _run(["-t", "comp2seq", "--wide-kmers", "-k", k, "-cf", cf, "--split", "-w", c2s, "-c"], tmp_path)
        assert "SUCCESS file found for tool comp2seq" in r.stderr
        assert _tree(c2s) == got
        os.unlink(c2s / "SUCCESS")
        for p in glob.glob(str(c2s / "seq-builder-many" / "sequences" / "*")):
            os.unlink(p)
        r = _run(["-t", "comp2seq", "-w", c2s, "-c"], tmp_path)
        assert "SUCCESS file found" not in r.stderr and (c2s / "SUCCESS").exists()
        assert _tree(c2s) == got
        # no flag: the reference's limit
        r = _run(["-t", "comp2seq", "-k", k, "-cf", cf, "--split", "-w", tmp_path / "noflag"], tmp_path, ok=False)
        assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr
