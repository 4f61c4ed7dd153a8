"""NO-REFERENCE EXTENSION: `metafast.sh --wide-kmers -k K` (32 <= K <= 63) from FASTA files to the distance matrix, against
oracle.run_pipeline_wide on the same reads and the numpy restatement of the wide file formats (tests/wide_files_ref.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import wide_files_ref as R
from util import canon_seq, genome_reads, pack_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metafast.sh")
NAMES = ("a", "b", "c")
B, L_, B1, B2 = 1, 60, 20, 400
_CACHE = {}


def _samples():
    """three samples of ONE genome (3000 bases, 150 reads of 100 bases each, 0.5 % errors) at different depths along it"""
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


def _want(oracle, k):
    if k not in _CACHE:
        _CACHE[k] = oracle.run_pipeline_wide(_samples(), k, b=B, l=L_, b1=B1, b2=B2)
    return _CACHE[k]


def _run(args, cwd, ok=True):
    r = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=300, cwd=cwd)
    if ok:
        assert r.returncode == 0, r.stderr[-3000:]
    return r


def _builder(tmp_path, wd, k, extra=()):
    return _run(["--wide-kmers", "-k", k, "-b", B, "-l", L_, "-b1", B1, "-b2", B2, "-i", *_files(tmp_path), "-w", wd, *extra], tmp_path)


def _data_files(wd):
    """every file of a workDir that is a function of the inputs alone (no logs, no time stamps in names or content)"""
    out = {}
    for dp, _, fs in os.walk(wd):
        for f in fs:
            rel = os.path.relpath(os.path.join(dp, f), wd)
            if rel.startswith("log") or f in ("in.properties", "out.properties", "output_description.txt"):
                continue
            key = rel
            if f.startswith("dist_matrix_"):
                key = os.path.join(os.path.dirname(rel), "dist_matrix" + ("_original_order" if f.endswith("_original_order.txt") else ""))
            out[key] = open(os.path.join(dp, f), "rb").read()
    return out


def _fasta_seqs(text):
    seqs, cur = [], None
    for line in text.splitlines():
        if line.startswith(">"):
            if cur is not None:
                seqs.append(cur)
            cur = [line.split(" ", 1)[1], ""]
        else:
            cur[1] += line
    if cur is not None:
        seqs.append(cur)
    return sorted((canon_seq(s), h) for h, s in seqs)


def _check_workdir(oracle, wd, k):
    want = _want(oracle, k)
    comps = want["comps"].all()
    assert len(comps) >= 2
    for name, ws in zip(NAMES, want["samples"]):
        keys, vals = ws["good"].export()
        assert len(keys) > 0
        assert open(os.path.join(wd, "kmer-counter-many", "kmers", name + ".kmers.bin"), "rb").read() == R.encode_kmers(keys["hi"], keys["lo"], vals), name
        assert open(os.path.join(wd, "kmer-counter-many", "stats", name + ".stat.txt")).read() == R.stat_text(ws["table"].export()[1]), name
        got = _fasta_seqs(open(os.path.join(wd, "seq-builder-many", "sequences", name + ".seq.fasta")).read())
        exp = sorted((canon_seq(s), "length=%d av_weight=%d min_weight=%d max_weight=%d" % (len(s), a, mn, mx)) for s, a, mn, mx in ws["seqs"].all())
        assert got == exp and len(exp) > 0, name
    hi = np.concatenate([km["hi"] for _, _, _, km in comps]); lo = np.concatenate([km["lo"] for _, _, _, km in comps])
    assert open(os.path.join(wd, "component-cutter", "components.bin"), "rb").read() == R.encode_components(
        [n for n, _, _, _ in comps], [w for _, w, _, _ in comps], hi.astype(np.uint64), lo.astype(np.uint64))
    for name, v in zip(NAMES, want["vecs"]):
        assert open(os.path.join(wd, "features-calculator", "vectors", name + ".vec")).read().split() == [str(int(x)) for x in v], name
    m = want["matrix"]
    mats = [f for f in os.listdir(os.path.join(wd, "matrices")) if f.endswith("_original_order.txt")]
    assert len(mats) == 1
    text = "#\t" + "\t".join(NAMES) + "\n" + "".join(n + "\t" + "\t".join("%.4f" % m[i, j] for j in range(3)) + "\n" for i, n in enumerate(NAMES))
    assert open(os.path.join(wd, "matrices", mats[0])).read() == text
    assert m[0, 1] > 0 and m[1, 2] > m[0, 1]


@pytest.mark.parametrize("k", [33, 63])
def test_matrix_builder_wide(oracle, tmp_path, k):
    """files -> matrix at k = 33 and 63: every file against the oracle; a second run gives byte-identical files; -c -s component-cutter
    reuses the finished steps; the single tools chained by hand give the same files"""
    w1, w2 = tmp_path / "w1", tmp_path / "w2"
    _builder(tmp_path, w1, k)
    _check_workdir(oracle, str(w1), k)
    assert "wide-kmers = true" in open(w1 / "in.properties").read()
    _builder(tmp_path, w2, k)
    d1, d2 = _data_files(str(w1)), _data_files(str(w2))
    assert d1 == d2 and len(d1) >= 3 * 5 + 3
    # -c -s: the steps before the cutter are loaded, the cutter runs with another -b1 and what follows it runs again (the flag comes from in.properties)
    r = _run(["-c", "-s", "component-cutter", "-b1", 100, "-w", w1], tmp_path)
    log = open(w1 / "log").read()
    assert "SUCCESS file found for tool kmer-counter-many" in log and "SUCCESS file found for tool seq-builder-many" in log, log + r.stderr
    sizes = R.decode_components(open(w1 / "component-cutter" / "components.bin", "rb").read())[0]
    exp = [n for n, _, _, _ in oracle.wide_cut_components(_want(oracle, k)["cutter"], k, 100, B2).all()]
    assert sizes.tolist() == exp and min(exp) >= 100 and len(exp) < len(_want(oracle, k)["comps"].all())
    # the single tools, one by one
    w = tmp_path / "single"
    files = _files(tmp_path)
    _run(["--wide-kmers", "-t", "kmer-counter-many", "-k", k, "-b", B, "-i", *files, "-w", w / "kc"], tmp_path)
    kmers = [str(w / "kc" / "kmers" / (n + ".kmers.bin")) for n in NAMES]
    _run(["--wide-kmers", "-t", "seq-builder-many", "-k", k, "-b", B, "-l", L_, "-i", *kmers, "-w", w / "sb"], tmp_path)
    seqs = [str(w / "sb" / "sequences" / (n + ".seq.fasta")) for n in NAMES]
    _run(["--wide-kmers", "-t", "component-cutter", "-k", k, "-l", L_, "-b1", B1, "-b2", B2, "-i", *seqs, "-w", w / "cc"], tmp_path)
    _run(["--wide-kmers", "-t", "features-calculator", "-k", k, "-cm", w / "cc" / "components.bin", "-ka", *kmers, "-w", w / "fc"], tmp_path)
    vecs = [str(w / "fc" / "vectors" / (n + ".vec")) for n in NAMES]
    _run(["-t", "dist-matrix-calculator", "--features", *vecs, "-w", w / "dm"], tmp_path)
    pairs = [("kc/kmers/%s.kmers.bin", "kmer-counter-many/kmers/%s.kmers.bin"), ("kc/stats/%s.stat.txt", "kmer-counter-many/stats/%s.stat.txt"),
             ("sb/sequences/%s.seq.fasta", "seq-builder-many/sequences/%s.seq.fasta"), ("fc/vectors/%s.vec", "features-calculator/vectors/%s.vec"),
             ("fc/vectors/%s.breadth", "features-calculator/vectors/%s.breadth")]
    for mine, theirs in pairs:
        for n in NAMES:
            assert open(w / (mine % n), "rb").read() == d2[theirs % n], mine % n
    assert open(w / "cc" / "components.bin", "rb").read() == d2["component-cutter/components.bin"]
    dm = [f for f in os.listdir(w / "dm") if f.startswith("dist_matrix_")]
    assert len(dm) == 1 and open(w / "dm" / dm[0], "rb").read() == d2["matrices/dist_matrix_original_order"]
    # seq-builder on one file (not -many) gives that library's file too
    _run(["--wide-kmers", "-t", "seq-builder", "-k", k, "-b", B, "-l", L_, "-i", kmers[0], "-w", w / "sb1"], tmp_path)
    assert open(w / "sb1" / "sequences" / "a.seq.fasta", "rb").read() == d2["seq-builder-many/sequences/a.seq.fasta"]


def test_the_flag_changes_nothing_up_to_k31_and_is_needed_above(tmp_path):
    files = _files(tmp_path)
    count = iter(range(100))
    fresh = lambda: tmp_path / ("no%d" % next(count))                          # (a run that dies has left its in.properties behind)
    common = ["-k", 31, "-b", B, "-l", L_, "-b1", B1, "-b2", B2, "-i", *files]
    _run(["--wide-kmers", *common, "-w", tmp_path / "with"], tmp_path)
    _run([*common, "-w", tmp_path / "without"], tmp_path)
    a, b = _data_files(str(tmp_path / "with")), _data_files(str(tmp_path / "without"))
    assert a == b and len(a) >= 18
    # (the two runs start one after the other: a file name that carries a run's start time, yyyy.MM.dd_HH.mm.ss, differs whenever a second ticks between them)
    stamp = re.compile(r"\d{4}\.\d\d\.\d\d_\d\d\.\d\d\.\d\d")
    strip = lambda p: stamp.sub("TS", open(p).read().replace(str(tmp_path / "without"), "W").replace(str(tmp_path / "with"), "W"))
    for sub in ("", "kmer-counter-many", "seq-builder-many", "component-cutter", "features-calculator"):
        assert strip(tmp_path / "with" / sub / "in.properties") == strip(tmp_path / "without" / sub / "in.properties"), sub
    # without the flag k = 32 dies with the reference's message, for the builder and for a single tool
    for args in (["-k", 32, "-i", *files], ["-t", "kmer-counter", "-k", 32, "-i", files[0]], ["-t", "kmer-counter-many", "-k", 40, "-i", *files]):
        r = _run([*args, "-w", fresh()], tmp_path, ok=False)
        assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr
    # with it: k = 64 is too much, the other tools keep their limit, --selected and features from reads are refused by name
    r = _run(["--wide-kmers", "-k", 64, "-i", *files, "-w", fresh()], tmp_path, ok=False)
    assert r.returncode == 1 and "no more than 63" in r.stderr
    r = _run(["--wide-kmers", "-t", "kmers-samples-counter", "-k", 40, "-i", files[0], "-w", fresh()], tmp_path, ok=False)
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr
    r = _run(["--wide-kmers", "-k", 40, "-i", *files, "--selected", files[0], "-w", fresh()], tmp_path, ok=False)
    assert r.returncode == 1 and "--selected" in r.stderr
    r = _run(["--wide-kmers", "-k", 40, "-i", *files, "--use-reads-for-calculating-features", "-w", fresh()], tmp_path, ok=False)
    assert r.returncode == 1 and "--use-reads-for-calculating-features" in r.stderr
    # a k <= 31 file of 10-byte records (here: 10 bytes) given as a wide file is refused by name and does not load
    ten = tmp_path / "ten.kmers.bin"
    ten.write_bytes(b"\0" * 8 + b"\0\x05")
    r = _run(["--wide-kmers", "-t", "seq-builder", "-k", 40, "-l", 60, "-i", ten, "-w", tmp_path / "no10"], tmp_path, ok=False)
    assert r.returncode == 1 and "ten.kmers.bin" in r.stderr and "18-byte record" in r.stderr
    assert not (tmp_path / "no10" / "sequences" / "ten.seq.fasta").exists()
