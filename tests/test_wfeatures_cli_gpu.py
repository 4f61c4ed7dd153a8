"""`metafast.sh -t features-calculator --wide-kmers -k 40` with reads (-i), with k-mers files and --selected, with reads and --selected:
every .vec / .breadth byte-equal to the text of tests/wfeatures_ref.py; what stays refused."""
import os
import subprocess

import pytest

import wfeatures_ref as R
import wide_files_ref as WF
from test_wfeatures_gpu import _edge_case, _run_length  # noqa: F401  (the fixture reads the library's run length for the cases)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metafast.sh")
K = 40


def _run(*args):
    return subprocess.run([EXE, *[str(a) for a in args], "--device", "0"], capture_output=True, text=True, timeout=300)


def _kmers_file(path, table):
    keys = sorted(table)
    hi, lo = R.words(keys)
    path.write_bytes(WF.encode_kmers(hi, lo, [table[x] for x in keys]))


def _same_files(wd, name, exp):
    assert (wd / "vectors" / (name + ".vec")).read_text() == R.vec_text(exp[0]), name
    assert (wd / "vectors" / (name + ".breadth")).read_text() == R.breadth_text(exp[1]), name


def test_cli(gpu_ctx, tmp_path):
    comps, reads = _edge_case(K)
    hi, lo = R.words([x for m in comps for x in m])
    cb = tmp_path / "components.bin"
    cb.write_bytes(WF.encode_components([len(m) for m in comps], [len(m) for m in comps], hi, lo))
    half = len(reads) // 2
    ra, rb = reads[:half], reads[half:]
    (tmp_path / "a.fa").write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(ra)))
    (tmp_path / "b.fa").write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(rb)))
    sample = R.count(reads, K)
    _kmers_file(tmp_path / "x.kmers.bin", sample)
    sel = {x: 1 for x in comps[0][::2]}
    sel.update({x: 3 for x in comps[3]})
    _kmers_file(tmp_path / "sel.kmers.bin", sel)
    common = ["-t", "features-calculator", "--wide-kmers", "-k", K, "-cm", cb]
    # reads: one vector per file
    w1 = tmp_path / "w1"
    r = _run(*common, "-i", tmp_path / "a.fa", tmp_path / "b.fa", "-w", w1)
    assert r.returncode == 0, r.stderr
    _same_files(w1, "a", R.from_reads(comps, ra, K))
    _same_files(w1, "b", R.from_reads(comps, rb, K))
    assert "NaN" in (w1 / "vectors" / "a.breadth").read_text() and "wide-kmers" in (w1 / "in.properties").read_text() and (w1 / "SUCCESS").exists()
    assert f"Features for file a.fa printed to {w1}/vectors/a.vec" in (w1 / "log").read_text()
    # a k-mers file with --selected
    w2 = tmp_path / "w2"
    r = _run(*common, "-ka", tmp_path / "x.kmers.bin", "--selected", tmp_path / "sel.kmers.bin", "-w", w2)
    assert r.returncode == 0, r.stderr
    exp = R.from_kmers(comps, sample, 0, sel)
    _same_files(w2, "x", exp)
    assert (w2 / "vectors" / "x.breadth").read_text().count("NaN") >= 2 and exp[0][0] > 0
    # reads with --selected, a threshold
    w3 = tmp_path / "w3"
    r = _run(*common, "-i", tmp_path / "a.fa", "--selected", tmp_path / "sel.kmers.bin", "--threshold", 1, "-w", w3)
    assert r.returncode == 0, r.stderr
    _same_files(w3, "a", R.from_reads(comps, ra, K, 1, sel))
    # without the flag: the reference's message
    r = _run("-t", "features-calculator", "-k", K, "-cm", cb, "-i", tmp_path / "a.fa", "-w", tmp_path / "w4")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr
    # a file of 10-byte records as --selected: refused by name, nothing printed
    ten = tmp_path / "ten.kmers.bin"
    ten.write_bytes(b"\0" * 8 + b"\0\x05")
    r = _run(*common, "-i", tmp_path / "a.fa", "--selected", ten, "-w", tmp_path / "w5")
    assert r.returncode == 1 and "ten.kmers.bin" in r.stderr and "18-byte record" in r.stderr
    assert not (tmp_path / "w5" / "vectors" / "a.vec").exists()
    # matrix-builder keeps its refusal
    r = _run("--wide-kmers", "-k", K, "-i", tmp_path / "a.fa", "--selected", tmp_path / "sel.kmers.bin", "-w", tmp_path / "w6")
    assert r.returncode == 1 and "--selected" in r.stderr and "is not supported with --wide-kmers" in r.stderr
