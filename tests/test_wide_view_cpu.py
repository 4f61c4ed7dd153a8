"""view and bin2fasta on the wide files of --wide-kmers (k = 32 ... 63), on the host-only stub build of the driver (the recipe of
tests/test_driver_tools_cpu.py): both tools read the files themselves and call no library function.  The expected text is computed here
from Python ints, never recorded from the driver."""
import os
import struct
import subprocess

import pytest

import comp2seq_ref as R
import wcomp2seq_ref as W
import wide_files_ref as WF
from test_driver_tools_cpu import ENV, stub_driver


@pytest.fixture(scope="module")
def driver():
    return stub_driver()


def _run(driver, cwd, *args):
    return subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, env=ENV, timeout=120, cwd=str(cwd))


def _two_kmers(k):
    """two canonical k-mers, ascending: one whose high word is 0, one whose top base is T"""
    small = R.encode("A" * (k - 31) + "C" + "AGCT" * 7 + "GG")      # k - 31 leading A: below 4^31; its reverse complement starts with CC
    big = R.encode("T" + "A" * (k - 1))                            # its reverse complement is T x (k - 1) + A: above it
    assert len(R.decode(small, k)) == k and small >> 64 == 0
    assert big >> (2 * k - 2) == 3 and R.canon(big, k) == big and R.canon(small, k) == small
    return [small, big]


def _kmers_file(path, kmers, counts):
    hi, lo = W.words(kmers)
    path.write_bytes(WF.encode_kmers(hi, lo, counts))


def _comps(k):
    """two components of Python-int members, ascending inside each; the second lists a k-mer of the first again and a k-mer with its reverse complement"""
    a, b = _two_kmers(k)
    x = R.encode("A" * (k - 1) + "C")
    rx = R.encode("G" + "T" * (k - 1))
    assert x < a < rx < b
    return [[a, b], sorted([x, a, rx])], [7, -3]


def _view_comps_text(comps, weights, k):
    out = [f"{len(comps)} components:\n"]
    for i, (m, w) in enumerate(zip(comps, weights)):
        out.append(f"Component {i + 1}, size = {len(m)} kmers, weight = {w}. Kmers:\n")
        out += [R.decode(x, k) + "\n" for x in m]
        out.append("\n")
    return "".join(out)


@pytest.mark.parametrize("k", [33, 63])
def test_view_and_bin2fasta_of_a_wide_kmers_file(driver, tmp_path, k):
    kmers, counts = _two_kmers(k), [5, 32767]
    _kmers_file(tmp_path / "a.kmers.bin", kmers, counts)
    r = _run(driver, tmp_path, "-t", "view", "--wide-kmers", "-k", k, "-kf", "a.kmers.bin", "-o", "view.txt", "-w", "w1")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "view.txt").read_text() == "Kmer\tCount\n" + "".join(f"{R.decode(x, k)}\t{c}\n" for x, c in zip(kmers, counts))
    assert R.decode(kmers[0], k).startswith("A") and R.decode(kmers[1], k).startswith("T")
    r = _run(driver, tmp_path, "-t", "view", "--wide-kmers", "-k", k, "-kf", "a.kmers.bin", "-w", "w2")          # no -o: standard output
    assert r.returncode == 0 and ("Kmer\tCount\n" + "".join(f"{R.decode(x, k)}\t{c}\n" for x, c in zip(kmers, counts))) in r.stdout
    r = _run(driver, tmp_path, "-t", "bin2fasta", "--wide-kmers", "-k", k, "-kf", "a.kmers.bin", "-o", "out/p", "-w", "w3")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out" / "p.fasta").read_text() == "".join(f">{i + 1}\n{R.decode(x, k)}\n" for i, x in enumerate(kmers))


@pytest.mark.parametrize("k", [33, 63])
def test_view_and_bin2fasta_of_wide_components(driver, tmp_path, k):
    comps, weights = _comps(k)
    W.write_components(tmp_path / "components.bin", comps, weights)
    r = _run(driver, tmp_path, "-t", "view", "--wide-kmers", "-k", k, "-cf", "components.bin", "-o", "view.txt", "-w", "w1")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "view.txt").read_text() == _view_comps_text(comps, weights, k)
    assert "2 components loaded from components.bin" in r.stderr + r.stdout
    r = _run(driver, tmp_path, "-t", "bin2fasta", "--wide-kmers", "-k", k, "-cf", "components.bin", "--split", "-o", "s/p", "-w", "w2")
    assert r.returncode == 0, r.stderr
    for i, m in enumerate(comps):
        assert (tmp_path / "s" / f"p_{i + 1}.fasta").read_text() == "".join(f">{j + 1}\n{R.decode(x, k)}\n" for j, x in enumerate(m))
    assert sorted(os.listdir(tmp_path / "s")) == ["p_1.fasta", "p_2.fasta"]
    r = _run(driver, tmp_path, "-t", "bin2fasta", "--wide-kmers", "-k", k, "-cf", "components.bin", "-o", "u/p", "-w", "w3")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "u" / "p.fasta").read_text() == "".join(f">{i + 1}_{j + 1}\n{R.decode(x, k)}\n" for i, m in enumerate(comps) for j, x in enumerate(m))
    assert os.listdir(tmp_path / "u") == ["p.fasta"]


def test_a_file_that_is_no_whole_number_of_wide_records_is_refused_by_name(driver, tmp_path):
    k = 33
    _kmers_file(tmp_path / "good.kmers.bin", _two_kmers(k), [1, 2])
    whole = (tmp_path / "good.kmers.bin").read_bytes()
    (tmp_path / "ragged.kmers.bin").write_bytes(whole[:-1])
    (tmp_path / "narrow.kmers.bin").write_bytes(struct.pack(">QH", 5, 1) * 2)                  # two 10-byte records: 20 bytes
    comps, weights = _comps(k)
    cb = W.components_bytes(comps, weights)
    (tmp_path / "short.bin").write_bytes(cb[:-8])                                            # the last member list runs past the end
    (tmp_path / "long.bin").write_bytes(cb + bytes(16))                                      # bytes after the last component
    R.write_components(tmp_path / "narrow.bin", [[1, 2, 3], [4, 5]])                            # one word per member
    n = 0
    for tool in ("view", "bin2fasta"):
        for opt, name in (("-kf", "ragged.kmers.bin"), ("-kf", "narrow.kmers.bin"), ("-cf", "short.bin"), ("-cf", "long.bin"), ("-cf", "narrow.bin")):
            n += 1
            r = _run(driver, tmp_path, "-t", tool, "--wide-kmers", "-k", k, opt, name, "-o", f"o{n}", "-w", f"w{n}")
            assert r.returncode == 1, (tool, name, r.stdout, r.stderr)
            assert name in r.stderr + r.stdout, (tool, name, r.stderr)


def test_long_is_refused_with_a_wide_k(driver, tmp_path):
    _kmers_file(tmp_path / "a.kmers.bin", _two_kmers(33), [1, 2])
    r = _run(driver, tmp_path, "-t", "view", "--wide-kmers", "-k", 33, "-kf", "a.kmers.bin", "--long", "-w", "w1")
    assert r.returncode == 1 and "Option --long is not supported with --wide-kmers and k > 31" in r.stderr + r.stdout
    r = _run(driver, tmp_path, "-t", "view", "--wide-kmers", "-k", 64, "-kf", "a.kmers.bin", "-w", "w2")
    assert r.returncode == 1 and "The size of k-mer must be no more than 63." in r.stderr + r.stdout


def test_without_the_flag_k_33_dies_with_the_references_message(driver, tmp_path):
    comps, weights = _comps(33)
    W.write_components(tmp_path / "components.bin", comps, weights)
    r = _run(driver, tmp_path, "-t", "comp2seq", "-k", 33, "-cf", "components.bin", "--split", "-w", "w1")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr + r.stdout
    # ... and with it, the wide tool is asked for: the stub library has none, the run says so
    r = _run(driver, tmp_path, "-t", "comp2seq", "--wide-kmers", "-k", 33, "-cf", "components.bin", "--split", "-w", "w2")
    assert r.returncode == 1 and "this build of the library has no" in r.stderr + r.stdout
    assert not (tmp_path / "w2" / "SUCCESS").exists()


def test_the_flag_changes_nothing_at_k_31(driver, tmp_path):
    k = 31
    km = sorted(R.kmers_of("ACGTTGCAAGGCTTAACCGGATCAGTCATGCAAGT", k))
    (tmp_path / "n.kmers.bin").write_bytes(R.kmers_bin({x: i + 1 for i, x in enumerate(km)}))
    R.write_components(tmp_path / "n.bin", [km[:2], km[2:]])
    outs = {}
    for tag, flag in (("plain", []), ("flag", ["--wide-kmers"])):
        r = _run(driver, tmp_path, "-t", "view", *flag, "-k", k, "-kf", "n.kmers.bin", "-cf", "n.bin", "-o", f"v_{tag}.txt", "-w", f"wv_{tag}")
        assert r.returncode == 0, r.stderr
        r = _run(driver, tmp_path, "-t", "bin2fasta", *flag, "-k", k, "-cf", "n.bin", "--split", "-o", f"b_{tag}/p", "-w", f"wb_{tag}")
        assert r.returncode == 0, r.stderr
        outs[tag] = ((tmp_path / f"v_{tag}.txt").read_bytes(), [(tmp_path / f"b_{tag}" / f"p_{i}.fasta").read_bytes() for i in (1, 2)])
    assert outs["plain"] == outs["flag"]
    want = "Kmer\tCount\n" + "".join(f"{R.decode(x, k)}\t{i + 1}\n" for i, x in enumerate(km)) + _view_comps_text([km[:2], km[2:]], [2, len(km) - 2], k)
    assert outs["plain"][0].decode() == want
