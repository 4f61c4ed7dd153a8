"""comp2seq on the GPU (mf_comp2seq.hip): the segmented unitig build of all components against the oracle's builder run once per
component (tests/comp2seq_ref.py), the unsplit route against mf_build_unitigs_device on the union table, and the files of the library
call and of the driver's tool against the driver's three existing tools chained by hand."""
import glob
import os
import subprocess

import numpy as np
import pytest

import comp2seq_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metafast.sh")
DIRS = ("kmers_fasta", "kmer-counter-many/kmers", "kmer-counter-many/stats", "seq-builder-many/sequences")

CASES = {
    "a_adjacent_k21": lambda: R.case_adjacent(21),
    "a_adjacent_k31": lambda: R.case_adjacent(31),
    "b_shared": R.case_shared,
    "c_dense_k5": R.case_dense,
    "d_palindromes_k20": R.case_palindromes,
    "e_shapes": R.case_shapes,
    "f_long_path": R.case_long,
    "g_many_small": R.case_many,
    "h_70000_singles": R.case_singles,
}
# what the cases are about, so that a builder that loses its point fails here and not silently: sequences split / unsplit
COUNTS = {"a_adjacent_k21": (3, 1), "a_adjacent_k31": (3, 1), "b_shared": (2, None), "e_shapes": (5, None), "h_70000_singles": (70000, 1)}


def _load(ctx, tmp_path, comps):
    path = tmp_path / "components.bin"
    R.write_components(path, comps)
    return ctx.load_components(str(path)), str(path)


@pytest.mark.parametrize("name", list(CASES))
def test_every_component_by_itself_and_all_together(gpu_ctx, oracle, tmp_path, name):
    k, comps = CASES[name]()
    c, _ = _load(gpu_ctx, tmp_path, comps)
    seqs, ids = gpu_ctx.comps_unitigs(c, split=True, k=k)
    want, want_ids = R.flatten(R.expected_split(oracle, comps, k))
    got = seqs.export()
    assert len(got) == len(want)
    assert got == want                                       # bases, lengths, av / min / max weight, in export order
    assert ids.dtype == np.uint32 and np.array_equal(ids, want_ids)
    # all together: the unitigs of the union table
    s0, ids0 = gpu_ctx.comps_unitigs(c, split=False)
    ut = R.union_table(comps, k)
    keys = np.array(sorted(ut), dtype=np.uint64)
    t = gpu_ctx.table_from_host(keys, np.array([ut[int(x)] for x in keys], dtype=np.uint16), k)
    ref0 = gpu_ctx.build_unitigs(t, 0, k).export()
    got0 = s0.export()
    assert got0 == ref0 and got0 == R.expected_union(oracle, comps, k)
    assert len(ids0) == len(got0) and not ids0.any()
    if name in COUNTS:
        n_split, n_union = COUNTS[name]
        assert len(got) == n_split and (n_union is None or len(got0) == n_union)
    if name == "e_shapes":
        per = R.expected_split(oracle, comps, k)
        assert [len(p) for p in per] == [3, 1, 0, 1]         # fork, single k-mer, isolated cycle, path with a member listed twice
        assert per[3][0][2:] == (1, 2) and got[-1] == per[3][0]


def test_sequences_of_another_producer_carry_no_components(gpu_ctx):
    from metafast_amd import lib as L
    k, comps = R.case_adjacent(21)
    keys = np.array(sorted(R.union_table(comps, k)), dtype=np.uint64)
    s = gpu_ctx.build_unitigs(gpu_ctx.table_from_host(keys, np.ones(len(keys), dtype=np.uint16), k), 0, k)
    with pytest.raises(L.MetafastError, match="carry no component ids"):
        s.components()


def _run(*args):
    return subprocess.run([EXE, *[str(a) for a in args], "--device", "0"], capture_output=True, text=True, timeout=300)


def _tree(wd):
    out = {}
    for d in DIRS:
        for p in glob.glob(os.path.join(str(wd), d, "*")):
            out[os.path.relpath(p, str(wd))] = open(p, "rb").read()
    return out


def _chain(cf, k, split, wd):
    """bin2fasta -cf [--split] -> kmer-counter-many -b 0 -> seq-builder-many -b 0 -l k, with comp2seq's work directories"""
    r = _run("-t", "bin2fasta", "-k", k, "-cf", cf, *(["--split"] if split else []), "-o", wd / "kmers_fasta" / "component", "-w", wd / "bin2fasta")
    assert r.returncode == 0, r.stderr
    fastas = sorted(glob.glob(str(wd / "kmers_fasta" / "*.fasta")))
    r = _run("-t", "kmer-counter-many", "-k", k, "-b", 0, "-i", *fastas, "-w", wd / "kmer-counter-many")
    assert r.returncode == 0, r.stderr
    kbins = sorted(glob.glob(str(wd / "kmer-counter-many" / "kmers" / "*.kmers.bin")))
    assert len(kbins) == len(fastas)
    r = _run("-t", "seq-builder-many", "-k", k, "-b", 0, "-l", k, "-i", *kbins, "-w", wd / "seq-builder-many")
    assert r.returncode == 0, r.stderr
    return _tree(wd)


@pytest.mark.parametrize("split", [True, False], ids=["split", "unsplit"])
@pytest.mark.parametrize("name", ["a_adjacent_k21", "c_dense_k5", "e_shapes"])
def test_the_files_equal_the_three_tools_chained_by_hand(gpu_ctx, oracle, tmp_path, name, split):
    k, comps = CASES[name]()
    cf = tmp_path / "components.bin"
    R.write_components(cf, comps)
    want = _chain(cf, k, split, tmp_path / "chain")
    assert len(want) == 4 * (len(comps) if split else 1)
    nf, ns = gpu_ctx.comp2seq(str(cf), k, str(tmp_path / "lib"), split=split)
    assert nf == (len(comps) if split else 1)
    got = _tree(tmp_path / "lib")
    assert sorted(got) == sorted(want)
    for rel in want:
        assert got[rel] == want[rel], rel
    r = _run("-t", "comp2seq", "-k", k, "-cf", cf, *(["--split"] if split else []), "-w", tmp_path / "cli")
    assert r.returncode == 0, r.stderr
    cli = _tree(tmp_path / "cli")
    assert sorted(cli) == sorted(want)
    for rel in want:
        assert cli[rel] == want[rel], rel
    assert want == R.expected_files(oracle, comps, k, split)
    assert ns == sum(v.count(b">") for p, v in want.items() if p.endswith(".seq.fasta"))
    assert (tmp_path / "cli" / "SUCCESS").exists() and (tmp_path / "cli" / "in.properties").exists()
    if name == "e_shapes" and split:
        assert want["seq-builder-many/sequences/component_3.seq.fasta"] == b""      # the isolated cycle: its files are there, no sequence
        # -c continues a finished work directory
        r = _run("-t", "comp2seq", "-k", k, "-cf", cf, "--split", "-w", tmp_path / "cli", "-c")
        assert r.returncode == 0 and "SUCCESS file found for tool comp2seq" in r.stderr
        assert _tree(tmp_path / "cli") == want


def test_errors(gpu_ctx, tmp_path):
    from metafast_amd import lib as L
    k, comps = R.case_adjacent(21)
    c, cf = _load(gpu_ctx, tmp_path, comps)
    with pytest.raises(L.MetafastError, match="no more than 31"):
        gpu_ctx.comp2seq(cf, 32, str(tmp_path / "o1"), split=True)
    with pytest.raises(L.MetafastError, match="no more than 31"):
        gpu_ctx.comps_unitigs(c, split=True, k=32)
    with pytest.raises(L.MetafastError, match="do not know their k"):
        gpu_ctx.comps_unitigs(c, split=True)
    r = _run("-t", "comp2seq", "-k", 32, "-cf", cf, "--split", "-w", tmp_path / "w32")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr
    r = _run("-t", "comp2seq", "--split", "-w", tmp_path / "wnone")
    assert r.returncode == 1 and "Mandatory argument --components-file (-cf) not set" in r.stderr
    trunc = tmp_path / "truncated.bin"
    trunc.write_bytes(open(cf, "rb").read()[:-5])
    with pytest.raises(L.MetafastError, match="Can't load components: file corrupted or format mismatch"):
        gpu_ctx.comp2seq(str(trunc), 21, str(tmp_path / "o2"), split=True)
    r = _run("-t", "comp2seq", "-k", 21, "-cf", trunc, "--split", "-w", tmp_path / "wtrunc")
    assert r.returncode == 1 and "Can't load components: file corrupted or format mismatch" in r.stderr
    R.write_components(tmp_path / "wide.bin", [[1 << 50]])                              # a member that is no 21-mer
    for split in (True, False):
        with pytest.raises(L.MetafastError, match="does not fit 21 bases"):
            gpu_ctx.comp2seq(str(tmp_path / "wide.bin"), 21, str(tmp_path / "o3"), split=split)
