"""comp2seq on wide components (mf_wcomp2seq.hip, 32 <= k <= 63): the segmented unitig build of all components against the 128-bit
oracle's builder run once per component (tests/wcomp2seq_ref.py), with split and without, and the files of the library call.  The
shapes are the smallest at which a stage can go wrong: the boundary k, a k-mer shared by two components, palindromes, k-mers that agree
in one of their two words, a long path, more than 2^16 components, empty components."""
import glob
import os

import numpy as np
import pytest

import comp2seq_ref as R
import wcomp2seq_ref as W

pytestmark = pytest.mark.gpu

DIRS = ("kmers_fasta", "kmer-counter-many/kmers", "kmer-counter-many/stats", "seq-builder-many/sequences")


def _sorted(comps):
    """the members ascending inside a component, as the wide loader demands"""
    return [sorted(int(x) for x in m) for m in comps]


def _palindromes(k):
    """even k: a palindromic k-mer inside a path, one as a whole component, one at the start of a path (comp2seq_ref.case_palindromes for any even k)"""
    assert k % 2 == 0
    rng = np.random.default_rng(k)
    h = R._rand_seq(rng, k // 2)
    p = h + R.rc_str(h)
    assert R.encode(p) == R.encode(R.rc_str(p))
    h2 = R._rand_seq(rng, k // 2)
    p2 = h2 + R.rc_str(h2)
    # (next to a palindrome a k-mer and its reverse complement may both lie on the path: one canonical k-mer, one member -- the file is strictly ascending)
    return k, [sorted(set(m)) for m in (R.kmers_of(R._rand_seq(rng, 6) + p + R._rand_seq(rng, 6), k), [R.encode(p)], R.kmers_of(p2 + R._rand_seq(rng, 7), k))]


def _shapes(k):
    """a fork, a single k-mer, an isolated cycle (no sequence), a path one of whose k-mers is listed as x and as rc(x)"""
    rng = np.random.default_rng(31 + k)
    trunk = R._simple_path(rng, 10, k)
    fork = sorted(set(R.kmers_of(trunk + "A" + R._rand_seq(rng, 7), k) + R.kmers_of(trunk + "C" + R._rand_seq(rng, 7), k)))
    single = R.kmers_of(R._simple_path(rng, 1, k), k)
    while True:                                            # the 15 k-mers of a circular sequence of 15 bases
        circ = R._rand_seq(rng, 15)
        cyc = R.kmers_of((circ * (k // 15 + 2))[:15 + k - 1], k)
        if len(set(cyc)) == 15:
            break
    path = R.kmers_of(R._simple_path(rng, 9, k), k)
    both = path + [R.encode(R.rc_str(R.decode(path[3], k)))]
    assert len(set(both)) == 10                            # (a 63- or 33-mer is no palindrome: x and rc(x) are two members)
    return k, [fork, single, cyc, both]


def _one_word_apart(same_component):
    """k = 63: k-mers that agree in their low word (the last 32 bases) and differ in the high word, and the mirror image"""
    k = 63
    rng = np.random.default_rng(6363)
    tail, head = R._rand_seq(rng, 31) + "A", "A" + R._rand_seq(rng, 31)
    # forward = canonical: they start with A and end with A (the reverse complement starts with T)
    lo_same = [R.encode("A" + R._rand_seq(rng, 30) + tail) for _ in range(3)]
    hi_same = [R.encode(head + R._rand_seq(rng, 30) + "A") for _ in range(3)]
    assert len({x & W.MASK64 for x in lo_same}) == 1 and len({x >> 64 for x in lo_same}) == 3
    assert len({x >> 64 for x in hi_same}) == 1 and len({x & W.MASK64 for x in hi_same}) == 3
    assert all(R.canon(x, k) == x for x in lo_same + hi_same)
    # ... and paths that run into the shared stretch / out of it
    t32, h32 = R._rand_seq(rng, 32), R._rand_seq(rng, 32)
    into = [R.kmers_of(R._rand_seq(rng, 33) + t32, k) for _ in range(2)]
    out_of = [R.kmers_of(h32 + R._rand_seq(rng, 33), k) for _ in range(2)]
    groups = [[x] for x in lo_same] + [[x] for x in hi_same] + into + out_of
    assert len({x for g in groups for x in g}) == sum(len(g) for g in groups)
    return k, ([sum(groups, [])] if same_component else groups)


CASES = {
    "1_boundary_k32": lambda: R.case_adjacent(32),
    "1_boundary_k33": lambda: R.case_adjacent(33),
    "1_boundary_k47": lambda: R.case_adjacent(47),
    "1_boundary_k62": lambda: R.case_adjacent(62),
    "1_boundary_k63": lambda: R.case_adjacent(63),
    "2_shared_k33": lambda: R.case_shared(33),
    "3_palindromes_k32": lambda: _palindromes(32),
    "3_palindromes_k62": lambda: _palindromes(62),
    "4_shapes_k33": lambda: _shapes(33),
    "4_shapes_k63": lambda: _shapes(63),
    "5_one_word_apart_same_component": lambda: _one_word_apart(True),
    "5_one_word_apart_different_components": lambda: _one_word_apart(False),
    "6_long_path_k63": lambda: R.case_long(63),
    "7_many_small_k33": lambda: R.case_many(33),
    "7_70000_singles_k33": lambda: R.case_singles(33),
    "8_no_components": lambda: (33, []),
    "8_empty_component_between_two": lambda: (33, [R.case_adjacent(33)[1][0], [], R.case_adjacent(33)[1][2]]),
}
# what the cases are about, so that a builder that loses its point fails here and not silently: sequences split / unsplit
COUNTS = {"1_boundary_k32": (3, 1), "1_boundary_k33": (3, 1), "1_boundary_k47": (3, 1), "1_boundary_k62": (3, 1), "1_boundary_k63": (3, 1),
          "2_shared_k33": (2, None), "5_one_word_apart_different_components": (10, None),
          "7_70000_singles_k33": (70000, 1), "8_no_components": (0, 0), "8_empty_component_between_two": (2, 2)}


def _load(ctx, tmp_path, k, comps):
    path = tmp_path / "components.bin"
    W.write_components(path, comps)
    return ctx.load_components_wide(str(path), k), str(path)


@pytest.mark.parametrize("name", list(CASES))
def test_every_component_by_itself_and_all_together(gpu_ctx, oracle, tmp_path, name):
    k, comps = CASES[name]()
    comps = _sorted(comps)
    c, _ = _load(gpu_ctx, tmp_path, k, comps)
    seqs = gpu_ctx.wcomps_unitigs(c, split=True)
    want, want_ids = R.flatten(W.expected_split(oracle, comps, k))
    got, ids = seqs.export(), seqs.components()
    assert len(got) == len(want)
    assert got == want                                       # bases, lengths, av / min / max weight, in export order
    assert ids.dtype == np.uint32 and np.array_equal(ids, want_ids)
    s0 = gpu_ctx.wcomps_unitigs(c, split=False)
    got0, ids0 = s0.export(), s0.components()
    assert got0 == W.expected_union(oracle, comps, k)
    assert len(ids0) == len(got0) and not ids0.any()
    if name in COUNTS:
        n_split, n_union = COUNTS[name]
        assert len(got) == n_split and (n_union is None or len(got0) == n_union)
    if name.startswith("1_boundary_k32"):
        assert all(x >> 64 == 0 for m in comps for x in m)   # k = 32: every high word is 0
    if name.startswith("4_shapes"):
        per = W.expected_split(oracle, comps, k)
        # fork (trunk and branches: which of them the emission rule prints depends on the k-mers), single k-mer, isolated cycle, path with x and rc(x)
        assert len(per[0]) >= 2 and [len(p) for p in per[1:]] == [1, 0, 1]
        assert per[3][0][2:] == (1, 2) and got[-1] == per[3][0]
    if name == "2_shared_k33":
        assert len(got0) > 2                                 # linear in both components, a branch point in the union


def _tree(wd):
    out = {}
    for d in DIRS:
        for p in glob.glob(os.path.join(str(wd), d, "*")):
            out[os.path.relpath(p, str(wd))] = open(p, "rb").read()
    return out


@pytest.mark.parametrize("split", [True, False], ids=["split", "unsplit"])
@pytest.mark.parametrize("name", ["4_shapes_k63", "7_many_small_k33", "8_empty_component_between_two"])
def test_the_files(gpu_ctx, oracle, tmp_path, name, split):
    k, comps = CASES[name]()
    comps = _sorted(comps)
    cf = tmp_path / "components.bin"
    W.write_components(cf, comps)
    nf, ns = gpu_ctx.comp2seq_wide(str(cf), k, str(tmp_path / "out"), split=split)
    want = W.expected_files(oracle, comps, k, split)
    got = _tree(tmp_path / "out")
    assert len(want) == 4 * (len(comps) if split else 1) and sorted(got) == sorted(want)
    for rel in want:
        assert got[rel] == want[rel], rel
    assert nf == (len(comps) if split else 1)
    assert ns == sum(v.count(b">") for p, v in want.items() if p.endswith(".seq.fasta"))
    if name == "8_empty_component_between_two" and split:
        assert [got[f"{d}/component_2{e}"] for d, e in zip(DIRS, (".fasta", ".kmers.bin", ".stat.txt", ".seq.fasta"))] == [
            b"", b"", b"# k-mer frequency\tnumber of such k-mers\n\n", b""]


def test_refusals_name_the_file_and_write_nothing(gpu_ctx, tmp_path):
    from metafast_amd import lib as L
    k, comps = R.case_adjacent(21)
    narrow = tmp_path / "narrow_components.bin"
    R.write_components(narrow, comps)
    with pytest.raises(L.MetafastError, match="narrow_components.bin"):
        gpu_ctx.comp2seq_wide(str(narrow), 40, str(tmp_path / "o1"), split=True)
    assert not os.path.exists(tmp_path / "o1") or not os.listdir(tmp_path / "o1")
    # a wide file of 40-mers read as 33-mers: its first member is not below 4^33
    k40, comps40 = R.case_adjacent(40)
    comps40 = _sorted(comps40)
    assert comps40[0][0] >> 66
    wide40 = tmp_path / "wide40_components.bin"
    W.write_components(wide40, comps40)
    for split in (True, False):
        with pytest.raises(L.MetafastError, match=r"wide40_components.bin.*member 0.*not below 4\^k"):
            gpu_ctx.comp2seq_wide(str(wide40), 33, str(tmp_path / "o2"), split=split)
        assert not os.path.exists(tmp_path / "o2") or not os.listdir(tmp_path / "o2")
    with pytest.raises(L.MetafastError, match="32 <= k <= 63"):
        gpu_ctx.comp2seq_wide(str(wide40), 31, str(tmp_path / "o3"))
    with pytest.raises(L.MetafastError, match="32 <= k <= 63"):
        gpu_ctx.comp2seq_wide(str(wide40), 64, str(tmp_path / "o3"))
    assert not os.path.exists(tmp_path / "o3")
