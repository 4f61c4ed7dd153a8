"""tests/component_paths_ref.py -- the restatement of ComponentPathsMain.java:82-206 the GPU tests compare with -- pinned with answers
written by hand, the committed fixture pinned by it, and the ABI of the new calls."""
import os
import re

import numpy as np

import component_paths_ref as R
import seq2comp_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "component_paths")


def _comp(kmers, k, weight=None):
    """a component of the canonical k-mers of the given strings"""
    m = np.unique(np.array([min(S.encode(x), S.encode(S.rc_str(x))) for x in kmers], dtype=np.uint64))
    assert all(len(x) == k for x in kmers)
    return (m, len(m), len(m) if weight is None else weight)


def _of(seq, k):
    return S.component(seq, k)


def _paths(comps, k, files, **kw):
    """-> {component number: [path strings in file order]}, after checking the two scans against each other"""
    out, reached = R.component_paths(comps, k, files, **kw)
    fast, reached2 = R.component_paths(comps, k, files, runs=R.find_runs(comps, k, files), **kw)
    assert out == fast and reached == reached2
    res = {}
    for name, data in out.items():
        no = int(re.fullmatch(r"component-(\d+)\.seq\.fasta", name).group(1))
        recs = data.decode().split(">")[1:]
        res[no] = ["".join(r.split("\n")[1:]) for r in recs]
        for i, r in enumerate(recs):
            assert re.fullmatch(rf"{i + 1} length={len(res[no][i])} av_weight=-?\d+ min_weight=0 max_weight=0", r.split("\n")[0])
    return res


def test_the_issue_example():
    # rc(ACG) = CGT: positions 0 (ACG), 1 (CGT), 4, 5 of ACGTACGT match -> two runs of 2 positions, length 2 + 3 - 1 = 4
    c = [_comp(["ACG"], 3)]
    assert S.occurrences("ACGTACGT", 3).tolist() == [S.encode("ACG"), S.encode("ACG"), S.encode("GTA"), S.encode("GTA"), S.encode("ACG"), S.encode("ACG")]       # (rc(TAC) = GTA)
    assert _paths(c, 3, [["ACGTACGT"]], min_len=4) == {1: ["ACGT", "ACGT"]}
    assert _paths(c, 3, [["ACGTACGT"]], min_len=5) == {1: []}


def test_runs_at_the_ends_and_over_the_whole_sequence():
    k = 5
    gene = "ACGGTCATTGCA"
    c = [_of(gene, k)]
    assert _paths(c, k, [[gene + "TTTTTTTT"]], min_len=k) == {1: [gene]}                 # at the start
    assert _paths(c, k, [["TTTTTTTT" + gene]], min_len=k) == {1: [gene]}                 # at the end
    assert _paths(c, k, [[gene]], min_len=k) == {1: [gene]}                              # the whole sequence
    assert _paths(c, k, [["TTTTTT" + gene + "TTTTTT"]], min_len=k) == {1: [gene]}
    assert _paths(c, k, [[S.rc_str(gene)]], min_len=k) == {1: [S.rc_str(gene)]}           # forward as given, not canonicalised


def test_min_length_at_and_above_the_path_length():
    k = 5
    gene = "ACGGTCATTGCA"
    c = [_of(gene, k)]
    q = "TTTTTT" + gene + "TTTTTT"
    assert _paths(c, k, [[q]], min_len=len(gene)) == {1: [gene]}
    assert _paths(c, k, [[q]], min_len=len(gene) + 1) == {1: []}
    # -l <= k keeps runs of one k-mer: GGTCA alone (the gene goes on with T, here a G follows)
    assert _paths(c, k, [["TTTTTGGTCAGTTTT"]], min_len=k) == {1: ["GGTCA"]}
    assert _paths(c, k, [["TTTTTGGTCAGTTTT"]], min_len=0) == {1: ["GGTCA"]}
    assert _paths(c, k, [["TTTTTGGTCAGTTTT"]], min_len=k + 1) == {1: []}


def test_runs_do_not_join_across_sequences():
    k = 5
    gene = "ACGGTCATTGCA"
    c = [_of(gene, k)]
    # the first sequence ends inside the component, the next starts inside it: two paths, in one file or in two
    assert _paths(c, k, [["TTTTTT" + gene[:8], gene[4:] + "TTTTTT"]], min_len=k) == {1: [gene[:8], gene[4:]]}
    assert _paths(c, k, [["TTTTTT" + gene[:8]], [gene[4:] + "TTTTTT"]], min_len=k) == {1: [gene[:8], gene[4:]]}
    assert _paths(c, k, [[gene, gene]], min_len=k) == {1: [gene, gene]}


def test_short_sequences_palindromes_and_lower_case():
    k = 6
    pal = "ACGCGT"
    assert S.rc_str(pal) == pal
    c = [_comp([pal], k)]
    assert _paths(c, k, [["ACGC", "", "TT" + pal + "TT"]], min_len=1) == {1: [pal]}       # shorter than k: no positions
    assert _paths(c, k, [[("tt" + pal + "tt").lower()]], min_len=1) == {1: [pal]}        # lower case reads as upper case
    assert _paths(c, k, [[pal + pal]], min_len=1) == {1: [pal, pal]}                     # CGCGTA ... are no members: two runs


def test_ties_keep_encounter_order():
    k = 5
    g1, g2, g3 = "ACGGTCATT", "GGATCCTAA", "CTTGACGAT"                                     # three stretches of the component, all of length 9
    c = [(np.unique(np.concatenate([_of(g, k)[0] for g in (g1, g2, g3)])), 15, 15)]
    f1 = ["TTTTTT" + g2 + "TTTTTT" + g1 + "TTTTTT", g3 + "TTTTTT" + g1]
    f2 = [g1 + "TTTTTT" + g3]
    got = _paths(c, k, [f1, f2], min_len=9)
    assert got == {1: [g2, g1, g3, g1, g1, g3]}                                            # file, then record, then position
    # a longer path comes first wherever it was met
    c2 = [(np.unique(np.concatenate([_of(g, k)[0] for g in (g1, g2, g3, g3 + "AC")])), 17, 17)]
    assert _paths(c2, k, [f1, [g1, g3 + "AC"]], min_len=9) == {1: [g3 + "AC", g2, g1, g3, g1, g1]}


def test_cap_keeps_the_first_encountered():
    k = 5
    short, long_ = "ACGGTCATT", "GGATCCTAACTTGAC"
    c = [(np.unique(np.concatenate([_of(short, k)[0], _of(long_, k)[0]])), 16, 16)]
    files = [[short, "TTTTTT" + short], [short + "TTTTTT" + long_, long_]]                  # 5 candidates, the longer ones last
    out, reached = R.component_paths(c, k, files, min_len=k, max_paths=3)
    assert reached == [1] and _paths(c, k, files, min_len=k, max_paths=3) == {1: [short, short, short]}
    assert _paths(c, k, files, min_len=k, max_paths=4) == {1: [long_, short, short, short]}
    out, reached = R.component_paths(c, k, files, min_len=k, max_paths=5)
    assert reached == [1]                                                                   # ans.size() == MAX_PATHS_COUNT warns, dropped or not
    out, reached = R.component_paths(c, k, files, min_len=k, max_paths=6)
    assert reached == [] and _paths(c, k, files, min_len=k, max_paths=6) == {1: [long_, long_, short, short, short]}


def test_java_rounding_of_the_average_weight():
    assert R.java_round(2.5) == 3 and R.java_round(1.5) == 2 and R.java_round(0.49) == 0 and R.java_round(-2.5) == -2 and round(2.5) == 2
    m = _comp(["ACGGT", "CGGTC"], 5)[0]
    for weight, w in ((5, 3), (3, 2), (2, 1), (0, 0)):
        out, _ = R.component_paths([(m, 2, weight)], 5, [["ACGGTC"]], min_len=5)
        assert out["component-1.seq.fasta"] == f">1 length=6 av_weight={w} min_weight=0 max_weight=0\nACGGTC\n".encode()
    try:
        R.component_paths([(m, 2, 2 ** 33)], 5, [["ACGGTC"]], min_len=5)
    except OverflowError:
        pass
    else:
        raise AssertionError("an average weight of 2^32 must be refused")


def test_line_wrap():
    rng = np.random.default_rng(70)
    for n in (69, 70, 71, 140, 141):
        s = "".join("ACGT"[i] for i in rng.integers(0, 4, n))
        out, _ = R.component_paths([_of(s, 21)], 21, [[s]], min_len=21)
        lines = out["component-1.seq.fasta"].decode().split("\n")
        assert lines[0] == f">1 length={n} av_weight=1 min_weight=0 max_weight=0" and lines[-1] == ""
        assert [len(x) for x in lines[1:-1]] == [70] * (n // 70) + ([n % 70] if n % 70 else [])
        assert "".join(lines[1:-1]) == s


def test_two_components_sharing_a_stretch():
    k = 9
    rng = np.random.default_rng(5)
    left, mid, right = ("".join("ACGT"[i] for i in rng.integers(0, 4, n)) for n in (16, 14, 16))
    a, b = left + mid, mid + right                                                           # a ends with the stretch b starts with
    comps = [_of(a, k), _of(b, k)]
    assert len(set(comps[0][0].tolist()) & set(comps[1][0].tolist())) == len(mid) - k + 1
    q = "TTTTTT" + left + mid + right + "TTTTTT"
    got = _paths(comps, k, [[q]], min_len=k)
    assert got == {1: [a], 2: [b]}                                                           # both hold the stretch, each goes on on its own side
    assert _paths(comps, k, [[mid]], min_len=k) == {1: [mid], 2: [mid]}


def test_empty_component_and_selection():
    k = 5
    gene = "ACGGTCATTGCA"
    comps = [_of(gene, k), _of("ACG", k), _of(S.rc_str(gene) + "GG", k)]
    assert comps[1][1] == 0
    out, _ = R.component_paths(comps, k, [[gene]], min_len=k)
    assert sorted(out) == ["component-1.seq.fasta", "component-2.seq.fasta", "component-3.seq.fasta"] and out["component-2.seq.fasta"] == b""
    sel, _ = R.component_paths(comps, k, [[gene]], selection=[3, 1, 3], min_len=k)
    assert sorted(sel) == ["component-1.seq.fasta", "component-3.seq.fasta"]
    assert sel["component-1.seq.fasta"] == out["component-1.seq.fasta"] and sel["component-3.seq.fasta"] == out["component-3.seq.fasta"]
    for bad in ([0], [4], [1, -1]):
        try:
            R.component_paths(comps, k, [[gene]], selection=bad, min_len=k)
        except IndexError:
            continue
        raise AssertionError(bad)


def test_fixture():
    """tests/golden/component_paths: contigs.fa (13 records, one with an N), genes.k21.components.bin = the first four surviving
    records as components (seq2comp at k = 21; the fourth is shorter than k), paths/ = -a at the default -l 50"""
    fa = os.path.join(GOLD, "contigs.fa")
    seqs = S.read_fasta(fa)
    names = [ln[1:].strip() for ln in open(fa) if ln.startswith(">")]
    assert len(names) == 13 and len(seqs) == 12 and "with_N" in names and any(ln[0] in "acgt" for ln in open(fa))
    comps = S.components(seqs[:4], 21)
    assert S.components_bin(comps) == open(os.path.join(GOLD, "genes.k21.components.bin"), "rb").read()
    out, reached = R.component_paths(comps, 21, [seqs])
    assert not reached and sorted(out) == sorted(os.listdir(os.path.join(GOLD, "paths"))) == [f"component-{i}.seq.fasta" for i in (1, 2, 3, 4)]
    for name, data in out.items():
        assert data == open(os.path.join(GOLD, "paths", name), "rb").read(), name
    assert out["component-4.seq.fasta"] == b"" and sum(len(d) for d in out.values()) < 4096
    got = _paths(comps, 21, [seqs])
    a, b, c = seqs[0], seqs[1], seqs[2]
    # gene_a: itself, then its stretches in contig_1, contig_3 (lower case in the file), contig_5, gene_c / contig_4 (the shared 70 bases), contig_7
    assert got[1][0] == a and [len(x) for x in got[1]] == sorted((len(x) for x in got[1]), reverse=True)
    # (a path may be a base or two longer than the piece that was planted: the filler next to it can happen to agree)
    def holds(no, piece, times=1):
        return sum(piece in x and len(x) <= len(piece) + 3 for x in got[no]) == times
    assert holds(1, a[10:100]) and holds(1, a[40:130]) and holds(1, a[0:75]) and holds(1, a[100:150]) and holds(1, a[50:120], 2) and len(got[1]) == 7
    assert got[2][:2] == [b, b] and holds(2, S.rc_str(b[5:90])) and holds(2, b[0:60]) and holds(2, b[20:80]) and len(got[2]) == 5
    assert got[3][0] == c and holds(3, c[20:120]) and sum(a[50:120] in x for x in got[3]) == 4 and sum(a[50:100] in x for x in got[3]) == 5 and len(got[3]) == 5


def test_header_declares_the_calls():
    from metafast_amd import lib as L
    text = open(L.HEADER_PATH).read()
    assert re.search(r"\bint\s+mf_paths_create\(mf_ctx \*ctx, mf_comps \*c, const uint32_t \*selection, uint64_t n_selection, int min_len, uint64_t max_paths,\s*mf_paths \*\*out\);", text)
    assert re.search(r"\bint\s+mf_paths_add\(mf_paths \*p, const void \*d_bases, const void \*d_offsets, uint64_t n_seqs, uint64_t n_bases\);", text)
    assert re.search(r"\bint\s+mf_component_paths\(mf_ctx \*ctx, const char \*components_bin, int k, const char \*const \*files, int nfiles, const uint32_t \*selection,\s*"
                     r"uint64_t n_selection, int min_len, uint64_t max_paths, const char \*out_dir, uint64_t \*n_components,\s*uint64_t \*n_paths\);", text)
    calls = {"mf_paths_create", "mf_paths_add", "mf_paths_finish", "mf_paths_destroy", "mf_paths_stats", "mf_paths_slots", "mf_paths_text", "mf_paths_write",
             "mf_component_paths"}
    assert calls <= set(L.exported_symbols()) and calls <= set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", text))
    assert L.MAX_PATHS_COUNT == R.MAX_PATHS_COUNT == 10 ** 6
