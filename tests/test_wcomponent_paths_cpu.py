"""component-paths for k = 32 ... 63 without a GPU: the Python-integer restatement (tests/wcomponent_paths_ref.py) against the k <= 31 one
and a literal, what the cases of tests/test_wcomponent_paths_gpu.py hold, the header, and the driver on the stub build."""
import os
import re
import subprocess

import numpy as np
import pytest

import component_paths_ref as N
import seq2comp_ref as S
import wcomponent_paths_cases as CASES
import wcomponent_paths_ref as R
import wseq2comp_ref as W
from test_driver_tools_cpu import ENV, stub_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK64 = (1 << 64) - 1


# ---- the restatement ----
@pytest.mark.parametrize("k", [21, 31])
def test_same_algorithm_as_the_narrow_reference(k):
    """on the narrow hand cases (two components that share a stretch, an empty one, reverse complements, lower case, three files) the
    runs are find_runs_plain's, and so are the files"""
    rng = np.random.default_rng(900 + k)
    r = lambda n: CASES.rnd(rng, n)
    gene, other, left, right, mid = r(150), r(90), r(40), r(40), r(3 * k)
    seqs = [gene, r(k - 1), left + mid, mid + right, other]
    files = [[gene + r(40), r(40) + gene, r(30) + gene[10:80] + r(30), r(k - 1), "", (r(25) + gene[20:100] + r(25)).lower(), r(30) + left + mid + right + r(30), mid],
             [r(20) + other[0:50] + r(20) + other[30:80] + r(20), S.rc_str(other)[0:50] + r(5) + gene[100:150]], [r(50), gene[3:53] + r(2) + gene[60:110]]]
    narrow = S.components(seqs, k)
    wide = W.components(seqs, k)
    assert [[int(x) for x in c[0]] for c in narrow] == [c[0] for c in wide]
    runs = R.find_runs(wide, k, files)
    assert runs == N.find_runs_plain(narrow, k, files) and sum(len(x) for x in runs) >= 12 and runs[1] == []
    for kw in ({"min_len": k}, {"min_len": 50}, {"min_len": k, "selection": [3, 1, 3]}, {"min_len": k, "max_paths": 2}):
        assert R.component_paths(wide, k, files, **kw) == N.component_paths(narrow, k, files, **kw)


def test_literal_k33():
    """the 35-base sequence of tests/test_wseq2comp_cpu.py has three windows; component 1 holds the k-mers of windows 0 and 1 (weight 5:
    5 / 2 = 2.5, Math.round gives 3), component 2 that of window 2.  The sequence itself: component 1 matches positions 0 .. 1, a path of
    34 bases from base 0; component 2 position 2, 33 bases from base 2.  Its reverse complement has window 2 at position 0 and windows 1, 0
    at positions 1, 2: component 2 gets its first 33 bases, component 1 the 34 from base 1.  Two paths of equal length stay in encounter
    order."""
    k = 33
    seq = "TCGATTGCAAGGCTTACCGATAGGCTAACGTTCAG"
    rc = "CTGAACGTTAGCCTATCGGTAAGCCTTGCAATCGA"
    assert W.rc_str(seq) == rc
    occ = W.occurrences(seq, k)
    comps = [(sorted(occ[:2]), 2, 5), ([occ[2]], 1, 1)]
    out, reached = R.component_paths(comps, k, [[seq, "ACGT", rc.lower()]], min_len=33)
    h = " min_weight=0 max_weight=0\n"
    assert out == {"component-1.seq.fasta": (">1 length=34 av_weight=3" + h + "TCGATTGCAAGGCTTACCGATAGGCTAACGTTCA\n"
                                             ">2 length=34 av_weight=3" + h + "TGAACGTTAGCCTATCGGTAAGCCTTGCAATCGA\n").encode(),
                   "component-2.seq.fasta": (">1 length=33 av_weight=1" + h + "GATTGCAAGGCTTACCGATAGGCTAACGTTCAG\n"
                                             ">2 length=33 av_weight=1" + h + "CTGAACGTTAGCCTATCGGTAAGCCTTGCAATC\n").encode()}
    assert reached == []
    assert R.component_paths(comps, k, [[seq, rc]], min_len=34)[0]["component-2.seq.fasta"] == b""
    assert R.component_paths(comps, k, [[seq, rc]], min_len=33, max_paths=1) == (
        {"component-1.seq.fasta": out["component-1.seq.fasta"][:out["component-1.seq.fasta"].index(b">2")],
         "component-2.seq.fasta": out["component-2.seq.fasta"][:out["component-2.seq.fasta"].index(b">2")]}, [1, 2])


# ---- what the cases hold ----
def _ends(runs):
    return [(first, cur - 1) for _, first, cur in runs]


@pytest.mark.parametrize("k", CASES.KS)
def test_case_both_words(k):
    comps, files, (a, b, c, d) = CASES.both_words(k)
    assert len({a, b, c, d}) == 4
    assert c >> 64 == d >> 64 and c & MASK64 != d & MASK64                     # one high word, two low words
    if k > 32:
        assert a & MASK64 == b & MASK64 and a >> 64 != b >> 64                 # one low word, two high words
    else:
        assert a >> 64 == b >> 64 == 0
    runs = R.find_runs(comps, k, files)
    # the sequence that walks from one k-mer into the other: each component gets ONE position, side by side
    assert _ends(runs[0])[:2] == [(21, 21), (0, 0)] and _ends(runs[1])[:2] == [(22, 22), (1, 1)]
    assert _ends(runs[2])[:2] == [(8, 8), (0, 0)] and _ends(runs[3])[:2] == [(9, 9), (1, 1)]
    out = R.component_paths(comps, k, files, min_len=k, runs=runs)[0]
    for text in out.values():
        assert text.count(b">") == 4 and text.count(f" length={k} ".encode()) == 4      # never k + 1: the run breaks between them
    assert R.component_paths(comps, k, files, min_len=k + 1, runs=runs)[0] == {f"component-{i}.seq.fasta": b"" for i in (1, 2, 3, 4)}


@pytest.mark.parametrize("k", CASES.KS)
def test_case_strand(k):
    comps, files, (s1, s2) = CASES.strand(k)
    out = R.component_paths(comps, k, files, min_len=k)[0]
    one = out["component-1.seq.fasta"].decode()
    assert one.startswith(">1 length=150 ") and "".join(one.split(">")[1].split("\n")[1:]) == W.rc_str(s1)       # forward as the sequence has it
    assert "".join(one.split(">")[2].split("\n")[1:]) == s1 and one.count(">") == 3 and " length=95 " in one
    two = out["component-2.seq.fasta"].decode()
    assert "".join(two.split(">")[1].split("\n")[1:]) == W.rc_str(s2) and files[0][2] == W.rc_str(s2).lower()      # lower case in, upper case out


@pytest.mark.parametrize("k", CASES.KS)
def test_case_borders(k):
    comps, files, plans = CASES.borders(k)
    run = CASES.RUN
    src = open(os.path.join(ROOT, "metafast_amd", "csrc", "mf_cp.h")).read()
    assert int(re.search(r"^#define CP_RUN (\d+)", src, re.M).group(1)) == run
    runs = R.find_runs(comps, k, files[:1])
    for i, plan in enumerate(plans):
        assert _ends(runs[i]) == list(plan), i                                 # the plan is what the restatement finds
    ends = [e for r in runs for e in _ends(r)]
    assert any(b == run - 1 for a, b in ends) and any(a == run for a, b in ends) and any(a < run <= b for a, b in ends)
    assert (0, 0) in ends and (2 * run - 1, 2 * run - 1) in ends
    assert [max(0, len(s) - k + 1) for s in files[1]] == [run, 0, run + 1, 0, 1, run - 1, 0, 2 * run, 1]
    seventh = _ends(R.find_runs(comps, k, files[1:])[6])
    assert seventh == [(0, run - 1), (0, run), (0, 0), (0, run - 2), (0, 2 * run - 1), (0, 0)]       # each whole, none joined across the short ones


@pytest.mark.parametrize("k", CASES.KS)
def test_case_shared(k):
    comps, files, (seqs, listings) = CASES.shared(k)
    assert listings == 5 and comps[0] == comps[1] == comps[3]
    dom = set(W.occurrences(seqs[0][40:150], k))
    assert all(dom <= set(c[0]) for c in comps)
    out = R.component_paths(comps, k, files, min_len=k)[0]
    assert out["component-1.seq.fasta"] == out["component-2.seq.fasta"] == out["component-4.seq.fasta"] != b""
    dom_text = seqs[0][40:150]
    for t in out.values():                                                     # every component gets the shared stretch, from every sequence that holds it
        paths = ["".join(rec.split("\n")[1:]) for rec in t.decode().split(">")[1:]]
        assert sum(dom_text in p for p in paths) == 3 and any(W.rc_str(dom_text) in p for p in paths)


@pytest.mark.parametrize("k", CASES.KS)
def test_case_capped(k):
    comps, files, once = CASES.capped(k)
    runs = R.find_runs(comps, k, files)
    assert len(runs[0]) == 6 and runs[1] == [] and len(runs[2]) == 2 and comps[1][1] == 0
    assert all(cur - first - 1 + k >= 80 for r in runs for _, first, cur in r)
    assert R.find_runs(comps, k, once) == runs
    for cap, reached in ((5, [1]), (6, [1]), (7, []), (2, [1, 3])):
        assert R.component_paths(comps, k, files, min_len=80, max_paths=cap, runs=runs)[1] == reached
    sel = R.component_paths(comps, k, files, selection=[3, 1, 3], min_len=80, runs=runs)[0]
    assert list(sel) == ["component-3.seq.fasta", "component-1.seq.fasta"]
    for bad in ([0], [4], [1, 4]):
        with pytest.raises(IndexError):
            R.component_paths(comps, k, files, selection=bad, runs=runs)


@pytest.mark.parametrize("k", CASES.KS)
def test_case_random(k):
    comps, files, genes = CASES.random_case(k)
    assert len(comps) == 200 and sum(len(f) for f in files) == 300
    out = R.component_paths(comps, k, files, min_len=k)[0]
    assert sum(t.count(b">") for t in out.values()) == CASES.RANDOM_PATHS[k]
    assert (sum(1 for c in comps if c[1] == 0) >= 1) == (k >= 47)                  # genes of 40 .. 400 bases: empty components at the larger k
    assert sum(len(t) > 0 for t in out.values()) >= 150


# ---- the header ----
def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "metafast_hip.h")).read())
    assert ("int mf_paths_create_wide(mf_ctx *ctx, mf_wcomps *c, const uint32_t *selection, uint64_t n_selection, int min_len, uint64_t max_paths, "
            "mf_paths **out);") in text
    assert ("int mf_component_paths_wide(mf_ctx *ctx, const char *components_bin, int k, const char *const *files, int nfiles, const uint32_t *selection, "
            "uint64_t n_selection, int min_len, uint64_t max_paths, const char *out_dir, uint64_t *n_components, uint64_t *n_paths);") in text


# ---- the driver on the stub build ----
@pytest.fixture(scope="module")
def driver():
    return stub_driver()


def _run(driver, cwd, *args):
    return subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, env=ENV, timeout=120, cwd=str(cwd))


def test_driver_takes_wide_component_paths(driver, tmp_path):
    (tmp_path / "s.fa").write_text(">a\n" + "ACGT" * 20 + "\n")
    (tmp_path / "c.bin").write_bytes(W.components_bin(W.components(["ACGGT" * 16], 33)))
    # with the flag and k > 31 the run gets past check_k to the library: the stub has no such entry, and the run names it
    r = _run(driver, tmp_path, "-t", "component-paths", "--wide-kmers", "-k", 33, "-cf", "c.bin", "--seq", "s.fa", "-a", "-w", "w1")
    assert r.returncode == 1 and "this build of the library has no mf_paths_create_wide" in r.stderr + r.stdout, r.stderr
    assert not (tmp_path / "w1" / "SUCCESS").exists() and not (tmp_path / "w1" / "paths").exists()
    # without the flag the reference's message, as ever; above 63 the wide one
    r = _run(driver, tmp_path, "-t", "component-paths", "-k", 33, "-cf", "c.bin", "--seq", "s.fa", "-a", "-w", "w2")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr + r.stdout
    r = _run(driver, tmp_path, "-t", "component-paths", "--wide-kmers", "-k", 64, "-cf", "c.bin", "--seq", "s.fa", "-a", "-w", "w3")
    assert r.returncode == 1 and "The size of k-mer must be no more than 63." in r.stderr + r.stdout
    # k <= 31: the flag changes nothing; the checks in front of the library are the narrow tool's
    r = _run(driver, tmp_path, "-t", "component-paths", "--wide-kmers", "-k", 21, "-cf", "c.bin", "--seq", "s.fa", "-a", "-w", "w4")
    out = r.stderr + r.stdout
    assert "mf_paths_create_wide" not in out and "no more than" not in out, out
    r = _run(driver, tmp_path, "-t", "component-paths", "--wide-kmers", "-k", 33, "-cf", "c.bin", "--seq", "s.fa", "-w", "w5")
    assert r.returncode == 1 and "No components to process!!! Do you forget to set --all-components or --components n1,n2,...?" in r.stderr + r.stdout
    r = _run(driver, tmp_path, "-t", "component-paths", "--wide-kmers", "-k", 33, "-cf", "c.bin", "--seq", "none.fa", "-a", "-w", "w6")
    assert r.returncode == 1 and "none.fa" in r.stderr + r.stdout
