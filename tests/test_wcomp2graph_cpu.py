"""comp2graph at k = 32 ... 63 without a GPU: the yardstick of tests/test_wcomp2graph_gpu.py -- tests/comp2graph_ref.py at wide k pinned on
GFA written out by hand, and WHERE it is a yardstick (the cases on which its canonical form does not depend on the iteration order of the
reference's hash map) --, and the driver's host side on the stub build (the recipe of tests/test_driver_tools_cpu.py)."""
import subprocess

import pytest

import comp2graph_ref as G
import comp2seq_ref as R
import wcomp2graph_cases as WC
import wcomp2seq_ref as W
from test_driver_tools_cpu import ENV, stub_driver

CASES = WC.crafted()


def test_a_path_of_three_33_mers_by_hand():
    k, comps, _ = CASES["2_path3_k33"]
    assert len(WC.PATH3) == 35 and len(comps[0]) == 3
    assert G.canon(G.gfa(comps, k)) == G.canon(WC.PATH3_TEXT)
    G.check_rules(WC.PATH3_TEXT, k, 1)
    WC.cover(WC.PATH3_TEXT, comps, k)


def test_a_fork_at_k_33_by_hand():
    k, comps, _ = CASES["2_fork_literal_k33"]
    assert len(WC.FORK_TRUNK) == 33 and WC.FORK_A[:-1] == WC.FORK_C[:-1] == WC.FORK_TRUNK[1:]
    assert G.canon(G.gfa(comps, k)) == G.canon(WC.FORK_TEXT)
    G.check_rules(WC.FORK_TEXT, k, 1)
    WC.cover(WC.FORK_TEXT, comps, k)
    # the names: the canonical k-mers in code order (the member list holds + C as written, which is not its canonical strand)
    assert comps[0] == sorted(R.encode(s) for s in (WC.FORK_TRUNK, WC.FORK_A, WC.FORK_C)) and R.canon(R.encode(WC.FORK_C), k) != R.encode(WC.FORK_C)
    assert R.canon(R.encode(WC.FORK_TRUNK), k) < R.canon(R.encode(WC.FORK_C), k) < R.canon(R.encode(WC.FORK_A), k)


@pytest.mark.parametrize("name", list(CASES))
def test_where_the_restatement_is_a_yardstick(name):
    k, comps, family = CASES[name]
    assert 32 <= k <= 63 and all(m == sorted(m) and all(0 <= x < 4 ** k for x in m) for m in comps)
    par = G.parity(comps, k)
    if family == "plain":
        assert all(par), name
    elif family == "hairpin":
        assert not all(par)
    else:
        assert G.gfa(comps, k) == ""                         # an isolated cycle merges itself away: the reference draws nothing


def test_the_cases_keep_their_point():
    assert all(x >> 64 == 0 for x in CASES["1_fork_k32"][1][0])                      # k = 32: every high word is 0
    assert any(x >> 64 for x in CASES["1_fork_k33"][1][0])
    k, comps, _ = CASES["3_rc_printed_k63"]
    segs = G.parse(G.gfa(comps, k))[0][0]
    walked = R.rc_str(segs[0][1])                            # the walk starts at the end with the smaller canonical k-mer, on its canonical strand
    assert len(segs) == 1 and R.canon(R.encode(walked[:k]), k) == R.encode(walked[:k]) < R.canon(R.encode(segs[0][1][:k]), k) and segs[0][1] < walked
    for k in (32, 62):
        text = G.gfa(CASES[f"5_palindromes_k{k}"][1], k)
        for c in range(3):
            seqs = [s[1] for s in G.parse(text)[c][0]]
            assert sum(1 for s in seqs if s == R.rc_str(s)) == 2, (k, c)             # two S lines per palindromic k-mer
    assert len(G.parse(G.gfa(CASES["9_bubble_k63"][1], 63))[0][0]) == 4
    k, comps, _ = CASES["7_x_and_rcx_k63"]
    assert len(comps[0]) == 10 and len(W.component_tables(comps, k)[0]) == 9
    assert set(W.component_tables(CASES["7_shared_k33"][1], 33)[0]) & set(W.component_tables(CASES["7_shared_k33"][1], 33)[1])


def test_generated_components_are_parity_cases(oracle):
    from metafast_amd import lib as L
    k, comps, samples = WC.generated(oracle, L)
    assert k == 33 and 100 <= len(comps) <= 1000
    par = G.parity(comps, k, G.sample_values(samples, False))
    assert par.count(False) <= len(comps) // 100, par.count(False)


# ---- the driver's host side ----
@pytest.fixture(scope="module")
def driver():
    return stub_driver()


def _run(driver, cwd, *args):
    return subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, env=ENV, timeout=120, cwd=str(cwd))


def test_the_driver_asks_for_the_wide_entry_point(driver, tmp_path):
    k, comps, _ = CASES["2_fork_literal_k33"]
    W.write_components(tmp_path / "components.bin", comps)
    r = _run(driver, tmp_path, "-t", "comp2graph", "-k", 33, "-cf", "components.bin", "-w", "w1")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr + r.stdout
    # with the flag the run gets past the options to the library: the stub has no such entry, and the run names it
    r = _run(driver, tmp_path, "-t", "comp2graph", "--wide-kmers", "-k", 33, "-cf", "components.bin", "-w", "w2")
    assert r.returncode == 1 and "this build of the library has no mf_comp2graph_wide" in r.stderr + r.stdout
    assert not (tmp_path / "w2" / "SUCCESS").exists()
    r = _run(driver, tmp_path, "-t", "comp2graph", "--wide-kmers", "-k", 33, "-cov", "-i", "a.kmers.bin", "--graph-file", "g.gfa", "-cf", "components.bin", "-w", "w3")
    assert r.returncode == 1 and "this build of the library has no mf_comp2graph_wide" in r.stderr + r.stdout
    r = _run(driver, tmp_path, "-t", "comp2graph", "--wide-kmers", "-k", 33, "-w", "w4")
    assert r.returncode == 1 and "Mandatory argument --components-file (-cf) not set" in r.stderr + r.stdout
    r = _run(driver, tmp_path, "-t", "comp2graph", "--wide-kmers", "-k", 64, "-cf", "components.bin", "-w", "w5")
    assert r.returncode == 1 and "The size of k-mer must be no more than 63." in r.stderr + r.stdout
    # k <= 31: the flag changes nothing, the narrow entry point is the one asked for
    r = _run(driver, tmp_path, "-t", "comp2graph", "--wide-kmers", "-k", 31, "-cf", "components.bin", "-w", "w6")
    assert r.returncode == 1 and "this build of the library has no mf_comp2graph" in r.stderr + r.stdout
    assert "mf_comp2graph_wide" not in r.stderr + r.stdout
