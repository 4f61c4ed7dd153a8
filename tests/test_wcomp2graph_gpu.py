"""comp2graph on wide components on the GPU (mf_wcomp2graph.hip, 32 <= k <= 63) against tests/comp2graph_ref.py, which holds for any k:
on every case the tool's own rules (names dense from 1, printed strand <= its reverse complement, L lines sorted, components in file
order) and the cover check (every canonical member k-mer on exactly one segment exactly once: no reference needed); on the plain cases
equality with the reference up to names and line order (they are order-independent: tests/test_wcomp2graph_cpu.py); on isolated cycles
and hairpins, where the reference has no answer, the stated rule.  The shapes are the smallest at which a stage can go wrong."""
import os
import subprocess

import numpy as np
import pytest

import comp2graph_ref as G
import comp2seq_ref as R
import wcomp2graph_cases as WC
import wcomp2seq_ref as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metafast.sh")
CASES = WC.crafted()


def _load(ctx, tmp_path, k, comps):
    path = tmp_path / "components.bin"
    W.write_components(path, comps)
    return ctx.load_components_wide(str(path), k), str(path)


def _run(*args, cwd=None):
    return subprocess.run([EXE, *[str(a) for a in args], "--device", "0"], capture_output=True, text=True, timeout=300, cwd=cwd)


def _checked(text, stats, k, comps):
    parsed = G.check_rules(text, k, len(comps))
    WC.cover(text, comps, k)
    assert stats["segments"] == sum(len({s[0] for s in v[0]}) for v in parsed.values())
    assert stats["links"] == sum(len(v[1]) for v in parsed.values())
    return parsed


@pytest.mark.parametrize("name", list(CASES))
def test_crafted(gpu_ctx, tmp_path, name):
    k, comps, family = CASES[name]
    c, _ = _load(gpu_ctx, tmp_path, k, comps)
    text, stats = gpu_ctx.wcomps_graph(c)
    parsed = _checked(text, stats, k, comps)
    if family == "plain":
        assert stats["cycles"] == 0
        assert G.canon(text) == G.canon(G.gfa(comps, k))
    if name.startswith("1_fork"):
        assert (stats["segments"], stats["links"]) == (3, 4)
    if name == "2_path3_k33":
        assert text == WC.PATH3_TEXT
    if name == "2_fork_literal_k33":
        assert text == WC.FORK_TEXT
    if name == "3_rc_printed_k63":
        assert len(parsed[0][0]) == 1 and not parsed[0][1]
    if name.startswith("4_one_word_apart"):
        assert stats["segments"] == 10 and stats["links"] == 0
    if name.startswith("5_palindromes"):
        for ci in range(3):
            seqs = [s[1] for s in parsed[ci][0]]
            assert sum(1 for s in seqs if s == R.rc_str(s)) == 2, ci
    if name == "6_cycle_k33":
        n, m, circ = len(comps[0]), min(comps[0]), WC.CYCLE[k]
        assert n == 15 and len(circ) == n
        rots = [(s[i:] + s[:i]) for s in (circ, R.rc_str(circ)) for i in range(n)]
        q = [(r * 4)[:n + k - 1] for r in rots if R.encode((r * 4)[:k]) == m]
        assert len(q) == 1                                   # opened at its smallest canonical k-mer, on the canonical strand
        assert stats["cycles"] == 1
        assert parsed[0][0] == [("1_i0", min(q[0], R.rc_str(q[0])), n + k - 1, n + k - 1)]
        assert parsed[0][1] == [("1_i0", "+", "1_i0", "+", f"{k - 1}M"), ("1_i0", "-", "1_i0", "-", f"{k - 1}M")]
    if family == "hairpin":
        s = WC.HAIRPIN[k]
        assert parsed[0][0] == [("1_i0", R.rc_str(s), k + 2, k + 2)] and R.rc_str(s) < s
        assert parsed[0][1] == [("1_i0", "-", "1_i0", "+", f"{k - 1}M")]
    if name == "7_shared_k33":
        assert set(W.component_tables(comps, k)[0]) & set(W.component_tables(comps, k)[1]) and list(parsed) == [0, 1]
    if name == "7_empty_between_k33":
        assert list(parsed) == [0, 2]
    if name == "7_no_components":
        assert text == "" and stats == {"segments": 0, "links": 0, "cycles": 0}
    if name == "7_x_and_rcx_k63":                            # one row, KC as if listed once
        assert [(s[2], s[3]) for s in parsed[0][0]] == [(9 + k - 1, 9 + k - 1)]


def test_one_path_of_70000_kmers_k63(gpu_ctx, tmp_path):
    """beyond 2^16 rows and 17 doubling rounds; the single S line computed directly"""
    k, n = 63, 70000
    seq = R._simple_path(np.random.default_rng(7063), n, k)
    c, _ = _load(gpu_ctx, tmp_path, k, [sorted(R.kmers_of(seq, k))])
    text, stats = gpu_ctx.wcomps_graph(c)
    assert text == f"S\t1_i0\t{min(seq, R.rc_str(seq))}\tLN:i:{n + k - 1}\tKC:i:{n + k - 1}\n"
    assert stats == {"segments": 1, "links": 0, "cycles": 0}


def test_70000_single_kmer_components_k33(gpu_ctx, tmp_path):
    """more than 2^16 components; the text computed directly"""
    k, comps = R.case_singles(33)
    assert len(comps) == 70000
    c, _ = _load(gpu_ctx, tmp_path, k, comps)
    text, stats = gpu_ctx.wcomps_graph(c)
    want = "".join(f"S\t1_i{i}\t{G.normalize(R.decode(m[0], k))}\tLN:i:{k}\tKC:i:{k}\n" for i, m in enumerate(comps))
    assert text == want
    assert stats == {"segments": 70000, "links": 0, "cycles": 0}


def test_values_in_three_modes(gpu_ctx, tmp_path):
    k, comps, _ = CASES["9_bubble_k63"]
    km = sorted(W.component_tables(comps, k)[0])
    # km[0]: no file holds it; km[1]: all hold it with counts > 1; km[5]: 30 000 + 30 000 -> 32 767; the others: some
    tabs = [{km[1]: 3, km[2]: 1, km[5]: 30000}, {km[1]: 2, km[3]: 7, km[5]: 30000}, {km[1]: 5, km[2]: 2, km[7]: 1}]
    files = []
    for i, t in enumerate(tabs):
        files.append(str(tmp_path / f"s{i}.kmers.bin"))
        open(files[-1], "wb").write(W.kmers_bin(t))
    _, cf = _load(gpu_ctx, tmp_path, k, comps)
    seen = []
    for cov, vals in ((False, G.sample_values(tabs, False)), (True, G.sample_values(tabs, True)), (None, None)):
        out = tmp_path / f"g_{cov}.gfa"
        nc, ns, nl = gpu_ctx.comp2graph_wide(cf, k, str(out), kmers_files=files if cov is not None else (), coverage=bool(cov))
        text = open(out).read()
        G.check_rules(text, k, 1)
        WC.cover(text, comps, k)
        assert G.canon(text) == G.canon(G.gfa(comps, k, vals))
        assert (nc, ns, nl) == (1, 4, 8)
        seen.append(sorted(s[3] for s in G.parse(text)[0][0]))
    assert len({tuple(s) for s in seen}) == 3
    assert G.sample_values(tabs, True)[km[5]] == 32767 and km[0] not in G.sample_values(tabs, False)
    # resident tables give the same bytes
    tables = [gpu_ctx.load_kmers_wide([f], k) for f in files]
    c = gpu_ctx.load_components_wide(cf, k)
    for cov in (False, True):
        text, _ = gpu_ctx.wcomps_graph(c, samples=tables, coverage=cov)
        assert text == open(tmp_path / f"g_{cov}.gfa").read()


@pytest.fixture(scope="module")
def generated(oracle):
    from metafast_amd import lib as L
    k, comps, samples = WC.generated(oracle, L)
    vals = G.sample_values(samples, False)
    return k, comps, samples, vals, G.parity(comps, k, vals), G.canon(G.gfa(comps, k, vals))


def test_generated_through_the_driver(generated, tmp_path):
    k, comps, samples, vals, par, want = generated
    assert par.count(False) <= len(comps) // 100
    cf = tmp_path / "components.bin"
    W.write_components(cf, comps)
    files = []
    for i, t in enumerate(samples):
        files.append(tmp_path / f"s{i}.kmers.bin")
        open(files[-1], "wb").write(W.kmers_bin({x: min(c, 32767) for x, c in t.items()}))
    texts = []
    for run in range(2):
        wd = tmp_path / f"w{run}"
        r = _run("-t", "comp2graph", "--wide-kmers", "-k", k, "-cf", cf, "-i", *files, "-w", wd)
        assert r.returncode == 0, r.stderr
        assert (wd / "SUCCESS").exists() and (wd / "in.properties").exists()
        assert "components loaded from" in r.stderr and "Graph components saved to GFA format!" in r.stderr
        texts.append(open(wd / "components-graph.gfa", "rb").read())
    assert texts[0] == texts[1] and texts[0]
    text = texts[0].decode()
    G.check_rules(text, k, len(comps))
    WC.cover(text, comps, k)
    got = G.canon(text)
    assert sorted(got) == sorted(want)
    for c in want:
        if par[c]:
            assert got[c] == want[c], c


def test_round_trip_from_reads(ref_files, tmp_path):
    """metafast.sh --wide-kmers -k 33 over the three golden read files, then comp2graph --wide-kmers on its components.bin and .kmers.bin"""
    k, wd = 33, tmp_path / "wd"
    r = _run("--wide-kmers", "-k", k, "-i", *ref_files, "-w", wd)
    assert r.returncode == 0, r.stderr[-3000:]
    cf = wd / "component-cutter" / "components.bin"
    kmers = sorted(str(p) for p in (wd / "kmer-counter-many" / "kmers").glob("*.kmers.bin"))
    assert len(kmers) == 3
    g = tmp_path / "g"
    r = _run("-t", "comp2graph", "--wide-kmers", "-k", k, "-cf", cf, "-i", *kmers, "-w", g)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (g / "SUCCESS").exists() and "wide-kmers" in open(g / "in.properties").read()
    import wide_files_ref as WF
    sizes, _, hi, lo = WF.decode_components(open(cf, "rb").read())
    flat = [(int(h) << 64) | int(x) for h, x in zip(np.asarray(hi).tolist(), np.asarray(lo).tolist())]
    comps, at = [], 0
    for s in sizes:
        comps.append(flat[at:at + int(s)])
        at += int(s)
    assert comps and at == len(flat)
    text = open(g / "components-graph.gfa").read()
    assert text
    G.check_rules(text, k, len(comps))
    WC.cover(text, comps, k)
    r = _run("-t", "comp2graph", "--wide-kmers", "-k", k, "-cf", cf, "-i", *kmers, "-w", g, "-c")
    assert r.returncode == 0 and "SUCCESS file found for tool comp2graph" in r.stderr


def test_refusals_name_the_file_and_write_nothing(gpu_ctx, tmp_path):
    from metafast_amd import lib as L
    _, comps21 = R.case_adjacent(21)
    narrow = tmp_path / "narrow_components.bin"
    R.write_components(narrow, comps21)
    out = tmp_path / "x.gfa"
    with pytest.raises(L.MetafastError, match="narrow_components.bin"):
        gpu_ctx.comp2graph_wide(str(narrow), 40, str(out))
    assert not out.exists()
    _, comps40 = R.case_adjacent(40)
    comps40 = WC.sorted_comps(comps40)
    assert comps40[0][0] >> 66
    wide40 = tmp_path / "wide40_components.bin"
    W.write_components(wide40, comps40)
    with pytest.raises(L.MetafastError, match=r"wide40_components.bin.*member 0.*not below 4\^k"):
        gpu_ctx.comp2graph_wide(str(wide40), 33, str(out))
    assert not out.exists()
    for k in (31, 64):
        with pytest.raises(L.MetafastError, match="32 <= k <= 63"):
            gpu_ctx.comp2graph_wide(str(wide40), k, str(out))
        assert not out.exists()
    # a sample table of another k: the file form reads the file as a table of k = 40 -- a file of 33-mers is in range for it, so the resident form is the one that can hold another k
    k33, c33, _ = CASES["2_fork_literal_k33"]
    f33 = tmp_path / "s33.kmers.bin"
    f33.write_bytes(W.kmers_bin({R.canon(x, k33): 1 for x in c33[0]}))
    t33 = gpu_ctx.load_kmers_wide([str(f33)], k33)
    c40 = gpu_ctx.load_components_wide(str(wide40), 40)
    with pytest.raises(L.MetafastError, match="a sample table has k = 33, the components k = 40"):
        gpu_ctx.wcomps_graph(c40, samples=[t33])
    text, _ = gpu_ctx.wcomps_graph(c40)                       # (and the components are fine by themselves)
    assert text
    assert not out.exists()
