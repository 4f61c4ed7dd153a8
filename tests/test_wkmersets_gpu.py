"""NO-REFERENCE EXTENSION: unique-kmers-multi, kmers-filter and kmer-counter-posneg for k = 32 ... 63 -- the wide join (mf_wjoin.hip) and
mf_wtable_write_kmers_filtered compared exactly with the Python-integer reference of tests/wkmersets_ref.py, for every number of slices; the driver's
chain of pipeline 2 with --wide-kmers, byte by byte."""
import glob
import os
import subprocess

import numpy as np
import pytest

import wfeatures_ref as FR
import wide_files_ref as WF
import wkmersets_cases as CASES
import wkmersets_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metafast.sh")
KS = (32, 33, 47, 63)


def _write(path, table):
    path.write_bytes(R.kmers_bin(table))
    return str(path)


def _load(ctx, tmp_path, name, table, k):
    """a table as the library holds it: written as a wide file, loaded uncut"""
    return ctx.load_kmers_wide([_write(tmp_path / (name + ".kmers.bin"), table)], k, 0)


def _export(t):
    return R.from_words(*t.export())


def _same(got_tables, got_union, got_counts, want):
    assert got_union == want["n_union"] and got_counts == want["counts"]
    assert len(got_tables) == len(want["tables"])
    for t, w in zip(got_tables, want["tables"]):
        hi, lo, cnt = t.export()
        keys = [(int(h) << 64) | int(l) for h, l in zip(hi, lo)]
        assert keys == sorted(w) and [int(c) for c in cnt] == [w[x] for x in keys]


@pytest.mark.parametrize("k", KS)
def test_crafted_cases(gpu_ctx, tmp_path, k):
    ins, flt, _ = CASES.crafted(k)
    ti = [_load(gpu_ctx, tmp_path, f"i{j}", t, k) for j, t in enumerate(ins)]
    tf = [_load(gpu_ctx, tmp_path, f"f{j}", t, k) for j, t in enumerate(flt)]
    want = R.unique_kmers_multi(ins, flt, 1, 1, 9)
    try:
        for S in (1, 3, 7):
            gpu_ctx.set_option("stats_slices", S)
            _same(*gpu_ctx.unique_kmers_multi_wide(ti, tf, 1, 1, 9), want)
        gpu_ctx.set_option("stats_slices", 3)
        # no filters; one input (the list runs past it); b = 0 (the filters' counts of 1 knock out too) with min ... max inside the inputs; an empty input alone
        _same(*gpu_ctx.unique_kmers_multi_wide(ti, [], 1, 1, 9), R.unique_kmers_multi(ins, [], 1, 1, 9))
        _same(*gpu_ctx.unique_kmers_multi_wide(ti[:1], tf, 1, 1, 9), R.unique_kmers_multi(ins[:1], flt, 1, 1, 9))
        _same(*gpu_ctx.unique_kmers_multi_wide(ti, tf, 0, 2, 3), R.unique_kmers_multi(ins, flt, 0, 2, 3))
        _same(*gpu_ctx.unique_kmers_multi_wide(ti[3:], tf, 1, 1, 2), R.unique_kmers_multi([{}], flt, 1, 1, 2))
    finally:
        gpu_ctx.set_option("stats_slices", 0)


@pytest.mark.parametrize("k", (33, 63))
def test_random_cohort(gpu_ctx, tmp_path, k):
    rng = np.random.default_rng(1000 + k)
    mask = (1 << (2 * k)) - 1
    pool = sorted({R.canonical(int.from_bytes(rng.bytes(16), "big") & mask, k) for _ in range(40000)})
    tables = []
    for j in range(7):
        pick = rng.choice(len(pool), 20000, replace=False)
        cnt = rng.choice(np.array([1, 2, 3, 5, 9000, 20000, 32767]), len(pick), p=[0.3, 0.25, 0.2, 0.1, 0.05, 0.05, 0.05])
        tables.append({pool[int(i)]: int(c) for i, c in zip(pick, cnt)})
    ins, flt = tables[:5], tables[5:]
    ti = [_load(gpu_ctx, tmp_path, f"i{j}", t, k) for j, t in enumerate(ins)]
    tf = [_load(gpu_ctx, tmp_path, f"f{j}", t, k) for j, t in enumerate(flt)]
    want = R.unique_kmers_multi(ins, flt, 1, 1, 6)
    assert all(c > 0 for c in want["counts"][:5]) and want["counts"][5] == 0
    try:
        for S in (1, 7):
            gpu_ctx.set_option("stats_slices", S)
            _same(*gpu_ctx.unique_kmers_multi_wide(ti, tf, 1, 1, 6), want)
    finally:
        gpu_ctx.set_option("stats_slices", 0)
    # the file form: the same tables from their files, one resident at a time
    out = tmp_path / "out"
    out.mkdir()
    n_union, counts = gpu_ctx.unique_kmers_multi_wide_files([str(tmp_path / f"i{j}.kmers.bin") for j in range(5)],
                                                            [str(tmp_path / f"f{j}.kmers.bin") for j in range(2)], k, str(out), 1, 1, 6)
    assert n_union == want["n_union"] and counts == want["counts"]
    for i, w in enumerate(want["tables"], 1):
        assert (out / f"filtered_{i}.kmers.bin").read_bytes() == R.kmers_bin(w), i
    assert not (out / "filtered_7.kmers.bin").exists()


@pytest.mark.parametrize("k", (32, 47))
def test_write_kmers_filtered(gpu_ctx, tmp_path, k):
    ins, flt, _ = CASES.crafted(k)
    table, filt = ins[0], R.load(ins[1:], 0)
    t, f = _load(gpu_ctx, tmp_path, "t", table, k), _load(gpu_ctx, tmp_path, "f", filt, k)
    e = _load(gpu_ctx, tmp_path, "e", {}, k)
    out = tmp_path / "o.kmers.bin"
    some = 0
    for thr, fthr in ((1, 0), (0, 0), (2, 4), (0, 5), (1, 32766), (0, -1)):      # the thresholds on both sides; absent = 0 > -1
        want = R.filter_kmers(table, thr, filt, fthr)
        assert t.write_kmers_filtered(thr, f, fthr, str(out)) == len(want), (thr, fthr)
        assert out.read_bytes() == R.kmers_bin(want), (thr, fthr)
        some += 0 < len(want) < len(table)
    assert some >= 3 and set(table) - set(filt) and set(table) & set(filt)
    assert t.write_kmers_filtered(0, e, 0, str(out)) == 0 and out.read_bytes() == b""                   # an empty filter
    assert t.write_kmers_filtered(0, e, -1, str(out)) == len(table) and out.read_bytes() == R.kmers_bin(table)
    assert e.write_kmers_filtered(0, f, 0, str(out)) == 0 and out.read_bytes() == b""                   # an empty table


def test_refusals(gpu_ctx, tmp_path):
    from metafast_amd import lib as L
    ins = CASES.crafted(33)[0]
    a, b = _load(gpu_ctx, tmp_path, "a", ins[0], 33), _load(gpu_ctx, tmp_path, "b", ins[1], 33)
    other_k = _load(gpu_ctx, tmp_path, "c", CASES.crafted(47)[0][1], 47)
    with pytest.raises(L.MetafastError, match="--min-samples parameter cannot be greater than --max-samples parameter."):
        gpu_ctx.unique_kmers_multi_wide([a, b], [], 1, 3, 2)
    with pytest.raises(L.MetafastError, match="negative"):
        gpu_ctx.unique_kmers_multi_wide([a, b], [], -1, 1, 1)
    with pytest.raises(L.MetafastError, match=r"\(inputs\): table 1 has k = 47"):
        gpu_ctx.unique_kmers_multi_wide([a, other_k], [], 1, 1, 1)
    with pytest.raises(L.MetafastError, match=r"\(filters\): table 0 has k = 47"):
        gpu_ctx.unique_kmers_multi_wide([a], [other_k], 1, 1, 1)
    with pytest.raises(L.MetafastError, match="different k"):
        a.write_kmers_filtered(0, other_k, 0, str(tmp_path / "no.bin"))
    import torch
    ctx2 = L.Context(0, stream=torch.cuda.current_stream())
    try:
        foreign = ctx2.load_kmers_wide([str(tmp_path / "b.kmers.bin")], 33, 0)
        with pytest.raises(L.MetafastError, match=r"\(inputs\): table 1 belongs to another context"):
            gpu_ctx.unique_kmers_multi_wide([a, foreign], [], 1, 1, 1)
        with pytest.raises(L.MetafastError, match="another context"):
            a.write_kmers_filtered(0, foreign, 0, str(tmp_path / "no.bin"))
        foreign.close()
    finally:
        ctx2.close()
    with pytest.raises(L.MetafastError, match="32 <= k <= 63"):
        gpu_ctx.unique_kmers_multi_wide_files([str(tmp_path / "a.kmers.bin")], [], 31, str(tmp_path), 1, 1, 1)
    assert not (tmp_path / "no.bin").exists() and not (tmp_path / "filtered_1.kmers.bin").exists()


# ---- the driver: pipeline 2 with --wide-kmers ----
def _run(*args):
    return subprocess.run([EXE, *[str(a) for a in args], "--device", "0"], capture_output=True, text=True, timeout=300)


def test_cli_round_trip(gpu_ctx, tmp_path):
    k, b = 40, 1
    rng = np.random.default_rng(40)
    genome = "".join(rng.choice(list("ACGT"), 700))
    spans = {"p1": (0, 420), "p2": (80, 500), "n1": (300, 700), "n2": (360, 640)}
    files = {}
    for name, (s, e) in spans.items():
        reads = []
        for i in range(90):
            at = int(rng.integers(s, e - 64))
            r = genome[at:at + 64]
            reads.append(FR.revcomp_str(r) if i % 3 == 0 else r)
        files[name] = tmp_path / (name + ".fa")
        files[name].write_text("".join(f">r{i}\n{r}\n" for i, r in enumerate(reads)))
    sample = {name: _export(gpu_ctx.count_reads_wide([str(f)], k)) for name, f in files.items()}
    cut = {name: {x: c for x, c in t.items() if c > b} for name, t in sample.items()}
    # 1 kmer-counter-posneg
    w1 = tmp_path / "posneg"
    common = ["--wide-kmers", "-k", k, "-b", b]
    r = _run("-t", "kmer-counter-posneg", *common, "--positiveReads", files["p1"], files["p2"], "--negativeReads", files["n1"], files["n2"], "-w", w1)
    assert r.returncode == 0, r.stderr
    pos = sorted(glob.glob(str(w1 / "pos" / "kmers" / "*.kmers.bin"))), sorted(glob.glob(str(w1 / "neg" / "kmers" / "*.kmers.bin")))
    pos, neg = pos
    assert [os.path.basename(p) for p in pos + neg] == ["p1.kmers.bin", "p2.kmers.bin", "n1.kmers.bin", "n2.kmers.bin"]
    for p in pos + neg:
        assert open(p, "rb").read() == R.kmers_bin(cut[os.path.basename(p)[:2]]), p
    assert "wide-kmers = true" in (w1 / "in.properties").read_text() and (w1 / "SUCCESS").exists()
    # 2 unique-kmers-multi
    w2 = tmp_path / "unique"
    r = _run("-t", "unique-kmers-multi", *common, "-i", *pos, "--filter-kmers", *neg, "--min-samples", 1, "--max-samples", 2, "-w", w2)
    assert r.returncode == 0, r.stderr
    want = R.unique_kmers_multi([cut["p1"], cut["p2"]], [cut["n1"], cut["n2"]], b, 1, 2)
    assert want["counts"][0] > want["counts"][1] > 0
    for i, t in enumerate(want["tables"], 1):
        assert (w2 / "kmers" / f"filtered_{i}.kmers.bin").read_bytes() == R.kmers_bin(t), i
    log = (w2 / "log").read_text()
    assert f"Good k-mers printed to {w2}/kmers/filtered_2.kmers.bin" in log and "k-mers found, " in log
    # 3 kmers-filter: filtered_1 against the positive samples
    w3 = tmp_path / "filter"
    f1 = w2 / "kmers" / "filtered_1.kmers.bin"
    r = _run("-t", "kmers-filter", *common, "-i", f1, "--filter-kmers", *pos, "--max-thresh", 2, "-w", w3)
    assert r.returncode == 0, r.stderr
    kept = R.filter_kmers(R.load([want["tables"][0]], b), b, R.load([cut["p1"], cut["p2"]], b), 2 * 2)
    assert 0 < len(kept) < len(want["tables"][0])
    sel = w3 / "kmers" / "filtered_1.kmers.bin"
    assert sel.read_bytes() == R.kmers_bin(kept)
    # 4 features-calculator --selected on the components of the genome's halves
    (tmp_path / "seqs.fa").write_text(f">a\n{genome[:300]}\n>b\n{genome[300:]}\n")
    w4 = tmp_path / "comps"
    r = _run("-t", "seq2comp", "--wide-kmers", "-k", k, "-i", tmp_path / "seqs.fa", "-w", w4)
    assert r.returncode == 0, r.stderr
    sizes, _, hi, lo = WF.decode_components((w4 / "components.bin").read_bytes())
    members = [(int(h) << 64) | int(l) for h, l in zip(hi, lo)]
    comps, at = [], 0
    for s in sizes:
        comps.append(members[at:at + int(s)])
        at += int(s)
    w5 = tmp_path / "features"
    r = _run("-t", "features-calculator", "--wide-kmers", "-k", k, "-cm", w4 / "components.bin", "-ka", pos[0], "--selected", sel, "-w", w5)
    assert r.returncode == 0, r.stderr
    vec, br = FR.from_kmers(comps, cut["p1"], 0, kept)
    assert (w5 / "vectors" / "p1.vec").read_text() == FR.vec_text(vec) and (w5 / "vectors" / "p1.breadth").read_text() == FR.breadth_text(br)
    assert int(vec[0]) > 0
    # -c re-uses the finished steps; the pinned refusal holds
    r = _run("-t", "kmer-counter-posneg", *common, "--positiveReads", files["p1"], files["p2"], "--negativeReads", files["n1"], files["n2"], "-w", w1, "-c")
    assert r.returncode == 0 and "SUCCESS file found" in r.stdout + r.stderr + (w1 / "log").read_text()
    r = _run("-t", "unique-kmers-multi", *common, "-i", *pos, "--filter-kmers", *neg, "--min-samples", 1, "--max-samples", 2, "-w", w2, "-c")
    assert r.returncode == 0 and "SUCCESS file found" in r.stdout + r.stderr + (w2 / "log").read_text()
    r = _run("--wide-kmers", "-t", "kmers-samples-counter", "-k", k, "-i", pos[0], "-w", tmp_path / "no")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr
    r = _run("-t", "unique-kmers-multi", "-k", k, "-i", *pos, "--filter-kmers", *neg, "-w", tmp_path / "no2")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr
