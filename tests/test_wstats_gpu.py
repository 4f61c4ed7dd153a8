"""NO-REFERENCE EXTENSION: stats-kmers and the sample counter for k = 32 ... 63 (mf_wstats.hip on the wide join core mf_wjoin.hip and the row
kernels of mf_stats.hip) through the C-ABI and the driver, compared exactly with tests/wstats_ref.py (tests/stats_ref.py on ranked k-mers): the
three tables and the nine counters, for every number of slices; the bytes of the file form; the errors by message."""
import ctypes as C
import functools
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import stats_ref as SR
import wfeatures_ref as FR
import wide_files_ref as WF
import wkmersets_ref as WR
import wkps_ref as KR
import wstats_cases as CASES
import wstats_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metafast.sh")
B = CASES.MAX_BAD


def _write(tmp_path, samples, prefix):
    files = []
    for j, t in enumerate(samples):
        f = tmp_path / ("%s%d.kmers.bin" % (prefix, j))
        if not f.exists():
            f.write_bytes(WR.kmers_bin(t))
        files.append(str(f))
    return files


def _load(ctx, files, k):
    return [ctx.load_kmers_wide([f], k, 0) for f in files]


def _table(t):
    hi, lo, v = t.export()
    return [(int(h) << 64) | int(l) for h, l in zip(hi, lo)], v


def _same(got, want, where):
    """got: (chi, A, B WideTables, counters) of the library; want: the reference's dict"""
    chi, ga, gb, ctr = got
    assert ctr == want["counters"], (where, ctr, want["counters"])
    out = []
    for name, t in (("chi", chi), ("A", ga), ("B", gb)):
        keys, vals = _table(t)
        assert keys == want[name][0], (where, name)
        assert vals.dtype == np.uint16 and np.array_equal(vals, want[name][1]), (where, name)
        out.append((keys, vals))
        t.close()
    return out


@functools.lru_cache(maxsize=None)
def _crafted(k, empty):
    A, Bs, names = CASES.crafted(k, empty)
    want = {pm: R.stats_kmers(A, Bs, b=B, p_chi2=CASES.P_CHI2, p_mw=pm) for pm in (CASES.P_MW, 0.0)}
    return A, Bs, names, want


@functools.lru_cache(maxsize=None)
def _random(k, na, nb):
    A, Bs = CASES.random_cohort(k, na, nb)
    want = {(pc, pm): R.stats_kmers(A, Bs, b=B, p_chi2=pc, p_mw=pm) for pc, pm in CASES.RANDOM_PS}
    return A, Bs, want


@pytest.mark.parametrize("k", (32, 33, 63))
@pytest.mark.parametrize("empty", (None, "A", "B"))
def test_crafted_cohort(gpu_ctx, tmp_path, k, empty):
    A, Bs, _, want = _crafted(k, empty)
    ta, tb = _load(gpu_ctx, _write(tmp_path, A, "a"), k), _load(gpu_ctx, _write(tmp_path, Bs, "b"), k)
    first = {}
    try:
        for S in (1, 3, 7):
            gpu_ctx.set_option("stats_slices", S)
            for pm, w in want.items():
                got = _same(gpu_ctx.stats_kmers_wide(ta, tb, p_chi2=CASES.P_CHI2, p_mw=pm, max_bad=B), w, (k, empty, S, pm))
                for (k0, v0), (k1, v1) in zip(first.setdefault(pm, got), got):           # identical arrays for every number of slices
                    assert k0 == k1 and np.array_equal(v0, v1)
    finally:
        gpu_ctx.set_option("stats_slices", 0)
    if empty is None:
        assert want[CASES.P_MW]["counters"]["group_a"] > 0 and 0 in want[0.0]["A"][1].tolist()


@pytest.mark.parametrize("k", (32, 33, 63))
@pytest.mark.parametrize("shape", CASES.RANDOM_SHAPES)
def test_row_kernel_shapes(gpu_ctx, tmp_path, k, shape):
    """N = 2, 32 (the last thread-per-row shape), 33 (the first wave-per-row shape), 70 (a wave's lanes loop twice over the row); p_mw = 0 and
    > 0; p_chi2 = 0 leaves no survivor in any slice"""
    na, nb = shape
    A, Bs, want = _random(k, na, nb)
    base = min(5, na)
    fa, fb = _write(tmp_path, A[:base], "a"), _write(tmp_path, Bs[:min(5, nb)], "b")
    la, lb = _load(gpu_ctx, fa, k), _load(gpu_ctx, fb, k)
    ta, tb = [la[j % len(la)] for j in range(na)], [lb[j % len(lb)] for j in range(nb)]       # (the groups are filled up by repeating samples)
    first = {}
    try:
        for S in (1, 3, 7):
            gpu_ctx.set_option("stats_slices", S)
            for (pc, pm), w in want.items():
                got = _same(gpu_ctx.stats_kmers_wide(ta, tb, p_chi2=pc, p_mw=pm, max_bad=B), w, (k, shape, S, pc, pm))
                for (k0, v0), (k1, v1) in zip(first.setdefault((pc, pm), got), got):
                    assert k0 == k1 and np.array_equal(v0, v1)
    finally:
        gpu_ctx.set_option("stats_slices", 0)
    assert want[(0.0, 0.05)]["chi"][0] == []


def _records_of(path):
    hi, lo, v = WF.decode_kmers(open(path, "rb").read())
    return [(int(h) << 64) | int(l) for h, l in zip(hi, lo)], v.astype(np.uint16)


def test_file_form_and_view(gpu_ctx, tmp_path):
    k = 33
    A, Bs, names, want = _crafted(k, None)
    fa, fb = _write(tmp_path, A, "a"), _write(tmp_path, Bs, "b")
    for S, pm in ((1, CASES.P_MW), (3, 0.0), (7, 0.0)):
        out = tmp_path / ("out_%d" % S)
        out.mkdir()
        w = want[pm]
        try:
            gpu_ctx.set_option("stats_slices", S)
            ctr = gpu_ctx.stats_kmers_wide_files(fa, fb, k, str(out), p_chi2=CASES.P_CHI2, p_mw=pm, max_bad=B)
            chi, ga, gb, ctr_t = gpu_ctx.stats_kmers_wide(_load(gpu_ctx, fa, k), _load(gpu_ctx, fb, k), p_chi2=CASES.P_CHI2, p_mw=pm, max_bad=B)
        finally:
            gpu_ctx.set_option("stats_slices", 0)
        assert ctr == ctr_t == w["counters"]
        # the four files' bytes are the table form's export encoded as wide records
        for name, t in (("chisquared", chi), ("groupA", ga), ("groupB", gb)):
            keys, vals = _table(t)
            got = (out / ("filtered_%s.kmers.bin" % name)).read_bytes()
            assert got == R.records(keys, vals) and len(got) == 18 * len(keys), (S, name)
            t.close()
        assert (out / "filtered_groupA.kmers.bin").read_bytes() == R.records(*w["A"]) and (out / "filtered_groupB.kmers.bin").read_bytes() == R.records(*w["B"])
        assert (out / "filtered_chisquared.stat.txt").read_text() == SR.stat_txt(w["chi"][1])
    # a group file with a record of value 0 (the mean that truncates): the loader refuses it by design, view reads it on the host
    ga_file = tmp_path / "out_7" / "filtered_groupA.kmers.bin"
    keys, vals = _records_of(ga_file)
    assert vals[keys.index(names["mean_zero"])] == 0
    from metafast_amd import lib as L
    with pytest.raises(L.MetafastError, match=re.escape(os.path.basename(str(ga_file)))):
        gpu_ctx.load_kmers_wide([str(ga_file)], k, 0)
    r = subprocess.run([EXE, "-t", "view", "--wide-kmers", "-k", str(k), "-kf", str(ga_file), "-o", str(tmp_path / "view.txt"), "-w", str(tmp_path / "wview")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = (tmp_path / "view.txt").read_text().split("\n")
    assert lines[0] == "Kmer\tCount" and lines[-1] == ""
    assert lines[1:-1] == ["%s\t%d" % (KR.kmer_text(x, k), int(v) - (0x10000 if v >= 0x8000 else 0)) for x, v in zip(keys, vals)]


def test_fresh_tables_and_loaded_ones_agree(gpu_ctx, tmp_path):
    """tables fresh from the count (in the order of their counting units, maybe in several pieces) and the same tables loaded from their files"""
    k = 33
    rng = np.random.default_rng(77)
    genome = "".join(rng.choice(list("ACGT"), 900))
    spans = [(0, 520), (60, 600), (120, 560), (300, 900), (380, 860), (340, 800)]
    fresh, counted = [], []
    for j, (s, e) in enumerate(spans):
        fasta = tmp_path / ("r%d.fa" % j)
        fasta.write_text("".join(">r%d\n%s\n" % (i, genome[at:at + 90]) for i, at in enumerate(rng.integers(s, e - 90, 60 + 25 * j))))
        t = gpu_ctx.count_reads_wide([str(fasta)], k)
        fresh.append(t)
        counted.append(WR.from_words(*t.export()))
    assert all(len(t) > 300 for t in counted)
    want = R.stats_kmers(counted[:3], counted[3:], b=1, p_chi2=0.3, p_mw=0.0)
    assert want["counters"]["group_a"] > 20 and want["counters"]["group_b"] > 20
    a = _same(gpu_ctx.stats_kmers_wide(fresh[:3], fresh[3:], p_chi2=0.3, p_mw=0.0, max_bad=1), want, "fresh")
    loaded = _load(gpu_ctx, _write(tmp_path, counted, "c"), k)
    b = _same(gpu_ctx.stats_kmers_wide(loaded[:3], loaded[3:], p_chi2=0.3, p_mw=0.0, max_bad=1), want, "loaded")
    assert all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    # the sample counter takes them as they are, too
    keys, n = _table(gpu_ctx.kmers_samples_count_wide(fresh, max_bad=1))
    wk, wn = R.kmers_samples_count(counted, 1)
    assert keys == wk and np.array_equal(n, wn)


def _rc(call):
    from metafast_amd import lib as L
    rc = call(L.lib())
    return rc, L.lib().mf_last_error().decode(errors="replace")


def test_errors_leave_the_context_usable(gpu_ctx, tmp_path):
    import torch
    from metafast_amd import lib as L
    k = 33
    A, Bs, _, want = _crafted(k, None)
    fa, fb = _write(tmp_path, A, "a"), _write(tmp_path, Bs, "b")
    ta, tb = _load(gpu_ctx, fa, k), _load(gpu_ctx, fb, k)
    run = lambda a, b, **kw: gpu_ctx.stats_kmers_wide(a, b, **dict(dict(p_chi2=CASES.P_CHI2, p_mw=CASES.P_MW, max_bad=B), **kw))
    ok = lambda: _same(run(ta, tb), want[CASES.P_MW], "after an error")
    out = tmp_path / "never"
    out.mkdir()
    with pytest.raises(L.MetafastError, match=r"stats-kmers: both groups need at least one sample \(\|A\| = 0, \|B\| = 4\)"):
        run([], tb)
    ok()
    with pytest.raises(L.MetafastError, match=r"stats-kmers: both groups need at least one sample \(\|A\| = 4, \|B\| = 0\)"):
        gpu_ctx.stats_kmers_wide_files(fa, [], k, str(out))
    with pytest.raises(L.MetafastError, match=r"stats-kmers: 1025 samples, this build supports at most 1024"):
        run([ta[0]] * 1000, [tb[0]] * 25)
    ok()
    with pytest.raises(L.MetafastError, match=r"p-value-chi2 = 1.5 is not in \[0, 1\]"):
        run(ta, tb, p_chi2=1.5)
    with pytest.raises(L.MetafastError, match=r"stats-kmers: maximal-bad-frequence = -1 is negative"):
        run(ta, tb, max_bad=-1)
    ok()
    with pytest.raises(L.MetafastError, match=r"mf_stats_kmers_wide_tables: table 5 is NULL"):
        run(ta, [tb[0], None, tb[2]])
    chi, ga, gb = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ctr = np.zeros(9, np.uint64)
    rc, msg = _rc(lambda lib: lib.mf_stats_kmers_wide_tables(gpu_ctx.h, None, 2, None, 2, 0, 0.05, 0.05, C.byref(chi), C.byref(ga), C.byref(gb), ctr.ctypes.data))
    assert rc == -1 and "mf_stats_kmers_wide_tables: NULL argument" in msg and not (chi.value or ga.value or gb.value)
    other_k, = _load(gpu_ctx, _write(tmp_path, [CASES.crafted(35)[0][0]], "k35_"), 35)
    with pytest.raises(L.MetafastError, match=r"mf_stats_kmers_wide_tables: table 6 has k = 35, the others k = 33"):
        run(ta, [tb[0], tb[1], other_k])
    ok()
    ctx2 = L.Context(0, stream=torch.cuda.current_stream())
    try:
        foreign = ctx2.load_kmers_wide([fa[1]], k, 0)
        with pytest.raises(L.MetafastError, match=r"mf_stats_kmers_wide_tables: table 1 belongs to another context"):
            run([ta[0], foreign], tb)
        with pytest.raises(L.MetafastError, match=r"mf_kmers_samples_count_wide_tables: table 0 belongs to another context"):
            gpu_ctx.kmers_samples_count_wide([foreign, ta[0]])
        foreign.close()
    finally:
        ctx2.close()
    ok()
    for bad_k in (31, 64):
        with pytest.raises(L.MetafastError, match=r"mf_stats_kmers_wide: 32 <= k <= 63 \(k <= 31: mf_stats_kmers\)"):
            gpu_ctx.stats_kmers_wide_files(fa, fb, bad_k, str(out))
        with pytest.raises(L.MetafastError, match=r"mf_kmers_samples_count_wide: 32 <= k <= 63"):
            gpu_ctx.kmers_samples_count_wide_files(fa, bad_k, str(out / "n.kmers.bin"))
    # a file of another k: the loader refuses it by name, the tool's name in front
    f35 = str(tmp_path / "k35_0.kmers.bin")
    with pytest.raises(L.MetafastError, match=r"stats-kmers \(--wide-kmers\): .*k35_0\.kmers\.bin"):
        gpu_ctx.stats_kmers_wide_files(fa, [fb[0], f35], k, str(out))
    with pytest.raises(L.MetafastError, match=r"can't open '.*nowhere.kmers.bin'"):
        gpu_ctx.stats_kmers_wide_files(fa, [str(tmp_path / "nowhere.kmers.bin")], k, str(out))
    assert os.listdir(out) == []
    ok()


@pytest.mark.parametrize("k", (32, 33, 63))
def test_sample_counter(gpu_ctx, tmp_path, k):
    from metafast_amd import lib as L
    A, Bs, _, _ = _crafted(k, "B")
    samples = A + Bs
    files = _write(tmp_path, samples, "s")
    tabs = _load(gpu_ctx, files, k)
    want = {b: R.kmers_samples_count(samples, b) for b in (0, 1, B)}
    try:
        for S in (1, 3, 7):
            gpu_ctx.set_option("stats_slices", S)
            for b, (wk, wn) in want.items():
                keys, n = _table(gpu_ctx.kmers_samples_count_wide(tabs, max_bad=b))
                assert keys == wk and np.array_equal(n, wn), (k, S, b)
            out, st = tmp_path / ("n%d.kmers.bin" % S), tmp_path / ("n%d.stat.txt" % S)
            wk, wn = want[B]
            assert gpu_ctx.kmers_samples_count_wide_files(files, k, str(out), str(st), max_bad=B) == len(wk)
            assert out.read_bytes() == R.records(wk, wn) and st.read_text() == SR.stat_txt(wn)
    finally:
        gpu_ctx.set_option("stats_slices", 0)
    assert int(want[B][1].max()) == 8 and int(want[0][1].max()) == 8 and not np.array_equal(want[0][1], want[B][1])      # (max_bad shows)
    keys, n = _table(gpu_ctx.kmers_samples_count_wide([], max_bad=1))
    assert keys == [] and len(n) == 0
    with pytest.raises(L.MetafastError, match=r"kmers-samples-counter: 32768 input files, at most 32767"):
        gpu_ctx.kmers_samples_count_wide([tabs[0]] * 32768)
    with pytest.raises(L.MetafastError, match=r"kmers-samples-counter: 32768 input files, at most 32767"):
        gpu_ctx.kmers_samples_count_wide_files([files[0]] * 32768, k, str(tmp_path / "never.kmers.bin"))
    assert not (tmp_path / "never.kmers.bin").exists()


def test_cli(gpu_ctx, tmp_path):
    k, b = 33, 1
    rng = np.random.default_rng(33)
    genome = "".join(rng.choice(list("ACGT"), 800))
    spans = {"p1": (0, 420), "p2": (80, 500), "p3": (40, 460), "n1": (300, 700), "n2": (360, 640), "n3": (330, 800)}
    files = {}
    for name, (s, e) in spans.items():
        reads = []
        for i in range(300):
            at = int(rng.integers(s, e - 64))
            r = genome[at:at + 64]
            reads.append(FR.revcomp_str(r) if i % 3 == 0 else r)
        files[name] = tmp_path / (name + ".fa")
        files[name].write_text("".join(f">r{i}\n{r}\n" for i, r in enumerate(reads)))
    run = lambda *args: subprocess.run([EXE, *[str(a) for a in args], "--device", "0"], capture_output=True, text=True, timeout=300)
    w1 = tmp_path / "posneg"
    r = run("-t", "kmer-counter-posneg", "--wide-kmers", "-k", k, "-b", b, "--positiveReads", files["p1"], files["p2"], files["p3"], "--negativeReads",
            files["n1"], files["n2"], files["n3"], "-w", w1)
    assert r.returncode == 0, r.stderr
    pos, neg = sorted(glob.glob(str(w1 / "pos" / "kmers" / "*.kmers.bin"))), sorted(glob.glob(str(w1 / "neg" / "kmers" / "*.kmers.bin")))
    assert len(pos) == len(neg) == 3
    w2 = tmp_path / "stats"
    args = ["--wide-kmers", "-t", "stats-kmers", "-k", k, "-A", *pos, "-B", *neg, "-b", b, "--p-value-chi2", 0.3, "--p-value-mw", 0.0, "-w", w2]
    r = run(*args)
    assert r.returncode == 0, r.stderr
    lib_out = tmp_path / "lib"
    lib_out.mkdir()
    ctr = gpu_ctx.stats_kmers_wide_files(pos, neg, k, str(lib_out), p_chi2=0.3, p_mw=0.0, max_bad=b)
    assert ctr["group_a"] > 20 and ctr["group_b"] > 20
    for name in ("filtered_chisquared.kmers.bin", "filtered_chisquared.stat.txt", "filtered_groupA.kmers.bin", "filtered_groupB.kmers.bin"):
        assert (w2 / "kmers" / name).read_bytes() == (lib_out / name).read_bytes(), name
    samples = [WR.from_words(*WF.decode_kmers(open(f, "rb").read())) for f in pos + neg]
    want = R.stats_kmers(samples[:3], samples[3:], b=b, p_chi2=0.3, p_mw=0.0)
    assert ctr == want["counters"] and (lib_out / "filtered_groupA.kmers.bin").read_bytes() == R.records(*want["A"])
    log = (w2 / "log").read_text()
    for line in ("Loading k-mers occurrences...", "Survived after chi-squared test k-mers printed to: %s" % (w2 / "kmers" / "filtered_chisquared.kmers.bin"),
                 "Total group A k-mers = %d" % ctr["group_a"], "Total group B k-mers = %d" % ctr["group_b"]):
        assert line in log, line
    props = (w2 / "in.properties").read_text()
    assert (w2 / "SUCCESS").exists() and "wide-kmers = true" in props and "\nk = 33\n" in "\n" + props
    assert "filtered_groupA.kmers.bin" in (w2 / "out.properties").read_text()
    # -c finds the finished run, with and without the options repeated
    for more in (args, ["-t", "stats-kmers", "-w", w2]):
        r = run(*more, "-c")
        assert r.returncode == 0 and "SUCCESS file found" in r.stdout + r.stderr + (w2 / "log").read_text(), r.stderr


def test_narrow_tool_gives_what_it_gave(gpu_ctx, tmp_path):
    """the row kernels' launcher moved (mf_stats_rows_launch): mf_stats_kmers on a k = 21 cohort, both row kernels, against tests/stats_ref.py"""
    rng = np.random.default_rng(21)
    pool = np.unique(rng.integers(0, 1 << 42, 400).astype(np.uint64))
    base = []
    for j in range(10):
        lean = (np.arange(len(pool)) % 3 == (0 if j < 5 else 1))
        has = rng.random(len(pool)) < np.where(lean, 0.9, 0.2)
        cnt = np.where(lean, rng.integers(20, 3000, len(pool)), rng.integers(1, 30, len(pool)))
        base.append((pool[has], cnt[has].astype(np.int16)))
    files = []
    for j, (keys, cnt) in enumerate(base):
        f = tmp_path / ("n%d.kmers.bin" % j)
        f.write_bytes(SR.records_to_bytes(keys, cnt))
        files.append(str(f))
    for na in (5, 20):                                      # N = 10: a thread per row; N = 40: a wave per row
        a = [j % 5 for j in range(na)]
        bsel = [5 + j % 5 for j in range(na)]
        want = SR.stats_kmers([base[j] for j in a], [base[j] for j in bsel], b=1, p_chi2=0.05, p_mw=0.05)
        out = tmp_path / ("narrow%d" % na)
        out.mkdir()
        ctr = gpu_ctx.stats_kmers_files([files[j] for j in a], [files[j] for j in bsel], str(out), p_chi2=0.05, p_mw=0.05, max_bad=1)
        assert ctr == want["counters"] and min(ctr["group_a"], ctr["group_b"], ctr["mw_rejected"]) > 5, ctr
        assert (out / "filtered_chisquared.kmers.bin").read_bytes() == SR.records_to_bytes(*want["chi"])
        assert (out / "filtered_groupA.kmers.bin").read_bytes() == SR.records_to_bytes(*want["A"])
        assert (out / "filtered_groupB.kmers.bin").read_bytes() == SR.records_to_bytes(*want["B"])
