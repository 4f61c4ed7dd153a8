"""NO-REFERENCE EXTENSION: stats-kmers-3 and kmers-grouped-counter for k = 32 ... 63 (mf_wstats.hip on the wide join core's group word,
mf_wjoin.hip, and the three-group row kernels of mf_stats.hip) through the C-ABI and the driver, compared exactly with tests/wstats3_ref.py
(tests/stats3_ref.py on ranked k-mers): the four tables and the ten counters, for every number of slices; the grouped counter's arrays and text;
the bytes of the file forms; the errors by message."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import stats3_ref as S3
import stats_ref as SR
import wkmersets_ref as WR
import wstats3_cases as CASES
import wstats3_ref as R

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
    """got: (chi, A, B, C WideTables, counters) of the library; want: the reference's dict"""
    chi, ga, gb, gc, ctr = got
    assert ctr == want["counters"], (where, ctr, want["counters"])
    out = []
    for name, t in (("chi", chi), ("A", ga), ("B", gb), ("C", gc)):
        keys, vals = _table(t)
        assert keys == want[name][0], (where, name)
        assert vals.dtype == np.uint16 and np.array_equal(vals, want[name][1]), (where, name)
        out.append((keys, vals))
        t.close()
    return out


@functools.lru_cache(maxsize=None)
def _crafted(k, empty):
    A, Bs, Cs, names = CASES.crafted(k, empty)
    want = {pm: R.stats_kmers3(A, Bs, Cs, b=B, p_chi2=CASES.P_CHI2, p_mw=pm) for pm in (CASES.P_MW, 0.0)}
    return A, Bs, Cs, names, want


@functools.lru_cache(maxsize=None)
def _random(k, shape):
    A, Bs, Cs = CASES.random_cohort(k, *shape)
    want = {(pc, pm): R.stats_kmers3(A, Bs, Cs, b=B, p_chi2=pc, p_mw=pm) for pc, pm in CASES.RANDOM_PS}
    return A, Bs, Cs, want


def _every_slicing(gpu_ctx, tabs, want, where):
    """the library on (A, B, C tables) for S = 1, 3, 7 and every (p_chi2, p_mw) of want: the reference's result, in identical arrays for every S"""
    first = {}
    try:
        for S in (1, 3, 7):
            gpu_ctx.set_option("stats_slices", S)
            for (pc, pm), w in want.items():
                got = _same(gpu_ctx.stats_kmers3_wide(*tabs, p_chi2=pc, p_mw=pm, max_bad=B), w, (where, S, pc, pm))
                for (k0, v0), (k1, v1) in zip(first.setdefault((pc, pm), got), got):
                    assert k0 == k1 and np.array_equal(v0, v1)
    finally:
        gpu_ctx.set_option("stats_slices", 0)


@pytest.mark.parametrize("k", (32, 33, 63))
@pytest.mark.parametrize("empty", (None, "A", "B", "C"))
def test_crafted_cohort(gpu_ctx, tmp_path, k, empty):
    A, Bs, Cs, _, want = _crafted(k, empty)
    tabs = [_load(gpu_ctx, _write(tmp_path, g, p), k) for g, p in ((A, "a"), (Bs, "b"), (Cs, "c"))]
    _every_slicing(gpu_ctx, tabs, {(CASES.P_CHI2, pm): w for pm, w in want.items()}, (k, empty))
    if empty is None:
        c = want[CASES.P_MW]["counters"]
        assert min(c.values()) > 0 and 0 in want[0.0]["A"][1].tolist()


@pytest.mark.parametrize("k", (32, 33, 63))
@pytest.mark.parametrize("shape", CASES.RANDOM_SHAPES)
def test_row_kernel_shapes(gpu_ctx, tmp_path, k, shape):
    """N = 3, 32 (the last thread-per-row shape), 33 (the first wave-per-row shape), 70 (a wave's lanes loop twice over the row); p_mw = 0 and
    > 0; p_chi2 = 0 leaves no survivor in any slice"""
    A, Bs, Cs, want = _random(k, shape)
    tabs = []
    for g, p, n in ((A, "a", shape[0]), (Bs, "b", shape[1]), (Cs, "c", shape[2])):
        loaded = _load(gpu_ctx, _write(tmp_path, g[:min(5, n)], p), k)
        tabs.append([loaded[j % len(loaded)] for j in range(n)])                    # (the groups are filled up by repeating samples)
    _every_slicing(gpu_ctx, tabs, want, (k, shape))
    assert want[(0.0, 0.05)]["chi"][0] == []


def _grouped(k):
    kf, cd, uc, ni = CASES.grouped_case(k)
    return kf, cd, uc, ni, {b: R.kmers_grouped_count(kf, cd, uc, ni, b) for b in (0, 1)}


def _merged(samples):
    """the -kf files as the loader merges them: counts of equal k-mers added"""
    out = {}
    for t in samples:
        for x, c in t.items():
            out[x] = min(out.get(x, 0) + c, 32767)
    return out


def _counts_of(got):
    hi, lo, n = got
    assert hi.dtype == lo.dtype == np.uint64 and n.dtype == np.int64 and n.shape == (len(hi), 3)
    return [(int(h) << 64) | int(l) for h, l in zip(hi, lo)], n


@pytest.mark.parametrize("k", (32, 33, 63))
def test_grouped_counter(gpu_ctx, tmp_path, k):
    kf, cd, uc, ni, want = _grouped(k)
    f_kf, f_cd, f_uc, f_ni = (_write(tmp_path, g, p) for g, p in ((kf, "kf"), (cd, "cd"), (uc, "uc"), (ni, "ni")))
    t_kf = gpu_ctx.load_kmers_wide(f_kf, k, 0)
    t_cd, t_uc, t_ni = _load(gpu_ctx, f_cd, k), _load(gpu_ctx, f_uc, k), _load(gpu_ctx, f_ni, k)
    empty_kf = gpu_ctx.load_kmers_wide([], k, 0)
    try:
        for S in (1, 3, 7):
            gpu_ctx.set_option("stats_slices", S)
            for b, (wk, wn) in want.items():
                keys, n = _counts_of(gpu_ctx.kmers_grouped_count_wide(t_kf, t_cd, t_uc, t_ni, max_bad=b))
                assert keys == wk and np.array_equal(n, wn), (k, S, b)
                out = tmp_path / ("g_%d_%d.txt" % (S, b))
                assert gpu_ctx.kmers_grouped_count_wide_files(f_kf, f_cd, f_uc, f_ni, k, str(out), max_bad=b) == len(wk)
                assert out.read_bytes() == R.groups_txt(wk, wn, k).encode(), (k, S, b)
            # an empty group, and all three
            wk, wn = R.kmers_grouped_count(kf, cd, [], ni, 1)
            keys, n = _counts_of(gpu_ctx.kmers_grouped_count_wide(t_kf, t_cd, [], t_ni, max_bad=1))
            assert keys == wk and np.array_equal(n, wn) and not n[:, 1].any() and n[:, 0].any()
            keys, n = _counts_of(gpu_ctx.kmers_grouped_count_wide(t_kf, [], [], [], max_bad=1))
            assert keys == wk and not n.any()
            out = tmp_path / ("none_%d.txt" % S)
            assert gpu_ctx.kmers_grouped_count_wide_files(f_kf, [], [], [], k, str(out)) == len(wk)
            assert out.read_bytes() == R.groups_txt(wk, np.zeros((len(wk), 3), np.int64), k).encode()
            # an empty -kf: the header alone
            keys, n = _counts_of(gpu_ctx.kmers_grouped_count_wide(empty_kf, t_cd, t_uc, t_ni))
            assert keys == [] and n.shape == (0, 3)
            out = tmp_path / ("empty_%d.txt" % S)
            assert gpu_ctx.kmers_grouped_count_wide_files([], f_cd, f_uc, f_ni, k, str(out)) == 0
            assert out.read_text() == "Kmer\tcd_count\tuc_count\tnonibd_count\n"
    finally:
        gpu_ctx.set_option("stats_slices", 0)
    assert _merged(kf).keys() == set(want[1][0])


def test_grouped_counter_field_carry(gpu_ctx, tmp_path):
    """1022 samples in the first and in the last field of the word and one in the middle: exactly (1022, 1, 1022), no carry between the fields"""
    k = 33
    x, y = sorted(CASES.border_keys(k, 3))[1:3]            # (two canonical k-mers on either side of a slice border)
    f, = _write(tmp_path, [{x: 3, y: 1}], "tiny")
    t = gpu_ctx.load_kmers_wide([f], k, 0)
    try:
        for S in (1, 3):
            gpu_ctx.set_option("stats_slices", S)
            keys, n = _counts_of(gpu_ctx.kmers_grouped_count_wide(t, [t] * 1022, [t], [t] * 1022, max_bad=1))
            assert keys == [x, y] and n.tolist() == [[1022, 1, 1022], [0, 0, 0]]
            keys, n = _counts_of(gpu_ctx.kmers_grouped_count_wide(t, [t] * 1022, [t], [t] * 1022, max_bad=0))
            assert n.tolist() == [[1022, 1, 1022], [1022, 1, 1022]]
    finally:
        gpu_ctx.set_option("stats_slices", 0)


def test_file_form(gpu_ctx, tmp_path):
    k = 33
    A, Bs, Cs, names, want = _crafted(k, None)
    fa, fb, fc = _write(tmp_path, A, "a"), _write(tmp_path, Bs, "b"), _write(tmp_path, Cs, "c")
    for S, pm in ((1, CASES.P_MW), (3, 0.0), (7, 0.0)):
        out = tmp_path / ("out_%d" % S)
        out.mkdir()
        w = want[pm]
        try:
            gpu_ctx.set_option("stats_slices", S)
            ctr = gpu_ctx.stats_kmers3_wide_files(fa, fb, fc, k, str(out), p_chi2=CASES.P_CHI2, p_mw=pm, max_bad=B)
        finally:
            gpu_ctx.set_option("stats_slices", 0)
        assert ctr == w["counters"]
        for name, key in (("chisquared", "chi"), ("groupA", "A"), ("groupB", "B"), ("groupC", "C")):
            got = (out / ("filtered_%s.kmers.bin" % name)).read_bytes()
            assert got == R.records(*w[key]) and len(got) == 18 * len(w[key][0]), (S, name)
        assert (out / "filtered_chisquared.stat.txt").read_text() == SR.stat_txt(w["chi"][1])
        assert sorted(os.listdir(out)) == sorted(["filtered_chisquared.kmers.bin", "filtered_chisquared.stat.txt", "filtered_groupA.kmers.bin",
                                                  "filtered_groupB.kmers.bin", "filtered_groupC.kmers.bin"])
    # values are Java shorts: a record of value 0 is written (threshold -1)
    assert 0 in want[0.0]["A"][1].tolist() and names["mean_zero"] in want[0.0]["A"][0]


def test_cli_grouped_counter(gpu_ctx, tmp_path):
    k = 41
    kf, cd, uc, ni, want = _grouped(k)
    f_kf, f_cd, f_uc, f_ni = (_write(tmp_path, g, p) for g, p in ((kf, "kf"), (cd, "cd"), (uc, "uc"), (ni, "ni")))
    run = lambda *args: subprocess.run([EXE, *[str(a) for a in args], "--device", "0"], capture_output=True, text=True, timeout=300)
    w = tmp_path / "grouped"
    args = ["--wide-kmers", "-t", "kmers-grouped-counter", "-k", k, "-kf", *f_kf, "-cd", *f_cd, "-uc", *f_uc, "-nonibd", *f_ni, "-w", w]
    r = run(*args)
    assert r.returncode == 0, r.stderr
    out = w / "kmers" / "kmers.groups.txt"
    assert out.read_bytes() == R.groups_txt(*want[1], k).encode()
    assert "K-mers printed to %s" % out in (w / "log").read_text()
    props = (w / "in.properties").read_text()
    assert (w / "SUCCESS").exists() and "wide-kmers = true" in props and "\nk = 41\n" in "\n" + props and "maximal-bad-frequence = 1" in props
    r = run(*args, "-c")
    assert r.returncode == 0 and "SUCCESS file found" in r.stdout + r.stderr + (w / "log").read_text(), r.stderr


def _rc(call):
    from metafast_amd import lib as L
    rc = call(L.lib())
    return rc, L.lib().mf_last_error().decode(errors="replace")


def test_errors_leave_the_context_usable(gpu_ctx, tmp_path):
    from metafast_amd import lib as L
    k = 33
    A, Bs, Cs, _, want = _crafted(k, None)
    fa, fb, fc = _write(tmp_path, A, "a"), _write(tmp_path, Bs, "b"), _write(tmp_path, Cs, "c")
    ta, tb, tc = _load(gpu_ctx, fa, k), _load(gpu_ctx, fb, k), _load(gpu_ctx, fc, k)
    run = lambda a, b, c, **kw: gpu_ctx.stats_kmers3_wide(a, b, c, **dict(dict(p_chi2=CASES.P_CHI2, p_mw=CASES.P_MW, max_bad=B), **kw))
    ok = lambda: _same(run(ta, tb, tc), want[CASES.P_MW], "after an error")
    out = tmp_path / "never"
    out.mkdir()
    with pytest.raises(L.MetafastError, match=r"stats-kmers-3: every group needs at least one sample \(\|A\| = 3, \|B\| = 0, \|C\| = 3\)"):
        run(ta, [], tc)
    with pytest.raises(L.MetafastError, match=r"stats-kmers-3: every group needs at least one sample \(\|A\| = 3, \|B\| = 3, \|C\| = 0\)"):
        gpu_ctx.stats_kmers3_wide_files(fa, fb, [], k, str(out))
    ok()
    with pytest.raises(L.MetafastError, match=r"stats-kmers-3: 1025 samples, this build supports at most 1024"):
        run([ta[0]] * 1000, [tb[0]] * 24, [tc[0]])
    with pytest.raises(L.MetafastError, match=r"p-value-chi2 = 2 is not in \[0, 1\]"):
        run(ta, tb, tc, p_chi2=2.0)
    with pytest.raises(L.MetafastError, match=r"stats-kmers-3: maximal-bad-frequence = -1 is negative"):
        run(ta, tb, tc, max_bad=-1)
    ok()
    with pytest.raises(L.MetafastError, match=r"mf_stats_kmers3_wide_tables: table 7 is NULL"):
        run(ta, tb, [tc[0], None, tc[2]])
    chi, ga, gb, gc = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ctr = np.zeros(10, np.uint64)
    rc, msg = _rc(lambda lib: lib.mf_stats_kmers3_wide_tables(gpu_ctx.h, None, 2, None, 2, None, 2, 0, 0.05, 0.05, C.byref(chi), C.byref(ga), C.byref(gb),
                                                              C.byref(gc), ctr.ctypes.data))
    assert rc == -1 and "mf_stats_kmers3_wide_tables: NULL argument" in msg and not (chi.value or ga.value or gb.value or gc.value)
    other_k, = _load(gpu_ctx, _write(tmp_path, [CASES.crafted(35)[0][0]], "k35_"), 35)
    with pytest.raises(L.MetafastError, match=r"mf_stats_kmers3_wide_tables: table 5 has k = 35, the others k = 33"):
        run(ta, [tb[0], tb[1], other_k], tc)
    ok()
    for bad_k in (31, 64):
        with pytest.raises(L.MetafastError, match=r"mf_stats_kmers3_wide: 32 <= k <= 63 \(k <= 31: mf_stats_kmers3\)"):
            gpu_ctx.stats_kmers3_wide_files(fa, fb, fc, bad_k, str(out))
        with pytest.raises(L.MetafastError, match=r"mf_kmers_grouped_count_wide: 32 <= k <= 63 \(k <= 31: mf_kmers_grouped_count\)"):
            gpu_ctx.kmers_grouped_count_wide_files(fa, fa, fb, fc, bad_k, str(out / "g.txt"))
    # a file of another k: the loader refuses it by name, the tool's name in front
    f35 = str(tmp_path / "k35_0.kmers.bin")
    with pytest.raises(L.MetafastError, match=r"stats-kmers-3 \(--wide-kmers\): .*k35_0\.kmers\.bin"):
        gpu_ctx.stats_kmers3_wide_files(fa, [fb[0], f35], fc, k, str(out))
    with pytest.raises(L.MetafastError, match=r"kmers-grouped-counter \(--wide-kmers\): .*k35_0\.kmers\.bin"):
        gpu_ctx.kmers_grouped_count_wide_files(fa, fa, [f35], fc, k, str(out / "g.txt"))
    # the grouped counter: 1023 tables in a group, a NULL table, a table of another k, a negative max_bad
    with pytest.raises(L.MetafastError, match=r"kmers-grouped-counter: 0, 1023 and 1 files, at most 1022 in a group"):
        gpu_ctx.kmers_grouped_count_wide(ta[0], [], [tb[0]] * 1023, [tc[0]])
    with pytest.raises(L.MetafastError, match=r"mf_kmers_grouped_count_wide_tables: table 1 is NULL"):
        gpu_ctx.kmers_grouped_count_wide(ta[0], [ta[1], None], [], [])
    with pytest.raises(L.MetafastError, match=r"mf_kmers_grouped_count_wide_tables: NULL argument"):
        gpu_ctx.kmers_grouped_count_wide(None, [ta[1]], [], [])
    with pytest.raises(L.MetafastError, match=r"mf_kmers_grouped_count_wide_tables: table 0 has k = 35, the others k = 33"):
        gpu_ctx.kmers_grouped_count_wide(ta[0], [other_k], [], [])
    with pytest.raises(L.MetafastError, match=r"kmers-grouped-counter: maximal-bad-frequence = -1 is negative"):
        gpu_ctx.kmers_grouped_count_wide(ta[0], [ta[1]], [], [], max_bad=-1)
    assert os.listdir(out) == []
    ok()


def test_narrow_three_group_tool_gives_what_it_gave(gpu_ctx, tmp_path):
    """the three-group row kernels' launcher moved (mf_stats3_rows_launch): mf_stats_kmers3 on a k = 21 cohort, both row kernels, against
    tests/stats3_ref.py"""
    rng = np.random.default_rng(23)
    pool = np.unique(rng.integers(0, 1 << 42, 400).astype(np.uint64))
    base = []
    for j in range(9):
        lean = (np.arange(len(pool)) % 4 == j // 3)
        has = rng.random(len(pool)) < np.where(lean, 0.9, 0.2)
        cnt = np.where(lean, rng.integers(20, 3000, len(pool)), rng.integers(1, 30, len(pool)))
        base.append((pool[has], cnt[has].astype(np.int16)))
    files = []
    for j, (keys, cnt) in enumerate(base):
        f = tmp_path / ("n%d.kmers.bin" % j)
        f.write_bytes(SR.records_to_bytes(keys, cnt))
        files.append(str(f))
    for n in (3, 12):                                       # N = 9: a thread per row; N = 36: a wave per row
        sel = [[3 * g + j % 3 for j in range(n)] for g in range(3)]
        want = S3.stats_kmers3(*[[base[j] for j in s] for s in sel], b=1, p_chi2=0.05, p_mw=0.05)
        out = tmp_path / ("narrow%d" % n)
        out.mkdir()
        ctr = gpu_ctx.stats_kmers3_files(*[[files[j] for j in s] for s in sel], str(out), p_chi2=0.05, p_mw=0.05, max_bad=1)
        assert ctr == want["counters"] and ctr["group_a"] + ctr["group_b"] + ctr["group_c"] > 5, ctr
        assert (out / "filtered_chisquared.kmers.bin").read_bytes() == SR.records_to_bytes(*want["chi"])
        for g in "ABC":
            assert (out / ("filtered_group%s.kmers.bin" % g)).read_bytes() == SR.records_to_bytes(*want[g])
