"""NO-REFERENCE EXTENSION: kmers-color and component-colored for k = 32 ... 63 (mf_wcolor.hip on the wide join core mf_wjoin.hip; the wide front
end of mf_cc.hip's coloured passes in mf_wgraph.hip) through the C-ABI and the driver, compared exactly with tests/wcolor_ref.py: tables, files'
bytes and components for every number of slices; the errors by message.  tests/test_wcolor_cpu.py holds the guards over the inputs used here."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import wcolor_cases as CASES
import wcolor_ref as R
import wfeatures_ref as FR
import wide_files_ref as WF
import wkmersets_ref as WR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metafast.sh")
M64 = R.MASK64


def _write(tmp_path, samples, prefix="s"):
    files = []
    for j, t in enumerate(samples):
        f = tmp_path / ("%s%d.kmers.bin" % (prefix, j))
        if not f.exists():
            f.write_bytes(WR.kmers_bin(t))
        files.append(str(f))
    return files


def _load(ctx, samples, tmp_path, k, prefix="s"):
    """distinct samples are loaded once: a cohort that repeats samples repeats handles"""
    seen, out = {}, []
    for t in samples:
        if id(t) not in seen:
            seen[id(t)] = ctx.load_kmers_wide(_write(tmp_path, [t], "%s%d_" % (prefix, len(seen))), k, 0)
        out.append(seen[id(t)])
    return out


def _table(ct):
    hi, lo, v = ct.export()
    assert hi.dtype == lo.dtype == v.dtype == np.uint64
    return [((int(h) << 64) | int(l), int(x)) for h, l, x in zip(hi, lo, v)]


def _same(ct, want, where, k):
    got = _table(ct)
    assert got == sorted(want.items()), where
    assert ct.stats() == (len(want), k), where
    ct.close()
    return got


def _wct(ctx, table, k):
    keys = sorted(table)
    return ctx.wctable_from_host([x >> 64 for x in keys], [x & M64 for x in keys], [table[x] for x in keys], k)


def _comps(wc):
    e = wc.export()
    assert np.array_equal(e["sizes"].astype(np.int64), e["weights"])
    off = e["offsets"]
    return [[(int(h) << 64) | int(l) for h, l in zip(e["hi"][int(a):int(b)], e["lo"][int(a):int(b)])] for a, b in zip(off[:-1], off[1:])]


@functools.lru_cache(maxsize=None)
def _random(k, n):
    samples, classes = CASES.random_cohort(k, n)
    return samples, classes, {(b, val): R.kmers_color(samples, classes, b=b, val=val) for b in CASES.MAX_BADS for val in (False, True)}


@pytest.mark.parametrize("k", CASES.KS)
@pytest.mark.parametrize("n", (3, 40))
def test_random_cohorts(gpu_ctx, tmp_path, k, n):
    samples, classes, want = _random(k, n)
    tabs = _load(gpu_ctx, samples, tmp_path, k)
    first = {}
    try:
        for S in (1, 3, 7):
            gpu_ctx.set_option("stats_slices", S)
            for (b, val), w in want.items():
                got = _same(gpu_ctx.kmers_color_wide(tabs, classes, b=b, val=val), w, (k, n, S, b, val), k)
                assert first.setdefault((b, val), got) == got           # identical for every number of slices
    finally:
        gpu_ctx.set_option("stats_slices", 0)


@pytest.mark.parametrize("k", CASES.KS)
def test_file_form(gpu_ctx, tmp_path, k):
    samples, classes, want = _random(k, 3)
    files = _write(tmp_path, samples)
    try:
        for S, b, val in ((1, 0, False), (3, 2, True), (7, 0, True)):
            gpu_ctx.set_option("stats_slices", S)
            out, st = tmp_path / ("c%d.kmers.bin" % S), tmp_path / ("c%d.stat.txt" % S)
            w = want[b, val]
            assert gpu_ctx.kmers_color_wide_files(files, classes, k, str(out), str(st), b=b, val=val) == len(w)
            assert out.read_bytes() == R.table_bytes(w) and st.read_text() == R.stat_text(w), (k, S)
    finally:
        gpu_ctx.set_option("stats_slices", 0)


@pytest.mark.parametrize("k", CASES.KS)
@pytest.mark.parametrize("b", CASES.MAX_BADS)
def test_crafted_edges(gpu_ctx, tmp_path, k, b):
    """k = 32: the slice comes from the low word alone; the smallest and the largest canonical k-mer; keys on both sides of every slice border; an
    empty sample; counts of exactly max_bad and max_bad + 1; a class with no sample"""
    samples, classes, nm = CASES.crafted(k, b)
    tabs = _load(gpu_ctx, samples, tmp_path, k)
    no1 = [0 if c == 1 else c for c in classes]
    first = {}
    try:
        for S in (1, 3, 7):
            gpu_ctx.set_option("stats_slices", S)
            for val in (False, True):
                for name, cl in (("all", classes), ("no class 1", no1)):
                    got = _same(gpu_ctx.kmers_color_wide(tabs, cl, b=b, val=val), R.kmers_color(samples, cl, b=b, val=val), (k, b, S, val, name), k)
                    assert first.setdefault((val, name), got) == got
    finally:
        gpu_ctx.set_option("stats_slices", 0)
    t = dict(first[False, "all"])
    assert t[nm["at_max_bad"]] == R.pack(1, 1, 1) and nm["only_low"] not in t and 0 in t and nm["largest"] in t
    assert all(R.field(v, 1) == 0 for _, v in first[False, "no class 1"])
    # no sample at all, and samples that hold nothing above max_bad
    assert _table(gpu_ctx.kmers_color_wide([], [])) == [] and _table(gpu_ctx.kmers_color_wide(tabs[6:], [1])) == []
    assert _table(gpu_ctx.kmers_color_wide(tabs, classes, b=32767)) == []


def test_fresh_tables(gpu_ctx, tmp_path):
    """tables fresh from the count (in the order of their counting units, maybe in several pieces) are taken as they are"""
    k = 33
    rng = np.random.default_rng(78)
    genome = "".join(rng.choice(list("ACGT"), 700))
    fresh, counted = [], []
    for j, (s, e) in enumerate([(0, 400), (100, 520), (300, 700)]):
        fasta = tmp_path / ("r%d.fa" % j)
        fasta.write_text("".join(">r%d\n%s\n" % (i, genome[at:at + 90]) for i, at in enumerate(rng.integers(s, e - 90, 50 + 20 * j))))
        t = gpu_ctx.count_reads_wide([str(fasta)], k)
        fresh.append(t)
        counted.append(WR.from_words(*t.export()))
    for b, val in ((1, False), (0, True)):
        want = R.kmers_color(counted, [2, 0, 1], b=b, val=val)
        assert len(want) > 200
        _same(gpu_ctx.kmers_color_wide(fresh, [2, 0, 1], b=b, val=val), want, (b, val), k)


def test_saturation_and_sample_limit(gpu_ctx, tmp_path):
    from metafast_amd import lib as L
    k = 33
    x = R.canonical(R.encode("ACGTTGCAGGATCCATGACCGTTAGCAATGCCA"), k)
    one, = _load(gpu_ctx, [{x: 32767}], tmp_path, k)
    assert _table(gpu_ctx.kmers_color_wide([one] * 33, [1] * 33, b=0, val=True)) == [(x, R.pack(0, R.FIELD_MAX, 0))]
    assert _table(gpu_ctx.kmers_color_wide([one] * 32, [1] * 32, b=0, val=True)) == [(x, R.pack(0, 32 * 32767, 0))]
    assert _table(gpu_ctx.kmers_color_wide([one] * 33, [1] * 33, b=0)) == [(x, R.pack(0, 33, 0))]
    cl = [j % 3 for j in range(1024)]
    assert _table(gpu_ctx.kmers_color_wide([one] * 1024, cl, b=0)) == [(x, R.pack(342, 341, 341))]
    assert _table(gpu_ctx.kmers_color_wide([one] * 1024, cl, b=0, val=True)) == [(x, R.pack(R.FIELD_MAX, R.FIELD_MAX, R.FIELD_MAX))]
    with pytest.raises(L.MetafastError, match=r"kmers-color: 1025 samples, at most 1024"):
        gpu_ctx.kmers_color_wide([one] * 1025, [0] * 1025)
    f = _write(tmp_path, [{x: 32767}], "lim")
    with pytest.raises(L.MetafastError, match=r"kmers-color: 1025 samples, at most 1024"):
        gpu_ctx.kmers_color_wide_files(f * 1025, [0] * 1025, k, str(tmp_path / "never.kmers.bin"))
    assert not (tmp_path / "never.kmers.bin").exists()
    assert _table(gpu_ctx.kmers_color_wide([one], [2], b=0)) == [(x, R.pack(0, 0, 1))]


def test_errors_leave_the_context_usable(gpu_ctx, tmp_path):
    import torch
    from metafast_amd import lib as L
    k = 33
    samples, classes, want = _random(k, 3)
    files = _write(tmp_path, samples)
    tabs = _load(gpu_ctx, samples, tmp_path, k)
    ok = lambda: _same(gpu_ctx.kmers_color_wide(tabs, classes, b=0), want[0, False], "after an error", k)
    never = tmp_path / "never.kmers.bin"
    for bad, text in ((3, "class 3"), (-1, "class -1")):
        with pytest.raises(L.MetafastError, match=r"kmers-color: sample 1 has %s \(the classes are 0, 1 and 2\)" % text):
            gpu_ctx.kmers_color_wide(tabs, [0, bad, 2])
        with pytest.raises(L.MetafastError, match=r"kmers-color: sample 1 has %s" % text):
            gpu_ctx.kmers_color_wide_files(files, [0, bad, 2], k, str(never))
        ok()
    with pytest.raises(L.MetafastError, match=r"kmers-color: maximal-bad-frequency = -1 is negative"):
        gpu_ctx.kmers_color_wide(tabs, classes, b=-1)
    ok()
    with pytest.raises(L.MetafastError, match=r"mf_kmers_color_wide_tables: table 1 is NULL"):
        gpu_ctx.kmers_color_wide([tabs[0], None, tabs[2]], classes)
    other_k, = _load(gpu_ctx, [CASES.random_cohort(35, 3)[0][0]], tmp_path, 35, "k35_")
    with pytest.raises(L.MetafastError, match=r"mf_kmers_color_wide_tables: table 2 has k = 35, the others k = 33"):
        gpu_ctx.kmers_color_wide([tabs[0], tabs[1], other_k], classes)
    ok()
    ctx2 = L.Context(0, stream=torch.cuda.current_stream())
    try:
        foreign = ctx2.load_kmers_wide([files[1]], k, 0)
        with pytest.raises(L.MetafastError, match=r"mf_kmers_color_wide_tables: table 1 belongs to another context"):
            gpu_ctx.kmers_color_wide([tabs[0], foreign, tabs[2]], classes)
        foreign.close()
    finally:
        ctx2.close()
    ok()
    for bad_k in (31, 64):
        with pytest.raises(L.MetafastError, match=r"mf_kmers_color_wide: 32 <= k <= 63 \(k <= 31: mf_kmers_color\)"):
            gpu_ctx.kmers_color_wide_files(files, classes, bad_k, str(never))
        with pytest.raises(L.MetafastError, match=r"mf_colored_components_wide: 32 <= k <= 63 \(k <= 31: mf_colored_components\)"):
            gpu_ctx.colored_components_wide_files([str(never)], bad_k, str(tmp_path))
    with pytest.raises(L.MetafastError, match=r"kmers-color \(--wide-kmers\): .*k35_0_0\.kmers\.bin"):
        gpu_ctx.kmers_color_wide_files([files[0], str(tmp_path / "k35_0_0.kmers.bin")], [0, 1], k, str(never))
    with pytest.raises(L.MetafastError, match=r"can't open '.*nowhere.kmers.bin'"):
        gpu_ctx.kmers_color_wide_files([str(tmp_path / "nowhere.kmers.bin")], [0], k, str(never))
    assert not never.exists()
    ok()
    # a narrow handle given to the wide calls and the reverse: refused by name
    narrow = gpu_ctx.ctable_from_host([1, 2], [40, 50], 21)
    wide = _wct(gpu_ctx, want[0, False], k)
    with pytest.raises(L.MetafastError, match=r"mf_colored_components_wide_device: the handle is a narrow coloured table \(k = 21\): mf_colored_components_device"):
        gpu_ctx.colored_components_wide(narrow, k=k)
    with pytest.raises(L.MetafastError, match=r"mf_colored_components_device: the handle is a wide coloured table \(k = 33\): mf_colored_components_wide_device"):
        gpu_ctx.colored_components(wide, k=21)
    n, kk = L.C.c_uint64(), L.C.c_int()
    lib = L.lib()
    assert lib.mf_wctable_stats(narrow.h, L.C.byref(n), L.C.byref(kk)) == -1 and b"mf_wctable_stats: the handle is a narrow coloured table (k = 21): mf_ctable_stats" in lib.mf_last_error()
    assert lib.mf_ctable_stats(wide.h, L.C.byref(n), L.C.byref(kk)) == -1 and b"mf_ctable_stats: the handle is a wide coloured table (k = 33): mf_wctable_stats" in lib.mf_last_error()
    assert lib.mf_ctable_export(wide.h, None, None, 0, L.C.byref(n)) == -1 and b"mf_wctable_export" in lib.mf_last_error()
    assert lib.mf_wctable_write(narrow.h, str(never).encode(), None, None) == -1 and b"mf_ctable_write" in lib.mf_last_error() and not never.exists()
    assert narrow.export()[1].tolist() == [40, 50] and _table(wide) == sorted(want[0, False].items())
    ok()


def test_wctable(gpu_ctx, tmp_path):
    from metafast_amd import lib as L
    k = 33
    rng = np.random.default_rng(5)
    keys = CASES._fresh(rng, k, 40, set())
    table = {x: int(v) for x, v in zip(keys, rng.integers(0, 1 << 62, 40))}
    table[keys[0]] = 0                                       # (a value of 0 is kept in HBM and not written)
    table[keys[1]] = R.LONG_MAX
    order = rng.permutation(40)                              # any order in
    ct = gpu_ctx.wctable_from_host([keys[i] >> 64 for i in order], [keys[i] & M64 for i in order], [table[keys[i]] for i in order], k)
    assert _table(ct) == sorted(table.items()) and ct.k == k and len(ct) == 40
    out, st = tmp_path / "t.kmers.bin", tmp_path / "t.stat.txt"
    assert ct.write(str(out), str(st)) == 39
    assert out.read_bytes() == R.table_bytes(table) and len(out.read_bytes()) == 24 * 39 and st.read_text() == R.stat_text(table)
    recs = R.table_from_bytes(out.read_bytes())
    for mv in (-1, 0, 1 << 61):
        assert _table(gpu_ctx.wctable_load([str(out)], mv, k)) == sorted(R.load_long([recs], mv, k).items()), mv
    assert 0 < len(R.load_long([recs], 1 << 61, k)) < 39
    # a k-mer in two files: added, saturating at 2^63 - 1; a negative value is never kept
    a, b, c = keys[2], keys[3], keys[4]
    f1, f2 = [(a, 5), (b, R.LONG_MAX - 3), (c, -7)], [(b, 10), (a, 70), (c, 1)]
    p1, p2 = tmp_path / "f1.bin", tmp_path / "f2.bin"
    for p, f in ((p1, f1), (p2, f2)):
        p.write_bytes(b"".join(R.struct.pack(">QQq", x >> 64, x & M64, v) for x, v in f))
    assert _table(gpu_ctx.wctable_load([str(p1), str(p2)], 0, k)) == sorted({a: 75, b: R.LONG_MAX, c: 1}.items()) == sorted(R.load_long([f1, f2], 0, k).items())
    assert _table(gpu_ctx.wctable_load([str(p1), str(p2)], 5, k)) == sorted({a: 70, b: R.LONG_MAX}.items())
    assert _table(gpu_ctx.wctable_from_host([a >> 64] * 2, [a & M64] * 2, [R.LONG_MAX, 1], k)) == [(a, R.LONG_MAX)]
    assert _table(gpu_ctx.wctable_load([], 0, k)) == []
    bad = tmp_path / "odd.kmers.bin"
    bad.write_bytes(out.read_bytes()[:24] + b"x")
    with pytest.raises(L.MetafastError, match=r"odd\.kmers\.bin.*24-byte"):
        gpu_ctx.wctable_load([str(bad)], 0, k)
    wide = tmp_path / "wide.kmers.bin"
    wide.write_bytes(R.struct.pack(">QQq", 1 << 2, 5, 9))     # bit 66 of the k-mer: k = 33 has 66 bits
    with pytest.raises(L.MetafastError, match=r"wide\.kmers\.bin.*does not fit 33-mers"):
        gpu_ctx.wctable_load([str(wide)], 0, k)
    assert _table(gpu_ctx.wctable_load([str(wide)], 0, 34)) == [((1 << 66) | 5, 9)]
    with pytest.raises(L.MetafastError, match=r"mf_wctable_from_host: the k-mer of entry 0 does not fit 33-mers"):
        gpu_ctx.wctable_from_host([1 << 2], [5], [9], k)
    with pytest.raises(L.MetafastError, match=r"mf_wctable_from_host: value of entry 0 has the sign bit set"):
        gpu_ctx.wctable_from_host([0], [5], [1 << 63], k)
    for bad_k in (31, 64):
        with pytest.raises(L.MetafastError, match=r"mf_wctable_from_host: 32 <= k <= 63"):
            gpu_ctx.wctable_from_host([0], [5], [1], bad_k)
        with pytest.raises(L.MetafastError, match=r"mf_wctable_load: 32 <= k <= 63"):
            gpu_ctx.wctable_load([str(out)], 0, bad_k)


@functools.lru_cache(maxsize=None)
def _graph(k):
    return CASES.graph(k)


@pytest.mark.parametrize("k", (33, 63))
@pytest.mark.parametrize("separate", (False, True))
def test_colored_components(gpu_ctx, k, separate):
    from metafast_amd import lib as L
    table = _graph(k)
    ct = _wct(gpu_ctx, table, k)
    for perc in (0.9, 0.5):
        for g in (1, 2, 3, 4):
            part = table if g >= 3 else CASES.restrict(table, g, perc)
            cp = ct if g >= 3 else _wct(gpu_ctx, part, k)
            want = R.colored_components(part, k, g, separate, perc)
            got = [_comps(c) for c in gpu_ctx.colored_components_wide(cp, n_groups=g, separate=separate, perc=perc)]
            assert got == want, (k, separate, perc, g)
            if g < 3:
                bad = min(x for x, c in R.colors_of(table, perc).items() if c >= g)
                with pytest.raises(L.MetafastError, match=r"component-colored: k-mer %s has colour %d, but n_groups = %d \(colours 0 .. %d\)"
                                   % (R.decode(bad, k), R.get_color(table[bad], perc), g, g - 1)):
                    gpu_ctx.colored_components_wide(ct, n_groups=g, separate=separate, perc=perc)
    for g in (0, 65):
        with pytest.raises(L.MetafastError, match=r"component-colored: n_groups = %d \(1 .. 64\)" % g):
            gpu_ctx.colored_components_wide(ct, n_groups=g)
    with pytest.raises(L.MetafastError, match=r"mf_colored_components_wide_device: k = 40, the table has k = %d" % k):
        gpu_ctx.colored_components_wide(ct, k=40)
    assert [_comps(c) for c in gpu_ctx.colored_components_wide(_wct(gpu_ctx, {}, k))] == [[], [], []]


def test_hand_worked_graphs(gpu_ctx):
    xs, table = CASES.path(33)
    pick = lambda *idx: sorted(xs[i] for i in idx)
    order = lambda comps: sorted(comps, key=lambda c: (-len(c), c[0]))
    run = lambda t, k, sep: [_comps(c) for c in gpu_ctx.colored_components_wide(_wct(gpu_ctx, t, k), separate=sep)]
    assert run(table, 33, False) == [order([pick(0, 1, 2), pick(5, 6, 7)]), [pick(2, 3, 4, 5, 6)], []]
    assert run(table, 33, True) == [[pick(0, 1), pick(7)], [pick(3, 4)], []]
    xs, table = CASES.palindrome_path()
    pick = lambda *idx: sorted(xs[i] for i in idx)
    assert run(table, 32, False) == [[pick(0, 1, 2, 3)], [pick(3, 4, 5, 6)], []]
    assert run(table, 32, True) == [[pick(0, 1, 2)], [pick(4, 5, 6)], []]


def _components_bin(comps):
    return WF.encode_components(*R.components_words(comps))


def test_components_file_form(gpu_ctx, tmp_path):
    from metafast_amd import lib as L
    k = 33
    table = CASES.graph(k, count=70)
    src = tmp_path / "colored_kmers.kmers.bin"
    src.write_bytes(R.table_bytes(table))
    for separate in (False, True):
        out = tmp_path / ("out%d" % separate)
        out.mkdir()
        st = tmp_path / ("stat%d.txt" % separate)
        want = R.colored_components(R.load_long([R.table_from_bytes(src.read_bytes())], k, k), k, 3, separate, 0.9)
        assert gpu_ctx.colored_components_wide_files([str(src)], k, str(out), str(st), separate=separate) == [len(c) for c in want]
        for c in range(3):
            assert (out / ("components_color_%d.bin" % c)).read_bytes() == _components_bin(want[c]), (separate, c)
        assert st.read_text() == R.components_stat(want)
    # the value cut of the file form (the reference passes k): a table of counts of 1 loses every k-mer of class 0 alone
    low = tmp_path / "low.kmers.bin"
    low.write_bytes(R.table_bytes(CASES.graph(k)))
    kept = R.load_long([R.table_from_bytes(low.read_bytes())], k, k)
    assert 0 < len(kept) < len(table) and all(R.field(v, 1) or R.field(v, 2) for v in kept.values())
    out = tmp_path / "outlow"
    out.mkdir()
    want = R.colored_components(kept, k, 3, False, 0.9)
    assert gpu_ctx.colored_components_wide_files([str(low)], k, str(out)) == [len(c) for c in want]
    assert (out / "components_color_1.bin").read_bytes() == _components_bin(want[1])
    # a colour >= n_groups: the named error, and no file
    out = tmp_path / "outbad"
    out.mkdir()
    with pytest.raises(L.MetafastError, match=r"component-colored: k-mer [AGCT]{33} has colour \d, but n_groups = 2"):
        gpu_ctx.colored_components_wide_files([str(src)], k, str(out), str(tmp_path / "statbad.txt"), n_groups=2)
    assert os.listdir(out) == [] and not (tmp_path / "statbad.txt").exists()


def test_pipeline_through_the_driver(gpu_ctx, tmp_path):
    k = 33
    gs = CASES.genomes(k)
    names = ["g0", "g1", "g2", "h0"]
    samples = [{x: 70 + 3 * j for contig in g for x in R.kmers_of(contig, k)} for j, g in enumerate(gs)]
    samples.append({x: 40 for x in R.kmers_of(gs[0][0], k)[::2]})
    classes = [0, 1, 2, 0]
    files = []
    for n, t in zip(names, samples):
        f = tmp_path / (n + ".kmers.bin")
        f.write_bytes(WR.kmers_bin(t))
        files.append(f)
    cls = tmp_path / "classes.txt"
    cls.write_text("".join("%s\t%d\n" % (n, c) for n, c in zip(names, classes)))
    run = lambda *args: subprocess.run([EXE, *[str(a) for a in args], "--device", "0"], capture_output=True, text=True, timeout=300)
    w1 = tmp_path / "kc"
    args1 = ["--wide-kmers", "-t", "kmers-color", "-k", k, "-kf", *files, "--class", cls, "-b", 0, "-val", "-w", w1]
    r = run(*args1)
    assert r.returncode == 0, r.stderr
    table = R.kmers_color(samples, classes, b=0, val=True)
    colored = w1 / "colored-kmers" / "colored_kmers.kmers.bin"
    assert colored.read_bytes() == R.table_bytes(table) and (w1 / "colored-kmers" / "colored_kmers.stat.txt").read_text() == R.stat_text(table)
    log = (w1 / "log").read_text()
    for line in ("Loading class file...", "Loading kmers files...", "%d colored k-mers printed to %s" % (len(table), colored)):
        assert line in log, line
    props = (w1 / "in.properties").read_text()
    assert (w1 / "SUCCESS").exists() and "wide-kmers = true" in props and "\nk = 33\n" in "\n" + props and "val = true" in props
    r = run(*args1, "-c")
    assert r.returncode == 0 and "SUCCESS file found" in r.stdout + r.stderr + (w1 / "log").read_text(), r.stderr
    hm = R.load_long([R.table_from_bytes(colored.read_bytes())], k, k)
    assert len(hm) == len(table)
    for separate in (False, True):
        w2 = tmp_path / ("cc%d" % separate)
        r = run("--wide-kmers", "-t", "component-colored", "-k", k, "-i", colored, *(["--separate"] if separate else []), "-w", w2)
        assert r.returncode == 0, r.stderr
        want = R.colored_components(hm, k, 3, separate, 0.9)
        for c in range(3):
            assert (w2 / "colored-components" / ("components_color_%d.bin" % c)).read_bytes() == _components_bin(want[c]), (separate, c)
        assert (w2 / "components-stat.txt").read_text() == R.components_stat(want)
        log = (w2 / "log").read_text()
        for line in ["%d components were found for class %d" % (len(want[c]), c) for c in range(3)] + ["Total %d components were found" % sum(map(len, want))]:
            assert line in log, line
        props = (w2 / "in.properties").read_text()
        assert "wide-kmers = true" in props and ("separate = true" if separate else "separate = false") in props
        w3 = tmp_path / ("fc%d" % separate)
        cm = w2 / "colored-components" / "components_color_0.bin"
        r = run("--wide-kmers", "-t", "features-calculator", "-k", k, "-cm", cm, "-ka", files[3], files[1], "-w", w3)
        assert r.returncode == 0, r.stderr
        for n, t in ((names[3], samples[3]), (names[1], samples[1])):
            vec, br = FR.from_kmers(want[0], t)
            assert (w3 / "vectors" / (n + ".vec")).read_text() == FR.vec_text(vec) and (w3 / "vectors" / (n + ".breadth")).read_text() == FR.breadth_text(br)
        assert len(want[0]) >= 2 and FR.from_kmers(want[0], samples[3])[0].sum() > 0
