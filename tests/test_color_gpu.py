"""kmers-color (src/tools/ColorKmersMain.java:89-136) and component-colored (src/tools/ColoredComponentMain.java:83-119, default and
--separate modes) on the GPU, through the C-ABI, against the independent restatement tests/color_ref.py: records, stat files and
component sets byte-identical."""
import os
import re
import subprocess

import numpy as np
import pytest

import color_ref as CR
import stats_ref as R
from conftest import ROOT
from test_color_cpu import PATH_K, path_table

pytestmark = pytest.mark.gpu

EMPTY = (np.zeros(0, np.uint64), np.zeros(0, np.int16))
CSRC = os.path.join(ROOT, "metafast_amd", "csrc")


def _tab(ctx, sample, k=31):
    return ctx.table_from_host(np.asarray(sample[0], np.uint64), np.asarray(sample[1]).astype(np.uint16), k)


def _pool(n, seed):
    keys = np.unique(np.random.default_rng(seed).integers(1, 1 << 62, size=n + 64, dtype=np.uint64))[:n]
    keys[0] = 0
    return keys


def _sample(rng, pool, frac, lo, hi):
    m = rng.random(len(pool)) < frac
    return pool[m], rng.integers(lo, hi, size=int(m.sum())).astype(np.int16)


def _check_color(ctx, samples, classes, b, val, tabs, tmp_path):
    wk, wv = CR.kmers_color(samples, classes, b, val)
    ct = ctx.kmers_color(tabs, classes, b, val)
    gk, gv = ct.export()
    assert CR.ctable_to_bytes(gk, gv) == CR.ctable_to_bytes(wk, wv)
    out, st = str(tmp_path / "c.kmers.bin"), str(tmp_path / "c.stat.txt")
    assert ct.write(out, st) == len(wk)
    assert open(out, "rb").read() == CR.ctable_to_bytes(wk, wv) and open(st).read() == CR.stat_txt(wv)
    return wk, wv


@pytest.mark.parametrize("n", [5, 40])
def test_kmers_color_random_cohort(gpu_ctx, tmp_path, n):
    rng = np.random.default_rng(n)
    pool = _pool(3000, 21)
    samples = [_sample(rng, pool, rng.uniform(0.05, 0.6), 0, 6) for _ in range(n)]          # counts that straddle b = 0, 1, 3
    classes = [int(c) for c in rng.integers(0, 3, size=n)]
    classes[:3] = [0, 1, 2]
    tabs = [_tab(gpu_ctx, s) for s in samples]
    try:
        for slices in (1, 3):
            gpu_ctx.set_option("stats_slices", slices)
            for b in (0, 1, 3):
                for val in (False, True):
                    wk, wv = _check_color(gpu_ctx, samples, classes, b, val, tabs, tmp_path)
                    assert wk[0] == 0 and len(wk) > 1000 and len(np.unique(wv)) > 5
    finally:
        gpu_ctx.set_option("stats_slices", 0)


def test_kmers_color_saturation_and_edges(gpu_ctx, tmp_path):
    rng = np.random.default_rng(5)
    pool = _pool(3000, 22)
    full = (pool[:200], np.full(200, 32767, np.int16))
    t = _tab(gpu_ctx, full)
    # 1024 samples of one class at 32767: -val saturates its field at 2^20 - 1 (the sum is 2^25 - 1024); the count is 1024, the largest a
    # run can reach
    wk, wv = _check_color(gpu_ctx, [full] * 1024, [1] * 1024, 1, True, [t] * 1024, tmp_path)
    assert set(wv.tolist()) == {((1 << 20) - 1) << 20}
    wk, wv = _check_color(gpu_ctx, [full] * 1024, [1] * 1024, 1, False, [t] * 1024, tmp_path)
    assert set(wv.tolist()) == {1024 << 20}
    # saturation exactly at the boundary: 32 x 32767 < 2^20 - 1 <= 33 x 32767
    for m in (32, 33):
        _check_color(gpu_ctx, [full] * m, [2] * m, 0, True, [t] * m, tmp_path)
    with pytest.raises(Exception, match="1025 samples"):
        gpu_ctx.kmers_color([t] * 1025, [0] * 1025)
    # a class without a sample, an empty sample, nothing but empty samples, no sample at all
    s = [_sample(rng, pool, 0.4, 1, 9) for _ in range(4)]
    _check_color(gpu_ctx, s, [0, 2, 2, 0], 1, False, [_tab(gpu_ctx, x) for x in s], tmp_path)
    s2 = [s[0], EMPTY, s[1]]
    _check_color(gpu_ctx, s2, [0, 1, 2], 1, True, [_tab(gpu_ctx, x) for x in s2], tmp_path)
    wk, _ = _check_color(gpu_ctx, [EMPTY, EMPTY], [0, 1], 1, False, [_tab(gpu_ctx, EMPTY)] * 2, tmp_path)
    assert len(wk) == 0
    _check_color(gpu_ctx, [], [], 1, False, [], tmp_path)
    # errors that name the offender
    with pytest.raises(Exception, match="sample 1 has class 3"):
        gpu_ctx.kmers_color([t, t], [0, 3])
    with pytest.raises(Exception, match="class -1"):
        gpu_ctx.kmers_color([t], [-1])
    big = _tab(gpu_ctx, (np.array([5, 1 << 62], np.uint64), np.array([3, 3], np.int16)))
    with pytest.raises(Exception, match=r"2\^62"):
        gpu_ctx.kmers_color([t, big], [0, 1])


# ---- component-colored ----
def _genomes():
    rng = np.random.default_rng(77)
    shared = "".join(rng.choice(list("ACGT"), size=2000))
    return ["".join(rng.choice(list("ACGT"), size=4000)) + shared for _ in range(3)], shared


def _graph_files(k, tmp):
    """the k-mers of three genomes with a common stretch -> two files of 16-byte records (a few keys in both) and the same as arrays"""
    rng = np.random.default_rng(k)
    genomes, shared = _genomes()
    sets = [set(CR.kmers_of(g, k)) for g in genomes]
    lean = set(CR.kmers_of(shared[-(200 + k - 1):], k))          # the last 200 k-mers of the common stretch lean to colour 0
    table = {}
    for x in sorted(set().union(*sets)):
        owners = [g for g in range(3) if x in sets[g]]
        f = [0, 0, 0]
        if len(owners) == 3:                                     # the common stretch: mixed, its end leaning to one colour
            f = [60, 3, 2] if x in lean else [20, 20, 20]
        else:
            g = owners[0]
            r = rng.random()
            f[g] = int(rng.integers(35, 60))
            if r < 0.15:
                f[(g + 1) % 3] = f[g] - 10                       # 0.5 <= share < 0.9: neutral at 0.9, coloured at 0.5
            elif r < 0.20:
                f[(g + 1) % 3] = f[(g + 2) % 3] = f[g]           # a third each: neutral at both
            elif r < 0.27 and g == 0:
                f[g] = int(rng.integers(1, k + 1))               # value <= k: not loaded at min_value = k
        table[x] = CR.pack(*f)
    keys = np.array(sorted(table), dtype=np.uint64)
    vals = np.array([table[int(x)] for x in keys], dtype=np.int64)
    # two files; every 50th key in both, its value split between them (both parts above k: the cut is per record)
    in_b = rng.random(len(keys)) < 0.5
    dup = (np.arange(len(keys)) % 50 == 0) & (vals > 4 * k)
    ka, va = keys[~in_b | dup], vals[~in_b | dup].copy()
    kb, vb = keys[in_b | dup], vals[in_b | dup].copy()
    da, db = dup[~in_b | dup], dup[in_b | dup]
    va[da] = 2 * k
    vb[db] = vb[db] - 2 * k
    perm = rng.permutation(len(kb))
    files = []
    for name, kk, vv in (("a", ka, va), ("b", kb[perm], vb[perm])):
        p = os.path.join(tmp, "graph_k%d_%s.kmers.bin" % (k, name))
        open(p, "wb").write(CR.ctable_to_bytes(kk, vv.astype(np.uint64)))
        files.append(p)
    return files, [(ka, va), (kb, vb)], table


@pytest.fixture(scope="module")
def graphs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("graphs"))
    return {k: _graph_files(k, tmp) for k in (21, 31)}


def _comps_lists(comps):
    """Comps -> [ascending k-mer list], checking size and weight of each"""
    out = []
    for size, weight, _, kmers in comps.export():
        assert size == weight == len(kmers)
        out.append(kmers.tolist())
    return out


@pytest.mark.parametrize("k", [21, 31])
def test_colored_components_against_the_restatement(gpu_ctx, graphs, k):
    files, arrays, table = graphs[k]
    tile = int(re.search(r"#define CC_TILE (\d+)", open(os.path.join(CSRC, "mf_cc.hip")).read()).group(1))
    src = open(os.path.join(CSRC, "mf_table.hip")).read()
    part_min = int(re.search(r"n < (\d+) \|\| n >= 0xFFFFFFFFull\) return 1;", src).group(1))      # fewer entries: no minimizer partitions
    part_len = int(re.search(r"\(n >> bits\) > (\d+)", src).group(1))                              # mean partition length aimed at
    try:
        for min_value in (0, k):
            hm = CR.load_long(arrays, min_value)
            ct = gpu_ctx.load_ctable(files, min_value, k)
            gk, gv = ct.export()
            assert gk.tolist() == sorted(hm) and gv.tolist() == [hm[x] for x in sorted(hm)]
            assert min_value == 0 and hm == table or len(hm) < len(table)
            assert len(hm) > 2 * tile and len(hm) >= part_min and len(hm) > 2 * part_len
            for perc in (0.5, 0.9):
                for separate in (False, True):
                    want = CR.colored_components(hm, k, 3, separate, perc)
                    assert all(len(w) > 0 for w in want) and (not separate or sum(len(w) for w in want) > 100)
                    if not separate and perc == 0.9:
                        shared = set(want[0][0]) & set(want[1][0]) & set(want[2][0])
                        assert len(shared) > 500                  # the neutral common stretch sits in a component of every colour
                    for nbr_global in (-1, 1):
                        gpu_ctx.set_option("nbr_global", nbr_global)
                        got = gpu_ctx.colored_components(ct, 3, separate, perc)
                        for c in range(3):
                            assert _comps_lists(got[c]) == want[c], (min_value, perc, separate, nbr_global, c)
    finally:
        gpu_ctx.set_option("nbr_global", 0)


def test_hand_worked_path_and_n_groups(gpu_ctx):
    km, hm = path_table()
    keys = np.array(sorted(hm), np.uint64)
    ct = gpu_ctx.ctable_from_host(keys[::-1], np.array([hm[int(x)] for x in keys[::-1]], np.uint64), PATH_K)      # any order in
    assert ct.export()[0].tolist() == keys.tolist()
    d = [_comps_lists(c) for c in gpu_ctx.colored_components(ct, 3, False, 0.9)]
    assert d == [[sorted(km[3:6]), sorted(km[0:2])], [sorted(km[1:4])], []]
    s = [_comps_lists(c) for c in gpu_ctx.colored_components(ct, 3, True, 0.9)]
    assert s == [sorted([[km[0]], [km[4]]]), [[km[2]]], []]
    assert d == CR.colored_components(hm, PATH_K, 3, False, 0.9) and s == CR.colored_components(hm, PATH_K, 3, True, 0.9)
    # duplicates of a key are added
    two = gpu_ctx.ctable_from_host(np.array([9, 4, 9], np.uint64), np.array([5, 1, (1 << 63) - 3], np.uint64), PATH_K)
    assert two.export()[1].tolist() == [1, (1 << 63) - 1]
    # n_groups = 2 with a colour-2 k-mer: the error names it; without one: two lists
    with pytest.raises(Exception, match="colour 1, but n_groups = 1"):
        gpu_ctx.colored_components(ct, 1, False, 0.9)
    hm2 = dict(hm)
    hm2[km[5]] = CR.pack(0, 0, 7)
    ct2 = gpu_ctx.ctable_from_host(keys, np.array([hm2[int(x)] for x in keys], np.uint64), PATH_K)
    with pytest.raises(Exception, match="k-mer %d has colour 2, but n_groups = 2" % km[5]):
        gpu_ctx.colored_components(ct2, 2, False, 0.9)
    g2 = gpu_ctx.colored_components(ct, 2, False, 0.9)
    assert len(g2) == 2 and [_comps_lists(c) for c in g2] == d[:2]
    assert [_comps_lists(c) for c in gpu_ctx.colored_components(ct2, 3, True, 0.9)] == CR.colored_components(hm2, PATH_K, 3, True, 0.9)
    empty = gpu_ctx.ctable_from_host(np.zeros(0, np.uint64), np.zeros(0, np.uint64), PATH_K)
    assert [len(c) for c in gpu_ctx.colored_components(empty, 3, False, 0.9)] == [0, 0, 0]


def _cohort(tmp_path, k=21):
    """six samples, two per class, of the k-mers of three small genomes with a common stretch -> files, records, classes"""
    rng = np.random.default_rng(9)
    shared = "".join(rng.choice(list("ACGT"), size=150))
    genomes = ["".join(rng.choice(list("ACGT"), size=300)) + shared for _ in range(3)]
    files, samples, classes = [], [], []
    for g in range(3):
        km = np.array(CR.kmers_of(genomes[g], k), np.uint64)
        for rep in range(2):
            keep = rng.random(len(km)) < 0.9
            s = (km[keep], rng.integers(1, 40, size=int(keep.sum())).astype(np.int16))
            p = tmp_path / ("s%d_%d.kmers.bin" % (g, rep))
            p.write_bytes(R.records_to_bytes(*s))
            files.append(str(p)); samples.append(s); classes.append(g)
    return files, samples, classes


def _expected_outputs(samples, classes, k, b, val, separate, perc):
    wk, wv = CR.kmers_color(samples, classes, b, val)
    hm = CR.load_long([(wk, wv.astype(np.int64))], k)
    comps = CR.colored_components(hm, k, 3, separate, perc)
    return (wk, wv), comps


def test_file_round_trip_to_features(gpu_ctx, tmp_path):
    k = 21
    files, samples, classes = _cohort(tmp_path, k)
    out = tmp_path / "out"
    out.mkdir()
    ck, cs = str(out / "colored_kmers.kmers.bin"), str(out / "colored_kmers.stat.txt")
    (wk, wv), want = _expected_outputs(samples, classes, k, 1, True, False, 0.9)
    assert gpu_ctx.kmers_color_files(files, classes, k, ck, cs, b=1, val=True) == len(wk)
    assert open(ck, "rb").read() == CR.ctable_to_bytes(wk, wv) and open(cs).read() == CR.stat_txt(wv)
    counts = gpu_ctx.colored_components_files([ck], k, str(out), str(out / "components-stat.txt"))
    assert counts == [len(w) for w in want] and all(counts)
    for c in range(3):
        assert (out / ("components_color_%d.bin" % c)).read_bytes() == CR.components_bytes(want[c]), c
    assert (out / "components-stat.txt").read_text() == CR.components_stat(want)
    comps = gpu_ctx.load_components(str(out / "components_color_0.bin"))
    sample = _tab(gpu_ctx, samples[0], k)
    vec, _ = gpu_ctx.features(comps, sample, 0)
    sk, sc = CR.load_sample(samples[0], 0)
    look = dict(zip(sk.tolist(), sc.tolist()))
    assert vec.tolist() == [sum(look.get(x, 0) for x in comp) for comp in want[0]] and vec.sum() > 0


def test_cli_kmers_color_then_component_colored(gpu_ctx, tmp_path):
    k = 21
    files, samples, classes = _cohort(tmp_path, k)
    cls = tmp_path / "classes.txt"
    cls.write_text("".join("%s\t%d\n" % (os.path.basename(f)[:-len(".kmers.bin")], c) for f, c in zip(files, classes)))
    exe = os.path.join(ROOT, "metafast.sh")
    run = lambda *args: subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    w1, w2 = tmp_path / "w1", tmp_path / "w2"
    r = run("-t", "kmers-color", "-k", str(k), "-kf", *files, "--class", str(cls), "-b", "1", "-val", "-w", str(w1))
    assert r.returncode == 0, r.stderr
    (wk, wv), want = _expected_outputs(samples, classes, k, 1, True, True, 0.8)
    ck = w1 / "colored-kmers" / "colored_kmers.kmers.bin"
    assert ck.read_bytes() == CR.ctable_to_bytes(wk, wv)
    assert (w1 / "colored-kmers" / "colored_kmers.stat.txt").read_text() == CR.stat_txt(wv)
    assert "%d colored k-mers printed to %s" % (len(wk), ck) in r.stderr.replace("'", "") and (w1 / "SUCCESS").exists()
    r = run("-t", "component-colored", "-k", str(k), "-i", str(ck), "--separate", "--perc", "0.8", "-w", str(w2))
    assert r.returncode == 0, r.stderr
    # the same through the library
    lib_out = tmp_path / "lib"
    lib_out.mkdir()
    gpu_ctx.colored_components_files([str(ck)], k, str(lib_out), str(lib_out / "components-stat.txt"), separate=True, perc=0.8)
    for c in range(3):
        b = (w2 / "colored-components" / ("components_color_%d.bin" % c)).read_bytes()
        assert b == CR.components_bytes(want[c]) == (lib_out / ("components_color_%d.bin" % c)).read_bytes(), c
        assert "%d components were found for class %d" % (len(want[c]), c) in r.stderr
    assert (w2 / "components-stat.txt").read_text() == CR.components_stat(want) == (lib_out / "components-stat.txt").read_text()
    assert "Total %d components were found" % sum(len(w) for w in want) in r.stderr and (w2 / "SUCCESS").exists()
    assert "n_groups = 3" in (w2 / "in.properties").read_text()
    r = run("-ts")
    assert "kmers-color" in r.stdout and "component-colored" in r.stdout
