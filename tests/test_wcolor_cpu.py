"""The wide (k = 32 ... 63) kmers-color and component-colored without a GPU: the restatement (tests/wcolor_ref.py) tied to tests/color_ref.py at
k = 21 and 31 and pinned by hand-worked cases, the guards over every cohort and graph of tests/test_wcolor_gpu.py (no GPU test passes vacuously),
and the driver's two tools with --wide-kmers on the host-only stub build."""
import struct
import subprocess

import numpy as np
import pytest

import color_ref as CR
import wcolor_cases as CASES
import wcolor_ref as R
import wide_files_ref as WF
import wstats_cases as SC
from test_driver_tools_cpu import ENV, stub_driver


# ---- the restatement ----
def test_packed_add_and_colour_by_hand():
    v = R.add_value(0, 1, 7)
    assert v == 7 << 20 and R.field(v, 1) == 7 and R.field(v, 0) == R.field(v, 2) == 0
    v = R.add_value(R.pack(3, R.FIELD_MAX - 2, 9), 1, 5)                      # the clamp leaves the other fields alone
    assert v == R.pack(3, R.FIELD_MAX, 9) and R.add_value(v, 1, 32767) == v
    assert R.add_value(R.pack(0, 0, R.FIELD_MAX - 1), 2) == R.pack(0, 0, R.FIELD_MAX)
    # 33 x 32767 passes 2^20 - 1 = 1048575 at the 33rd add (32 x 32767 = 1048544)
    v = 0
    for _ in range(32):
        v = R.add_value(v, 1, 32767)
    assert R.field(v, 1) == 1048544 and R.field(R.add_value(v, 1, 32767), 1) == R.FIELD_MAX
    assert R.get_color(R.pack(9, 1, 0), 0.9) == 0 and R.get_color(R.pack(8, 1, 1), 0.9) == -1 and R.get_color(R.pack(1, 9, 0), 0.9) == 1
    assert R.get_color(R.pack(1, 1, 0), 0.5) == 0 and R.get_color(R.pack(0, 1, 1), 0.5) == 1 and R.get_color(R.pack(1, 1, 1), 0.5) == -1
    assert R.get_color(R.pack(0, 0, 4), 0.9) == 2 and R.get_color(0, 0.9) == -1 and R.get_color(0, 0.0) == -1      # 0 / 0 is NaN
    # 9 / 10 in double is 0.9 exactly as the literal is: the share is compared as a double, not as a fraction
    assert R.get_color(R.pack(9, 1, 0), 0.9) == 0 and R.get_color(R.pack(899999, 100001, 0), 0.9) == -1


def test_kmers_color_by_hand():
    X, Y, Z = (5 << 64) | 7, (5 << 64) | 8, 3
    s = [{X: 2, Y: 1}, {X: 5, Z: 2}, {X: 3, Y: 9}, {}]
    t = R.kmers_color(s, [0, 0, 2, 1], b=1)
    assert t == {X: R.pack(2, 0, 1), Z: R.pack(1, 0, 0), Y: R.pack(0, 0, 1)}
    t = R.kmers_color(s, [0, 0, 2, 1], b=1, val=True)
    assert t == {X: R.pack(7, 0, 3), Z: R.pack(2, 0, 0), Y: R.pack(0, 0, 9)}
    assert R.kmers_color(s, [0, 0, 2, 1], b=0)[Y] == R.pack(1, 0, 1)
    raw = R.table_bytes(t)
    assert raw == (struct.pack(">QQq", 0, 3, 2) + struct.pack(">QQq", 5, 7, 7 | (3 << 40)) + struct.pack(">QQq", 5, 8, 9 << 40)) and len(raw) == 72
    assert R.table_from_bytes(raw) == [(Z, 2), (X, 7 | (3 << 40)), (Y, 9 << 40)]
    assert R.stat_text({1: 5, 2: 5, 3: 4}) == "# k-mer frequency\tnumber of such k-mers\n4\t1\n5\t2\n\n"
    with pytest.raises(ValueError):
        R.table_from_bytes(raw + b"x")
    for bad in ([0, 0, 3, 1], [0, 0, -1, 1]):
        with pytest.raises(ValueError):
            R.kmers_color(s, bad)
    with pytest.raises(ValueError):
        R.kmers_color([{}] * 1025, [0] * 1025)
    assert R.kmers_color([{}] * 1024, [0] * 1024) == {}
    # the loader: a signed cut per record, then a saturating add
    hm = R.load_long([[(X, 40), (Y, 33), (Z, -1)], [(X, R.LONG_MAX - 10), (Y, 34)]], 33, 34)
    assert hm == {X: R.LONG_MAX, Y: 34}
    with pytest.raises(ValueError):
        R.load_long([[(1 << 68, 40)]], 0, 34)


def test_reverse_complement_and_neighbours_for_any_k():
    assert R.revcomp(R.encode("AAGC"), 4) == R.encode("GCTT") and R.decode(R.encode("GATTACA"), 7) == "GATTACA"
    rng = np.random.default_rng(1)
    for k in (5, 21, 31, 32, 33, 63):
        s = "".join(rng.choice(list("AGCT"), k))
        x = R.encode(s)
        assert R.decode(R.revcomp(x, k), k) == s.translate(str.maketrans("ACGT", "TGCA"))[::-1] and R.revcomp(R.revcomp(x, k), k) == x
        if k <= 31:
            assert R.revcomp(x, k) == CR.rc(x, k) and R.neighbours(R.canonical(x, k), k) == CR.neighbours(CR.canon(x, k), k)
        y = R.canonical(x, k)
        nb = R.neighbours(y, k)
        assert len(nb) == 8 and all(y in R.neighbours(z, k) for z in nb)               # adjacency is symmetric
        assert R.canonical(R.encode(s[1:] + "G"), k) in nb and R.canonical(R.encode("T" + s[:-1]), k) in nb


@pytest.mark.parametrize("k", (21, 31))
def test_tied_to_the_narrow_restatement(k):
    """the same inputs through tests/color_ref.py and through this restatement: the same tables and the same components"""
    rng = np.random.default_rng(100 + k)
    gs = CASES.genomes(k)
    samples = []
    for g in gs + gs[:2]:
        t = {x: int(rng.choice(CASES.COUNTS)) for contig in g for x in R.kmers_of(contig, k) if rng.random() < 0.9}
        samples.append(t)
    classes = [0, 1, 2, 1, 0]
    narrow = [(np.array(sorted(t), np.uint64), np.array([t[x] for x in sorted(t)], np.int64)) for t in samples]
    for b in (0, 2):
        for val in (False, True):
            keys, vals = CR.kmers_color(narrow, classes, b=b, val=val)
            mine = R.kmers_color(samples, classes, b=b, val=val)
            assert [int(x) for x in keys] == sorted(mine) and [int(v) for v in vals] == [mine[x] for x in sorted(mine)]
            assert R.stat_text(mine) == CR.stat_txt(vals)
            assert [(x, v) for x, v in zip(keys.tolist(), vals.tolist())] == [(x, v) for x, v in sorted(mine.items())]
    table = R.kmers_color(samples, classes, b=0)
    assert len(set(R.colors_of(table, 0.9).values())) == 4
    for separate in (False, True):
        for perc in (0.9, 0.5):
            want = CR.colored_components(table, k, 3, separate, perc)
            got = R.colored_components(table, k, 3, separate, perc)
            assert got == want and sum(len(c) for c in got) > 6
            assert R.components_stat(got) == CR.components_stat(want)
    assert R.kmers_of(gs[0][0], k) == CR.kmers_of(gs[0][0].replace("G", "g").replace("g", "G"), k)


def test_hand_worked_path():
    """0 0 N 1 1 N N 0 along a path: default mode keeps the neutral k-mers that hang on a coloured one, --separate cuts at them"""
    xs, table = CASES.path(33)
    assert len(set(xs)) == 8 and [R.get_color(table[x], 0.9) for x in xs] == list(CASES.PATH_COLOURS)
    for i, x in enumerate(xs):                              # a path: a k-mer touches its neighbours in the sequence and no other k-mer of it
        assert {j for j, y in enumerate(xs) if y in R.neighbours(x, 33)} == {j for j in (i - 1, i + 1) if 0 <= j < 8}
    pick = lambda *idx: sorted(xs[i] for i in idx)
    order = lambda comps: sorted(comps, key=lambda c: (-len(c), c[0]))
    assert R.colored_components(table, 33, 3, False, 0.9) == [order([pick(0, 1, 2), pick(5, 6, 7)]), [pick(2, 3, 4, 5, 6)], []]
    assert R.colored_components(table, 33, 3, True, 0.9) == [[pick(0, 1), pick(7)], [pick(3, 4)], []]
    assert R.colored_components(table, 33, 4, True, 0.9)[3] == []
    with pytest.raises(ValueError, match="has colour 1, but n_groups = 1"):
        R.colored_components(table, 33, 1, False, 0.9)
    comps = R.colored_components(table, 33, 3, True, 0.9)
    assert R.components_stat(comps) == R.STAT_HEADER + "1\t2\t2\t0\n2\t1\t1\t0\n3\t2\t2\t1\n"
    sizes, weights, hi, lo = R.components_words(comps[0])
    raw = WF.encode_components(sizes, weights, hi, lo)
    assert len(raw) == 4 + 2 * 12 + 3 * 16 and raw[:4] == struct.pack(">i", 2) and raw[4:16] == struct.pack(">iq", 2, 2)
    assert raw[16:32] == struct.pack(">QQ", pick(0, 1)[0] >> 64, pick(0, 1)[0] & R.MASK64)


def test_hand_worked_self_complement():
    xs, table = CASES.palindrome_path()
    assert len(set(xs)) == 7 and R.revcomp(xs[3], 32) == xs[3] and [R.get_color(table[x], 0.9) for x in xs] == list(CASES.PAL_COLOURS)
    # the palindrome's left and right extensions are the same eight k-mers taken twice: four distinct neighbours
    assert len(set(R.neighbours(xs[3], 32))) == 4 and xs[2] in R.neighbours(xs[3], 32) and xs[4] in R.neighbours(xs[3], 32)
    for i, x in enumerate(xs):
        assert {j for j, y in enumerate(xs) if y in R.neighbours(x, 32)} == {j for j in (i - 1, i + 1) if 0 <= j < 7}
    pick = lambda *idx: sorted(xs[i] for i in idx)
    assert R.colored_components(table, 32, 3, False, 0.9) == [[pick(0, 1, 2, 3)], [pick(3, 4, 5, 6)], []]
    assert R.colored_components(table, 32, 3, True, 0.9) == [[pick(0, 1, 2)], [pick(4, 5, 6)], []]


# ---- guards over what the GPU tests run ----
def _fields_and_colours(table):
    for c in range(3):
        assert sum(1 for v in table.values() if R.field(v, c)) > 5, c
    cols = list(R.colors_of(table, 0.9).values())
    assert all(cols.count(c) > 0 for c in (0, 1, 2, -1)), [cols.count(c) for c in (0, 1, 2, -1)]


@pytest.mark.parametrize("k", CASES.KS)
@pytest.mark.parametrize("n", (3, 40))
def test_random_cohorts_are_tests(k, n):
    samples, classes = CASES.random_cohort(k, n)
    assert len(samples) == len(classes) == n and set(classes) == {0, 1, 2}
    union = set().union(*samples)
    assert 200 < len(union) <= 300 and all(x == R.canonical(x, k) and x < 1 << (2 * k) for x in union)
    assert {1, 2, 3, 32767} <= {c for t in samples for c in t.values()}
    for S in (3, 7):
        assert {SC.slice_of(x, k, S) for x in union} == set(range(S))
    tables = {}
    for b in CASES.MAX_BADS:
        for val in (False, True):
            tables[b, val] = t = R.kmers_color(samples, classes, b=b, val=val)
            _fields_and_colours(t)
    assert tables[0, False] != tables[2, False] and tables[0, False] != tables[0, True] and len(tables[2, True]) < len(tables[0, True])
    assert all(R.field(v, c) <= n for v in tables[0, False].values() for c in range(3))


@pytest.mark.parametrize("k", CASES.KS)
def test_crafted_cohort_is_a_test(k):
    for b in CASES.MAX_BADS:
        samples, classes, nm = CASES.crafted(k, b)
        assert classes == [0, 0, 1, 1, 2, 2, 1] and samples[6] == {}
        union = set().union(*samples)
        assert all(x == R.canonical(x, k) and x < 1 << (2 * k) for x in union) and all(0 < c <= 32767 for t in samples for c in t.values())
        assert nm["smallest"] == 0 == min(union) and nm["largest"] == max(union)
        assert nm["lo_x"] >> 64 == nm["lo_y"] >> 64 and nm["hi_x"] ^ nm["hi_y"] == 1 << (64 if k > 32 else 63)
        for S in (3, 7):
            for s in range(1, S):
                below = [x for x in nm["borders"] if SC.slice_of(x, k, S) == s - 1]
                above = [x for x in nm["borders"] if SC.slice_of(x, k, S) == s]
                assert below and above and max(below) >> (2 * k - 24) == (min(above) >> (2 * k - 24)) - 1
            assert {SC.slice_of(x, k, S) for x in union} == set(range(S))
        t = R.kmers_color(samples, classes, b=b)
        _fields_and_colours(t)
        assert all(x in t for x in nm["borders"]) and 0 in t and nm["largest"] in t
        # exactly max_bad is no presence, max_bad + 1 is: one sample of each class holds it
        assert t[nm["at_max_bad"]] == R.pack(1, 1, 1) and (nm["only_low"] not in t)
        assert R.kmers_color(samples, classes, b=b, val=True)[nm["at_max_bad"]] == R.pack(b + 1, b + 1, b + 1)
        # a class with no sample: class 1 relabelled 0 leaves field 1 empty everywhere
        t01 = R.kmers_color(samples, [0 if c == 1 else c for c in classes], b=b)
        assert set(t01) == set(t) and all(R.field(v, 1) == 0 for v in t01.values()) and t01 != t


@pytest.mark.parametrize("k", (33, 63))
def test_graphs_are_tests(k):
    table = CASES.graph(k)
    assert 100 < len(table) < 600
    _fields_and_colours(table)
    for perc in (0.9, 0.5):
        d = R.colored_components(table, k, 3, False, perc)
        s = R.colored_components(table, k, 3, True, perc)
        assert d != s and all(len(d[c]) >= 2 and len(s[c]) >= 2 for c in range(3)), (perc, [len(x) for x in d], [len(x) for x in s])
        assert -1 in R.colors_of(table, perc).values()
        assert R.colored_components(table, k, 4, False, perc) == d + [[]]
        for g in (1, 2):
            with pytest.raises(ValueError):
                R.colored_components(table, k, g, False, perc)
            part = CASES.restrict(table, g, perc)
            assert 0 < len(part) < len(table) and len(R.colored_components(part, k, g, True, perc)[g - 1]) >= 2
    assert R.colored_components(table, k, 3, False, 0.9) != R.colored_components(table, k, 3, False, 0.5)
    # the pipeline's table (-val, counts above k): the file form's cut at value > k drops nothing
    assert all(v > k for v in CASES.graph(k, count=70).values())


# ---- the driver on the stub build ----
@pytest.fixture(scope="module")
def driver():
    return stub_driver()


def _run(driver, cwd, *args):
    return subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, env=ENV, timeout=120, cwd=str(cwd))


def test_driver_takes_wide_kmers_color(driver, tmp_path):
    for name in ("a.kmers.bin", "b.kmers.bin"):
        (tmp_path / name).write_bytes(b"")
    cls = tmp_path / "classes.txt"
    cls.write_text("a\t0\nb\t2\n")
    args = ["-t", "kmers-color", "-kf", "a.kmers.bin", "b.kmers.bin", "--class", "classes.txt"]
    r = _run(driver, tmp_path, "--wide-kmers", *args, "-k", 40, "-b", 2, "-val", "-w", "w1")
    out = r.stderr + r.stdout
    assert r.returncode == 1 and "this build of the library has no mf_kmers_color_wide" in out, out
    props = (tmp_path / "w1" / "in.properties").read_text()
    assert "wide-kmers = true" in props and "\nk = 40\n" in "\n" + props and "maximal-bad-frequency = 2" in props and "val = true" in props
    assert not (tmp_path / "w1" / "SUCCESS").exists()
    # the class file's errors come before the library, as for k <= 31
    for i, (text, want) in enumerate([("a\t0\nb\t3\n", "class 3"), ("a\t0\n", "'b'"), ("a\t0\nb\n", "line 2")]):
        cls.write_text(text)
        r = _run(driver, tmp_path, "--wide-kmers", *args, "-k", 40, "-w", "wb%d" % i)
        out = r.stderr + r.stdout
        assert r.returncode == 1 and want in out and "classes.txt" in out and "mf_kmers_color" not in out, (want, out)
    cls.write_text("a\t0\nb\t2\n")
    r = _run(driver, tmp_path, *args, "-k", 40, "-w", "w2")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr + r.stdout
    r = _run(driver, tmp_path, "--wide-kmers", *args, "-k", 64, "-w", "w3")
    assert r.returncode == 1 and "The size of k-mer must be no more than 63." in r.stderr + r.stdout
    outs = []
    for w, more in (("n0", []), ("n1", ["--wide-kmers"])):
        r = _run(driver, tmp_path, *more, *args, "-k", 21, "-w", w)
        out = r.stderr + r.stdout
        assert r.returncode == 1 and "this build of the library has no mf_kmers_color" in out and "mf_kmers_color_wide" not in out, out
        props = (tmp_path / w / "in.properties").read_text()
        assert "wide-kmers" not in props and "\nk = 21\n" in "\n" + props
        outs.append(props.replace("/" + w + "/", "/W/"))
    assert outs[0] == outs[1]


def test_driver_takes_wide_component_colored(driver, tmp_path):
    (tmp_path / "colored_kmers.kmers.bin").write_bytes(b"")
    args = ["-t", "component-colored", "-i", "colored_kmers.kmers.bin"]
    r = _run(driver, tmp_path, "--wide-kmers", *args, "-k", 40, "-group", 2, "--separate", "--perc", 0.75, "-w", "w1")
    out = r.stderr + r.stdout
    assert r.returncode == 1 and "this build of the library has no mf_colored_components_wide" in out, out
    props = (tmp_path / "w1" / "in.properties").read_text()
    assert "wide-kmers = true" in props and "\nk = 40\n" in "\n" + props and "n_groups = 2" in props and "separate = true" in props and "perc = 0.75" in props
    for i, (more, want) in enumerate(((["--linear"], "--linear"), (["--n_comps", 5], "--n_comps"))):
        r = _run(driver, tmp_path, "--wide-kmers", *args, "-k", 40, *more, "-w", "wr%d" % i)
        out = r.stderr + r.stdout
        assert r.returncode == 1 and want in out and "iteration order" in out and "mf_colored_components" not in out, out
    r = _run(driver, tmp_path, *args, "-k", 40, "-w", "w2")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr + r.stdout
    r = _run(driver, tmp_path, "--wide-kmers", *args, "-k", 64, "-w", "w3")
    assert r.returncode == 1 and "The size of k-mer must be no more than 63." in r.stderr + r.stdout
    outs = []
    for w, more in (("n0", []), ("n1", ["--wide-kmers"])):
        r = _run(driver, tmp_path, *more, *args, "-k", 21, "-w", w)
        out = r.stderr + r.stdout
        assert r.returncode == 1 and "this build of the library has no mf_colored_components" in out and "mf_colored_components_wide" not in out, out
        props = (tmp_path / w / "in.properties").read_text()
        assert "wide-kmers" not in props and "\nk = 21\n" in "\n" + props
        outs.append(props.replace("/" + w + "/", "/W/"))
    assert outs[0] == outs[1]
    # view --long stays refused under the flag
    r = _run(driver, tmp_path, "--wide-kmers", "-t", "view", "-k", 40, "-kf", "colored_kmers.kmers.bin", "--long", "-w", "w4")
    assert r.returncode == 1 and "long" in r.stderr + r.stdout
