"""NO-REFERENCE EXTENSION: kmers-per-sample for k = 32 ... 63 (mf_wkps.hip on the wide join core mf_wjoin.hip) through the C-ABI and the driver,
compared exactly with the Python-integer reference of tests/wkps_ref.py: the arrays of the table form, the text of every row, the bytes of the
file form, for every number of slices."""
import os
import subprocess

import numpy as np
import pytest

import wkmersets_ref as WR
import wkps_cases as CASES
import wkps_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "metafast.sh")
WIDTHS = np.array([1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 32767])          # every digit width of the formatter
SCAN_ONE_BLOCK = 65536        # mf_scan (mf_common.h): up to here one block scans a row's widths, above it tiles of MF_SCAN_TILE = 4096 and an add-back


def _write(tmp_path, samples, prefix="s"):
    files = []
    for j, t in enumerate(samples):
        f = tmp_path / ("%s%d.kmers.bin" % (prefix, j))
        f.write_bytes(WR.kmers_bin(t))
        files.append(str(f))
    return files


def _load(ctx, files, k):
    return [ctx.load_kmers_wide([f], k, 0) for f in files]


def _keys(hi, lo):
    return [(int(h) << 64) | int(l) for h, l in zip(hi, lo)]


def _check_tables(ctx, tabs, samples, k, perc, count_first=False, max_bad=0, want=None):
    wk, wn, wm = want or R.select(samples, perc, count_first, max_bad)
    r = ctx.kmers_per_sample_wide(tabs, percent=perc, max_bad=max_bad, count_first=count_first)
    where = (k, perc, count_first, max_bad)
    assert r.shape() == (len(samples), len(wk)), where
    hi, lo, gn, gm = r.export()
    assert _keys(hi, lo) == wk and np.array_equal(gn, wn) and np.array_equal(gm, wm), where
    assert r.header_text(k) == R.header_text(wk, k), where
    for j in range(len(samples)):
        assert r.row_text(j) == R.row_text(wm[j]), (where, j)
    r.close()
    return wk, wn, wm


def _check_files(ctx, tmp_path, files, samples, k, perc, count_first=False, tag="o"):
    out = tmp_path / ("%s_%d_%d.txt" % (tag, perc, count_first))
    wk, want = R.file_text(samples, files, k, perc, count_first)
    assert ctx.kmers_per_sample_wide_files(files, k, str(out), percent=perc, count_first=count_first) == len(wk)
    got = out.read_bytes()
    assert len(got) == len(want) and got == want, (perc, count_first, got[:200], want[:200])
    return wk, got


@pytest.mark.parametrize("k", (32, 33, 47, 63))
def test_crafted_cohort(gpu_ctx, tmp_path, k):
    samples, _ = CASES.cohort(k)
    tabs = _load(gpu_ctx, _write(tmp_path, samples), k)
    want = {(p, cf, mb): R.select(samples, p, cf, mb) for p in (-50, 0, 20, 50, 100, 150) for cf in (False, True) for mb in (0, 1)}
    try:
        for S in (1, 3, 7):
            gpu_ctx.set_option("stats_slices", S)
            for (p, cf, mb), w in want.items():
                _check_tables(gpu_ctx, tabs, samples, k, p, cf, mb, want=w)
    finally:
        gpu_ctx.set_option("stats_slices", 0)


def _distinct_kmers(rng, k, n):
    mask = (1 << (2 * k)) - 1
    out = set()
    while len(out) < n:
        out.add(WR.canonical(int.from_bytes(rng.bytes(16), "big") & mask, k))
    keys = sorted(out)
    rng.shuffle(keys)
    return keys


@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, 257])
def test_small_column_counts(gpu_ctx, tmp_path, M):
    """perc 34 of 3 samples: thresh 1 -- exactly the M k-mers of samples 1 and 2 are columns, the 500 of sample 0 alone are not"""
    k = 33
    rng = np.random.default_rng(100 + M)
    keys = _distinct_kmers(rng, k, 500 + M)
    own, sel = keys[:500], keys[500:]
    cnt = lambda n: [int(c) for c in rng.choice(WIDTHS, size=n)]
    samples = [dict(zip(own + sel[: M // 2], cnt(500 + M // 2))), dict(zip(sel, cnt(M))), dict(zip(sel[M // 3:], cnt(M - M // 3)))]
    files = _write(tmp_path, samples)
    wk, got = _check_files(gpu_ctx, tmp_path, files, samples, k, 34)
    assert wk == sorted(sel)
    if M == 0:
        assert got == b"\ns0\ns1\ns2\n"                      # the empty selection: a lone newline, then the bare names
    _check_tables(gpu_ctx, _load(gpu_ctx, files, k), samples, k, 34)


@pytest.mark.parametrize("k", (33, 63))
def test_random_cohort(gpu_ctx, tmp_path, k):
    """the union of the cohort is wider than one block of the formatter's scan takes: the row text crosses its tiles"""
    rng = np.random.default_rng(1000 + k)
    mask = (1 << (2 * k)) - 1
    # (a pool of 40 000 gives a union of about 39 700: 80 000 is what 7 samples of 20 000 need to pass 65 536 with room)
    pool = sorted({WR.canonical(int.from_bytes(rng.bytes(16), "big") & mask, k) for _ in range(80000)})
    samples = []
    for j in range(7):
        pick = rng.choice(len(pool), 20000, replace=False)
        cnt = rng.choice(np.array([1, 2, 3, 5, 9000, 20000, 32767]), len(pick), p=[0.3, 0.25, 0.2, 0.1, 0.05, 0.05, 0.05])
        samples.append({pool[int(i)]: int(c) for i, c in zip(pick, cnt)})
    files = _write(tmp_path, samples)
    tabs = _load(gpu_ctx, files, k)
    want0, want50 = R.select(samples, 0), R.select(samples, 50)
    assert len(want0[0]) > SCAN_ONE_BLOCK and 0 < len(want50[0]) < len(want0[0]) and int(want50[1].min()) == 3
    blobs = []
    try:
        for S in (1, 7):
            gpu_ctx.set_option("stats_slices", S)
            _check_tables(gpu_ctx, tabs, samples, k, 0, want=want0)
            blobs.append(_check_files(gpu_ctx, tmp_path, files, samples, k, 0, tag="S%d" % S)[1])
            _check_tables(gpu_ctx, tabs, samples, k, 50, want=want50)
    finally:
        gpu_ctx.set_option("stats_slices", 0)
    assert blobs[0] == blobs[1]
    _check_files(gpu_ctx, tmp_path, files, samples, k, 50)


def test_sample_edge_cases(gpu_ctx, tmp_path):
    k = 33
    rng = np.random.default_rng(11)
    pool = _distinct_kmers(rng, k, 900)
    def sample(frac):
        return {x: int(rng.choice(WIDTHS)) for x in pool if rng.random() < frac}
    a, b, c = sample(0.6), sample(0.5), sample(0.4)
    fa, fb, fc, fe = _write(tmp_path, [a, b, c, {}])
    ta, tb, tc, te = _load(gpu_ctx, [fa, fb, fc, fe], k)
    # N = 1: thresh 0, every k-mer of the one sample, all with n = 0; counted, n = 1 and perc 100 still keeps them; not counted, thresh 1 keeps none
    wk, wn, _ = _check_tables(gpu_ctx, [ta], [a], k, 20)
    assert wk == sorted(a) and not wn.any()
    wk, wn, _ = _check_tables(gpu_ctx, [ta], [a], k, 100, count_first=True)
    assert wk == sorted(a) and (wn == 1).all()
    assert _check_tables(gpu_ctx, [ta], [a], k, 100)[0] == []
    _check_files(gpu_ctx, tmp_path, [fa], [a], k, 20, tag="n1")
    # N = 2
    for perc in (20, 50, 100):
        _check_tables(gpu_ctx, [ta, tb], [a, b], k, perc)
    _check_files(gpu_ctx, tmp_path, [fa, fb], [a, b], k, 50, tag="n2")
    # an empty sample first, last, and nothing but empty samples
    cohorts = (([te, ta, tb, tc], [fe, fa, fb, fc], [{}, a, b, c]), ([ta, tb, tc, te], [fa, fb, fc, fe], [a, b, c, {}]), ([te, te], [fe, fe], [{}, {}]))
    for i, (tabs, files, samples) in enumerate(cohorts):
        for perc, cf in ((20, False), (50, False), (50, True)):
            _check_tables(gpu_ctx, tabs, samples, k, perc, cf)
        _check_files(gpu_ctx, tmp_path, files, samples, k, 50, tag="e%d" % i)
    # a table fresh from the count: in the order of its counting units, maybe in pieces -- the same result as from its file (the writer orders
    # the table in place, so the fresh one goes first)
    genome = "".join(rng.choice(list("ACGT"), 1500))
    fasta = tmp_path / "r.fa"
    fasta.write_text("".join(">r%d\n%s\n" % (i, genome[at:at + 100]) for i, at in enumerate(rng.integers(0, 1400, 200))))
    fresh = gpu_ctx.count_reads_wide([str(fasta)], k)
    counted = WR.from_words(*fresh.export())
    assert len(counted) > 1000
    shared = dict(list(counted.items())[::3])
    fs, = _write(tmp_path, [shared], prefix="shared")
    ts, = _load(gpu_ctx, [fs], k)
    for perc in (0, 34, 67):
        _check_tables(gpu_ctx, [ta, fresh, ts], [a, counted, shared], k, perc)
        _check_tables(gpu_ctx, [fresh, ts, ta], [counted, shared, a], k, perc, max_bad=1)
    r = gpu_ctx.kmers_per_sample_wide([ta, fresh, ts], percent=34)
    before = [x.copy() for x in r.export()]
    r.close()
    ffresh = tmp_path / "fresh.kmers.bin"
    assert fresh.write_kmers(0, str(ffresh)) == len(counted)
    loaded, = _load(gpu_ctx, [str(ffresh)], k)
    r = gpu_ctx.kmers_per_sample_wide([ta, loaded, ts], percent=34)
    after = r.export()
    r.close()
    assert len(before[0]) > 300 and all(np.array_equal(x, y) for x, y in zip(before, after))


def _rc(call):
    """(the return code, the message) of a C-ABI call made past the wrappers"""
    from metafast_amd import lib as L
    rc = call(L.lib())
    return rc, L.lib().mf_last_error().decode(errors="replace")


def test_handle_and_argument_errors(gpu_ctx, tmp_path):
    import ctypes as C
    from metafast_amd import lib as L
    k = 33
    samples, _ = CASES.cohort(k)
    tabs = _load(gpu_ctx, _write(tmp_path, samples), k)
    wide = gpu_ctx.kmers_per_sample_wide(tabs, percent=20)
    n, m = wide.shape()
    assert m > 10
    buf = np.zeros(max(n * m, 16), np.uint64)
    p = C.c_void_p()
    # the one-word calls on a wide handle, the two-word calls on a narrow one: refused by name, nothing written
    rc, msg = _rc(lambda lib: lib.mf_kps_export(wide.h, buf.ctypes.data, None, None))
    assert rc == -1 and "mf_kps_export:" in msg and "mf_kps_export_wide" in msg and not buf.any()
    rc, msg = _rc(lambda lib: lib.mf_kps_device_view(wide.h, C.byref(p), None, None))
    assert rc == -1 and "mf_kps_device_view:" in msg and "mf_kps_device_view_wide" in msg and not p.value
    narrow = gpu_ctx.kmers_per_sample([gpu_ctx.table_from_host(np.array([5, 9], np.uint64), np.array([3, 4], np.uint16), 31)], percent=0)
    assert narrow.shape() == (1, 2)
    rc, msg = _rc(lambda lib: lib.mf_kps_export_wide(narrow.h, buf.ctypes.data, None, None, None))
    assert rc == -1 and "mf_kps_export_wide:" in msg and "call mf_kps_export" in msg and not buf.any()
    rc, msg = _rc(lambda lib: lib.mf_kps_device_view_wide(narrow.h, C.byref(p), None, None, None))
    assert rc == -1 and "mf_kps_device_view_wide:" in msg and "call mf_kps_device_view" in msg and not p.value
    assert narrow.header_text(31) == b"\t" + b"A" * 29 + b"GG" + b"\t" + b"A" * 29 + b"CG"           # (the narrow handle is what it was)
    narrow.close()
    # the calls that take both; any pointer of the wide ones may be NULL
    assert all(wide.device_view()) and len(wide.device_view()) == 4
    rc, msg = _rc(lambda lib: lib.mf_kps_export_wide(wide.h, None, None, None, None))
    assert rc == 0
    lo = np.zeros(m, np.uint64)
    assert _rc(lambda lib: lib.mf_kps_export_wide(wide.h, None, lo.ctypes.data, None, None))[0] == 0 and np.array_equal(lo, wide.export()[1])
    # the header of another k
    for other in (31, 32, 34, 63):
        with pytest.raises(L.MetafastError, match=r"mf_kps_header_text: k = %d, the result holds k-mers of k = 33" % other):
            wide.header_text(other)
    assert wide.header_text(33) == R.header_text(R.select(samples, 20)[0], 33)
    wide.close()
    # the arguments: checked on the host, before anything is launched
    with pytest.raises(L.MetafastError, match=r"mf_kmers_per_sample_wide_tables: kmers-per-sample needs at least one sample"):
        gpu_ctx.kmers_per_sample_wide([])
    with pytest.raises(L.MetafastError, match=r"mf_kmers_per_sample_wide: kmers-per-sample needs at least one sample"):
        gpu_ctx.kmers_per_sample_wide_files([], k, str(tmp_path / "never.txt"))
    with pytest.raises(L.MetafastError, match=r"mf_kmers_per_sample_wide_tables: .*at most 32767"):
        gpu_ctx.kmers_per_sample_wide([tabs[0]] * 32768)
    other_k, = _load(gpu_ctx, _write(tmp_path, [CASES.cohort(35)[0][1]], prefix="k35_"), 35)
    with pytest.raises(L.MetafastError, match=r"mf_kmers_per_sample_wide_tables: table 2 has k = 35, the others k = 33"):
        gpu_ctx.kmers_per_sample_wide([tabs[0], tabs[1], other_k])
    with pytest.raises(L.MetafastError, match=r"mf_kmers_per_sample_wide_tables: table 1 is NULL"):
        gpu_ctx.kmers_per_sample_wide([tabs[0], None, tabs[2]])
    r = C.c_void_p()
    rc, msg = _rc(lambda lib: lib.mf_kmers_per_sample_wide_tables(gpu_ctx.h, None, 3, 0, 20, 0, C.byref(r)))
    assert rc == -1 and "mf_kmers_per_sample_wide_tables: NULL argument" in msg and not r.value
    for bad_k in (31, 64):
        with pytest.raises(L.MetafastError, match=r"mf_kmers_per_sample_wide: 32 <= k <= 63"):
            gpu_ctx.kmers_per_sample_wide_files([str(tmp_path / "s0.kmers.bin")], bad_k, str(tmp_path / "never.txt"))
    # the matrix has to fit: the budget is an option of the context, so the limit is reached with numbers and no allocation
    try:
        gpu_ctx.set_option("kps_matrix_bytes", 6 * m * 2 - 1)
        with pytest.raises(L.MetafastError, match=r"kmers-per-sample: the count matrix of 6 samples x %d k-mers x 2 bytes does not fit .*-perc" % m):
            gpu_ctx.kmers_per_sample_wide(tabs, percent=20)
        gpu_ctx.set_option("kps_matrix_bytes", 6 * m * 2)
        gpu_ctx.kmers_per_sample_wide(tabs, percent=20).close()
    finally:
        gpu_ctx.set_option("kps_matrix_bytes", 0)
    assert not (tmp_path / "never.txt").exists()
    _check_tables(gpu_ctx, tabs, samples, k, 20)                               # the errors left nothing behind on the context


def test_cli(gpu_ctx, tmp_path):
    k = 40
    samples = CASES.cohort(k)[0][:3]
    files = []
    for name, t in zip("abc", samples):
        f = tmp_path / (name + ".kmers.bin")
        f.write_bytes(WR.kmers_bin(t))
        files.append(str(f))
    run = lambda *args: subprocess.run([EXE, *[str(a) for a in args], "--device", "0"], capture_output=True, text=True, timeout=300)
    w = tmp_path / "w"
    r = run("--wide-kmers", "-t", "kmers-per-sample", "-k", k, "-i", *files, "-perc", 40, "-w", w)
    assert r.returncode == 0, r.stderr
    wk, want = R.file_text(samples, files, k, 40)
    out = w / "kmers_per_samples" / "selected_kmers_40.txt"
    assert 0 < len(wk) < len(set().union(*samples)) and out.read_bytes() == want
    log = (w / "log").read_text()
    for line in ("Loading all k-mers...", "Starting to print k-mers to %s" % out, "Selected k-mers = %d" % len(wk), "K-mers printed to %s" % out):
        assert line in log, line
    assert (w / "SUCCESS").exists() and "percent-present = 40" in (w / "in.properties").read_text()
    # without the flag the reference's message; the tool next door keeps its refusal
    r = run("-t", "kmers-per-sample", "-k", k, "-i", *files, "-perc", 40, "-w", tmp_path / "no")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr
    r = run("--wide-kmers", "-t", "kmers-samples-counter", "-k", k, "-i", files[0], "-w", tmp_path / "no2")
    assert r.returncode == 1 and "The size of k-mer must be no more than 31." in r.stderr
