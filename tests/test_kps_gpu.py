"""kmers-per-sample (src/tools/KmersPerSampleCounter.java:56-157) on the GPU (mf_kps.hip on the join core mf_join.hip), through the C-ABI
and the driver, against the independent restatement tests/kps_ref.py: the file's bytes and the arrays of the tables form."""
import os
import subprocess

import numpy as np
import pytest

import kps_ref as K
from conftest import ROOT

pytestmark = pytest.mark.gpu

WIDTHS = np.array([1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 32767])          # every digit width of the formatter


def _write(tmp_path, samples, prefix="s"):
    files = []
    for i, (k, c) in enumerate(samples):
        f = tmp_path / ("%s%d.kmers.bin" % (prefix, i))
        f.write_bytes(K.records_to_bytes(k, c))
        files.append(str(f))
    return files


def _tab(ctx, sample, k=31):
    keys, cnt = K.load_kmers(sample)                  # (a resident table holds a k-mer once)
    return ctx.table_from_host(keys, cnt.astype(np.uint16), k)


def _check_files(ctx, tmp_path, samples, k, perc, count_first=False, tag="o", files=None):
    files = files or _write(tmp_path, samples)
    out = tmp_path / ("%s_%d_%d.txt" % (tag, perc, count_first))
    wk, wn, wm, want = K.kmers_per_sample(samples, files, k, perc, count_first)
    assert ctx.kmers_per_sample_files(files, k, str(out), percent=perc, count_first=count_first) == len(wk)
    got = out.read_bytes()
    assert len(got) == len(want) and got == want, (perc, count_first, got[:200], want[:200])
    return wk, wn, wm, got


def _check_tables(ctx, samples, k, perc, count_first=False, max_bad=0, tabs=None, want=None):
    """want: (keys, n, matrix) of the restatement, where the caller has them already"""
    tabs = tabs or [_tab(ctx, s) for s in samples]
    wk, wn, wm = want or K.select(samples, perc, count_first, max_bad)
    r = ctx.kmers_per_sample(tabs, percent=perc, max_bad=max_bad, count_first=count_first)
    assert r.shape() == (len(samples), len(wk))
    gk, gn, gm = r.export()
    assert np.array_equal(gk, wk) and np.array_equal(gn, wn) and np.array_equal(gm, wm), (perc, count_first, max_bad)
    assert r.header_text(k) == K.header_text(wk, k).encode()
    for j in range(len(samples)):
        assert r.row_text(j) == K.row_text(wm[j]).encode(), j
    r.close()
    return wk, wn, wm


def _cohort(seed, k, n=6, records=3000):
    """n overlapping samples over one pool of k-mers of this k, key 0 and key 4^k - 1 among them; records drawn with replacement, so some
    k-mers are listed twice (at k = 5, where there are 1024 k-mers in all, most are); a few records with the values 0 and -3"""
    rng = np.random.default_rng(seed)
    space = 4 ** k
    pool = np.unique(np.concatenate([rng.integers(0, space, size=min(6000, space), dtype=np.uint64), np.array([0, space - 1], np.uint64)]))
    samples = []
    for j in range(n):
        sub = pool[rng.random(len(pool)) < (0.7, 0.45, 0.6)[j % 3]]
        keys = rng.choice(sub, size=records, replace=True)
        cnt = rng.choice(WIDTHS, size=records)
        cnt[:20] = (0, -3) * 10
        if j in (1, 2):
            keys[-2:] = (0, space - 1)
            cnt[-2:] = (9, 10000)
        samples.append((keys, cnt))
    return samples


@pytest.mark.parametrize("k", [5, 21, 31])
def test_random_cohorts(gpu_ctx, tmp_path, k):
    samples = _cohort(0x4B5053 + k, k)
    wk, wn, wm, _ = _check_files(gpu_ctx, tmp_path, samples, k, 20)
    assert wk[0] == 0 and wk[-1] == 4 ** k - 1 and wn.max() == 5 and {len(str(v)) for v in np.unique(wm)} == {1, 2, 3, 4, 5}
    _check_tables(gpu_ctx, samples, k, 20)
    _check_tables(gpu_ctx, samples, k, 50, max_bad=9)


@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, 257])
def test_small_column_counts(gpu_ctx, tmp_path, M):
    """perc 34 of 3 samples: thresh 1 -- exactly the M k-mers of samples 1 and 2 are columns, the 500 of sample 0 alone are not"""
    rng = np.random.default_rng(100 + M)
    keys = rng.choice(1 << 40, size=500 + M, replace=False).astype(np.uint64)
    own, sel = keys[:500], keys[500:]
    samples = [(np.concatenate([own, sel[: M // 2]]), rng.choice(WIDTHS, size=500 + M // 2)), (sel, rng.choice(WIDTHS, size=M)),
               (sel[M // 3:], rng.choice(WIDTHS, size=M - M // 3))]
    wk, _, _, got = _check_files(gpu_ctx, tmp_path, samples, 21, 34)
    assert len(wk) == M
    if M == 0:
        assert got == b"\ns0\ns1\ns2\n"                      # the empty selection: a lone newline, then the bare names
    _check_tables(gpu_ctx, samples, 21, 34)


def test_wide_row_crosses_the_scan_blocks(gpu_ctx, tmp_path):
    """about 70 000 columns of mixed widths: the formatter's scan runs tile by tile (above 65536 values) and adds the tiles' offsets back"""
    rng = np.random.default_rng(7)
    pool = np.unique(rng.integers(0, 1 << 62, size=70_500, dtype=np.uint64))
    samples = []
    for j in range(3):
        m = rng.random(len(pool)) < (0.95, 0.6, 0.3)[j]
        samples.append((pool[m], rng.choice(WIDTHS, size=int(m.sum()))))
    wk, wn, wm, got = _check_files(gpu_ctx, tmp_path, samples, 31, 0)
    assert 65536 < len(wk) < 70_500 and {len(str(v)) for v in np.unique(wm)} == {1, 2, 3, 4, 5}
    _check_tables(gpu_ctx, samples, 31, 0, want=(wk, wn, wm))


def test_sample_edge_cases(gpu_ctx, tmp_path):
    rng = np.random.default_rng(11)
    pool = rng.choice(1 << 50, size=900, replace=False).astype(np.uint64)
    def sample(frac):
        m = rng.random(len(pool)) < frac
        return pool[m], rng.choice(WIDTHS, size=int(m.sum()))
    empty = (np.zeros(0, np.uint64), np.zeros(0, np.int64))
    a, b, c = sample(0.6), sample(0.5), sample(0.4)
    # N = 1: thresh 0, every k-mer of the one file, all with n = 0; counted, n = 1 and perc 100 still keeps them
    wk, wn, _ = _check_tables(gpu_ctx, [a], 31, 20)
    assert len(wk) == len(np.unique(a[0])) and not wn.any()
    wk, wn, _ = _check_tables(gpu_ctx, [a], 31, 100, count_first=True)
    assert len(wk) == len(np.unique(a[0])) and (wn == 1).all()
    assert len(_check_tables(gpu_ctx, [a], 31, 100)[0]) == 0                     # thresh 1, n = 0
    _check_files(gpu_ctx, tmp_path, [a], 31, 20, tag="n1")
    # N = 2
    for perc in (20, 50, 100):
        _check_tables(gpu_ctx, [a, b], 31, perc)
    _check_files(gpu_ctx, tmp_path, [a, b], 31, 50, tag="n2")
    # an empty sample first, in the middle, last
    for i, cohort in enumerate(([empty, a, b, c], [a, empty, b, c], [a, b, c, empty], [empty, empty])):
        for perc, cf in ((20, False), (50, False), (50, True)):
            _check_tables(gpu_ctx, cohort, 31, perc, cf)
        _check_files(gpu_ctx, tmp_path, cohort, 31, 50, tag="e%d" % i)


def test_percent_values_and_count_first(gpu_ctx, tmp_path):
    samples = _cohort(0x50455243, 5, n=6, records=800)               # (k = 5: few k-mers, so some are in every sample and some in one)
    tabs = [_tab(gpu_ctx, s) for s in samples]
    files = _write(tmp_path, samples)
    sizes = {}
    for perc in (0, 20, 50, 100, 101, -5):
        for cf in (False, True):
            sizes[perc, cf] = len(_check_tables(gpu_ctx, samples, 5, perc, cf, tabs=tabs)[0])
            _check_files(gpu_ctx, tmp_path, samples, 5, perc, cf, files=files)
    assert sizes[0, False] == sizes[-5, False] == sizes[0, True] > sizes[20, False] > sizes[50, False] > sizes[100, False] == 0
    # (6 files: thresh 6 at perc 100 and at perc 101 -- out of reach of the 5 files the reference counts, reached by a k-mer of all 6)
    assert sizes[20, True] > sizes[20, False] and sizes[101, True] == sizes[100, True] > 0 and sizes[101, False] == 0


def test_slices_give_identical_files(gpu_ctx, tmp_path):
    samples = _cohort(0x534C, 31, n=5, records=2000)
    files = _write(tmp_path, samples)
    blobs = []
    try:
        for S in (1, 3, 7):
            gpu_ctx.set_option("stats_slices", S)
            blobs.append(_check_files(gpu_ctx, tmp_path, samples, 31, 20, tag="S%d" % S, files=files)[3])
            _check_tables(gpu_ctx, samples, 31, 50, True)
    finally:
        gpu_ctx.set_option("stats_slices", 0)
    assert blobs[0] == blobs[1] == blobs[2] and len(blobs[0]) > 10000


def test_tables_form_matches_the_file_and_its_limits(gpu_ctx, tmp_path):
    samples = _cohort(0x544142, 21, n=4, records=1500)
    files = _write(tmp_path, samples)
    out = tmp_path / "t.txt"
    m = gpu_ctx.kmers_per_sample_files(files, 21, str(out), percent=50)
    tabs = [gpu_ctx.load_kmers([f], 0, 21) for f in files]
    r = gpu_ctx.kmers_per_sample(tabs, percent=50)
    keys, ns, mat = r.export()
    lines = out.read_text().split("\n")
    assert lines[0].split("\t")[1:] == [K.kmer_text(x, 21) for x in keys] and len(keys) == m > 100
    for j in range(4):
        cells = lines[1 + j].split("\t")
        assert cells[0] == "s%d" % j and [int(x) for x in cells[1:]] == mat[j].tolist()
    dk, dn, dm = r.device_view()
    assert dk and dn and dm
    # the N x M matrix has to fit: the budget is an option of the context, so the limit is reached with numbers and no allocation
    try:
        gpu_ctx.set_option("kps_matrix_bytes", 4 * m * 2 - 1)
        with pytest.raises(Exception, match=r"4 samples x %d k-mers x 2 bytes does not fit .*-perc" % m):
            gpu_ctx.kmers_per_sample(tabs, percent=50)
        gpu_ctx.set_option("kps_matrix_bytes", 4 * m * 2)
        gpu_ctx.kmers_per_sample(tabs, percent=50).close()
    finally:
        gpu_ctx.set_option("kps_matrix_bytes", 0)
    # more than 32767 samples (n(x) is a Java short), no sample at all, a key >= 2^62
    with pytest.raises(Exception, match="at most 32767"):
        gpu_ctx.kmers_per_sample([tabs[0]] * 32768)
    with pytest.raises(Exception, match="at most 32767"):
        gpu_ctx.kmers_per_sample_files([files[0]] * 32768, 21, str(tmp_path / "never.txt"))
    with pytest.raises(Exception, match="no input files"):
        gpu_ctx.kmers_per_sample([])
    big = gpu_ctx.table_from_host(np.array([5, 1 << 62], np.uint64), np.array([3, 3], np.uint16), 31)
    for cohort in ([big, tabs[0]], [tabs[0], big]):
        with pytest.raises(Exception, match=r"2\^62"):
            gpu_ctx.kmers_per_sample(cohort)
    with pytest.raises(Exception, match=r"k must be in \[1,31\]"):
        gpu_ctx.kmers_per_sample_files(files, 32, str(tmp_path / "never.txt"))
    g2, n2, m2 = gpu_ctx.kmers_per_sample(tabs, percent=50).export()              # the errors left nothing behind on the context
    assert np.array_equal(g2, keys) and np.array_equal(n2, ns) and np.array_equal(m2, mat)
    r.close()


def test_cli_round_trip(gpu_ctx, ref_files, tmp_path):
    exe = os.path.join(ROOT, "metafast.sh")
    wd = tmp_path / "w"
    r = subprocess.run([exe, "-t", "kmer-counter-many", "-k", "31", "-i", *ref_files[:3], "-w", str(wd)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    f = sorted(str(p) for p in (wd / "kmers").iterdir())
    assert len(f) == 3
    samples = []
    for p in f:
        a = np.frombuffer(open(p, "rb").read(), dtype=np.dtype([("k", ">u8"), ("c", ">i2")]))
        samples.append((a["k"].astype(np.uint64), a["c"].astype(np.int64)))
    for perc in (20, 100):
        wk, _, _, want = K.kmers_per_sample(samples, f, 31, perc)
        wp = tmp_path / ("wp%d" % perc)
        cmd = [exe, "-t", "kmers-per-sample", "-k", "31", "-i", *f, "-perc", str(perc), "-w", str(wp)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert (wp / "kmers_per_samples" / ("selected_kmers_%d.txt" % perc)).read_bytes() == want
        assert (wp / "SUCCESS").exists() and "percent-present = %d" % perc in (wp / "in.properties").read_text()
        r = subprocess.run(cmd + ["-c"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "SUCCESS file found" in r.stderr, r.stderr
        # 3 files: thresh 0 at perc 20 (the whole union), 3 at perc 100 (no k-mer is in 3 of the 2 counted files)
        assert (len(wk) > 1000) == (perc == 20) and (len(wk) == 0) == (perc == 100)
