"""The device read parser (metafast_amd/csrc/mf_dparse.hip) unit by unit on the crafted texts of tests/dparse_cases.py.

mf_debug_dparse (the end of mf_dparse.hip; bound here with ctypes, not part of the C-ABI) puts a text into a buffer of whole chunks + 64
bytes that holds a fill byte everywhere else -- 'A' and '\\r': what a base or a line end behind the text's end would do, if a kernel looked
there -- and runs dparse_kernels, the launches dparse_source makes, on it.  Everything the passes hand on is held against
tests/dparse_ref.py bit for bit: the return code, the anomaly word as the host read it last (equal to the reference's staged set, and it
holds the bit a case is about), n_rec, rec_seq + flag bytes or ls + drop, rec_place, offsets, bases, and 256 bytes of 0xA5 behind the
bases that nothing may touch (the bases themselves lie on 0xA5 too: a byte the flush leaves out shows).  A case that is marked taken must
come back with rc 0: a step back would pass every whole-file comparison through the host parser.

The same texts as files through Context.load_reads with device_parse_min_bytes = 1, after a larger file, so that the workspace holds old
text behind a text's end: the oracle's reads, and the counter the case names moves.

Not here: k_dp_fa_scan's own second step needs more than 1024 chunks, a text of 268 MB -- the full-size tests' matter.  The uploader
threads and the .gz sink."""
import ctypes as C

import numpy as np
import pytest

import dparse_cases as DC
import dparse_ref as R

pytestmark = pytest.mark.gpu
FILLS = (ord("A"), ord("\r"))
CANARY = 0xA5


def run_debug(ctx, text, fmt, qoff, fill):
    """-> what mf_debug_dparse hands back, as a dict"""
    from metafast_amd import lib as L
    so = L.lib()
    fn, info, cp, free = so.mf_debug_dparse, so.mf_debug_dparse_info, so.mf_debug_dparse_copy, so.mf_debug_dparse_free
    fn.restype = info.restype = cp.restype = C.c_int
    free.restype = None
    fn.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    info.argtypes = [C.c_void_p, C.c_void_p]
    cp.argtypes = [C.c_void_p] * 6
    free.argtypes = [C.c_void_p]
    h = C.c_void_p()
    L._check(fn(ctx.h, text, len(text), fmt, qoff, fill, C.byref(h)))
    try:
        v = np.zeros(8, dtype=np.uint64)
        L._check(info(h, v.ctypes.data))
        rc, anomaly, n_rec, n_lines, n_reads, n_bases, have, _ = (int(x) for x in v)
        d = dict(rc=rc, anomaly=anomaly, n_rec=n_rec, n_lines=n_lines, n_reads=n_reads, n_bases=n_bases, have=have)
        d["rec_a"] = np.zeros(((n_rec if fmt == 1 else n_lines) + 1) if have >= 1 else 0, dtype=np.uint64)
        d["rec_b"] = np.zeros(n_rec if have >= 1 else 0, dtype=np.uint8)
        d["rec_place"] = np.zeros(n_rec + 1 if have == 2 else 0, dtype=np.uint64)
        d["offsets"] = np.zeros(n_reads + 1 if have == 2 else 0, dtype=np.uint64)
        d["bases"] = np.zeros(n_bases + 256 if have == 2 else 0, dtype=np.uint8)
        L._check(cp(h, *(d[k].ctypes.data if len(d[k]) else None for k in ("rec_a", "rec_b", "rec_place", "offsets", "bases"))))
        return d
    finally:
        free(h)


def _names(word):
    return [n for b, n in R.BIT_NAMES.items() if word & b]


def _first_diff(a, b):
    if len(a) != len(b):
        return "%d entries, the reference has %d" % (len(a), len(b))
    at = np.flatnonzero(np.asarray(a) != np.asarray(b))
    return "first at %d: %s, the reference has %s" % (at[0], a[at[0]], b[at[0]]) if len(at) else "equal"


def check(out, ref, where, bit=0, sure=False, final_only=False):
    assert out["rc"] == ref.rc, (where, "rc %d, anomaly %s; the reference: rc %d, %s" % (out["rc"], _names(out["anomaly"]), ref.rc, ref.names()))
    if sure:
        assert out["rc"] == 0, (where, "a text the device parser must be sure about stepped back", _names(out["anomaly"]))
    assert out["anomaly"] == ref.anomaly, (where, _names(out["anomaly"]), ref.names())
    assert out["anomaly"] & bit == bit, (where, _names(out["anomaly"]), _names(bit))
    assert out["have"] == ref.have, (where, out["have"], ref.have)
    assert out["n_rec"] == ref.n_rec and out["n_lines"] == ref.n_lines, (where, out["n_rec"], ref.n_rec, out["n_lines"], ref.n_lines)
    if ref.have >= 1 and not final_only:
        assert np.array_equal(out["rec_a"], ref.rec_a), (where, "rec_seq / ls", _first_diff(out["rec_a"], ref.rec_a))
        assert np.array_equal(out["rec_b"], ref.rec_b), (where, "flags / drop", _first_diff(out["rec_b"], ref.rec_b))
    if ref.have == 2:
        nb = len(ref.bases)
        assert out["n_reads"] == len(ref.offsets) - 1 and out["n_bases"] == nb, (where, out["n_reads"], out["n_bases"], len(ref.offsets) - 1, nb)
        if not final_only:
            assert np.array_equal(out["rec_place"], ref.rec_place), (where, "rec_place", _first_diff(out["rec_place"], ref.rec_place))
        assert np.array_equal(out["offsets"], ref.offsets), (where, "offsets", _first_diff(out["offsets"], ref.offsets))
        tail = out["bases"][nb:]
        assert len(tail) == 256 and np.all(tail == CANARY), (where, "bytes written behind the bases, the first %d behind the end" % np.flatnonzero(tail != CANARY)[0])
        assert np.array_equal(out["bases"][:nb], ref.bases), (where, "bases", _first_diff(out["bases"][:nb], ref.bases))


@pytest.fixture(scope="module")
def file_ctx(gpu_ctx, tmp_path_factory):
    """files of any size go to the device parser; a file of 1.3 MB first, whose text stays in the workspace"""
    gpu_ctx.set_option("device_parse_min_bytes", 1)
    try:
        p = tmp_path_factory.mktemp("dparse") / "first.fa"
        p.write_bytes(b"".join(b">first %d\n%s\n" % (i, b"ACGTTGCAAC" * 13) for i in range(9000)))
        before = gpu_ctx.stat("device_parsed_files")
        b, o = gpu_ctx.load_reads([str(p)])
        assert len(o) == 9001 and len(b) == 9000 * 130 and gpu_ctx.stat("device_parsed_files") == before + 1
        yield gpu_ctx
    finally:
        gpu_ctx.set_option("device_parse_min_bytes", 1 << 20)


def check_file(ctx, oracle, case, tmp_path):
    from metafast_amd import lib as L
    p = tmp_path / ("t" + case.ext)
    p.write_bytes(case.text)
    before = ctx.stat("device_parsed_files"), ctx.stat("device_parser_stepped_back")
    if case.expect == "error":
        with pytest.raises(oracle.OracleError):
            oracle.read_file(str(p))
        with pytest.raises(L.MetafastError):
            ctx.load_reads([str(p)])
    else:
        ob, oo = oracle.read_file(str(p))
        db, do = ctx.load_reads([str(p)])
        assert np.array_equal(do, oo), (case.name, "offsets", _first_diff(do, oo))
        assert np.array_equal(db, ob), (case.name, "bases", _first_diff(db, ob))
    moved = ctx.stat("device_parsed_files") - before[0], ctx.stat("device_parser_stepped_back") - before[1]
    assert moved == ((1, 0) if case.expect == "taken" else (0, 1)), (case.name, case.expect, moved)


@pytest.mark.parametrize("case", DC.SMALL, ids=[c.name for c in DC.SMALL])
def test_units(gpu_ctx, case):
    ref = DC.reference(case, quick=True)
    # (the sweep's texts at the two chunk borders are 260 KB each and their feature stands far from the text's end: one fill byte each, by turns)
    fills = FILLS if case.border_at is None or case.border_at < DC.CHUNK - 2 else FILLS[case.border_at % 2:][:1]
    for fill in fills:
        out = run_debug(gpu_ctx, case.text, case.fmt, case.qoff, fill)
        check(out, ref, "%s (%s), behind the text: %r" % (case.name, case.reach, chr(fill)), bit=case.bit, sure=case.expect == "taken")


@pytest.mark.parametrize("case", DC.SMALL, ids=[c.name for c in DC.SMALL])
def test_as_a_file(file_ctx, oracle, tmp_path, case):
    check_file(file_ctx, oracle, case, tmp_path)


@pytest.mark.parametrize("case", DC.LARGE, ids=[c.name for c in DC.LARGE])
def test_large_texts(file_ctx, oracle, tmp_path, case):
    """2 099 201 records (k_dp_scan2's second step) unit by unit; the records of 2^24 - 1 and 2^24 bases by their final arrays only.  One
    fill byte: these are 8 and 16 MB"""
    ref = R.parse_vec(case.text, case.fmt, case.qoff)
    out = run_debug(file_ctx, case.text, case.fmt, case.qoff, FILLS[0])
    check(out, ref, "%s (%s)" % (case.name, case.reach), bit=case.bit, sure=case.expect == "taken", final_only=case.n_rec is None)
    check_file(file_ctx, oracle, case, tmp_path)
