"""The crafted texts of tests/dparse_cases.py and the reference of tests/dparse_ref.py, without a GPU: every feature stands at the byte its
case is named after, every long line leaves a whole tile or chunk without a line start, the record counts are the named ones, and the
serial reference makes the oracle's reads (oracle/mf_oracle.c: read_fasta, read_fastq) of every text it calls taken -- while the oracle
refuses the texts whose expectation is the readers' error and reads the ones that merely make the device parser step back."""
import numpy as np
import pytest

import dparse_cases as DC
import dparse_ref as R


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", DC.SMALL, ids=_ids(DC.SMALL))
def test_case_is_what_its_name_says(case, oracle, tmp_path):
    t = case.text
    ref = DC.reference(case)
    # the feature at its place
    for P, what in case.at:
        assert t[P:P + len(what)] == what, (P, what, t[max(P - 4, 0):P + 8])
    if case.line_at:
        P, k = case.line_at
        at = np.flatnonzero(ref.line_starts == P)
        assert len(at) == 1 and at[0] % 4 == k and t[P - 1:P] == b"\n", (P, k, at)
    if case.name.startswith("fa-end-") or case.name.startswith("fq-end-"):
        assert len(t) == int(case.name.split("-")[2])
    # the long lines: a whole tile / chunk without a line start (a line starts behind a '\n')
    if case.span:
        B = DC.CHUNK if case.span == "chunk" else DC.TILE
        nl = np.flatnonzero(np.frombuffer(t, dtype=np.uint8) == 10) + 1
        per = np.bincount(nl // B, minlength=len(t) // B + 1)[:len(t) // B]
        assert np.any(per[1:] == 0), (case.span, per[:8])
    if case.n_rec is not None:
        assert ref.n_rec == case.n_rec
    # the serial and the vectorised reference agree
    assert R.same(ref, R.parse_vec(t, case.fmt, case.qoff)) == []
    if case.fmt == 2:
        assert R.sniff_qoff(t) == case.qoff
    # what is expected of it
    assert ref.rc == (0 if case.expect == "taken" else 1), (ref.rc, ref.names())
    if case.bit:
        assert ref.anomaly & case.bit, ref.names()
    if case.expect == "taken":
        assert ref.anomaly == 0 and ref.have == 2
    p = tmp_path / ("t" + case.ext)
    p.write_bytes(t)
    if case.expect == "error":
        with pytest.raises(oracle.OracleError):
            oracle.read_file(str(p))
        return
    ob, oo = oracle.read_file(str(p))
    if case.expect == "taken":
        assert np.array_equal(ref.offsets, oo), (len(ref.offsets), len(oo))
        assert np.array_equal(ref.bases, ob), np.flatnonzero(ref.bases != ob)[:5]


@pytest.mark.parametrize("e", DC.FLUSH_E)
def test_flush_cases_sweep_every_alignment(e):
    """every second tile of fa-flush-e emits exactly e bytes, and the place of its first one takes every value mod 16; the tiles between
    them emit 1 .. 16 bytes, so that neighbouring tiles write into one 16-byte word"""
    ref = DC.reference(DC.BY_NAME["fa-flush-%d" % e])
    tile = ref.emit_pos // DC.TILE
    first = np.searchsorted(tile, np.arange(34))                       # the place of every tile's first emitted byte
    count = np.bincount(tile, minlength=34)
    assert count[0] == 0 and np.all(count[1:33:2] == e) and np.all((count[2:34:2] >= 1) & (count[2:34:2] <= 16))
    assert sorted(first[1:33:2] % 16) == list(range(16))
    ends = (first[1:33:2] + e) % 16
    assert len(set(ends.tolist())) == 16


@pytest.mark.parametrize("case", DC.LARGE, ids=_ids(DC.LARGE))
def test_large_cases(case, oracle, tmp_path):
    """the texts of several MB, by the vectorised reference: the oracle's reads (also of the record of 2^24 bases, which the device parser
    leaves to the host reader)"""
    t = case.text
    ref = R.parse_vec(t, case.fmt, case.qoff)
    assert ref.rc == (0 if case.expect == "taken" else 1) and ref.anomaly == case.bit
    if case.n_rec is not None:
        assert ref.n_rec == case.n_rec and (case.n_rec + 2047) // 2048 > 1024
    p = tmp_path / ("t" + case.ext)
    p.write_bytes(t)
    ob, oo = oracle.read_file(str(p))
    if case.expect == "taken":
        assert np.array_equal(ref.offsets, oo) and np.array_equal(ref.bases, ob)
    else:
        assert int(np.diff(oo.astype(np.int64)).max()) == 1 << 24


def test_the_sweep_is_complete():
    names = set(_ids(DC.CASES))
    for B in DC.BORDERS:
        for o in DC.OFFSETS:
            for f in DC.FA_FEATURES:
                assert "fa-%s-at-%d" % (f, B + o) in names
            for f in DC.FQ_FEATURES:
                assert "fq-%s-at-%d" % (f, B + o) in names
    for n in DC.ENDS:
        for e in DC.ENDINGS:
            assert ("fa-end-%d-%s" % (n, e) in names) == (not (n == 1 and e == "crlf"))
            assert ("fq-end-%d-%s" % (n, e) in names) == (n >= 15)
    assert max(len(c.text) for c in DC.SMALL) < 700_000
