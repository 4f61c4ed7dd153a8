"""The reverse complements of the minimizer scan, taken word by word (metafast_amd/csrc/mf_skm_scan.h: skm_rc16, skm_mmer_at), restated on the host
and compared with the reverse complement of the M-mer itself (mf_mmer_rc, restated as nbr_ref.revcomp).

The scan holds 64 bases in four dwords D[0..3], first base in the top bits of D[0].  It reverse-complements each dword once, R[3 - q] =
rc16(D[q]), and cuts the reverse complement of the M-mer at base i out of R at base 64 - M - i with the funnel shift that cuts the M-mer out
of D.  Checked here: every one of the 48 positions i = 0 .. 47 of a window, M = 13 and M = 15, exact."""
import numpy as np
import pytest

import nbr_ref as R

U32 = np.uint64(0xFFFFFFFF)
_U = np.uint64


def brev32(x):
    x = np.asarray(x, dtype=np.uint64)
    r = np.zeros_like(x)
    for b in range(32):
        r |= ((x >> _U(b)) & _U(1)) << _U(31 - b)
    return r


def rc16(d):
    """skm_rc16: 16 bases of a dword, reversed and complemented"""
    r = brev32(~np.asarray(d, dtype=np.uint64) & U32)
    return (((r & _U(0xAAAAAAAA)) >> _U(1)) | ((r & _U(0x55555555)) << _U(1))) & U32


def alignbit(hi, lo, s):
    """v_alignbit_b32: the low 32 bits of (hi:lo) >> s, 0 <= s < 32"""
    return (((hi << _U(32)) | lo) >> _U(s)) & U32


def mmer_at(X, p, M):
    """skm_mmer_at: M bases from base p of the 64 in X[0..3], right-aligned"""
    q, o = p >> 4, p & 15
    top = alignbit(X[q], X[q + 1] if q + 1 < 4 else np.zeros_like(X[q]), 32 - 2 * o) if o else X[q]
    return top >> _U(32 - 2 * M)


def words_of(codes):
    """[n, 64] base codes -> D[0..3], each uint64 [n] holding 32 bits"""
    D = []
    for q in range(4):
        d = np.zeros(len(codes), dtype=np.uint64)
        for b in range(16):
            d = (d << _U(2)) | codes[:, 16 * q + b].astype(np.uint64)
        D.append(d)
    return D


def windows():
    rng = np.random.default_rng(0x5243)
    fixed = [np.zeros(64), np.full(64, 3), np.arange(64) % 2 * 2, (np.arange(64) + 1) % 2 * 3, np.arange(64) % 3, (np.arange(64) % 3 + 1) % 4]
    return np.concatenate([np.array(fixed, dtype=np.uint8), rng.integers(0, 4, size=(4000, 64), dtype=np.uint8)])


@pytest.mark.parametrize("M", [13, 15])
def test_reverse_complement_from_reversed_words(M):
    codes = windows()
    D = words_of(codes)
    Rw = [rc16(D[3]), rc16(D[2]), rc16(D[1]), rc16(D[0])]
    for i in range(48):
        f = np.zeros(len(codes), dtype=np.uint64)
        for b in range(M):
            f = (f << _U(2)) | codes[:, i + b].astype(np.uint64)
        assert np.array_equal(mmer_at(D, i, M), f), (M, i, "forward M-mer")
        got = mmer_at(Rw, 64 - M - i, M)
        want = R.revcomp(f, M)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (M, i, f"window {bad[0] if len(bad) else 0}: {int(got[bad[0]]) if len(bad) else 0:#x} != {int(want[bad[0]]) if len(bad) else 0:#x}")


def test_the_halo_scan_reads_no_word_it_does_not_have():
    """k_skm_scatter's lanes hash M-mers 0 .. 31 only and hold R[1..3] (R[1] from the next lane): none of those reverse complements starts in R[0]"""
    for M in (13, 15):
        assert min(64 - M - i for i in range(32)) >= 16
