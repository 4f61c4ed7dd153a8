"""The file formats of the k = 32 ... 63 path, pinned by hand-written bytes: tests/wide_files_ref.py is the numpy restatement the GPU
tests check metafast_amd/csrc/mf_wio.hip against, so it is itself tied to literals here -- k = 32 (the high word is always 0), k = 33 (2 bits of
high word), k = 63 (62 bits); key 0 (poly-A) and the count 32767 among them."""
import re

import numpy as np
import pytest

import wide_files_ref as R
from metafast_amd import lib as L

NEW_CALLS = ("mf_count_reads_wide", "mf_wtable_write_kmers", "mf_wtable_load_kmers", "mf_wcomps_write", "mf_wcomps_load", "mf_features_wide")


def _h(s):
    return bytes.fromhex(s.replace(" ", ""))


# (k, [(k-mer as text or int, count)], the file's bytes)
K32 = _h("0000000000000000 0000000000000000 7fff"          # A x 32 = key 0, count 32767
         "0000000000000000 0000000000000002 0001"          # A x 31 + C
         "0000000000000000 4000000000000000 0102")         # G + A x 31, count 258
K33 = _h("0000000000000000 0000000000000000 0001"          # A x 33
         "0000000000000001 0000000000000005 0003"          # G + A x 30 + GG: the high word holds the first base
         "0000000000000002 fffffffffffffffc 7fff")         # C + T x 31 + A
K63 = _h("0000000000000000 0000000000000000 0002"          # A x 63
         "0123456789abcdef fedcba9876543210 7fff"
         "2fffffffffffffff fffffffffffffffc 0004")         # C + T x 61 + A: 62 bits of high word in use


def _text_to_int(s):
    v = 0
    for ch in s:
        v = (v << 2) | "AGCT".index(ch)
    return v


@pytest.mark.parametrize("k,data,keys,counts", [
    (32, K32, [_text_to_int("A" * 32), _text_to_int("A" * 31 + "C"), _text_to_int("G" + "A" * 31)], [32767, 1, 258]),
    (33, K33, [_text_to_int("A" * 33), _text_to_int("G" + "A" * 30 + "GG"), _text_to_int("C" + "T" * 31 + "A")], [1, 3, 32767]),
    (63, K63, [0, (0x0123456789ABCDEF << 64) | 0xFEDCBA9876543210, _text_to_int("C" + "T" * 61 + "A")], [2, 32767, 4]),
])
def test_kmers_records_against_literal_bytes(k, data, keys, counts):
    hi = np.array([x >> 64 for x in keys], dtype=np.uint64)
    lo = np.array([x & R.MASK64 for x in keys], dtype=np.uint64)
    assert len(data) == 18 * len(keys)
    assert R.encode_kmers(hi, lo, counts) == data
    dh, dl, dc = R.decode_kmers(data)
    assert np.array_equal(dh, hi) and np.array_equal(dl, lo) and dc.tolist() == counts
    assert R.first_bad_record(hi, lo, k) is None
    assert all(int(h) >> max(2 * k - 64, 0) == 0 for h in hi)
    if k == 32:
        assert not hi.any()


def test_the_three_validity_rules():
    one = lambda x: (np.array([x >> 64], dtype=np.uint64), np.array([x & R.MASK64], dtype=np.uint64))
    # key >= 4^k: bit 66 at k = 33, bit 64 at k = 32, bit 126 at k = 63
    assert R.first_bad_record(*one(1 << 66), 33) == (0, "range")
    assert R.first_bad_record(*one(1 << 64), 32) == (0, "range")
    assert R.first_bad_record(*one(1 << 126), 63) == (0, "range")
    assert R.first_bad_record(*one((1 << 126) - 4), 63) == (0, "canonical")   # T x 62 + A is below 4^63 but above T + A x 62, its reverse complement
    # not canonical: T x k is above its reverse complement A x k
    for k in (32, 33, 63):
        assert R.first_bad_record(*one((1 << (2 * k)) - 1), k) == (0, "canonical")
        assert R.revcomp((1 << (2 * k)) - 1, k) == 0 and R.revcomp(0, k) == (1 << (2 * k)) - 1
    assert R.revcomp(_text_to_int("G" + "A" * 30 + "GG"), 33) == _text_to_int("CC" + "T" * 30 + "C")
    # order: equal and descending neighbours, also where only the high words differ
    hi, lo, _ = R.decode_kmers(K33)
    assert R.first_bad_record(hi[[0, 1, 1]], lo[[0, 1, 1]], 33) == (2, "order")
    assert R.first_bad_record(hi[[0, 2, 1]], lo[[0, 2, 1]], 33) == (2, "order")
    assert R.first_bad_record(hi[::-1], lo[::-1], 33) == (1, "order")
    # a 10-byte record file is refused by its size, or by its records where the size happens to divide
    with pytest.raises(ValueError):
        R.decode_kmers(b"\0" * 10)
    ten = np.zeros(9, dtype=np.dtype([("key", ">u8"), ("cnt", ">i2")]))
    ten["key"] = np.arange(1, 10) * 0x0123456789ABCDE; ten["cnt"] = 5
    h10, l10, _ = R.decode_kmers(ten.tobytes())
    assert len(h10) == 5 and R.first_bad_record(h10, l10, 40) is not None


def test_components_against_literal_bytes():
    data = _h("00000002"
              "00000002 0000000000000064" "0000000000000001 0000000000000005" "0000000000000002 ffffffffffffffff"
              "00000001 ffffffffffffffff" "0000000000000000 0000000000000000")
    sizes, weights = [2, 1], [100, -1]
    hi = np.array([1, 2, 0], dtype=np.uint64); lo = np.array([5, R.MASK64, 0], dtype=np.uint64)
    assert R.encode_components(sizes, weights, hi, lo) == data
    s, w, h, l = R.decode_components(data)
    assert s.tolist() == sizes and w.tolist() == weights and np.array_equal(h, hi) and np.array_equal(l, lo)
    assert R.encode_components([], [], hi[:0], lo[:0]) == _h("00000000")
    for bad in (data[:-1], data + b"\0", data[:20]):
        with pytest.raises(ValueError):
            R.decode_components(bad)


def test_stat_text():
    assert R.stat_text([1, 1, 3, 32767]) == "# k-mer frequency\tnumber of such k-mers\n1\t2\n3\t1\n32767\t1\n\n"


def test_the_new_calls_are_declared_bound_and_exported():
    import ctypes
    hdr = open(L.HEADER_PATH).read()
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", hdr))
    so = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_CALLS:
        assert name in declared and name in L.exported_symbols() and hasattr(so, name), name
    for method in ("count_reads_wide", "load_kmers_wide", "load_components_wide", "features_wide_files"):
        assert hasattr(L.Context, method)
    assert hasattr(L.WideTable, "write_kmers") and hasattr(L.WideComps, "write")
