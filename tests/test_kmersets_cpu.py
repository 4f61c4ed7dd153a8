"""Hand-worked cases that pin tests/kmersets_ref.py, the restatement of unique-kmers-multi
(src/tools/UniqueKmersMultipleSamplesFinder.java:84-185) and kmers-multiple-filters (src/tools/KmersMultipleFilters.java:77-133,
src/io/IOUtils.java:125-213) that the GPU tests compare the library with.  Every expected value below was worked out by hand from
the Java."""
import numpy as np
import pytest

import kmersets_ref as K


def S(*recs):
    """a sample from (key, count) records"""
    return np.array([r[0] for r in recs], dtype=np.uint64), np.array([r[1] for r in recs], dtype=np.int16)


def files_of(res):
    return [(i, k.tolist(), v.tolist()) for i, k, v in res["files"]]


def test_wrap_to_a_java_short():
    # (short)(a + b) wraps: 60000 - 65536, 131068 - 131072, 163835 - 131072
    assert int(K.java_short(3 * 20000)) == -5536
    assert int(K.java_short(4 * 32767)) == -4
    assert int(K.java_short(5 * 32767)) == 32763
    three = K.unique_kmers_multi([S((7, 20000))] * 3, [], b=1, min_samples=1, max_samples=3)
    assert three["n_union"] == 1 and files_of(three) == [(1, [], [])] and three["counts"] == [0]          # -5536 is not > b
    four = K.unique_kmers_multi([S((7, 32767))] * 4, [], b=1)
    assert four["n_union"] == 1 and files_of(four) == [(1, [], [])]                                          # -4
    five = K.unique_kmers_multi([S((7, 32767))] * 5, [], b=1, min_samples=5, max_samples=5)
    assert files_of(five) == [(5, [7], [32763])] and five["counts"] == [1]
    # 2 x 16384 = 32768 -> -32768; 4 x 16384 = 65536 -> 0; one more 2 -> 2
    assert files_of(K.unique_kmers_multi([S((7, 16384))] * 2, [], b=0)) == [(1, [], [])]
    assert files_of(K.unique_kmers_multi([S((7, 16384))] * 4, [], b=0)) == [(1, [], [])]
    assert files_of(K.unique_kmers_multi([S((7, 16384))] * 4 + [S((7, 2))], [], b=0, min_samples=5, max_samples=5)) == [(5, [7], [2])]


def test_knock_out_and_filter_only_keys():
    a = S((10, 5), (20, 5))
    r = K.unique_kmers_multi([a], [S((10, 3), (30, 9))], b=1)
    assert r["n_union"] == 2                                  # 10 and 20: key 30 is only in a filter file and never enters the map
    assert files_of(r) == [(1, [20], [5])] and r["counts"] == [1]
    # a filter record that is not > b knocks nothing out; the order of the filter files does not matter
    assert files_of(K.unique_kmers_multi([a], [S((20, 1))], b=1)) == [(1, [10, 20], [5, 5])]
    f1, f2 = S((10, 2)), S((20, 7), (10, 4))
    assert files_of(K.unique_kmers_multi([a], [f1, f2], b=1)) == files_of(K.unique_kmers_multi([a], [f2, f1], b=1)) == [(1, [], [])]
    # an input record that is not > b is no presence: key 10 is held by one sample only
    r = K.unique_kmers_multi([a, S((10, 1), (20, 2))], [], b=1, min_samples=2, max_samples=2)
    assert r["n_union"] == 2 and files_of(r) == [(2, [20], [7])]


def test_duplicates_in_one_file_saturate_before_the_wrapping_sum():
    # file 1: 30000 + 30000 -> 32767 (addAndBound); then 32767 + 32767 + 5 = 65539 -> 3  (unsaturated it would be 27236)
    ins = [S((9, 30000), (9, 30000)), S((9, 32767)), S((9, 5))]
    r = K.unique_kmers_multi(ins, [], b=1, min_samples=3, max_samples=3)
    assert files_of(r) == [(3, [9], [3])]
    # records that are not > b are dropped one by one, before they are summed: (9, 1) + (9, 1) is not 2
    r = K.unique_kmers_multi([S((9, 1), (9, 1), (4, 2))], [], b=1)
    assert r["n_union"] == 1 and files_of(r) == [(1, [4], [2])]


def test_the_file_list_ends_with_the_first_empty_one():
    ins = [S((1, 4), (2, 4)), S((1, 4), (2, 4)), S((1, 4))]
    r = K.unique_kmers_multi(ins, [], b=1, min_samples=1, max_samples=6)
    assert files_of(r) == [(1, [1, 2], [12, 8]), (2, [1, 2], [12, 8]), (3, [1], [12]), (4, [], [])]
    assert r["counts"] == [2, 2, 1, 0] and r["n_union"] == 2
    with pytest.raises(ValueError, match="--min-samples parameter cannot be greater than --max-samples parameter."):
        K.unique_kmers_multi(ins, [], min_samples=3, max_samples=2)
    with pytest.raises(ValueError):
        K.unique_kmers_multi(ins, [], b=-1)


def test_triple_histogram_and_its_text():
    sample = S((1, 5), (2, 5), (3, 5), (4, 5), (5, 5), (6, 5), (7, 1))           # (7, 1) is not > b = 1
    cd = [S((1, 1), (2, 2)), S((1, 1), (3, 2))]                                    # one table over both files: cd(1) = 2
    uc = [S((1, 1), (2, 1), (4, 3), (9, 8))]
    nonibd = [S((1, 4), (2, 5), (5, 0))]                                            # a record of 0 is not > 0: absent
    r = K.kmers_multiple_filters(sample, cd, uc, nonibd, b=1)
    assert r["found"] == 6
    assert r["kept"][0].tolist() == [1, 2, 3, 4] and r["kept"][1].tolist() == [5, 5, 5, 5]
    assert r["triples"].tolist() == [[0, 0, 0], [0, 3, 0], [2, 0, 0], [2, 1, 4], [2, 1, 5]] and r["counts"].tolist() == [2, 1, 1, 1, 1]
    assert r["stat_txt"] == ("# cd k-mer samples\tuc k-mer samples\tnonIBD k-mer samples\tnumber of such k-mers\n"
                             "0\t0\t0\t2\n0\t3\t0\t1\n2\t0\t0\t1\n2\t1\t4\t1\n2\t1\t5\t1\n\n")
    # no key in any filter: nothing kept, one (0, 0, 0) line
    r = K.kmers_multiple_filters(sample, [S((100, 1))], [], [], b=1)
    assert len(r["kept"][0]) == 0 and r["triples"].tolist() == [[0, 0, 0]] and r["counts"].tolist() == [6]
    # filter values saturate at 32767 over the files of a list
    r = K.kmers_multiple_filters(S((1, 2)), [S((1, 32767)), S((1, 32767))], [], [], b=1)
    assert r["triples"].tolist() == [[32767, 0, 0]]


def test_output_name_is_a_regular_expression_replace():
    assert K.output_name("/x/s1.kmers.bin") == "s1"
    assert K.output_name("n_samples.kmers.bin") == "n_samples"
    assert K.output_name("a_kmers_bin.kmers.bin") == "a"           # '.' matches any character: "_kmers_bin" goes too
    assert K.output_name("xkmersybin") == ""
    assert K.output_name("/d.kmers.bin/abc") == "abc"              # File.getName(): the last path element only
    assert K.output_name("s.kmers.bin.kmers.binz") == "sz"
