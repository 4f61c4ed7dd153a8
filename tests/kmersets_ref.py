"""Independent restatement of unique-kmers-multi (src/tools/UniqueKmersMultipleSamplesFinder.java:84-185) and kmers-multiple-filters
(src/tools/KmersMultipleFilters.java:77-133, IOUtils.MultipleFiltersAndPrintKmers src/io/IOUtils.java:125-213) in numpy, written from
the Java; it shares no code with the library.  tests/test_kmersets_cpu.py pins it with hand-worked cases.

A sample is given as its .kmers.bin records: (keys uint64[n], counts int16[n]), duplicates allowed.  Outputs are (keys, values) in
ascending key order."""
import re

import numpy as np

from stats_ref import MAX_COUNT

TRIPLE_HEADER = "# cd k-mer samples\tuc k-mer samples\tnonIBD k-mer samples\tnumber of such k-mers\n"


def load_table(samples, t):
    """IOUtils.loadKmers(files, t): the records with value > t, duplicates of a key (in one file or across the files) summed with
    saturation at 32767 (BigLong2ShortHashMap.addAndBound) -> (ascending unique keys, int64 values)"""
    if not samples:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    k = np.concatenate([np.asarray(s[0], dtype=np.uint64) for s in samples])
    c = np.concatenate([np.asarray(s[1]).astype(np.int16).astype(np.int64) for s in samples])
    m = c > t
    uk, inv = np.unique(k[m], return_inverse=True)
    s = np.zeros(len(uk), dtype=np.int64)
    np.add.at(s, inv, c[m])
    return uk, np.minimum(s, MAX_COUNT)


def java_short(x):
    """(short)x of an int: the low 16 bits, two's complement"""
    return ((np.asarray(x, dtype=np.int64) + 32768) % 65536) - 32768


def _member(sorted_keys, keys):
    """for each of `keys`: is it in sorted_keys, and where"""
    pos = np.searchsorted(sorted_keys, keys)
    hit = pos < len(sorted_keys)
    hit[hit] = sorted_keys[pos[hit]] == keys[hit]
    return hit, pos


def unique_kmers_multi(inputs, filters, b=1, min_samples=1, max_samples=1):
    """-> dict(n_union, files=[(i, keys, values int64)], counts=[c_i]); files ends with the first empty one"""
    if b < 0:
        raise ValueError("maximal-bad-frequence must not be negative")
    if min_samples > max_samples:
        raise ValueError("--min-samples parameter cannot be greater than --max-samples parameter.")
    if len(inputs) > 32767:
        raise ValueError("more than 32767 input files")
    tables = [load_table([s], b) for s in inputs]
    union = np.unique(np.concatenate([t[0] for t in tables])) if tables else np.zeros(0, np.uint64)
    total = np.zeros(len(union), dtype=np.int64)
    cnt = np.zeros(len(union), dtype=np.int64)
    for uk, uv in tables:
        pos = np.searchsorted(union, uk)
        total[pos] += uv            # hm.put(key, (short)(hm.getWithZero(key) + value)): wrapping each time = wrapping the sum once
        cnt[pos] += 1
    value = java_short(total)
    for f in filters:
        fk, _ = load_table([f], b)
        hit, _ = _member(fk, union)
        value[hit & (value > b)] = 0     # hm.get(key) > b -> hm.put(key, 0)
    files, counts = [], []
    for i in range(min_samples, max_samples + 1):
        sel = (value > b) & (cnt > i - 1)
        files.append((i, union[sel], value[sel]))
        counts.append(int(sel.sum()))
        if counts[-1] == 0:
            break
    return dict(n_union=len(union), files=files, counts=counts)


def triple_stat_txt(triples, counts):
    return TRIPLE_HEADER + "".join("%d\t%d\t%d\t%d\n" % (t[0], t[1], t[2], c) for t, c in zip(triples, counts)) + "\n"


def kmers_multiple_filters(sample, cd, uc, nonibd, b=1):
    """one input file against the three filter file lists -> dict(kept=(keys, values), triples int64[m][3] in Triple.compareTo order,
    counts int64[m], found, stat_txt)"""
    if b < 0:
        raise ValueError("maximal-bad-frequence must not be negative")
    tk, tv = load_table([sample], b)
    cols = []
    for lst in (cd, uc, nonibd):
        fk, fv = load_table(list(lst), 0)
        hit, pos = _member(fk, tk)
        v = np.zeros(len(tk), dtype=np.int64)
        v[hit] = fv[pos[hit]]
        cols.append(v)
    tri = np.stack(cols, axis=1) if len(tk) else np.zeros((0, 3), np.int64)
    keep = (tri > 0).any(axis=1)
    if len(tk):
        ut, n = np.unique(tri, axis=0, return_counts=True)      # rows in lexicographic order: cd, then uc, then nonibd
    else:
        ut, n = np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    return dict(kept=(tk[keep], tv[keep]), triples=ut, counts=n, found=len(tk), stat_txt=triple_stat_txt(ut, n))


def output_name(path):
    """file.getName().replaceAll(".kmers.bin", ""): the pattern is a regular expression, every '.' matches any character"""
    return re.sub(r".kmers.bin", "", path.rsplit("/", 1)[-1])
