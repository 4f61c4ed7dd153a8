"""Python-integer reference of the wide (k = 32 ... 63) set tools: unique-kmers-multi and kmers-filter on tables given as
{(hi << 64) | lo: count} dicts, written from the definition in include/metafast_hip.h (UniqueKmersMultipleSamplesFinder.java:84-185,
IOUtils.filterAndPrintKmers src/io/IOUtils.java:101-123); shares no code with the library or with tests/kmersets_ref.py."""
import wide_files_ref as WF

MASK64 = (1 << 64) - 1


def java_short(x):
    """(short)x of an int"""
    x &= 0xFFFF
    return x - 0x10000 if x >= 0x8000 else x


def canonical(x, k):
    return min(x, WF.revcomp(x, k))


def unique_kmers_multi(inputs, filters, b=1, min_samples=1, max_samples=1):
    """inputs, filters: lists of {kmer: count} -> dict(n_union, tables=[{kmer: sum} for i = min_samples ...], counts=[c_i]); the list
    ends with the first empty table (included)"""
    if b < 0:
        raise ValueError("maximal-bad-frequence must not be negative")
    if min_samples > max_samples:
        raise ValueError("--min-samples parameter cannot be greater than --max-samples parameter.")
    if len(inputs) > 32767:
        raise ValueError("more than 32767 input files")
    cnt, total = {}, {}
    for t in inputs:
        for x, c in t.items():
            if c > b:
                cnt[x] = cnt.get(x, 0) + 1
                total[x] = total.get(x, 0) + c
    value = {x: java_short(s) for x, s in total.items()}
    for f in filters:
        for x, c in f.items():
            if c > b and x in value and value[x] > b:
                value[x] = 0
    tables, counts = [], []
    for i in range(min_samples, max_samples + 1):
        t = {x: v for x, v in value.items() if v > b and cnt[x] >= i}
        tables.append(t)
        counts.append(len(t))
        if not t:
            break
    return dict(n_union=len(value), tables=tables, counts=counts)


def filter_kmers(table, threshold, filt, filter_threshold):
    """the records of `table` with count > threshold whose k-mer has a value > filter_threshold in `filt` (absent: 0)"""
    return {x: c for x, c in table.items() if c > threshold and filt.get(x, 0) > filter_threshold}


def load(tables, b):
    """mf_wtable_load_kmers(files, b): records with count > b, the counts of a k-mer in several files added up, bounded at 32767"""
    out = {}
    for t in tables:
        for x, c in t.items():
            if c > b:
                out[x] = min(out.get(x, 0) + c, 32767)
    return out


def kmers_bin(table):
    """the wide .kmers.bin of a table: ascending 18-byte records"""
    keys = sorted(table)
    return WF.encode_kmers([x >> 64 for x in keys], [x & MASK64 for x in keys], [table[x] for x in keys])


def from_words(hi, lo, cnt):
    return {(int(h) << 64) | int(l): int(c) for h, l, c in zip(hi, lo, cnt)}
