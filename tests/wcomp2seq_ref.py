"""comp2seq restated for 2k-bit k-mers (32 <= k <= 63; no reference exists there): tests/comp2seq_ref.py with the unitigs built by the
pinned oracle's text compiled for 128-bit keys (oracle.WTable, oracle.wide_build_unitigs) and the files in the wide formats of
tests/wide_files_ref.py.  The helpers of comp2seq_ref work on Python ints of any size and are used as they are; k-mers are Python ints."""
import numpy as np

import wide_files_ref as WF
from comp2seq_ref import canon, component_tables, decode, encode, flatten, kmers_of, order_key, seq_fasta, union_table  # noqa: F401

MASK64 = (1 << 64) - 1


def sequences_of_table(O, table, k):
    """the 128-bit oracle's unitigs (threshold 0, minimal length k) of one {k-mer: count}, in export order: [(bases, av, min, max)]"""
    if not table:
        return []
    t = O.WTable()
    for x, c in table.items():
        t.add(x, c)
    seqs = O.wide_build_unitigs(t, k, 0, k).all()
    return sorted(seqs, key=lambda s: (order_key(s[0], k), s))


def expected_split(O, comps, k):
    """-> per component its sequences"""
    return [sequences_of_table(O, t, k) for t in component_tables(comps, k)]


def expected_union(O, comps, k):
    return sequences_of_table(O, union_table(comps, k), k)


# ---- files ----
def words(members):
    """-> (hi uint64[], lo uint64[]) of Python-int k-mers"""
    return (np.array([int(x) >> 64 for x in members], dtype=np.uint64), np.array([int(x) & MASK64 for x in members], dtype=np.uint64))


def components_bytes(comps, weights=None):
    """a wide components.bin of lists of Python-int members (as given: the loader wants them ascending inside a component)"""
    flat = [x for members in comps for x in members]
    hi, lo = words(flat)
    sizes = [len(m) for m in comps]
    return WF.encode_components(sizes, weights if weights is not None else sizes, hi, lo)


def write_components(path, comps, weights=None):
    with open(path, "wb") as f:
        f.write(components_bytes(comps, weights))


def kmers_bin(table):
    """the 18-byte big-endian records of a {k-mer: count}, ascending k-mers"""
    keys = sorted(table)
    hi, lo = words(keys)
    return WF.encode_kmers(hi, lo, [table[x] for x in keys])


def stat_txt(table):
    return WF.stat_text(list(table.values())) if table else "# k-mer frequency\tnumber of such k-mers\n\n"


def expected_files(O, comps, k, split):
    """{path under the output directory: bytes} of comp2seq's layout with wide records"""
    files = {}
    if split:
        tables, seqs = component_tables(comps, k), expected_split(O, comps, k)
        for i, members in enumerate(comps):
            name = f"component_{i + 1}"
            files[f"kmers_fasta/{name}.fasta"] = "".join(f">{j + 1}\n{decode(int(x), k)}\n" for j, x in enumerate(members)).encode()
            files[f"kmer-counter-many/kmers/{name}.kmers.bin"] = kmers_bin(tables[i])
            files[f"kmer-counter-many/stats/{name}.stat.txt"] = stat_txt(tables[i]).encode()
            files[f"seq-builder-many/sequences/{name}.seq.fasta"] = seq_fasta(seqs[i]).encode()
    else:
        t = union_table(comps, k)
        files["kmers_fasta/component.fasta"] = "".join(f">{i + 1}_{j + 1}\n{decode(int(x), k)}\n" for i, members in enumerate(comps)
                                                       for j, x in enumerate(members)).encode()
        files["kmer-counter-many/kmers/component.kmers.bin"] = kmers_bin(t)
        files["kmer-counter-many/stats/component.stat.txt"] = stat_txt(t).encode()
        files["seq-builder-many/sequences/component.seq.fasta"] = seq_fasta(expected_union(O, comps, k)).encode()
    return files
