"""comp2seq restated in Python (ComponentsToSequences.java:41-76: bin2fasta --split, kmer-counter-many -b 0, seq-builder-many -b 0 -l k):
components -> per component {canonical k-mer: multiplicity} -> the component's sequences, by the oracle's unitig builder (threshold 0,
minimal length k) run once per component, ordered by oriented start k-mer as the GPU export orders them.  Also the files of the
reference's layout, and the builders of the test cases."""
import struct

import numpy as np

NUC = "AGCT"                      # A0 G1 C2 T3 (DnaTools.java:31)
MAX_COUNT = 32767
_RC = str.maketrans("ACGT", "TGCA")


def encode(s):
    v = 0
    for ch in s:
        v = (v << 2) | NUC.index(ch)
    return v


def decode(v, k):
    return "".join(NUC[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


def rc_str(s):
    return s[::-1].translate(_RC)


def canon(v, k):
    r, x = 0, v
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return min(v, r)


_CODE = {ch: i for i, ch in enumerate(NUC)}


def kmers_of(seq, k, canonical=True):
    mask, top = (1 << (2 * k)) - 1, 2 * k - 2
    f = r = 0
    out = []
    for i, ch in enumerate(seq):
        c = _CODE[ch]
        f = ((f << 2) | c) & mask
        r = (r >> 2) | ((3 - c) << top)
        if i >= k - 1:
            out.append(min(f, r) if canonical else f)
    return out


def component_tables(comps, k):
    """per component {canonical k-mer: multiplicity in its member list, capped as the counter caps}"""
    out = []
    for members in comps:
        t = {}
        for x in members:
            c = canon(int(x), k)
            t[c] = min(t.get(c, 0) + 1, MAX_COUNT)
        out.append(t)
    return out


def union_table(comps, k):
    t = {}
    for members in comps:
        for x in members:
            c = canon(int(x), k)
            t[c] = min(t.get(c, 0) + 1, MAX_COUNT)
    return t


def order_key(seq, k):
    """what the GPU export sorts by: (canonical start k-mer, strand of the start k-mer)"""
    x = encode(seq[:k])
    c = canon(x, k)
    return (c, 0 if x == c else 1)


def sequences_of_table(O, table, k):
    """the oracle's unitigs (threshold 0, minimal length k) of one {k-mer: count}, in export order: [(bases, av, min, max)]"""
    if not table:
        return []
    t = O.Table()
    for x, c in table.items():
        t.add(x, c)
    seqs = O.build_unitigs(t, k, 0, k).all()
    return sorted(seqs, key=lambda s: (order_key(s[0], k), s))


def expected_split(O, comps, k):
    """-> per component its sequences"""
    return [sequences_of_table(O, t, k) for t in component_tables(comps, k)]


def expected_union(O, comps, k):
    return sequences_of_table(O, union_table(comps, k), k)


def flatten(per_comp):
    """-> (sequences in export order, their component ids)"""
    seqs, ids = [], []
    for i, ss in enumerate(per_comp):
        seqs += ss
        ids += [i] * len(ss)
    return seqs, np.array(ids, dtype=np.uint32)


# ---- files ----
def write_components(path, comps, weights=None):
    """ConnectedComponent.saveComponents (ConnectedComponent.java:80-93)"""
    with open(path, "wb") as f:
        f.write(struct.pack(">I", len(comps)))
        for i, members in enumerate(comps):
            f.write(struct.pack(">Iq", len(members), weights[i] if weights else len(members)))
            f.write(np.asarray(members, dtype=">u8").tobytes())


def kmers_bin(table):
    """the 10-byte big-endian records of a {k-mer: count}, ascending k-mers"""
    return b"".join(struct.pack(">QH", x, table[x]) for x in sorted(table))


def stat_txt(table):
    hist = {}
    for c in table.values():
        hist[c] = hist.get(c, 0) + 1
    return "# k-mer frequency\tnumber of such k-mers\n" + "".join(f"{c}\t{hist[c]}\n" for c in sorted(hist)) + "\n"


def seq_fasta(seqs):
    """Sequence.printSequences: numbered from 1, 70 columns"""
    out = []
    for i, (s, a, mn, mx) in enumerate(seqs):
        out.append(f">{i + 1} length={len(s)} av_weight={a} min_weight={mn} max_weight={mx}\n")
        out += [s[j:j + 70] + "\n" for j in range(0, len(s), 70)]
    return "".join(out)


def expected_files(O, comps, k, split):
    """{path under the work directory: bytes} of the reference's layout"""
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


# ---- the cases: each returns (k, components = lists of canonical k-mers) ----
def _rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def _simple_path(rng, n_kmers, k):
    """a random sequence whose n_kmers k-mers are all different, strands included"""
    while True:
        s = _rand_seq(rng, n_kmers + k - 1)
        if len(set(kmers_of(s, k))) == n_kmers:
            return s


def case_adjacent(k):
    """(a) one linear path of 12 k-mers cut into {0-4}, {5-8}, {9-11}"""
    km = kmers_of(_simple_path(np.random.default_rng(100 + k), 12, k), k)
    return k, [km[0:5], km[5:9], km[9:12]]


def case_shared(k=21):
    """(b) one k-mer X in two components, with different neighbours in each: linear in both, a branch point in the union"""
    rng = np.random.default_rng(7)
    x = _simple_path(rng, 1, k)
    a, b = "ACG" + x + "TCA", "GAT" + x + "CAG"          # (the bases next to X differ on both sides)
    return k, [kmers_of(a, k), kmers_of(b, k)]


def case_dense():
    """(c) all 512 canonical 5-mers dealt into 7 components, 30 of them given to a second component too"""
    k = 5
    rng = np.random.default_rng(5)
    allk = sorted({canon(x, k) for x in range(4 ** k)})
    assert len(allk) == 512
    where = rng.integers(0, 7, size=512)
    comps = [[] for _ in range(7)]
    for x, c in zip(allk, where):
        comps[c].append(x)
    for j in rng.choice(512, size=30, replace=False):
        comps[(where[j] + 1 + rng.integers(0, 6)) % 7].append(allk[j])
    return k, comps


def case_palindromes():
    """(d) k = 20: a palindromic k-mer inside a path, one as a whole component, one at the start of a path"""
    k = 20
    rng = np.random.default_rng(20)
    h = _rand_seq(rng, 10)
    p = h + rc_str(h)
    assert encode(p) == encode(rc_str(p))
    h2 = _rand_seq(rng, 10)
    p2 = h2 + rc_str(h2)
    return k, [kmers_of(_rand_seq(rng, 6) + p + _rand_seq(rng, 6), k), [encode(p)], kmers_of(p2 + _rand_seq(rng, 7), k)]


def case_shapes(k=21):
    """(e) a fork, a single k-mer, an isolated cycle (no sequence), a path with a member listed twice"""
    rng = np.random.default_rng(31)
    trunk = _simple_path(rng, 10, k)
    fork = sorted(set(kmers_of(trunk + "A" + _rand_seq(rng, 7), k) + kmers_of(trunk + "C" + _rand_seq(rng, 7), k)))
    single = kmers_of(_simple_path(rng, 1, k), k)
    while True:                                            # the 15 k-mers of a circular sequence of 15 bases
        circ = _rand_seq(rng, 15)
        cyc = kmers_of((circ * (k // 15 + 2))[:15 + k - 1], k)
        if len(set(cyc)) == 15:
            break
    path = kmers_of(_simple_path(rng, 9, k), k)
    dup = path[:4] + [path[3]] + path[4:]
    return k, [fork, single, cyc, dup]


def case_long(k=31):
    """(f) a path of 5 000 k-mers next to 50 small components"""
    rng = np.random.default_rng(5000)
    comps = [kmers_of(_simple_path(rng, 5000, k), k)]
    for _ in range(50):
        comps.append(kmers_of(_simple_path(rng, int(rng.integers(1, 41)), k), k))
    return k, comps


def case_many(k=31, n_comps=3000, length=60000):
    """(g) 3 000 components of 1-40 k-mers cut from one random sequence, in the sequence's order (where the drawn sizes add up to more
    than the sequence has, the cuts are scaled back: neighbouring components then share a k-mer now and then)"""
    rng = np.random.default_rng(3000)
    km = kmers_of(_simple_path(rng, length - k + 1, k), k)
    sizes = rng.integers(1, 41, size=n_comps)
    cum = np.concatenate([[0], np.cumsum(sizes)])
    scale = min(1.0, (len(km) - 40) / cum[-1])
    return k, [km[int(cum[i] * scale):int(cum[i] * scale) + int(sizes[i])] for i in range(n_comps)]


def case_singles(k=31, n=70000):
    """(h) more than 2^16 components: the k-mers of one sequence, a component each"""
    rng = np.random.default_rng(70000)
    return k, [[x] for x in kmers_of(_simple_path(rng, n, k), k)]
