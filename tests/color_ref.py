"""Independent restatement of kmers-color (src/tools/ColorKmersMain.java:89-136, src/algo/ColoredKmerOperations.java) and of the default
and --separate modes of component-colored (src/tools/ColoredComponentMain.java:83-119, src/algo/ColoredComponentsBuilder.java:85-124,
250-280) in numpy / plain Python, written from the Java; it shares no code with the library.  tests/test_color_cpu.py pins it with
hand-worked cases.

A sample is its .kmers.bin records (keys uint64[n], counts int16[n]), duplicates allowed.  A coloured table is (ascending keys uint64[n],
packed values as Python ints / uint64).  Components are lists of ascending k-mer lists."""
import functools
import struct

import numpy as np

POWER = 20
FIELD_MAX = (1 << POWER) - 1
LONG_MAX = (1 << 63) - 1
MAX_COUNT = 32767
STAT_HEADER = "# component.no\tcomponent.size\tcomponent.weight\tcomponent.color\n"


# ---- the packed value ----
def get_value(value, color):
    return (int(value) >> (color * POWER)) & FIELD_MAX


def add_value(value, color, add=1):
    new = min(get_value(value, color) + int(add), FIELD_MAX)
    return (int(value) & ~(FIELD_MAX << (color * POWER))) | (new << (color * POWER))


def pack(f0, f1, f2):
    return int(f0) | (int(f1) << POWER) | (int(f2) << (2 * POWER))


def get_color(value, perc):
    """the first colour whose share is >= perc, else -1; IEEE double division, 0 / 0 = NaN compares false"""
    f = [np.float64(get_value(value, c)) for c in range(3)]
    s = np.float64(get_value(value, 0) + get_value(value, 1) + get_value(value, 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(3):
            if f[c] / s >= np.float64(perc):
                return c
    return -1


# ---- kmers-color ----
def load_sample(sample, b):
    """IOUtils.loadKmers([file], b): records with value > b, duplicates of a key summed with saturation at 32767"""
    k = np.asarray(sample[0], dtype=np.uint64)
    c = np.asarray(sample[1]).astype(np.int16).astype(np.int64)
    m = c > b
    uk, inv = np.unique(k[m], return_inverse=True)
    s = np.zeros(len(uk), dtype=np.int64)
    np.add.at(s, inv, c[m])
    return uk, np.minimum(s, MAX_COUNT)


def kmers_color(samples, classes, b=1, val=False):
    """-> (ascending keys uint64, packed values uint64); one add per (sample, key), each saturating"""
    if len(samples) != len(classes):
        raise ValueError("one class per sample")
    if len(samples) > 1024:
        raise ValueError("more than 1024 samples")
    table = {}
    for sample, cl in zip(samples, classes):
        if cl not in (0, 1, 2):
            raise ValueError("class %r" % (cl,))
        keys, sums = load_sample(sample, b)
        for key, v in zip(keys.tolist(), sums.tolist()):
            if key >= 1 << 62:
                raise ValueError("key >= 2^62")
            table[key] = add_value(table.get(key, 0), cl, v if val else 1)
    keys = np.array(sorted(table), dtype=np.uint64)
    return keys, np.array([table[int(k)] for k in keys], dtype=np.uint64)


def ctable_to_bytes(keys, values):
    a = np.empty(len(keys), dtype=np.dtype([("k", ">u8"), ("v", ">u8")]))
    a["k"] = keys
    a["v"] = values
    return a.tobytes()


def ctable_from_bytes(raw):
    a = np.frombuffer(raw, dtype=np.dtype([("k", ">u8"), ("v", ">i8")]))
    return a["k"].astype(np.uint64), a["v"].astype(np.int64)


def stat_txt(values):
    vals, cnt = np.unique(np.asarray(values, dtype=np.uint64), return_counts=True)
    return "# k-mer frequency\tnumber of such k-mers\n" + "".join("%d\t%d\n" % (int(v), int(c)) for v, c in zip(vals, cnt)) + "\n"


# ---- component-colored ----
def load_long(files, min_value):
    """IOUtils.loadLongKmers: files = [(keys uint64, signed values int64)]; records with value > min_value, duplicates added with
    saturation at 2^63 - 1 -> dict key -> value"""
    hm = {}
    for keys, vals in files:
        for key, v in zip(np.asarray(keys, dtype=np.uint64).tolist(), np.asarray(vals, dtype=np.int64).tolist()):
            if v > min_value:
                hm[key] = min(hm.get(key, 0) + v, LONG_MAX)
    return hm


_CODE = {"A": 0, "G": 1, "C": 2, "T": 3}


def encode(s):
    x = 0
    for ch in s:
        x = (x << 2) | _CODE[ch]
    return x


def rc(x, k):
    """reverse complement: the 2-bit letters in reverse order, each turned into 3 - letter (A <-> T, G <-> C)"""
    x = ~x & 0xFFFFFFFFFFFFFFFF
    x = ((x >> 2) & 0x3333333333333333) | ((x & 0x3333333333333333) << 2)
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0F) | ((x & 0x0F0F0F0F0F0F0F0F) << 4)
    x = int.from_bytes(x.to_bytes(8, "little"), "big")
    return x >> (64 - 2 * k)


def canon(x, k):
    return min(x, rc(x, k))


def kmers_of(seq, k):
    return sorted({canon(encode(seq[i:i + k]), k) for i in range(len(seq) - k + 1)})


@functools.lru_cache(maxsize=None)
def neighbours(x, k):
    """KmerOperations.possibleNeighbours: the four right and four left extensions, canonical"""
    mask = (1 << (2 * k)) - 1
    out = []
    for nuc in range(4):
        out.append(canon(((x << 2) | nuc) & mask, k))
        out.append(canon((x >> 2) | (nuc << (2 * k - 2)), k))
    return out


def _components(vertices, k):
    """connected components of the subgraph induced by `vertices` (a set) -> list of ascending lists"""
    seen, comps = set(), []
    for start in sorted(vertices):
        if start in seen:
            continue
        seen.add(start)
        stack, comp = [start], []
        while stack:
            v = stack.pop()
            comp.append(v)
            for u in neighbours(v, k):
                if u in vertices and u not in seen:
                    seen.add(u)
                    stack.append(u)
        comps.append(sorted(comp))
    return comps


def colored_components(hm, k, n_groups=3, separate=False, perc=0.9):
    """-> [components of colour 0, ... n_groups - 1], each ordered by size descending, then smallest k-mer"""
    color = {key: get_color(v, perc) for key, v in hm.items()}
    for key, c in color.items():
        if c >= n_groups:
            raise ValueError("k-mer %d has colour %d, n_groups = %d" % (key, c, n_groups))
    out = []
    for c in range(n_groups):
        own = {key for key, cc in color.items() if cc == c}
        if separate:
            comps = _components(own, k)
        else:
            comps = [comp for comp in _components(own | {key for key, cc in color.items() if cc == -1}, k) if any(x in own for x in comp)]
        comps.sort(key=lambda comp: (-len(comp), comp[0]))
        out.append(comps)
    return out


def components_bytes(comps):
    """SequenceComponent.saveComponents: int count, per component int size, long weight (= size), the k-mers; big-endian"""
    raw = [struct.pack(">i", len(comps))]
    for comp in comps:
        raw.append(struct.pack(">iq", len(comp), len(comp)))
        raw.append(np.asarray(comp, dtype=">u8").tobytes())
    return b"".join(raw)


def components_stat(per_colour):
    out, no = [STAT_HEADER], 0
    for c, comps in enumerate(per_colour):
        for comp in comps:
            no += 1
            out.append("%d\t%d\t%d\t%d\n" % (no, len(comp), len(comp), c))
    return "".join(out)
