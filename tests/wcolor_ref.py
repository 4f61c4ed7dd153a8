"""Restatement of kmers-color and of the default and --separate modes of component-colored in plain Python integers, for any k <= 63: written
from the Java (src/tools/ColorKmersMain.java:89-136, src/algo/ColoredKmerOperations.java, src/tools/ColoredComponentMain.java:83-119,
src/algo/ColoredComponentsBuilder.java:85-124, 250-280, src/algo/KmerOperations.java:9-26) and from DESIGN.md section 7c.  It shares no code with
the library and none with tests/color_ref.py, which tests/test_wcolor_cpu.py ties it to at k = 21 and 31.

A k-mer is a Python int of 2k bits (A0 G1 C2 T3, the first base in the most significant bits); a sample is {k-mer: count}; a coloured table is
{k-mer: packed value}; the components of a colour are ascending lists of k-mers."""
import struct

FIELD_BITS = 20
FIELD_MAX = (1 << FIELD_BITS) - 1
LONG_MAX = (1 << 63) - 1
MASK64 = (1 << 64) - 1
MAX_SAMPLES = 1024
STAT_HEADER = "# component.no\tcomponent.size\tcomponent.weight\tcomponent.color\n"
LETTERS = "AGCT"


# ---- k-mers ----
def encode(s):
    x = 0
    for ch in s:
        x = (x << 2) | LETTERS.index(ch)
    return x


def decode(x, k):
    return "".join(LETTERS[(x >> (2 * (k - 1 - i))) & 3] for i in range(k))


def revcomp(x, k):
    """the letters in reverse order, each turned into 3 - letter"""
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def canonical(x, k):
    return min(x, revcomp(x, k))


def kmers_of(seq, k):
    return sorted({canonical(encode(seq[i:i + k]), k) for i in range(len(seq) - k + 1)})


def neighbours(x, k):
    """KmerOperations.possibleNeighbours: the four right and the four left extensions, canonical"""
    mask = (1 << (2 * k)) - 1
    out = []
    for nuc in range(4):
        out.append(canonical(((x << 2) | nuc) & mask, k))
        out.append(canonical((x >> 2) | (nuc << (2 * k - 2)), k))
    return out


# ---- the packed value ----
def field(value, c):
    return (value >> (FIELD_BITS * c)) & FIELD_MAX


def add_value(value, c, add=1):
    """ColoredKmerOperations.addValue: the field of class c grows by `add`, clamped at 2^20 - 1; the other fields stay"""
    new = min(field(value, c) + add, FIELD_MAX)
    return (value & ~(FIELD_MAX << (FIELD_BITS * c))) | (new << (FIELD_BITS * c))


def pack(f0, f1, f2):
    return f0 | (f1 << FIELD_BITS) | (f2 << (2 * FIELD_BITS))


def get_color(value, perc):
    """ColoredKmerOperations.getColor: the first class whose share (double)f_c / (double)(f_0 + f_1 + f_2) is >= perc, else -1.  A Python float is an
    IEEE double and int / int conversions below 2^53 are exact; 0.0 / 0.0 is NaN in Java, which compares false"""
    f = [field(value, c) for c in range(3)]
    total = float(f[0] + f[1] + f[2])
    if total == 0.0:
        return -1
    for c in range(3):
        if float(f[c]) / total >= float(perc):
            return c
    return -1


# ---- kmers-color ----
def kmers_color(samples, classes, b=1, val=False):
    """sample j of class c_j holds x iff its count is > b; each (sample, k-mer) adds 1 (val: its count) to the field of c_j -> {k-mer: value}"""
    if len(samples) != len(classes):
        raise ValueError("one class per sample")
    if len(samples) > MAX_SAMPLES:
        raise ValueError("more than 1024 samples")
    if b < 0:
        raise ValueError("maximal-bad-frequency must not be negative")
    for c in classes:
        if c not in (0, 1, 2):
            raise ValueError("class %r" % (c,))
    table = {}
    for t, c in zip(samples, classes):
        for x, n in t.items():
            if n > b:
                table[x] = add_value(table.get(x, 0), c, n if val else 1)
    return table


def table_bytes(table):
    """the wide colored_kmers.kmers.bin: 24-byte big-endian records (high word, low word, value) of the entries with value > 0, ascending"""
    return b"".join(struct.pack(">QQq", x >> 64, x & MASK64, v) for x, v in sorted(table.items()) if v > 0)


def table_from_bytes(raw):
    """-> [(k-mer, signed value)] in file order; ValueError when the size is no multiple of the record"""
    if len(raw) % 24:
        raise ValueError("size %d is not a multiple of the 24-byte record" % len(raw))
    out = []
    for o in range(0, len(raw), 24):
        h, l, v = struct.unpack(">QQq", raw[o:o + 24])
        out.append(((h << 64) | l, v))
    return out


def stat_text(table):
    """the .stat.txt of a coloured table: its distinct values ascending with the number of k-mers of each"""
    hist = {}
    for v in table.values():
        hist[v] = hist.get(v, 0) + 1
    return "# k-mer frequency\tnumber of such k-mers\n" + "".join("%d\t%d\n" % (v, hist[v]) for v in sorted(hist)) + "\n"


def load_long(files, min_value, k=None):
    """IOUtils.loadLongKmers: files = lists of (k-mer, signed value); the records with value > min_value, the values of a k-mer added with
    saturation at 2^63 - 1 -> {k-mer: value}"""
    hm = {}
    for recs in files:
        for x, v in recs:
            if k is not None and x >> (2 * k):
                raise ValueError("k-mer does not fit 2k bits")
            if v > min_value:
                hm[x] = min(hm.get(x, 0) + v, LONG_MAX)
    return hm


# ---- component-colored ----
def _components(vertices, k):
    """connected components of the graph induced by `vertices` (a set) -> ascending lists"""
    seen, comps = set(), []
    for start in sorted(vertices):
        if start in seen:
            continue
        seen.add(start)
        todo, comp = [start], []
        while todo:
            v = todo.pop()
            comp.append(v)
            for u in neighbours(v, k):
                if u in vertices and u not in seen:
                    seen.add(u)
                    todo.append(u)
        comps.append(sorted(comp))
    return comps


def colors_of(table, perc):
    return {x: get_color(v, perc) for x, v in table.items()}


def colored_components(table, k, n_groups=3, separate=False, perc=0.9):
    """-> [the components of colour 0, ... n_groups - 1], each list ordered by size descending, then smallest k-mer.  --separate: the
    components of the k-mers of colour c; default: the components of (colour c or neutral) that hold a k-mer of colour c"""
    color = colors_of(table, perc)
    for x in sorted(color):
        if color[x] >= n_groups:
            raise ValueError("k-mer %s has colour %d, but n_groups = %d" % (decode(x, k), color[x], n_groups))
    neutral = {x for x, c in color.items() if c == -1}
    out = []
    for c in range(n_groups):
        own = {x for x, cc in color.items() if cc == c}
        if separate:
            comps = _components(own, k)
        else:
            comps = [comp for comp in _components(own | neutral, k) if any(x in own for x in comp)]
        comps.sort(key=lambda comp: (-len(comp), comp[0]))
        out.append(comps)
    return out


def components_words(comps):
    """-> (sizes, weights, hi, lo) as tests/wide_files_ref.encode_components takes them: size = weight = k-mers"""
    sizes = [len(c) for c in comps]
    members = [x for c in comps for x in c]
    return sizes, sizes, [x >> 64 for x in members], [x & MASK64 for x in members]


def components_stat(per_colour):
    out, no = [STAT_HEADER], 0
    for c, comps in enumerate(per_colour):
        for comp in comps:
            no += 1
            out.append("%d\t%d\t%d\t%d\n" % (no, len(comp), len(comp), c))
    return "".join(out)
