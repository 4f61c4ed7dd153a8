"""The cohorts and graphs of the wide (k = 32 ... 63) kmers-color and component-colored tests.  tests/test_wcolor_cpu.py asserts on the restatement
(tests/wcolor_ref.py) what makes each of them a test; tests/test_wcolor_gpu.py runs the library on them."""
import numpy as np

import wcolor_ref as R
import wkmersets_cases as WC
import wstats_cases as SC

KS = (32, 33, 63)
MAX_BADS = (0, 2)
COUNTS = np.array([1, 2, 3, 5, 17, 250, 4000, 32767])


def _fresh(rng, k, n, taken):
    mask = (1 << (2 * k)) - 1
    out = []
    while len(out) < n:
        x = R.canonical(int.from_bytes(rng.bytes(16), "big") & mask, k)
        if x not in taken:
            taken.add(x)
            out.append(x)
    return out


def random_cohort(k, n_samples, n_kmers=300, base=6):
    """`base` distinct samples (fewer where N is smaller), repeated to fill the cohort, classes 0, 1, 2 in turn: a k-mer leans to one class, to
    none, or is rare; counts of 1, 2, 3 (max_bad and max_bad + 1 for max_bad = 0 and 2) and 32767 among them.  -> (samples, classes)"""
    rng = np.random.default_rng(4000 + 131 * k + n_samples)
    keys = _fresh(rng, k, n_kmers, set())
    nb = min(base, n_samples)
    lean = rng.integers(0, 5, n_kmers)                      # 0, 1, 2: that class; 3: every class; 4: rare
    distinct = []
    for j in range(nb):
        p = np.where(lean == j % 3, 0.9, np.where(lean == 3, 0.6, np.where(lean == 4, 0.05, 0.03)))
        has = rng.random(n_kmers) < p
        c = rng.choice(COUNTS, n_kmers, p=[0.1, 0.15, 0.15, 0.2, 0.2, 0.1, 0.07, 0.03])
        distinct.append({keys[i]: int(c[i]) for i in range(n_kmers) if has[i]})
    return [distinct[j % nb] for j in range(n_samples)], [j % nb % 3 for j in range(n_samples)]


def crafted(k, max_bad=2):
    """-> (samples, classes, names).  Seven samples: classes 0 0 1 1 2 2 and an empty one of class 1.  The k-mers: the smallest and the largest
    canonical one, the keys on both sides of every slice border of S = 3 and 7, a pair that differs in the low word only and one in the high word
    only (k = 32 has no high word: in its top bit), counts of exactly max_bad and max_bad + 1, and a filling of k-mers for every field"""
    rng = np.random.default_rng(5000 + k)
    b = max_bad
    samples = [dict() for _ in range(7)]
    classes = [0, 0, 1, 1, 2, 2, 1]
    names = {}

    def put(name, x, counts):
        assert len(counts) == 6 and x not in names.values()
        names[name] = x
        for t, c in zip(samples, counts):
            if c:
                t[x] = c

    taken = set()
    top = WC.largest_canonical(k)
    lo_x, lo_y = WC._pair(rng, k, 2)
    hi_x, hi_y = WC._pair(rng, k, 64) if k > 32 else WC._pair(rng, k, 63)
    borders = sorted(set(SC.border_keys(k, 3) + SC.border_keys(k, 7)))
    taken.update([0, top, lo_x, lo_y, hi_x, hi_y], borders)
    put("smallest", 0, [b + 1, 0, 0, 9, 0, 0])
    put("largest", top, [0, 0, b + 5, 0, 7, 32767])
    put("lo_x", lo_x, [3, 3, 0, 0, 0, 0])
    put("lo_y", lo_y, [0, 0, 3, 3, 0, 0])
    put("hi_x", hi_x, [0, 0, 0, 0, 4, 4])
    put("hi_y", hi_y, [5, 0, 5, 0, 5, 0])
    f = _fresh(rng, k, 30, taken)
    # a count of exactly max_bad is no presence, one of max_bad + 1 is
    put("at_max_bad", f[0], [b, b + 1, b, b + 1, b, b + 1] if b else [0, 1, 0, 1, 0, 1])
    put("only_low", f[1], [b, 0, 0, b, 0, 0])               # (max_bad = 0: in no sample at all)
    for i, x in enumerate(borders):
        put("border%d" % i, x, [(3 + i) if (i + j) % 3 else 0 for j in range(6)])
    for i, x in enumerate(f[2:]):
        put("fill%d" % i, x, [int(COUNTS[(i + j) % 8]) if (i >> (j // 2)) & 1 or i % 7 == j else 0 for j in range(6)])
    names["borders"] = borders
    return samples, classes, names


# ---- graphs: coloured tables whose k-mers come from sequences ----
def _dna(rng, n):
    return "".join(rng.choice(list(R.LETTERS), n))


def genomes(k, seed=0):
    """three genomes of two contigs each.  Contig 1 = own + a stretch two genomes share + own + a stretch all three share + own; contig 2 is the
    genome's own.  -> [[contig, contig], ...]"""
    rng = np.random.default_rng(6000 + 17 * k + seed)
    own = lambda: _dna(rng, 8)
    s01, s12, s02, s012 = (_dna(rng, k + 2) for _ in range(4))
    return [[own() + s01 + own() + s012 + own() + s02 + own(), _dna(rng, k + 6)],
            [own() + s01 + own() + s012 + own() + s12 + own(), _dna(rng, k + 6)],
            [own() + s12 + own() + s012 + own() + s02 + own(), _dna(rng, k + 6)]]


def graph(k, seed=0, count=1):
    """the coloured table of the three genomes as samples of class 0, 1, 2 (max_bad = 0): a k-mer of one genome has one field, one of a shared
    stretch two or three"""
    gs = genomes(k, seed)
    samples = [{x: count for contig in g for x in R.kmers_of(contig, k)} for g in gs]
    return R.kmers_color(samples, [0, 1, 2], b=0, val=True)


def restrict(table, n_groups, perc):
    """the entries whose colour is below n_groups (a table that n_groups < 3 accepts)"""
    return {x: v for x, v in table.items() if R.get_color(v, perc) < n_groups}


PATH_COLOURS = (0, 0, -1, 1, 1, -1, -1, 0)
VALUE_OF = {0: R.pack(5, 0, 0), 1: R.pack(0, 5, 0), 2: R.pack(0, 0, 5), -1: R.pack(1, 1, 0)}


def path(k=33):
    """a sequence of k + 7 bases: eight k-mers in a row, coloured 0, 0, neutral, 1, 1, neutral, neutral, 0 (perc = 0.9) -> (k-mers in path order,
    table)"""
    rng = np.random.default_rng(7100 + k)
    seq = _dna(rng, k + 7)
    xs = [R.canonical(R.encode(seq[i:i + k]), k) for i in range(8)]
    return xs, {x: VALUE_OF[c] for x, c in zip(xs, PATH_COLOURS)}


PAL_COLOURS = (0, 0, 0, -1, 1, 1, 1)


def palindrome_path():
    """k = 32: three bases, a 32-mer that is its own reverse complement, three bases -- seven k-mers in a row, the middle one the palindrome,
    coloured 0, 0, 0, neutral, 1, 1, 1 -> (k-mers in path order, table)"""
    pal = "ACGGTCAATTGACCGT" + "ACGGTCAATTGACCGT"
    seq = "GAC" + pal + "CAG"
    xs = [R.canonical(R.encode(seq[i:i + 32]), 32) for i in range(7)]
    return xs, {x: VALUE_OF[c] for x, c in zip(xs, PAL_COLOURS)}
