"""component-paths restated in plain Python from src/tools/ComponentPathsMain.java:82-206, on purpose in the reference's own shape: a
loop over the selected components, per component a set of its k-mers, per sequence a scan with `first` / `cur`, the cap on add, a
stable sort by length (descending), Java's rounding of the average weight, and the files as Sequence.printSequences writes them.
O(components x bases), like the reference.  k-mers: ShortKmer.toLong() = min(forward, reverse complement), A0 G1 C2 T3
(seq2comp_ref.occurrences).  Stated deviations of the library, restated here: a component number twice gives its one file (the
reference writes it twice, same bytes), a number out of range and an average weight that does not fit an int are errors.

The scan is there twice: scan_plain, the reference's loop k-mer by k-mer, and find_runs, the same runs of ALL components over whole
files with numpy (one table lookup per component and position instead of one set probe: still O(components x bases), a hundred times
faster) for the randomised GPU test; tests/test_component_paths_cpu.py holds the two against each other.  What follows the scan --
checkAndAddPath, the cap, the sort, the files -- is one piece of code for both."""
import math

import numpy as np

import comp2seq_ref as CR
import seq2comp_ref as S

MAX_PATHS_COUNT = 10 ** 6


def java_round(x):
    """Math.round(double): floor(x + 0.5) -- 2.5 -> 3, where Python's round gives 2"""
    return math.floor(x + 0.5)


def read_files(paths):
    """the sequences of every file, file by file (the readers of seq2comp_ref)"""
    return [S.read_files([p])[0] for p in paths]


def scan_plain(kmers, comp_kmers):
    """:138-157, one sequence on one component -> [(first, cur)]: the runs, `cur` one past the last position"""
    runs = []
    first, cur = -1, 0
    for kmer in kmers:
        if kmer in comp_kmers:
            if first == -1:
                first = cur
        elif first != -1:
            runs.append((first, cur))
            first = -1
        cur += 1
    if first != -1:
        runs.append((first, cur))
    return runs


def find_runs_plain(comps, k, files):
    """-> per component (all of them) [(dna, first, cur)] in encounter order: file, record, position"""
    comp_kmers = [set(int(x) for x in c[0]) for c in comps]
    runs = [[] for _ in comps]
    for seqs in files:
        for dna in seqs:
            dna = dna.upper()
            kmers = [int(x) for x in S.occurrences(dna, k)]
            for i in range(len(comps)):
                runs[i] += [(dna, first, cur) for first, cur in scan_plain(kmers, comp_kmers[i])]
    return runs


def find_runs(comps, k, files):
    """find_runs_plain with numpy: per file the k-mers of all sequences in one array (as places in the sorted list of all members, or
    none), per component one boolean table over that list; a run starts where the position before is no hit or belongs to another
    sequence"""
    universe = np.unique(np.concatenate([np.asarray(c[0], dtype=np.uint64) for c in comps] + [np.zeros(0, np.uint64)]))
    member_ids = [np.searchsorted(universe, np.asarray(c[0], dtype=np.uint64)) for c in comps]
    runs = [[] for _ in comps]
    for seqs in files:
        seqs = [s.upper() for s in seqs]
        occ = [S.occurrences(s, k) for s in seqs]
        allk = np.concatenate(occ + [np.zeros(0, np.uint64)])
        if not len(allk) or not len(universe):
            continue
        seq_of = np.repeat(np.arange(len(seqs)), [len(o) for o in occ])
        start_of = np.zeros(len(seqs) + 1, dtype=np.int64)
        start_of[1:] = np.cumsum([len(o) for o in occ])
        at = np.minimum(np.searchsorted(universe, allk), len(universe) - 1)
        ids = np.where(universe[at] == allk, at, len(universe))           # the last table entry: never a member
        table = np.zeros(len(universe) + 1, dtype=bool)
        for i in range(len(comps)):
            table[member_ids[i]] = True
            hit = np.flatnonzero(table[ids])
            table[member_ids[i]] = False
            if not len(hit):
                continue
            brk = np.flatnonzero((np.diff(hit) != 1) | (seq_of[hit[1:]] != seq_of[hit[:-1]]))
            firsts = hit[np.concatenate([[0], brk + 1])]
            lasts = hit[np.concatenate([brk, [len(hit) - 1]])]
            for f, l in zip(firsts.tolist(), lasts.tolist()):
                s = int(seq_of[f])
                runs[i].append((seqs[s], f - int(start_of[s]), l + 1 - int(start_of[s])))
    return runs


def component_paths(comps, k, files, selection=None, min_len=50, max_paths=MAX_PATHS_COUNT, runs=None):
    """comps: [(members, size, weight)] as seq2comp_ref.components gives them (numbered from 1 in this order); files: a list of
    lists of sequences, one per sequence file; selection: component numbers, or None for all; runs: what find_runs or
    find_runs_plain gave for these components, k and files (None: find_runs_plain) -> ({file name: bytes}, numbers of the
    components whose count reached max_paths)"""
    if selection is None:
        used = list(range(1, len(comps) + 1))                  # allComps.toArray(usedComps)
    else:
        used = []
        for no in selection:
            if no < 1 or no > len(comps):
                raise IndexError(f"there is no component {no}")       # allComps.get(no - 1) throws
            used.append(int(no))
    if runs is None:
        runs = find_runs_plain(comps, k, files)
    ans = [[] for _ in used]
    for i in range(len(used)):
        for dna, first, cur in runs[used[i] - 1]:
            _check_and_add_path(dna, first, cur, ans[i], comps[used[i] - 1], k, min_len, max_paths)
    reached = [used[i] for i in range(len(used)) if len(ans[i]) == max_paths]      # :163
    out = {}
    for i in range(len(used)):
        ans[i].sort(key=lambda s: -len(s[0]))                  # Collections.sort is stable: ties keep encounter order
        out[f"component-{used[i]}.seq.fasta"] = CR.seq_fasta(ans[i]).encode()
    return out, reached


def _check_and_add_path(dna, first, cur, ans, comp, k, min_len, max_paths):
    """:192-206"""
    length = cur - first - 1 + k
    if length >= min_len:
        w = java_round(comp[2] / float(comp[1]))
        if not -2 ** 31 <= w < 2 ** 31:
            raise OverflowError("the average k-mer weight does not fit an int")
        if len(ans) < max_paths:
            ans.append((dna[first:first + length], w, 0, 0))
