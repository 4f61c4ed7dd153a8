"""component-paths for any k <= 63 on Python integers (no reference exists for k > 31): the scan of tests/component_paths_ref.py --
one set per component, per sequence the `first` / `cur` loop of scan_plain -- on the k-mers of tests/wseq2comp_ref.py.  What follows
the scan (the min-length rule, the cap, the stable sort, Java's rounding, the file text) is component_paths_ref.component_paths itself,
given these runs: it reads only size and weight from a component.  A component is (members as ints, size, weight)."""
import component_paths_ref as P
import wseq2comp_ref as W

MAX_PATHS_COUNT = P.MAX_PATHS_COUNT


def find_runs(comps, k, files):
    """-> per component (all of them) [(dna, first, cur)] in encounter order: file, record, position"""
    comp_kmers = [set(int(x) for x in c[0]) for c in comps]
    runs = [[] for _ in comps]
    for seqs in files:
        for dna in seqs:
            dna = dna.upper()
            kmers = W.occurrences(dna, k)
            if not kmers:
                continue
            for i in range(len(comps)):
                if not comp_kmers[i].isdisjoint(kmers):    # (no hit, no run: the scan itself is skipped, nothing else)
                    runs[i] += [(dna, first, cur) for first, cur in P.scan_plain(kmers, comp_kmers[i])]
    return runs


def component_paths(comps, k, files, selection=None, min_len=50, max_paths=MAX_PATHS_COUNT, runs=None):
    """-> ({file name: bytes}, numbers of the components whose count reached max_paths)"""
    if runs is None:
        runs = find_runs(comps, k, files)
    return P.component_paths(comps, k, files, selection=selection, min_len=min_len, max_paths=max_paths, runs=runs)
