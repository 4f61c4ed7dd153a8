// mf_unitig.h -- what the unitig builder (mf_unitig.hip) shares with the 128-bit front end (mf_wgraph.hip, NO-REFERENCE EXTENSION).
#pragma once
#include <functional>
#include "mf_common.h"
struct ut_arrays {
    const uint64_t *gk; const uint16_t *gv; uint64_t n; int k;
    const uint64_t *ghi;      // != nullptr: 2k-bit k-mers, k >= 32 (mf_wgraph.hip): gk = their low words, ghi = their high words, and the table is
                              // ASCENDING, so a k-mer's index orders like the k-mer (k_ut_ends compares indices)
    uint8_t *info; uint32_t *ridx; uint32_t *lidx;
    uint8_t *pal;             // even k only: 1 if the k-mer equals its reverse complement (else nullptr)
    uint64_t *node;           // per oriented node: successor on its path (low 32 bits, UT_NONE = none) | count << 32 |
                              // last base of the oriented k-mer << 48: everything a walk needs per hop in ONE 8-byte load
    const uint64_t *jump;     // per oriented node: where its chain leaves the node's partition + hops (k_ut_contract)
    uint32_t *starts;         // compacted list of start nodes
    unsigned int *n_starts;
};


// U2 .. U5 of mf_unitig.hip on a table of n good k-mers: `flags` launches the kernel(s) that fill A.info / A.ridx / A.lidx (/ A.pal) -- U1, the
// only step that looks k-mers up --, everything after works on node ids.  d_part_off / part_bits: the table's minimizer partitions (0: none).
// trace (may be nullptr; for the tests, mf_debug_unitigs): what the host saw on its way -- nothing is launched or copied for it.
// d_row_group (may be nullptr; mf_comp2seq.hip): a group id per table entry -- every written path gets the id of its START node's entry
// (mf_seqs::d_comp; the caller sets mf_seqs::n_groups).
struct mf_ut_trace {
    uint64_t n_starts;        // start nodes (walks of U3)
    uint64_t walk_rounds;     // launches of k_ut_walk1
    uint64_t doubled;         // 1: U3b ran, the segment cuts came from the entries (k_utd_*); 0: from k_ut_segments
    uint64_t entries;         // doubled: entry nodes
    uint64_t double_rounds;   // doubled: rounds of k_utd_double
    uint64_t longest;         // doubled: nodes of the longest path
    uint64_t candidates;      // paths counted by pass 0 of k_ut_ends (before the equal-case arbitration)
    uint64_t paths;           // paths written
    uint64_t seg_slots;       // segment slots allocated (k_ut_seg_bound)
};
int mf_ut_build(mf_ctx *ctx, const uint64_t *gk, const uint64_t *ghi, const uint16_t *gv, uint64_t n, int k, int part_bits, const uint64_t *d_part_off,
                int min_len, const std::function<int(const ut_arrays &)> &flags, mf_seqs **out, mf_ut_trace *trace = nullptr,
                const uint32_t *d_row_group = nullptr);
// the sequences in their output order on the host (mf_seqs_export); comp (may be nullptr): their component ids, where the sequences carry them
int mf_seqs_to_host_grouped(const mf_seqs *s, std::vector<uint8_t> &bases, std::vector<uint64_t> &off, std::vector<int32_t> &avg, std::vector<int32_t> &mn,
                            std::vector<int32_t> &mx, std::vector<uint32_t> *comp);
