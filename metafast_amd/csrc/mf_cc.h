// mf_cc.h -- what the component cutter (mf_cc.hip) shares with the 128-bit front end (mf_wgraph.hip, NO-REFERENCE EXTENSION).
#pragma once
#include <functional>
#include <vector>
#include "mf_common.h"
// what one threshold level of mf_cc_build did, for the tests (mf_debug_components): which kernels saw the level and what they left behind
struct mf_cc_level {
    int thr = 0;
    int sparse = 0;                     // the level ran on the list of the survivors (k_ccs_init / k_cc_hook over the list / k_ccs_stats)
    uint64_t visited = 0;               // threads of the per-vertex kernels: n (dense) or the length of the list
    uint64_t ecount0 = 0, ecount1 = 0;  // dense: edges to smaller tiles that k_cc_hook_tile counted into the list; tiles whose edges the list does not hold
    uint32_t nkept = 0, nkm = 0, nbig = 0, na = 0;     // kept components, their vertices, oversize components, vertices that go on to thr + 1
    int want_list = 0, list_stands = 0; // k_cc_members was given a list to write; the next level runs on it
};
// C2 .. C5 of mf_cc.hip on n vertices: `adjacency` launches the kernel(s) that fill nbr[8 n] (C1, the only step that looks k-mers up: vertex
// ids of the 8 neighbours or 0xFFFFFFFF); d_keys: the vertices' k-mers (members, tie-break by the smallest) -- nullptr: the table is
// ascending, the vertex id stands for the k-mer (the components' d_kmers then hold ids).  trace != nullptr: one record per threshold
// level is appended (the only extra work: the edge counters of a dense level are read back).
int mf_cc_build(mf_ctx *ctx, uint64_t n, int k, const uint16_t *d_counts, const uint64_t *d_keys, int b1, int b2,
                const std::function<int(uint32_t *)> &adjacency, mf_comps **out, std::vector<mf_cc_level> *trace = nullptr);
// component-colored in the same shape: d_code[n] = a vertex's colour code (1 + colour, 4 = neutral), adjacency and d_keys as
// above; out[n_groups], one mf_comps per colour (size = weight = k-mers; size descending, then the smallest k-mer / vertex id)
int mf_cc_colored_build(mf_ctx *ctx, uint64_t n, int k, const uint16_t *d_code, const uint64_t *d_keys, int n_groups, int separate,
                        const std::function<int(uint32_t *)> &adjacency, mf_comps **out);
// packed values d_vals[n] -> d_code[n] (ColoredKmerOperations.getColor; k_color_classify); *d_first = the smallest position whose colour is not
// below n_groups, ~0: none.  Queued on the context's stream
int mf_color_classify_launch(mf_ctx *ctx, const uint64_t *d_vals, uint64_t n, double perc, int n_groups, uint16_t *d_code, unsigned long long *d_first);
