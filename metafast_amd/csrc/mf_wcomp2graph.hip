// mf_wcomp2graph.hip -- NO-REFERENCE EXTENSION (32 <= k <= 63): comp2graph on wide components -- the GFA of every component of a wide
// components.bin in one pass.  The semantics are those of mf_comp2graph.hip on 2k-bit k-mers, rule for rule, because the steps are the same
// code:
//
//   rows, pair index, k_wc2s_flags     mf_wcomp2seq.hip (mf_wc2s.h), unchanged; the flags pass is launched directly, on an ut_arrays of this
//                                      file (gk = the rows' low words, ghi = their high words)
//   links .. text                      mf_c2g.h (c2g_build), shared with the k <= 31 tool; its three k-mer reading kernels are instantiated here
//                                      over c2g_wide_keys: a k-mer is an mf_u128 of two row words, the reverse complement is mf_wrevcomp, a
//                                      base's shift addresses either word, the successor look-up is wc2s_find (both words and the component
//                                      are compared behind a matching tag)
//   k_c2g_wvalues                      the value pass over a wide sample table's index (mf_windex_find)
//
// Every device loop ends by construction: the pair index and a wide table's index have load <= 0.5, so a probe meets an empty slot; the
// cycle walks and the pointer doubling, with its round bound, are mf_c2g.h's.
#include <memory>
#include "mf_c2g.h"
#include "mf_wc2s.h"

struct c2g_wide_keys {
    typedef mf_u128 kmer;
    wc2s_index ix;
    __device__ __forceinline__ kmer oriented(uint32_t node, int k) const {
        const kmer x = ((kmer)ix.hi[node >> 1] << 64) | (kmer)ix.lo[node >> 1];
        return (node & 1u) ? mf_wrevcomp(x, k) : x;
    }
    // the last base of rc(x) is the complement of x's first
    __device__ __forceinline__ uint32_t last(uint32_t node, int k) const {
        if (!(node & 1u)) return (uint32_t)ix.lo[node >> 1] & 3u;
        const int sh = 2 * k - 2;
        return 3u - ((uint32_t)(sh >= 64 ? ix.hi[node >> 1] >> (sh - 64) : ix.lo[node >> 1] >> sh) & 3u);
    }
    __device__ static __forceinline__ uint32_t base(kmer y, int sh) { return (uint32_t)(sh >= 64 ? (uint64_t)(y >> 64) >> (sh - 64) : (uint64_t)y >> sh) & 3u; }
    __device__ static __forceinline__ kmer kmask(int k) { return (((kmer)1) << (2 * k)) - 1; }
    __device__ static __forceinline__ kmer revcomp(kmer y, int k) { return mf_wrevcomp(y, k); }
    __device__ __forceinline__ bool find(kmer cz, uint32_t c, uint32_t *row) const { *row = wc2s_find(ix, cz, c); return *row != C2S_NONE; }
};
struct c2g_wide_rows {
    typedef c2g_wide_keys keys;
    const wc2s_rows &R;
    mf_buf<unsigned long long> slots; wc2s_index ix{};
    explicit c2g_wide_rows(const wc2s_rows &r) : R(r) {}
    uint64_t n() const { return R.n; }
    const uint32_t *comp() const { return R.comp.p; }
    int index(mf_ctx *ctx, int) { return wc2s_pair_index(ctx, R, slots, &ix); }
    int flags(mf_ctx *ctx, ut_arrays &A) {
        A.gk = R.lo.p; A.ghi = R.hi.p; A.gv = R.cnt.p;
        return wc2s_flags_launch(ctx, ix, A);
    }
    keys get() const { return keys{ix}; }
};

// one sample: coverage = 0 adds 1 where the sample holds the k-mer, else its count
__global__ __launch_bounds__(256) void k_c2g_wvalues(mf_windex_view ix, const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint64_t n, int coverage,
                                                     uint32_t *__restrict__ val) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint32_t p = mf_windex_find(ix, hi[r], lo[r]);
    if (p == 0xFFFFFFFFu) return;
    const uint32_t cnt = ix.cnt[p];
    if (cnt == 0) return;
    val[r] = c2g_add_value(val[r], cnt, coverage);
}

static int wc2g_add_sample(mf_ctx *ctx, mf_wtable *t, const wc2s_rows &R, int k, int coverage, uint32_t *val) {
    if (t->ctx != ctx) return mf_set_error("comp2graph: a sample table belongs to another context");
    if (t->k != k) return mf_set_error("comp2graph: a sample table has k = %d, the components k = %d", t->k, k);
    if (!t->n || !R.n) return MF_OK;
    MF_TRY(mf_wtable_ensure_index(t));
    mf_ktimer tm(ctx, "k_c2g_values");
    k_c2g_wvalues<<<wc2s_grid(R.n), 256, 0, ctx->stream>>>(mf_wtable_view(t), R.hi.p, R.lo.p, R.n, coverage, val);
    return MF_OK;
}
static int wc2g_check_samples(const char *what, int n) {
    if (n > MF_MAX_COUNT) return mf_set_error("comp2graph: %d %s (they are counted in a 16-bit value, as for k <= 31: at most %d)", n, what, MF_MAX_COUNT);
    return MF_OK;
}

extern "C" int mf_wcomps_graph_device(mf_ctx *ctx, mf_wcomps *c, mf_wtable *const *samples, int n_samples, int coverage, mf_gfa **out) {
    mf_range rng_("mf:comp2graph_wide");
    if (!ctx || !c || !out) return mf_set_error("mf_wcomps_graph_device: NULL argument");
    *out = nullptr;
    if (c->ctx != ctx) return mf_set_error("mf_wcomps_graph_device: the components belong to another context");
    MF_TRY(wc2s_check_k("mf_wcomps_graph_device", c->k));
    if (n_samples < 0 || (n_samples > 0 && !samples)) return mf_set_error("mf_wcomps_graph_device: %d sample tables at NULL", n_samples);
    MF_TRY(wc2g_check_samples("samples", n_samples));
    MF_TRY(wc2s_member_count("comp2graph", c));
    MF_HIP(hipSetDevice(ctx->device));
    const int k = c->k;
    wc2s_rows R;
    MF_TRY(wc2s_build_rows(ctx, c, R));
    mf_buf<uint32_t> val;
    MF_TRY(c2g_values_first(ctx, R.n, n_samples ? 0u : 1u, val));
    for (int j = 0; j < n_samples; j++) {
        if (!samples[j]) return mf_set_error("comp2graph: sample table %d is NULL", j);
        MF_TRY(wc2g_add_sample(ctx, samples[j], R, k, coverage, val.p));
    }
    mf_gfa *g = new mf_gfa; g->ctx = ctx;
    c2g_wide_rows src(R);
    const int rc = c2g_build(ctx, src, val.p, c->n, k, g);
    if (rc < 0) { mf_gfa_destroy(g); return rc; }
    *out = g;
    return MF_OK;
}

// ---- the file form ----
extern "C" int mf_comp2graph_wide(mf_ctx *ctx, const char *components_bin, int k, const char *const *kmers_files, int n_files, int coverage, const char *out_gfa,
                                  uint64_t *n_components, uint64_t *n_segments, uint64_t *n_links) {
    mf_range rng_("mf:comp2graph_wide(files)");
    if (!ctx || !components_bin || !out_gfa) return mf_set_error("mf_comp2graph_wide: NULL argument");
    MF_TRY(wc2s_check_k("mf_comp2graph_wide", k));
    if (n_files < 0 || (n_files > 0 && !kmers_files)) return mf_set_error("mf_comp2graph_wide: %d k-mers files at NULL", n_files);
    MF_TRY(wc2g_check_samples("k-mers files", n_files));
    mf_wcomps *c = nullptr;
    MF_TRY(mf_wcomps_load(ctx, components_bin, k, &c));      // (a file of another width or another k stops here, before anything is written)
    std::unique_ptr<mf_wcomps, void (*)(mf_wcomps *)> gc(c, mf_wcomps_destroy);
    MF_TRY(wc2s_member_count("comp2graph", c));
    MF_HIP(hipSetDevice(ctx->device));
    wc2s_rows R;
    MF_TRY(wc2s_build_rows(ctx, c, R));
    mf_buf<uint32_t> val;
    MF_TRY(c2g_values_first(ctx, R.n, n_files > 0 ? 0u : 1u, val));
    // as mf_comp2graph: -cov: one table of all files, counts added and bounded; else the number of files whose own table holds the k-mer.
    // One sample is resident at a time.
    for (int j = 0; j < (n_files > 0 ? (coverage ? 1 : n_files) : 0); j++) {
        mf_wtable *t = nullptr;
        MF_TRY(mf_wtable_load_kmers(ctx, kmers_files + (coverage ? 0 : j), coverage ? n_files : 1, 0, k, &t));
        const int rc = wc2g_add_sample(ctx, t, R, k, coverage, val.p);
        if (rc == MF_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) { mf_wtable_destroy(t); return mf_set_error("comp2graph: hipStreamSynchronize failed"); }
        mf_wtable_destroy(t);
        MF_TRY(rc);
    }
    mf_gfa g; g.ctx = ctx;
    c2g_text_guard gt{g};
    c2g_wide_rows src(R);
    MF_TRY(c2g_build(ctx, src, val.p, c->n, k, &g));
    MF_TRY(c2g_write_text(ctx, g, out_gfa));
    if (n_components) *n_components = c->n;
    if (n_segments) *n_segments = g.n_segments;
    if (n_links) *n_links = g.n_links;
    return MF_OK;
}
