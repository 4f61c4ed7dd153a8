// mf_comp2graph.hip -- comp2graph for k <= 31: the compacted de Bruijn graph of every component of a components.bin as GFA text, all
// components in one pass (ComponentsToGraph.java:70-130, Comp2Graph.java, GFAWriter.java).
//
//   rows, pair index, k_c2s_flags      mf_comp2seq.hip (mf_c2s.h), unchanged
//   links .. text                      mf_c2g.h (c2g_build), shared with the wide tool (mf_wcomp2graph.hip); here: how a 64-bit row is read
//                                      (c2g_narrow_keys), the value pass over a sample table's index (k_c2g_values) and the entry points
#include "mf_c2g.h"

int mf_table_ensure_index(mf_table *t);

// the rows' k-mers as the kernels of mf_c2g.h read them
struct c2g_narrow_keys {
    typedef uint64_t kmer;
    const uint64_t *key; const mf_uslot *slots; uint64_t mask;
    __device__ __forceinline__ kmer oriented(uint32_t node, int k) const {
        const uint64_t x = key[node >> 1];
        return (node & 1u) ? mf_revcomp(x, k) : x;
    }
    __device__ __forceinline__ uint32_t last(uint32_t node, int k) const { return (uint32_t)oriented(node, k) & 3u; }
    __device__ static __forceinline__ uint32_t base(kmer y, int sh) { return (uint32_t)(y >> sh) & 3u; }
    __device__ static __forceinline__ kmer kmask(int k) { return (1ull << (2 * k)) - 1; }
    __device__ static __forceinline__ kmer revcomp(kmer y, int k) { return mf_revcomp(y, k); }
    __device__ __forceinline__ bool find(kmer cz, uint32_t c, uint32_t *row) const { return c2s_find(slots, mask, cz, c, row); }
};
struct c2g_narrow_rows {
    typedef c2g_narrow_keys keys;
    const c2s_rows &R;
    mf_buf<mf_uslot> slots; uint64_t cap = 0;
    explicit c2g_narrow_rows(const c2s_rows &r) : R(r) {}
    uint64_t n() const { return R.n; }
    const uint32_t *comp() const { return R.comp.p; }
    int index(mf_ctx *ctx, int k) { return c2s_pair_index(ctx, R, k, slots, &cap); }
    int flags(mf_ctx *ctx, ut_arrays &A) {
        A.gk = R.key.p; A.gv = R.cnt.p;
        return c2s_flags_launch(ctx, slots.p, cap, R, A);
    }
    keys get() const { return keys{R.key.p, slots.p, cap - 1}; }
};

// one sample: coverage = 0 adds 1 where the sample holds the k-mer, else its count
__global__ __launch_bounds__(256) void k_c2g_values(mf_index_view ix, const uint64_t *__restrict__ key, uint64_t n, int coverage, uint32_t *__restrict__ val) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    uint32_t idx, cnt;
    if (!mf_index_find(ix, key[r], &idx, &cnt) || cnt == 0) return;
    val[r] = c2g_add_value(val[r], cnt, coverage);
}

static int c2g_add_sample(mf_ctx *ctx, mf_table *t, const c2s_rows &R, int k, int coverage, uint32_t *val) {
    if (t->ctx != ctx) return mf_set_error("comp2graph: a sample table belongs to another context");
    if (t->k != k) return mf_set_error("comp2graph: a sample table has k = %d, the components k = %d", t->k, k);
    if (!t->n || !R.n) return MF_OK;
    MF_TRY(mf_table_ensure_index(t));
    mf_ktimer tm(ctx, "k_c2g_values");
    k_c2g_values<<<c2s_grid(R.n), 256, 0, ctx->stream>>>(mf_view(t->index), R.key.p, R.n, coverage, val);
    return MF_OK;
}

// val = first (1 without samples: every member k-mer is worth 1; 0 with them), then every resident sample added
static int c2g_values_of(mf_ctx *ctx, const c2s_rows &R, int k, uint32_t first, mf_table *const *samples, int n_samples, int coverage, mf_buf<uint32_t> &val) {
    MF_TRY(c2g_values_first(ctx, R.n, first, val));
    for (int j = 0; samples && j < n_samples; j++) {
        if (!samples[j]) return mf_set_error("comp2graph: sample table %d is NULL", j);
        MF_TRY(c2g_add_sample(ctx, samples[j], R, k, coverage, val.p));
    }
    return MF_OK;
}

extern "C" void mf_gfa_destroy(mf_gfa *g) {
    if (!g) return;
    if (g->d_text) mf_release(g->ctx, g->d_text, g->text_bytes);
    delete g;
}
extern "C" int mf_gfa_stats(const mf_gfa *g, uint64_t *n_segments, uint64_t *n_links, uint64_t *n_cycles, uint64_t *n_bytes) {
    if (!g) return mf_set_error("gfa is NULL");
    if (n_segments) *n_segments = g->n_segments;
    if (n_links) *n_links = g->n_links;
    if (n_cycles) *n_cycles = g->n_cycles;
    if (n_bytes) *n_bytes = g->n_bytes;
    return MF_OK;
}
extern "C" int mf_gfa_text(const mf_gfa *g, uint8_t *text, uint64_t cap, uint64_t *n) {
    if (!g) return mf_set_error("gfa is NULL");
    if (n) *n = g->n_bytes;
    if (!text || cap < g->n_bytes || !g->n_bytes) return MF_OK;
    MF_HIP(hipSetDevice(g->ctx->device));
    MF_HIP(hipMemcpyAsync(text, g->d_text, g->n_bytes, hipMemcpyDeviceToHost, g->ctx->stream));
    MF_HIP(hipStreamSynchronize(g->ctx->stream));
    return MF_OK;
}

extern "C" int mf_comps_graph_device(mf_ctx *ctx, mf_comps *c, mf_table *const *samples, int n_samples, int coverage, mf_gfa **out) {
    mf_range rng_("mf:comp2graph");
    if (!ctx || !c || !out) return mf_set_error("mf_comps_graph_device: NULL argument");
    *out = nullptr;
    if (c->ctx != ctx) return mf_set_error("mf_comps_graph_device: the components belong to another context");
    if (c->k == 0) return mf_set_error("mf_comps_graph_device: these components do not know their k (they were loaded from a file): mf_comps_set_k first");
    MF_TRY(c2s_check_k(c->k));
    if (n_samples < 0 || (n_samples > 0 && !samples)) return mf_set_error("mf_comps_graph_device: %d sample tables at NULL", n_samples);
    if (n_samples > MF_MAX_COUNT) return mf_set_error("comp2graph: %d samples (the reference counts them in a Java short: at most %d)", n_samples, MF_MAX_COUNT);
    MF_HIP(hipSetDevice(ctx->device));
    const int k = c->k;
    c2s_rows R;
    MF_TRY(c2s_build_rows(ctx, c, k, R));
    mf_buf<uint32_t> val;
    MF_TRY(c2g_values_of(ctx, R, k, n_samples ? 0u : 1u, samples, n_samples, coverage, val));
    mf_gfa *g = new mf_gfa; g->ctx = ctx;
    c2g_narrow_rows src(R);
    const int rc = c2g_build(ctx, src, val.p, c->n, k, g);
    if (rc < 0) { mf_gfa_destroy(g); return rc; }
    *out = g;
    return MF_OK;
}

// ---- the file form ----
extern "C" int mf_comp2graph(mf_ctx *ctx, const char *components_bin, int k, const char *const *kmers_files, int n_files, int coverage, const char *out_gfa,
                             uint64_t *n_components, uint64_t *n_segments, uint64_t *n_links) {
    mf_range rng_("mf:comp2graph(files)");
    if (!ctx || !components_bin || !out_gfa) return mf_set_error("mf_comp2graph: NULL argument");
    MF_TRY(c2s_check_k(k));
    if (n_files < 0 || (n_files > 0 && !kmers_files)) return mf_set_error("mf_comp2graph: %d k-mers files at NULL", n_files);
    if (n_files > MF_MAX_COUNT) return mf_set_error("comp2graph: %d k-mers files (the reference counts them in a Java short: at most %d)", n_files, MF_MAX_COUNT);
    mf_comps *c = nullptr;
    MF_TRY(mf_comps_load(ctx, components_bin, &c));
    struct guard { mf_comps *p; ~guard() { mf_comps_destroy(p); } } gc{c};
    if (c->k != 0 && c->k != k) return mf_set_error("mf_comp2graph: k = %d, the components of %s were built with k = %d", k, components_bin, c->k);
    MF_HIP(hipSetDevice(ctx->device));
    c2s_rows R;
    MF_TRY(c2s_build_rows(ctx, c, k, R));
    mf_buf<uint32_t> val;
    MF_TRY(c2g_values_of(ctx, R, k, n_files > 0 ? 0u : 1u, nullptr, 0, coverage, val));
    if (n_files > 0) {
        // ComponentsToGraph.java:85-102: -cov: one map of all files, IOUtils.loadKmers(files, 0) -- counts added and bounded; else the
        // number of files whose own map holds the k-mer.  One sample is resident at a time.
        for (int j = 0; j < (coverage ? 1 : n_files); j++) {
            mf_table *t = nullptr; uint64_t sum = 0;
            MF_TRY(mf_table_load_kmers_sum(ctx, kmers_files + (coverage ? 0 : j), coverage ? n_files : 1, 0, k, &t, &sum));
            const int rc = c2g_add_sample(ctx, t, R, k, coverage, val.p);
            if (rc == MF_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) { mf_table_destroy(t); return mf_set_error("comp2graph: hipStreamSynchronize failed"); }
            mf_table_destroy(t);
            MF_TRY(rc);
        }
    }
    mf_gfa g; g.ctx = ctx;
    c2g_text_guard gt{g};
    c2g_narrow_rows src(R);
    MF_TRY(c2g_build(ctx, src, val.p, c->n, k, &g));
    MF_TRY(c2g_write_text(ctx, g, out_gfa));
    if (n_components) *n_components = c->n;
    if (n_segments) *n_segments = g.n_segments;
    if (n_links) *n_links = g.n_links;
    return MF_OK;
}
