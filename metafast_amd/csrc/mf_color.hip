// mf_color.hip -- kmers-color (src/tools/ColorKmersMain.java:89-136, src/algo/ColoredKmerOperations.java) on the join core (mf_join.h;
// DESIGN.md section 7c): the slot's 64-bit payload IS the packed value -- three 20-bit fields, class c in bits 20c .. 20c + 19 -- and a
// sample's entry adds 1 (or its value, -val) to its class's field with the reference's saturation (MF_UNION_COLOR).  Read-out, one sort
// by key; the result is an mf_ctable (mf_ctable.hip), whose writer makes the distinct-value histogram for the .stat.txt.
#include "mf_join.h"

#define MF_COLOR_MAX_N 1024

static int color_check(int n, const int *classes, int max_bad) {
    if (n > MF_COLOR_MAX_N) return mf_set_error("kmers-color: %d samples, at most %d (a field of the packed value holds 20 bits)", n, MF_COLOR_MAX_N);
    if (max_bad < 0) return mf_set_error("kmers-color: maximal-bad-frequency = %d is negative", max_bad);
    for (int j = 0; j < n; j++)
        if (classes[j] < 0 || classes[j] > 2) return mf_set_error("kmers-color: sample %d has class %d (the classes are 0, 1 and 2)", j, classes[j]);
    return MF_OK;
}

static int color_join(mf_ctx *ctx, const mf_join_get &get, int N, const int *classes, uint64_t total, int b, int count_values, int k, mf_ctable **out) {
    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(plan_slices(ctx, total, &S, &cap));
    std::vector<uint32_t> add((size_t)N);
    for (int j = 0; j < N; j++) add[(size_t)j] = (uint32_t)classes[j] | (count_values ? 4u : 0u);
    mf_join_parts<uint64_t, uint64_t> parts;
    for (uint32_t s = 0; s < S; s++) {
        mf_buf<mf_uslot> slots; uint64_t nu = 0;
        MF_TRY(mf_join_union(ctx, get, N, b, MF_UNION_COLOR, add.data(), S, s, cap, slots, &nu));
        MF_TRY(mf_join_read(ctx, slots.p, cap, nu, mf_read_color{}, parts));
    }
    mf_buf<uint64_t> keys, vals; uint64_t n = 0;
    MF_TRY(parts.concat(ctx, keys, vals, &n));
    if (n > MF_JOIN_CURSOR_MAX) return mf_set_error("kmers-color: %llu k-mers, at most 2^32 - 1", (unsigned long long)n);
    // one sort by key
    mf_buf<uint64_t> sk, sv;
    MF_TRY(sk.alloc(ctx, n)); MF_TRY(sv.alloc(ctx, n));
    if (n) MF_TRY(mf_sort_u64_u64(ctx, keys.p, vals.p, n, 62, sk.p, sv.p));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    const size_t kb = sk.bytes(), vb = sv.bytes();
    return mf_ctable_adopt(ctx, k, n, sk.take(), kb, sv.take(), vb, out);
}

extern "C" int mf_kmers_color_tables(mf_ctx *ctx, mf_table *const *t, const int *classes, int n, int max_bad, int count_values, mf_ctable **out) {
    mf_range rng_("mf:kmers_color");
    if (!ctx || !out || n < 0 || (n && (!t || !classes))) return mf_set_error("mf_kmers_color_tables: NULL argument");
    *out = nullptr;
    MF_TRY(color_check(n, classes, max_bad));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    MF_TRY(tables_total(ctx, t, n, "mf_kmers_color_tables", &total));
    const int k = n ? t[0]->k : 31;
    return color_join(ctx, mf_join_tables(t), n, classes, total, max_bad, count_values, k, out);
}

extern "C" int mf_kmers_color(mf_ctx *ctx, const char *const *files, const int *classes, int n, int max_bad, int count_values, int k,
                              const char *kmers_bin, const char *stat_txt, uint64_t *n_kmers) {
    mf_range rng_("mf:kmers_color(files)");
    if (!ctx || !kmers_bin || n < 0 || (n && (!files || !classes))) return mf_set_error("mf_kmers_color: NULL argument");
    if (k < 1 || k > 31) return mf_set_error("k must be in [1,31]");
    MF_TRY(color_check(n, classes, max_bad));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    MF_TRY(file_records(files, n, &total));
    mf_ctable *t = nullptr;
    MF_TRY(color_join(ctx, mf_join_files(files, max_bad, k), n, classes, total, max_bad, count_values, k, &t));
    uint64_t w = 0;
    const int rc = mf_ctable_write(t, kmers_bin, stat_txt, &w);
    mf_ctable_destroy(t);
    if (rc == MF_OK && n_kmers) *n_kmers = w;
    return rc;
}
