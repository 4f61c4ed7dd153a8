// mf_kps.hip -- kmers-per-sample (src/tools/KmersPerSampleCounter.java:56-157) on the join core (mf_join.h): the cohort's k-mer x sample
// abundance table, as a resident matrix or streamed into the reference's text file.
//
// Passes:
//   union    per hash slice, MF_UNION_PRESENCE with add = 1 for every sample but the first, which adds count_first (0 = the reference: its
//            first file's map is the accumulator and is zeroed before it is iterated, :82-96, so file 0 brings keys and no increments)
//   select   mf_read_kps: n(x) >= thresh = N * percent / 100 in Java int arithmetic (:101); the pieces of all slices are sorted once:
//            M keys in ascending order, their n(x), column = rank
//   index    k_kps_index: 16-byte slots {key, n(x), column} at load <= 0.5, one compare-and-swap per key (the keys are distinct)
//   gather   k_kps_gather: one thread per entry of sample j, one read-only probe sequence, the count into the sample's row at the
//            found column (a table's keys are distinct: plain stores into a row zeroed beforehand)
//   text     k_kps_header (fixed width, "\t" + k bases per column); k_kps_widths + mf_scan + k_kps_format ("\t" + decimal, 2 .. 6
//            bytes a value, 64-bit offsets)
// The file form streams: one sample is loaded, gathered, formatted, downloaded and written before the next; the N x M matrix never
// exists and every file is read twice, as in the reference.
#include "mf_join.h"
#include "mf_kps.h"
#include <algorithm>

// ---------------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------------
// selected key i -> the first empty slot of its probe sequence: {key, n(x), column i}.  flags bit 1: the index is full (never with the
// capacity the host picks)
__global__ __launch_bounds__(256) void k_kps_index(mf_uslot *__restrict__ slots, uint64_t mask, const uint64_t *__restrict__ keys,
                                                   const uint16_t *__restrict__ ns, uint64_t m, unsigned int *__restrict__ flags) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t key = keys[i];
    uint64_t p = mf_hash64(key) & mask;
    for (uint64_t probe = 0; probe <= mask; probe++) {
        if (atomicCAS(reinterpret_cast<unsigned long long *>(&slots[p].key), (unsigned long long)MF_EMPTY, (unsigned long long)key) == (unsigned long long)MF_EMPTY) {
            *reinterpret_cast<uint64_t *>(&slots[p].cnt) = (uint64_t)ns[i] | (i << 32);
            return;
        }
        p = (p + 1) & mask;
    }
    atomicOr(flags, 2u);
}

// one sample's entries with count > thr into its row of the matrix (row[column] = count; a key that was not selected, or >= 2^62 -- the
// union pass has refused those -- is skipped)
__global__ __launch_bounds__(256) void k_kps_gather(const mf_uslot *__restrict__ slots, uint64_t mask, const uint64_t *__restrict__ keys,
                                                    const uint16_t *__restrict__ cnts, uint64_t n, int thr, uint16_t *__restrict__ row) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint16_t c = cnts[i];
        if ((int)c <= thr) continue;
        const uint64_t key = keys[i];
        if (key >= MF_STATS_KEY_LIMIT) continue;
        ulonglong2 raw;
        if (mf_join_find(slots, mask, mf_hash64(key), key, &raw) == MF_JOIN_NOT_FOUND) continue;
        row[raw.y >> 32] = c;
    }
}

// column i -> "\t" + ShortKmer.toString(key, k) at out[i * (k + 1)]  (A = 0, G = 1, C = 2, T = 3, first base in the top bits)
__global__ __launch_bounds__(256) void k_kps_header(const uint64_t *__restrict__ keys, uint64_t m, int k, uint8_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t key = keys[i];
    uint8_t *o = out + i * (uint64_t)(k + 1);
    o[0] = '\t';
    for (int q = 0; q < k; q++) o[1 + q] = (uint8_t)(0x54434741u >> (8u * (uint32_t)((key >> (2 * (k - 1 - q))) & 3ull)));   // "AGCT"
}

__device__ __forceinline__ uint32_t mf_kps_width(uint32_t v) { return 2u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u); }
// bytes of "\t" + decimal for every value of a row
__global__ __launch_bounds__(256) void k_kps_widths(const uint16_t *__restrict__ row, uint64_t m, uint32_t *__restrict__ w) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) w[i] = mf_kps_width(row[i]);
}
// value i -> "\t" + decimal at out[off[i]], off = the exclusive scan of the widths
__global__ __launch_bounds__(256) void k_kps_format(const uint16_t *__restrict__ row, const uint64_t *__restrict__ off, uint64_t m, uint8_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    uint32_t v = row[i];
    uint8_t *o = out + off[i];
    o[0] = '\t';
    for (uint32_t d = mf_kps_width(v) - 1u; d >= 1u; d--) { o[d] = (uint8_t)('0' + v % 10u); v /= 10u; }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
// the selected k-mers: ascending keys, n(x), and the index key -> column
struct kps_sel {
    uint64_t m = 0, cap = 0;
    mf_buf<uint64_t> keys; mf_buf<uint16_t> ns; mf_buf<mf_uslot> slots;
};

static int kps_check(const char *what, const void *ctx, const void *in, int n) {
    if (!ctx || (n > 0 && !in)) return mf_set_error("%s: NULL argument", what);
    if (n < 1) return mf_set_error("kmers-per-sample: no input files");
    if (n > MF_KPS_MAX_N) return mf_set_error("kmers-per-sample: %d input files, at most %d (the count is a Java short)", n, MF_KPS_MAX_N);
    return MF_OK;
}

static int kps_select(mf_ctx *ctx, const mf_join_get &get, int N, uint64_t total, int max_bad, int percent, int count_first, kps_sel &out) {
    const int thresh = kps_thresh(N, percent);
    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(plan_slices(ctx, total, &S, &cap));
    std::vector<uint32_t> add((size_t)N, 1u);
    add[0] = count_first ? 1u : 0u;
    mf_join_parts<uint64_t, uint16_t> parts;
    for (uint32_t s = 0; s < S; s++) {
        mf_buf<mf_uslot> slots; uint64_t nu = 0;
        MF_TRY(mf_join_union(ctx, get, N, max_bad, MF_UNION_PRESENCE, add.data(), S, s, cap, slots, &nu));
        MF_TRY(mf_join_read(ctx, slots.p, cap, nu, mf_read_kps{thresh}, parts));
    }
    mf_buf<uint64_t> keys; mf_buf<uint16_t> vals; uint64_t m = 0;
    MF_TRY(parts.concat(ctx, keys, vals, &m));
    if (m >= MF_JOIN_CURSOR_MAX)
        return mf_set_error("kmers-per-sample: %llu k-mers selected, at most 2^32 - 2 columns (raise -perc / --percent-present)", (unsigned long long)m);
    MF_TRY(out.keys.alloc(ctx, m)); MF_TRY(out.ns.alloc(ctx, m));
    if (m) MF_TRY(mf_sort_pairs(ctx, keys.p, vals.p, m, 62, out.keys.p, out.ns.p));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    keys.reset(); vals.reset();
    out.m = m;
    // the column index
    uint64_t icap = 2;
    while (icap < 2 * m) icap <<= 1;
    out.cap = icap;
    MF_TRY(out.slots.alloc(ctx, icap));
    mf_buf<unsigned int> flags; MF_TRY(flags.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(flags.p, 0, 4, ctx->stream));
    MF_HIP(hipMemsetAsync(out.slots.p, 0xFF, icap * sizeof(mf_uslot), ctx->stream));        // (every key word = MF_EMPTY)
    if (m) {
        mf_ktimer tm(ctx, "k_kps_index");
        k_kps_index<<<kps_grid(m), 256, 0, ctx->stream>>>(out.slots.p, icap - 1, out.keys.p, out.ns.p, m, flags.p);
    }
    return mf_join_flags(ctx, flags.p, "kmers-per-sample");
}

// sample j's row: zeroed, then filled from the sample's entries with count > max_bad
static int kps_gather(mf_ctx *ctx, const mf_join_get &get, int j, int max_bad, const kps_sel &sel, uint16_t *row) {
    if (sel.m) MF_HIP(hipMemsetAsync(row, 0, sel.m * 2, ctx->stream));
    return mf_join_pass(ctx, get, j, "kmers-per-sample: gather pass", [&](const mf_table *t) {
        if (!sel.m) return;
        mf_ktimer tm(ctx, "k_kps_gather");
        k_kps_gather<<<grid_for(ctx, t->n), 256, 0, ctx->stream>>>(sel.slots.p, sel.cap - 1, t->d_keys, t->d_counts, t->n, max_bad, row);
    });
}

// row[0 .. m) -> tx.out[0 .. *bytes) = "\t" + decimal per value (shared with the wide tool: mf_kps.h)
int kps_format(mf_ctx *ctx, const uint16_t *row, uint64_t m, kps_text &tx, uint64_t *bytes) {
    *bytes = 0;
    if (!m) return MF_OK;
    {
        mf_ktimer tm(ctx, "k_kps_widths");
        k_kps_widths<<<kps_grid(m), 256, 0, ctx->stream>>>(row, m, tx.w.p);
    }
    {
        mf_ktimer tm(ctx, "k_kps_scan");
        MF_TRY(mf_scan<1>(ctx, tx.w.p, tx.off.p, m, tx.total.p));
    }
    {
        mf_ktimer tm(ctx, "k_kps_format");
        k_kps_format<<<kps_grid(m), 256, 0, ctx->stream>>>(row, tx.off.p, m, tx.out.p);
    }
    uint64_t t = 0;
    MF_HIP(hipMemcpyAsync(&t, tx.total.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    if (t < 2 * m || t > m * MF_KPS_MAX_WIDTH) return mf_set_error("kmers-per-sample: %llu bytes of text for %llu values", (unsigned long long)t, (unsigned long long)m);
    *bytes = t;
    return MF_OK;
}
static int kps_header(mf_ctx *ctx, const uint64_t *keys, uint64_t m, int k, mf_buf<uint8_t> &out, uint64_t *bytes) {
    *bytes = m * (uint64_t)(k + 1);
    MF_TRY(out.alloc(ctx, *bytes));
    if (!m) return MF_OK;
    mf_ktimer tm(ctx, "k_kps_header");
    k_kps_header<<<kps_grid(m), 256, 0, ctx->stream>>>(keys, m, k, out.p);
    return MF_OK;
}

// device bytes -> the file, through two halves of the context's staging memory: a piece crosses while the one before it is written
int kps_write(mf_ctx *ctx, const uint8_t *d_src, uint64_t bytes, FILE *f, const char *path) {
    const size_t SLOT = (size_t)16 << 20;
    if (!bytes) return MF_OK;
    MF_TRY(mf_ensure_pin_pool(ctx, 8 * SLOT));                                 // (what the table writers of mf_io.hip ask for: one pool)
    uint8_t *slot[2] = {(uint8_t *)ctx->pin_pool, (uint8_t *)ctx->pin_pool + SLOT};
    const uint64_t np = (bytes + SLOT - 1) / SLOT;
    auto len = [&](uint64_t p) { return (size_t)std::min<uint64_t>(SLOT, bytes - p * SLOT); };
    MF_HIP(hipMemcpyAsync(slot[0], d_src, len(0), hipMemcpyDeviceToHost, ctx->stream));
    for (uint64_t p = 0; p < np; p++) {
        MF_HIP(hipStreamSynchronize(ctx->stream));
        if (p + 1 < np) MF_HIP(hipMemcpyAsync(slot[(p + 1) & 1], d_src + (p + 1) * SLOT, len(p + 1), hipMemcpyDeviceToHost, ctx->stream));
        if (fwrite(slot[p & 1], 1, len(p), f) != len(p)) { (void)hipStreamSynchronize(ctx->stream); return mf_set_error("can't write '%s'", path); }
    }
    return MF_OK;
}

// File.getName().replace(".kmers.bin", "") (:144): every occurrence goes, left to right, in one pass
std::string kps_row_name(const char *path) {
    std::string s(path);
    const size_t sl = s.rfind('/');
    if (sl != std::string::npos) s.erase(0, sl + 1);
    for (size_t q = 0; (q = s.find(".kmers.bin", q)) != std::string::npos;) s.erase(q, 10);
    return s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------------------------------------------------------
int kps_matrix_fits(mf_ctx *ctx, int n, uint64_t m) {
    size_t fr = 0, tot = 0;
    MF_HIP(hipMemGetInfo(&fr, &tot));
    const uint64_t room = ctx->opt_kps_matrix_bytes > 0 ? (uint64_t)ctx->opt_kps_matrix_bytes : (uint64_t)fr + mf_arena_idle(ctx);
    if (m && (uint64_t)n > room / 2 / m)
        return mf_set_error("kmers-per-sample: the count matrix of %d samples x %llu k-mers x 2 bytes does not fit the %llu bytes of free device memory: "
                            "select fewer k-mers with a higher -perc (--percent-present), or use the file form, which streams the rows",
                            n, (unsigned long long)m, (unsigned long long)room);
    return MF_OK;
}

extern "C" int mf_kmers_per_sample_tables(mf_ctx *ctx, mf_table *const *tables, int n, int max_bad, int percent, int count_first, mf_kps **out) {
    mf_range rng_("mf:kmers_per_sample");
    if (!out) return mf_set_error("mf_kmers_per_sample_tables: NULL argument");
    *out = nullptr;
    MF_TRY(kps_check("mf_kmers_per_sample_tables", ctx, tables, n));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    MF_TRY(tables_total(ctx, tables, n, "mf_kmers_per_sample_tables", &total));
    const mf_join_get get = mf_join_tables(tables);
    kps_sel sel;
    MF_TRY(kps_select(ctx, get, n, total, max_bad, percent, count_first, sel));
    MF_TRY(kps_matrix_fits(ctx, n, sel.m));
    std::unique_ptr<mf_kps> r(new mf_kps());
    r->ctx = ctx; r->n_samples = n; r->m = sel.m;
    MF_TRY(r->mat.alloc(ctx, (size_t)n * sel.m));
    for (int j = 0; j < n; j++) MF_TRY(kps_gather(ctx, get, j, max_bad, sel, r->mat.p + (uint64_t)j * sel.m));
    r->keys.swap(sel.keys); r->ns.swap(sel.ns);
    *out = r.release();
    return MF_OK;
}

extern "C" void mf_kps_destroy(mf_kps *r) {
    if (!r) return;
    (void)hipSetDevice(r->ctx->device);
    (void)hipStreamSynchronize(r->ctx->stream);
    delete r;
}

extern "C" int mf_kps_stats(const mf_kps *r, uint64_t *n_kmers, int *n_samples) {
    if (!r) return mf_set_error("mf_kps_stats: NULL argument");
    if (n_kmers) *n_kmers = r->m;
    if (n_samples) *n_samples = r->n_samples;
    return MF_OK;
}

extern "C" int mf_kps_device_view(const mf_kps *r, const void **d_keys, const void **d_nsamples, const void **d_matrix) {
    if (!r) return mf_set_error("mf_kps_device_view: NULL argument");
    if (r->wide_k) return mf_set_error("mf_kps_device_view: a result of k = %d holds two words a k-mer: call mf_kps_device_view_wide", r->wide_k);
    if (d_keys) *d_keys = r->keys.p;
    if (d_nsamples) *d_nsamples = r->ns.p;
    if (d_matrix) *d_matrix = r->mat.p;
    return MF_OK;
}

extern "C" int mf_kps_export(const mf_kps *r, uint64_t *keys, uint16_t *nsamples, uint16_t *matrix) {
    if (!r) return mf_set_error("mf_kps_export: NULL argument");
    if (r->wide_k) return mf_set_error("mf_kps_export: a result of k = %d holds two words a k-mer: call mf_kps_export_wide", r->wide_k);
    mf_ctx *ctx = r->ctx;
    MF_HIP(hipSetDevice(ctx->device));
    if (r->m) {
        if (keys) MF_HIP(hipMemcpyAsync(keys, r->keys.p, r->m * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (nsamples) MF_HIP(hipMemcpyAsync(nsamples, r->ns.p, r->m * 2, hipMemcpyDeviceToHost, ctx->stream));
        if (matrix) MF_HIP(hipMemcpyAsync(matrix, r->mat.p, (size_t)r->n_samples * r->m * 2, hipMemcpyDeviceToHost, ctx->stream));
    }
    MF_HIP(hipStreamSynchronize(ctx->stream));
    return MF_OK;
}

// copies min(bytes, cap) == bytes or nothing
static int kps_text_out(mf_ctx *ctx, const uint8_t *d_text, uint64_t bytes, uint8_t *text, uint64_t cap, uint64_t *n) {
    *n = bytes;
    if (cap < bytes || !bytes) return MF_OK;
    MF_HIP(hipMemcpyAsync(text, d_text, bytes, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    return MF_OK;
}

extern "C" int mf_kps_header_text(const mf_kps *r, int k, uint8_t *text, uint64_t cap, uint64_t *n) {
    if (!r || !n || (cap && !text)) return mf_set_error("mf_kps_header_text: NULL argument");
    if (r->wide_k && k != r->wide_k) return mf_set_error("mf_kps_header_text: k = %d, the result holds k-mers of k = %d", k, r->wide_k);
    if (!r->wide_k && (k < 1 || k > 31)) return mf_set_error("k must be in [1,31]");
    mf_ctx *ctx = r->ctx;
    MF_HIP(hipSetDevice(ctx->device));
    *n = r->m * (uint64_t)(k + 1);
    if (cap < *n) return MF_OK;                          // (the size alone: the caller comes again with room)
    mf_buf<uint8_t> d; uint64_t bytes = 0;
    if (r->wide_k) MF_TRY(mf_wkps_header(ctx, r->hi.p, r->lo.p, r->m, k, d, &bytes));
    else MF_TRY(kps_header(ctx, r->keys.p, r->m, k, d, &bytes));
    return kps_text_out(ctx, d.p, bytes, text, cap, n);
}

extern "C" int mf_kps_row_text(const mf_kps *r, int sample, uint8_t *text, uint64_t cap, uint64_t *n) {
    if (!r || !n || (cap && !text)) return mf_set_error("mf_kps_row_text: NULL argument");
    if (sample < 0 || sample >= r->n_samples) return mf_set_error("mf_kps_row_text: sample %d of %d", sample, r->n_samples);
    mf_ctx *ctx = r->ctx;
    MF_HIP(hipSetDevice(ctx->device));
    kps_text tx; uint64_t bytes = 0;
    MF_TRY(tx.alloc(ctx, r->m));
    MF_TRY(kps_format(ctx, r->mat.p + (uint64_t)sample * r->m, r->m, tx, &bytes));
    return kps_text_out(ctx, tx.out.p, bytes, text, cap, n);
}

extern "C" int mf_kmers_per_sample(mf_ctx *ctx, const char *const *files, int n, int k, int percent, int count_first, const char *out_txt,
                                   uint64_t *n_kmers) {
    mf_range rng_("mf:kmers_per_sample(files)");
    if (!out_txt) return mf_set_error("mf_kmers_per_sample: NULL argument");
    MF_TRY(kps_check("mf_kmers_per_sample", ctx, files, n));
    if (k < 1 || k > 31) return mf_set_error("k must be in [1,31]");
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    MF_TRY(file_records(files, n, &total));
    const mf_join_get get = mf_join_files(files, 0, k);            // IOUtils.loadKmers(file, 0), :78 and :140
    kps_sel sel;
    MF_TRY(kps_select(ctx, get, n, total, 0, percent, count_first, sel));
    FILE *f = fopen(out_txt, "w");
    if (!f) return mf_set_error("Couldn't open output file '%s'", out_txt);
    auto run = [&]() -> int {
        {
            mf_buf<uint8_t> hdr; uint64_t bytes = 0;
            MF_TRY(kps_header(ctx, sel.keys.p, sel.m, k, hdr, &bytes));
            MF_TRY(kps_write(ctx, hdr.p, bytes, f, out_txt));
        }
        fputc('\n', f);
        mf_buf<uint16_t> row; MF_TRY(row.alloc(ctx, sel.m));
        kps_text tx; MF_TRY(tx.alloc(ctx, sel.m));
        for (int j = 0; j < n; j++) {
            MF_TRY(kps_gather(ctx, get, j, 0, sel, row.p));
            uint64_t bytes = 0;
            MF_TRY(kps_format(ctx, row.p, sel.m, tx, &bytes));
            const std::string name = kps_row_name(files[j]);
            fwrite(name.data(), 1, name.size(), f);
            MF_TRY(kps_write(ctx, tx.out.p, bytes, f, out_txt));
            fputc('\n', f);
        }
        return MF_OK;
    };
    const int rc = run();
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || (bad && rc == MF_OK)) return mf_set_error("can't write '%s'", out_txt);
    if (rc == MF_OK && n_kmers) *n_kmers = sel.m;
    return rc;
}
