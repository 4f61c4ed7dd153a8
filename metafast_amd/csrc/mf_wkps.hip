// mf_wkps.hip -- NO-REFERENCE EXTENSION (32 <= k <= 63): kmers-per-sample on 2k-bit k-mers, the definition of mf_kmers_per_sample_tables
// (KmersPerSampleCounter.java:56-157) carried over to (hi, lo) keys on the wide join core (mf_wjoin.h).
//   union    per slice of the key range, mf_wjoin_slice_union with WEIGHTS: every sample brings 1 per k-mer it holds with count > max_bad, the
//            first one count_first -- the sum over a run of equal k-mers is n(x), and a k-mer of sample 0 alone is there with n = 0
//   select   the k-mers with n(x) >= thresh = N * percent / 100 (Java int arithmetic), order kept (mf_wjoin_select); the slices are ascending
//            ranges of the key, so their selections one after the other are the M columns in ascending order, for every number of slices
//   gather   k_wkps_gather: one thread per entry of sample j with count > max_bad, a binary search on two words in the M selected k-mers,
//            the count into the sample's row at the found column (a table's keys are distinct: plain stores into a row zeroed beforehand)
//   text     k_wkps_header ("\t" + k bases per column, fixed width); the rows by the narrow tool's formatter (kps_format, mf_kps.h)
// The file form streams as the narrow one does: a sample is loaded, gathered, formatted, downloaded and written before the next.
#include "mf_kps.h"
#include "mf_wjoin.h"
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

// ---------------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------------
// one sample's entries with count > thr into its row of the matrix: row[column] = count, column = the k-mer's place in the ascending selected
// k-mers (shi, slo)[m].  A k-mer that was not selected is skipped; the column of one that was is below m by the search itself.
__global__ __launch_bounds__(256) void k_wkps_gather(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, const uint16_t *__restrict__ cnt, uint64_t n, int thr,
                                                     const uint64_t *__restrict__ shi, const uint64_t *__restrict__ slo, uint64_t m, uint16_t *__restrict__ row) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint16_t c = cnt[i];
        if ((int)c <= thr) continue;
        const uint64_t h = hi[i], l = lo[i];
        uint64_t a = 0, e = m;
        while (a < e) {
            const uint64_t mid = a + (e - a) / 2, mh = shi[mid];
            if (mh < h || (mh == h && slo[mid] < l)) a = mid + 1; else e = mid;
        }
        if (a < m && shi[a] == h && slo[a] == l) row[a] = c;
    }
}

// column i -> "\t" + the k bases of (hi, lo)[i] at out[i * (k + 1)]  (A = 0, G = 1, C = 2, T = 3, first base in the top bits of the 2k-bit value:
// base q stands at bit 2 (k - 1 - q), in the high word while that is >= 64 -- an even number, so no base straddles the words; k = 32 has no high word)
__global__ __launch_bounds__(256) void k_wkps_header(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint64_t m, int k, uint8_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t h = hi[i], l = lo[i];
    uint8_t *o = out + i * (uint64_t)(k + 1);
    o[0] = '\t';
    for (int q = 0; q < k; q++) {
        const int sh = 2 * (k - 1 - q);
        const uint64_t two = sh >= 64 ? h >> (sh - 64) : l >> sh;
        o[1 + q] = (uint8_t)(0x54434741u >> (8u * (uint32_t)(two & 3ull)));   // "AGCT"
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
static unsigned wkps_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 0x7FFFFFFFull); }

// the selected k-mers: ascending (hi, lo), n(x); column = place
struct wkps_sel { uint64_t m = 0; mf_buf<uint64_t> hi, lo; mf_buf<uint16_t> ns; };

static int wkps_check(const char *what, const void *ctx, const void *in, int n) {
    if (!ctx || (n > 0 && !in)) return mf_set_error("%s: NULL argument", what);
    if (n < 1) return mf_set_error("%s: kmers-per-sample needs at least one sample, got %d", what, n);
    if (n > MF_KPS_MAX_N) return mf_set_error("%s: kmers-per-sample: %d samples, at most %d (the number of samples of a k-mer is a Java short)", what, n, MF_KPS_MAX_N);
    return MF_OK;
}
// an error of the join core or of a loader, with the tool's name in front
static int wkps_named(int rc) {
    if (rc >= 0) return rc;
    const std::string e = mf_last_error();
    return mf_set_error("kmers-per-sample (--wide-kmers): %s", e.c_str());
}

static int wkps_select(mf_ctx *ctx, int k, const mf_wjoin_get &get, int N, uint64_t total, int max_bad, int percent, int count_first, wkps_sel &out) {
    hipStream_t st = ctx->stream;
    // n(x) >= thresh as "n(x) > thr" on 0 <= n(x) <= 32767: thresh <= 0 takes every candidate, and no end of the int range is stepped over
    const int thresh = kps_thresh(N, percent);
    const int thr = thresh <= 0 ? -1 : std::min(thresh, MF_KPS_MAX_N + 1) - 1;
    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(wkps_named(mf_wjoin_plan(ctx, total, &S, &cap)));
    std::vector<uint16_t> weight((size_t)N, (uint16_t)1);
    weight[0] = count_first ? 1 : 0;
    struct part { mf_buf<uint64_t> hi, lo; mf_buf<uint16_t> ns; uint64_t n = 0; };
    std::vector<std::unique_ptr<part>> parts;
    uint64_t m = 0;
    for (uint32_t s = 0; s < S; s++) {
        mf_wjoin_union u;
        MF_TRY(wkps_named(mf_wjoin_slice_union(ctx, k, get, N, max_bad, S, s, cap, u, weight.data())));
        if (!u.n) continue;
        auto p = std::make_unique<part>();
        MF_TRY(mf_wjoin_select(ctx, u.hi.p, u.lo.p, u.sum.p, u.sum.p, u.n, thr, p->hi, p->lo, p->ns, nullptr, &p->n));
        m += p->n;
        if (m >= 0xFFFFFFFFull)
            return mf_set_error("kmers-per-sample: %llu k-mers selected, at most 2^32 - 2 columns (raise -perc / --percent-present)", (unsigned long long)m);
        if (p->n) parts.push_back(std::move(p));
    }
    // one ascending list: the slices are ranges of the key, in ascending order
    if (parts.size() == 1) { out.hi.swap(parts[0]->hi); out.lo.swap(parts[0]->lo); out.ns.swap(parts[0]->ns); }
    else {
        MF_TRY(out.hi.alloc(ctx, m)); MF_TRY(out.lo.alloc(ctx, m)); MF_TRY(out.ns.alloc(ctx, m));
        uint64_t at = 0;
        for (auto &p : parts) {
            MF_HIP(hipMemcpyAsync(out.hi.p + at, p->hi.p, p->n * 8, hipMemcpyDeviceToDevice, st));
            MF_HIP(hipMemcpyAsync(out.lo.p + at, p->lo.p, p->n * 8, hipMemcpyDeviceToDevice, st));
            MF_HIP(hipMemcpyAsync(out.ns.p + at, p->ns.p, p->n * 2, hipMemcpyDeviceToDevice, st));
            at += p->n;
        }
        MF_HIP(hipStreamSynchronize(st));
    }
    out.m = m;
    return MF_OK;
}

// sample j's row: zeroed, then filled from the sample's entries with count > max_bad, piece by piece (a sample need not be ascending or flat)
static int wkps_gather(mf_ctx *ctx, const mf_wjoin_get &get, int j, int max_bad, const wkps_sel &sel, uint16_t *row) {
    hipStream_t st = ctx->stream;
    if (sel.m) MF_HIP(hipMemsetAsync(row, 0, sel.m * 2, st));
    mf_wjoin_sample sm(ctx);
    MF_TRY(wkps_named(get(j, sm)));
    if (sel.m)
        for (auto &pc : sm.t->pieces) {
            if (!pc->n) continue;
            mf_ktimer tm(ctx, "k_wkps_gather");
            k_wkps_gather<<<wkps_grid(pc->n), 256, 0, st>>>(pc->hi.p, pc->lo.p, pc->cnt.p, pc->n, max_bad, sel.hi.p, sel.lo.p, sel.m, row);
        }
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return mf_set_error("kmers-per-sample: gather pass failed: %s", hipGetErrorString(e));
    return MF_OK;
}

int mf_wkps_header(mf_ctx *ctx, const uint64_t *hi, const uint64_t *lo, uint64_t m, int k, mf_buf<uint8_t> &out, uint64_t *bytes) {
    *bytes = m * (uint64_t)(k + 1);
    MF_TRY(out.alloc(ctx, *bytes));
    if (!m) return MF_OK;
    mf_ktimer tm(ctx, "k_wkps_header");
    k_wkps_header<<<kps_grid(m), 256, 0, ctx->stream>>>(hi, lo, m, k, out.p);
    return MF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int mf_kmers_per_sample_wide_tables(mf_ctx *ctx, mf_wtable *const *tables, int n, int max_bad, int percent, int count_first, mf_kps **out) {
    mf_range rng_("mf:kmers_per_sample_wide");
    if (!out) return mf_set_error("mf_kmers_per_sample_wide_tables: NULL argument");
    *out = nullptr;
    MF_TRY(wkps_check("mf_kmers_per_sample_wide_tables", ctx, tables, n));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0; int k = 0;
    MF_TRY(mf_wjoin_tables_check(ctx, tables, n, "mf_kmers_per_sample_wide_tables", &k, &total));
    const mf_wjoin_get get = [tables](int j, mf_wjoin_sample &s) { s.t = tables[j]; return MF_OK; };
    wkps_sel sel;
    MF_TRY(wkps_select(ctx, k, get, n, total, max_bad, percent, count_first, sel));
    MF_TRY(kps_matrix_fits(ctx, n, sel.m));
    std::unique_ptr<mf_kps> r(new mf_kps());
    r->ctx = ctx; r->n_samples = n; r->m = sel.m; r->wide_k = k;
    MF_TRY(r->mat.alloc(ctx, (size_t)n * sel.m));
    for (int j = 0; j < n; j++) MF_TRY(wkps_gather(ctx, get, j, max_bad, sel, r->mat.p + (uint64_t)j * sel.m));
    r->hi.swap(sel.hi); r->lo.swap(sel.lo); r->ns.swap(sel.ns);
    *out = r.release();
    return MF_OK;
}

extern "C" int mf_kps_device_view_wide(const mf_kps *r, const void **d_hi, const void **d_lo, const void **d_nsamples, const void **d_matrix) {
    if (!r) return mf_set_error("mf_kps_device_view_wide: NULL argument");
    if (!r->wide_k) return mf_set_error("mf_kps_device_view_wide: a result of k <= 31 holds one word a k-mer: call mf_kps_device_view");
    if (d_hi) *d_hi = r->hi.p;
    if (d_lo) *d_lo = r->lo.p;
    if (d_nsamples) *d_nsamples = r->ns.p;
    if (d_matrix) *d_matrix = r->mat.p;
    return MF_OK;
}

extern "C" int mf_kps_export_wide(const mf_kps *r, uint64_t *hi, uint64_t *lo, uint16_t *nsamples, uint16_t *matrix) {
    if (!r) return mf_set_error("mf_kps_export_wide: NULL argument");
    if (!r->wide_k) return mf_set_error("mf_kps_export_wide: a result of k <= 31 holds one word a k-mer: call mf_kps_export");
    mf_ctx *ctx = r->ctx;
    MF_HIP(hipSetDevice(ctx->device));
    if (r->m) {
        if (hi) MF_HIP(hipMemcpyAsync(hi, r->hi.p, r->m * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (lo) MF_HIP(hipMemcpyAsync(lo, r->lo.p, r->m * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (nsamples) MF_HIP(hipMemcpyAsync(nsamples, r->ns.p, r->m * 2, hipMemcpyDeviceToHost, ctx->stream));
        if (matrix) MF_HIP(hipMemcpyAsync(matrix, r->mat.p, (size_t)r->n_samples * r->m * 2, hipMemcpyDeviceToHost, ctx->stream));
    }
    MF_HIP(hipStreamSynchronize(ctx->stream));
    return MF_OK;
}

extern "C" int mf_kmers_per_sample_wide(mf_ctx *ctx, const char *const *files, int n, int k, int percent, int count_first, const char *out_txt,
                                        uint64_t *n_kmers) {
    mf_range rng_("mf:kmers_per_sample_wide(files)");
    if (!out_txt) return mf_set_error("mf_kmers_per_sample_wide: NULL argument");
    MF_TRY(wkps_check("mf_kmers_per_sample_wide", ctx, files, n));
    if (k < 32 || k > 63) return mf_set_error("mf_kmers_per_sample_wide: 32 <= k <= 63 (k <= 31: mf_kmers_per_sample)");
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    MF_TRY(mf_wjoin_file_records(files, n, &total));
    // one sample resident at a time, loaded like IOUtils.loadKmers(file, 0)
    const mf_wjoin_get get = [ctx, files, k](int j, mf_wjoin_sample &s) { s.own = true; return mf_wtable_load_kmers(ctx, files + j, 1, 0, k, &s.t); };
    wkps_sel sel;
    MF_TRY(wkps_select(ctx, k, get, n, total, 0, percent, count_first, sel));
    FILE *f = fopen(out_txt, "w");
    if (!f) return mf_set_error("Couldn't open output file '%s'", out_txt);
    auto run = [&]() -> int {
        {
            mf_buf<uint8_t> hdr; uint64_t bytes = 0;
            MF_TRY(mf_wkps_header(ctx, sel.hi.p, sel.lo.p, sel.m, k, hdr, &bytes));
            MF_TRY(kps_write(ctx, hdr.p, bytes, f, out_txt));
        }
        fputc('\n', f);
        mf_buf<uint16_t> row; MF_TRY(row.alloc(ctx, sel.m));
        kps_text tx; MF_TRY(tx.alloc(ctx, sel.m));
        for (int j = 0; j < n; j++) {
            MF_TRY(wkps_gather(ctx, get, j, 0, sel, row.p));
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
