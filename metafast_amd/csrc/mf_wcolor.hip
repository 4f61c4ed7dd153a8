// mf_wcolor.hip -- NO-REFERENCE EXTENSION (32 <= k <= 63): kmers-color on 2k-bit k-mers, the definition of mf_kmers_color_tables
// (src/tools/ColorKmersMain.java:89-136, src/algo/ColoredKmerOperations.java) carried over to (hi, lo) keys on the wide join
// core (mf_wjoin.h), and the mf_wctable handle it makes: ascending (hi, lo) with 64-bit values, its 24-byte file.
// The wide join claims no slot, so there is no payload word to add into while the union is made, and the union's 16-bit weighted sum holds one
// count, not three.  Per slice of the key range:
//   union   mf_wjoin_slice_union at threshold max_bad, no weights: the slice's distinct k-mers, ascending
//   add     the samples a second time (k_wcolor_add): one thread per entry with count > max_bad, a binary search on two words among the slice's
//           distinct k-mers, then the reference's add on that row's 64-bit value -- field + addend clamped at 2^20 - 1 -- by compare-and-swap
// A field is a clamped sum of non-negative addends, and min(a + b, M) is the same whatever the order the addends come in: the value is a function of
// the samples alone.  The slices are ascending ranges of the key, so their pieces one after the other are the ascending table, for every number of
// slices; there is no key < 2^62 limit here (the narrow union table keeps two key bits for itself, this one keeps none).
#include "mf_join.h"
#include "mf_wjoin.h"
#include <algorithm>
#include <cstddef>
#include <map>
#include <type_traits>
#include <memory>
#include <string>
#include <vector>

#define MF_WCOLOR_MAX_N 1024
#define WCREC_BYTES 24
static constexpr unsigned long long WCOLOR_FIELD_MAX = (1ull << 20) - 1;

// the two families of coloured tables are told apart by k, read through a handle of either type: both begin with their context, then k
static_assert(std::is_standard_layout<mf_ctable>::value && std::is_standard_layout<mf_wctable>::value, "mf_ctable / mf_wctable: offsetof needs standard layout");
static_assert(offsetof(mf_ctable, ctx) == 0 && offsetof(mf_wctable, ctx) == 0 && offsetof(mf_ctable, k) == offsetof(mf_wctable, k),
              "mf_ctable and mf_wctable must begin alike (ctx, then k): the calls of one family refuse the other's handle by its k");

// ---------------------------------------------------------------------------------------------------------------------------
// kernel
// ---------------------------------------------------------------------------------------------------------------------------
// a sample's entries with count > b: the row of the k-mer among the slice's ascending distinct k-mers (shi, slo)[m] gets 1 (use_count: the count)
// added to the 20-bit field at bit `sh` of val[row], clamped at 2^20 - 1 (ColoredKmerOperations.addValue).  A k-mer of another slice is not there:
// the row of one that is lies below m by the search itself.  The swap is retried on a lost race, so the result is right whatever else writes the row.
__global__ __launch_bounds__(256) void k_wcolor_add(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, const uint16_t *__restrict__ cnt, uint64_t n, int b,
                                                    uint32_t sh, int use_count, const uint64_t *__restrict__ shi, const uint64_t *__restrict__ slo, uint64_t m,
                                                    unsigned long long *__restrict__ val) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint16_t c = cnt[i];
        if ((int)c <= b) continue;
        const uint64_t h = hi[i], l = lo[i];
        uint64_t a = 0, e = m;
        while (a < e) {
            const uint64_t mid = a + (e - a) / 2, mh = shi[mid];
            if (mh < h || (mh == h && slo[mid] < l)) a = mid + 1; else e = mid;
        }
        if (!(a < m && shi[a] == h && slo[a] == l)) continue;
        const unsigned long long inc = use_count ? (unsigned long long)c : 1ull;
        unsigned long long cur = val[a];
        for (;;) {
            const unsigned long long f = (cur >> sh) & WCOLOR_FIELD_MAX;
            const unsigned long long nf = f + inc < WCOLOR_FIELD_MAX ? f + inc : WCOLOR_FIELD_MAX;
            const unsigned long long nw = (cur & ~(WCOLOR_FIELD_MAX << sh)) | (nf << sh);
            if (nw == cur) break;                            // (a full field)
            const unsigned long long was = atomicCAS(&val[a], cur, nw);
            if (was == cur) break;
            cur = was;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host: the join
// ---------------------------------------------------------------------------------------------------------------------------
static unsigned wcolor_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 0x7FFFFFFFull); }

// an error of the join core or of a loader, with the tool's name in front
static int wcolor_named(int rc) {
    if (rc >= 0) return rc;
    const std::string e = mf_last_error();
    return mf_set_error("kmers-color (--wide-kmers): %s", e.c_str());
}

static int wcolor_check(int n, const int *classes, int max_bad) {
    if (n > MF_WCOLOR_MAX_N) return mf_set_error("kmers-color: %d samples, at most %d (a field of the packed value holds 20 bits)", n, MF_WCOLOR_MAX_N);
    if (max_bad < 0) return mf_set_error("kmers-color: maximal-bad-frequency = %d is negative", max_bad);
    for (int j = 0; j < n; j++)
        if (classes[j] < 0 || classes[j] > 2) return mf_set_error("kmers-color: sample %d has class %d (the classes are 0, 1 and 2)", j, classes[j]);
    return MF_OK;
}

static int wctable_new(mf_ctx *ctx, int k, uint64_t n, mf_buf<uint64_t> &hi, mf_buf<uint64_t> &lo, mf_buf<uint64_t> &val, mf_wctable **out) {
    auto t = std::make_unique<mf_wctable>();
    t->ctx = ctx; t->k = k; t->n = n;
    t->hi.swap(hi); t->lo.swap(lo); t->val.swap(val);
    *out = t.release();
    return MF_OK;
}

// get(j): sample j as it is read in both passes (every entry: the kernels cut at max_bad)
static int wcolor_join(mf_ctx *ctx, int k, const mf_wjoin_get &get, int N, const int *classes, uint64_t total, int b, int count_values, mf_wctable **out) {
    hipStream_t st = ctx->stream;
    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(wcolor_named(mf_wjoin_plan(ctx, total, &S, &cap)));
    struct part { mf_buf<uint64_t> hi, lo, val; uint64_t n = 0; };
    std::vector<std::unique_ptr<part>> parts;
    uint64_t n = 0;
    for (uint32_t s = 0; s < S && N > 0; s++) {
        mf_wjoin_union u;
        MF_TRY(wcolor_named(mf_wjoin_slice_union(ctx, k, get, N, b, S, s, cap, u)));
        if (!u.n) continue;
        auto p = std::make_unique<part>();
        p->n = u.n;
        p->hi.swap(u.hi); p->lo.swap(u.lo);
        u.cnt.reset(); u.sum.reset(); u.knocked.reset();
        MF_TRY(p->val.alloc(ctx, p->n));
        MF_HIP(hipMemsetAsync(p->val.p, 0, p->n * 8, st));
        for (int j = 0; j < N; j++) {
            mf_wjoin_sample sm(ctx);
            MF_TRY(wcolor_named(get(j, sm)));
            for (auto &piece : sm.t->pieces) {
                if (!piece->n) continue;
                mf_ktimer tm(ctx, "k_wcolor_add");
                k_wcolor_add<<<wcolor_grid(piece->n), 256, 0, st>>>(piece->hi.p, piece->lo.p, piece->cnt.p, piece->n, b, 20u * (uint32_t)classes[j], count_values ? 1 : 0,
                                                                     p->hi.p, p->lo.p, p->n, reinterpret_cast<unsigned long long *>(p->val.p));
            }
            const hipError_t e = hipStreamSynchronize(st);
            if (e != hipSuccess) return mf_set_error("kmers-color (--wide-kmers): add pass failed: %s", hipGetErrorString(e));
        }
        n += p->n;
        parts.push_back(std::move(p));
    }
    mf_buf<uint64_t> hi, lo, val;
    if (parts.size() == 1) { hi.swap(parts[0]->hi); lo.swap(parts[0]->lo); val.swap(parts[0]->val); }
    else {
        MF_TRY(hi.alloc(ctx, n)); MF_TRY(lo.alloc(ctx, n)); MF_TRY(val.alloc(ctx, n));
        uint64_t at = 0;
        for (auto &p : parts) {
            MF_HIP(hipMemcpyAsync(hi.p + at, p->hi.p, p->n * 8, hipMemcpyDeviceToDevice, st));
            MF_HIP(hipMemcpyAsync(lo.p + at, p->lo.p, p->n * 8, hipMemcpyDeviceToDevice, st));
            MF_HIP(hipMemcpyAsync(val.p + at, p->val.p, p->n * 8, hipMemcpyDeviceToDevice, st));
            at += p->n;
        }
        MF_HIP(hipStreamSynchronize(st));
    }
    parts.clear();
    return wctable_new(ctx, k, n, hi, lo, val, out);
}

// ---------------------------------------------------------------------------------------------------------------------------
// mf_wctable
// ---------------------------------------------------------------------------------------------------------------------------
// a handle of the narrow family (mf_ctable, mf_common.h: the same first two members, k = 1 ... 31) given to a call of this one
static int wctable_wide(const mf_wctable *t, const char *what) {
    if (t->k < 32) return mf_set_error("%s: the handle is a narrow coloured table (k = %d): mf_ctable_%s", what, t->k, strrchr(what, '_') + 1);
    return MF_OK;
}
extern "C" void mf_wctable_destroy(mf_wctable *t) {
    if (!t || t->k < 32) return;                              // (a narrow handle is mf_ctable_destroy's: nothing of it is touched here)
    delete t;
}
extern "C" int mf_wctable_stats(const mf_wctable *t, uint64_t *n, int *k) {
    if (!t) return mf_set_error("mf_wctable_stats: NULL table");
    MF_TRY(wctable_wide(t, "mf_wctable_stats"));
    if (n) *n = t->n;
    if (k) *k = t->k;
    return MF_OK;
}
extern "C" int mf_wctable_export(const mf_wctable *t, uint64_t *hi, uint64_t *lo, uint64_t *values, uint64_t cap, uint64_t *n) {
    if (!t || !n) return mf_set_error("mf_wctable_export: NULL argument");
    MF_TRY(wctable_wide(t, "mf_wctable_export"));
    *n = t->n;
    if (!cap) return MF_OK;
    if (cap < t->n || !hi || !lo || !values) return mf_set_error("mf_wctable_export: room for %llu entries, the table has %llu", (unsigned long long)cap, (unsigned long long)t->n);
    mf_ctx *ctx = t->ctx;
    MF_HIP(hipSetDevice(ctx->device));
    if (t->n) {
        MF_HIP(hipMemcpyAsync(hi, t->hi.p, t->n * 8, hipMemcpyDeviceToHost, ctx->stream));
        MF_HIP(hipMemcpyAsync(lo, t->lo.p, t->n * 8, hipMemcpyDeviceToHost, ctx->stream));
        MF_HIP(hipMemcpyAsync(values, t->val.p, t->n * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    MF_HIP(hipStreamSynchronize(ctx->stream));
    return MF_OK;
}

struct wc_rec { uint64_t hi, lo, v; };
// host records, any order, duplicates allowed -> ascending table; the values of a k-mer are added as 64-bit integers, saturating at 2^63 - 1
// (BigLong2LongHashMap.addAndBound)
static int wctable_from_records(mf_ctx *ctx, std::vector<wc_rec> &rc, int k, mf_wctable **out) {
    std::sort(rc.begin(), rc.end(), [](const wc_rec &a, const wc_rec &b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; });
    const uint64_t VMAX = 0x7FFFFFFFFFFFFFFFull;
    std::vector<uint64_t> hi, lo, vals;
    for (const wc_rec &r : rc) {
        if (!hi.empty() && hi.back() == r.hi && lo.back() == r.lo) { uint64_t &v = vals.back(); v = v > VMAX - r.v ? VMAX : v + r.v; }
        else { hi.push_back(r.hi); lo.push_back(r.lo); vals.push_back(r.v); }
    }
    const uint64_t n = hi.size();
    mf_buf<uint64_t> dh, dl, dv;
    MF_TRY(dh.alloc(ctx, n)); MF_TRY(dl.alloc(ctx, n)); MF_TRY(dv.alloc(ctx, n));
    if (n) {
        MF_HIP(hipMemcpyAsync(dh.p, hi.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
        MF_HIP(hipMemcpyAsync(dl.p, lo.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
        MF_HIP(hipMemcpyAsync(dv.p, vals.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    MF_HIP(hipStreamSynchronize(ctx->stream));
    return wctable_new(ctx, k, n, dh, dl, dv, out);
}

extern "C" int mf_wctable_from_host(mf_ctx *ctx, const uint64_t *hi, const uint64_t *lo, const uint64_t *values, uint64_t n, int k, mf_wctable **out) {
    if (!ctx || !out || (n && (!hi || !lo || !values))) return mf_set_error("mf_wctable_from_host: NULL argument");
    *out = nullptr;
    if (k < 32 || k > 63) return mf_set_error("mf_wctable_from_host: 32 <= k <= 63 (k <= 31: mf_ctable_from_host)");
    MF_HIP(hipSetDevice(ctx->device));
    std::vector<wc_rec> rc((size_t)n);
    for (uint64_t i = 0; i < n; i++) {
        if (values[i] >> 63) return mf_set_error("mf_wctable_from_host: value of entry %llu has the sign bit set", (unsigned long long)i);
        if (hi[i] >> (2 * k - 64)) return mf_set_error("mf_wctable_from_host: the k-mer of entry %llu does not fit %d-mers (2k = %d bits)", (unsigned long long)i, k, 2 * k);
        rc[(size_t)i] = wc_rec{hi[i], lo[i], values[i]};
    }
    return wctable_from_records(ctx, rc, k, out);
}

static inline uint64_t wc_be64(const unsigned char *p) {
    uint64_t x = 0;
    for (int i = 0; i < 8; i++) x = (x << 8) | p[i];
    return x;
}
// IOUtils.loadLongKmers (src/io/IOUtils.java:260-281) on the wide record: 24 big-endian bytes (high word, low word, value); a record is kept iff its
// value is > min_value (signed: one with the sign bit set never is)
extern "C" int mf_wctable_load(mf_ctx *ctx, const char *const *files, int nfiles, int64_t min_value, int k, mf_wctable **out) {
    mf_range rng_("mf:wctable_load");
    if (!ctx || !out || nfiles < 0 || (nfiles && !files)) return mf_set_error("mf_wctable_load: NULL argument");
    *out = nullptr;
    if (k < 32 || k > 63) return mf_set_error("mf_wctable_load: 32 <= k <= 63 (k <= 31: mf_ctable_load)");
    MF_HIP(hipSetDevice(ctx->device));
    std::vector<wc_rec> rc;
    for (int j = 0; j < nfiles; j++) {
        if (!files[j]) return mf_set_error("mf_wctable_load: file %d is NULL", j);
        FILE *f = fopen(files[j], "rb");
        if (!f) return mf_set_error("can't open '%s'", files[j]);
        std::vector<unsigned char> buf((size_t)WCREC_BYTES << 15);
        size_t got, carry = 0;
        uint64_t rec = 0;
        while ((got = fread(buf.data() + carry, 1, buf.size() - carry, f)) > 0) {
            const size_t have = carry + got, whole = have / WCREC_BYTES * WCREC_BYTES;
            for (size_t o = 0; o < whole; o += WCREC_BYTES, rec++) {
                const uint64_t h = wc_be64(&buf[o]), l = wc_be64(&buf[o + 8]); const int64_t v = (int64_t)wc_be64(&buf[o + 16]);
                if (h >> (2 * k - 64)) {
                    fclose(f);
                    return mf_set_error("Can't load wide colored k-mers file '%s': the k-mer of record %llu does not fit %d-mers (2k = %d bits; is this a file of another k?)",
                                        files[j], (unsigned long long)rec, k, 2 * k);
                }
                if (v > min_value && v >= 0) rc.push_back(wc_rec{h, l, (uint64_t)v});
            }
            carry = have - whole;
            memmove(buf.data(), buf.data() + whole, carry);
        }
        fclose(f);
        if (carry)
            return mf_set_error("Can't load wide colored k-mers file '%s': its size is not a multiple of the %d-byte (high word, low word, value) record: %llu bytes are left over",
                                files[j], WCREC_BYTES, (unsigned long long)carry);
    }
    return wctable_from_records(ctx, rc, k, out);
}

extern "C" int mf_wctable_write(const mf_wctable *t, const char *kmers_bin, const char *stat_txt, uint64_t *n_written) {
    mf_range rng_("mf:wctable_write");
    if (!t || !kmers_bin) return mf_set_error("mf_wctable_write: NULL argument");
    MF_TRY(wctable_wide(t, "mf_wctable_write"));
    mf_ctx *ctx = t->ctx;
    MF_HIP(hipSetDevice(ctx->device));
    std::vector<uint64_t> hi((size_t)t->n), lo((size_t)t->n), vals((size_t)t->n);
    uint64_t n = 0;
    MF_TRY(mf_wctable_export(t, hi.data(), lo.data(), vals.data(), t->n, &n));
    FILE *f = fopen(kmers_bin, "wb");
    if (!f) return mf_set_error("can't write '%s'", kmers_bin);
    std::vector<unsigned char> buf;
    buf.reserve((size_t)WCREC_BYTES << 15);
    uint64_t w = 0;
    bool ok = true;
    for (uint64_t i = 0; i < n && ok; i++) {
        if (vals[(size_t)i] == 0) continue;                   // (printKmers writes the entries with value > 0)
        for (const uint64_t x : {hi[(size_t)i], lo[(size_t)i], vals[(size_t)i]})
            for (int s = 56; s >= 0; s -= 8) buf.push_back((unsigned char)(x >> s));
        w++;
        if (buf.size() + WCREC_BYTES > buf.capacity()) { ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); }
    }
    if (ok && !buf.empty()) ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    if (fclose(f) != 0 || !ok) return mf_set_error("can't write '%s'", kmers_bin);
    if (stat_txt) {
        // the distinct values with the number of k-mers of each, ascending: the narrow writer's text
        std::map<uint64_t, uint64_t> hist;
        if (t->n) {
            mf_buf<uint64_t> v; MF_TRY(v.alloc(ctx, t->n));
            MF_HIP(hipMemcpyAsync(v.p, t->val.p, t->n * 8, hipMemcpyDeviceToDevice, ctx->stream));
            MF_TRY(kmf_histogram(ctx, v, t->n, hist, 63));
        }
        FILE *g = fopen(stat_txt, "w");
        if (!g) return mf_set_error("can't write '%s'", stat_txt);
        fprintf(g, "# k-mer frequency\tnumber of such k-mers\n");
        for (auto &kv : hist) fprintf(g, "%llu\t%llu\n", (unsigned long long)kv.first, (unsigned long long)kv.second);
        fprintf(g, "\n");
        if (fclose(g) != 0) return mf_set_error("can't write '%s'", stat_txt);
    }
    if (n_written) *n_written = w;
    return MF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI: kmers-color
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int mf_kmers_color_wide_tables(mf_ctx *ctx, mf_wtable *const *t, const int *classes, int n, int max_bad, int count_values, mf_wctable **out) {
    mf_range rng_("mf:kmers_color_wide");
    if (!ctx || !out || n < 0 || (n && (!t || !classes))) return mf_set_error("mf_kmers_color_wide_tables: NULL argument");
    *out = nullptr;
    MF_TRY(wcolor_check(n, classes, max_bad));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0; int k = 0;
    MF_TRY(mf_wjoin_tables_check(ctx, t, n, "mf_kmers_color_wide_tables", &k, &total));
    if (!k) k = 32;                                         // (no table at all: one empty result)
    const mf_wjoin_get get = [t](int j, mf_wjoin_sample &s) { s.t = t[j]; return MF_OK; };
    return wcolor_join(ctx, k, get, n, classes, total, max_bad, count_values, out);
}

extern "C" int mf_kmers_color_wide(mf_ctx *ctx, const char *const *files, const int *classes, int n, int max_bad, int count_values, int k, const char *kmers_bin,
                                   const char *stat_txt, uint64_t *n_kmers) {
    mf_range rng_("mf:kmers_color_wide(files)");
    if (!ctx || !kmers_bin || n < 0 || (n && (!files || !classes))) return mf_set_error("mf_kmers_color_wide: NULL argument");
    if (k < 32 || k > 63) return mf_set_error("mf_kmers_color_wide: 32 <= k <= 63 (k <= 31: mf_kmers_color)");
    MF_TRY(wcolor_check(n, classes, max_bad));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    MF_TRY(mf_wjoin_file_records(files, n, &total));
    // one sample resident at a time, loaded like IOUtils.loadKmers(file, 0): read twice per slice, for the union and for the add
    const mf_wjoin_get get = [ctx, files, k](int j, mf_wjoin_sample &s) { s.own = true; return mf_wtable_load_kmers(ctx, files + j, 1, 0, k, &s.t); };
    mf_wctable *t = nullptr;
    MF_TRY(wcolor_join(ctx, k, get, n, classes, total, max_bad, count_values, &t));
    uint64_t w = 0;
    const int rc = mf_wctable_write(t, kmers_bin, stat_txt, &w);
    mf_wctable_destroy(t);
    if (rc == MF_OK && n_kmers) *n_kmers = w;
    return rc;
}
