// mf_ctable.hip -- the mf_ctable handle: ascending k-mers with 64-bit values (BigLong2LongHashMap).  kmers-color makes one
// (mf_color.hip), component-colored reads one (mf_cc.hip); the .stat.txt histogram runs on the join core's run-length pass.
#include "mf_join.h"
#include "mf_wide.h"
#include <algorithm>
#include <cstddef>
#include <type_traits>

// the two families of coloured tables are told apart by k, read through a handle of either type: both begin with their context, then k
static_assert(std::is_standard_layout<mf_ctable>::value && std::is_standard_layout<mf_wctable>::value, "mf_ctable / mf_wctable: offsetof needs standard layout");
static_assert(offsetof(mf_ctable, ctx) == 0 && offsetof(mf_wctable, ctx) == 0 && offsetof(mf_ctable, k) == offsetof(mf_wctable, k),
              "mf_ctable and mf_wctable must begin alike (ctx, then k): the calls of one family refuse the other's handle by its k");

// a handle of the wide family (mf_wctable, mf_wide.h: the same first two members, k = 32 ... 63) given to a call of this one
static int ctable_narrow(const mf_ctable *t, const char *what) {
    if (t->k > 31) return mf_set_error("%s: the handle is a wide coloured table (k = %d): mf_wctable_%s", what, t->k, strrchr(what, '_') + 1);
    return MF_OK;
}
int mf_ctable_adopt(mf_ctx *ctx, int k, uint64_t n, uint64_t *d_keys, size_t kb, uint64_t *d_vals, size_t vb, mf_ctable **out) {
    mf_ctable *t = new mf_ctable();
    t->ctx = ctx; t->k = k; t->n = n; t->d_keys = d_keys; t->keys_bytes = kb; t->d_vals = d_vals; t->vals_bytes = vb;
    *out = t;
    return MF_OK;
}
extern "C" void mf_ctable_destroy(mf_ctable *t) {
    if (!t || t->k > 31) return;                              // (a wide handle is mf_wctable_destroy's: nothing of it is touched here)
    if (t->d_keys) mf_release(t->ctx, t->d_keys, t->keys_bytes);
    if (t->d_vals) mf_release(t->ctx, t->d_vals, t->vals_bytes);
    delete t;
}
extern "C" int mf_ctable_stats(const mf_ctable *t, uint64_t *n, int *k) {
    if (!t) return mf_set_error("mf_ctable_stats: NULL table");
    MF_TRY(ctable_narrow(t, "mf_ctable_stats"));
    if (n) *n = t->n;
    if (k) *k = t->k;
    return MF_OK;
}
extern "C" int mf_ctable_export(const mf_ctable *t, uint64_t *keys, uint64_t *values, uint64_t cap, uint64_t *n) {
    if (!t || !n) return mf_set_error("mf_ctable_export: NULL argument");
    MF_TRY(ctable_narrow(t, "mf_ctable_export"));
    *n = t->n;
    if (!cap) return MF_OK;
    if (cap < t->n || !keys || !values) return mf_set_error("mf_ctable_export: room for %llu entries, the table has %llu", (unsigned long long)cap, (unsigned long long)t->n);
    mf_ctx *ctx = t->ctx;
    MF_HIP(hipSetDevice(ctx->device));
    if (t->n) {
        MF_HIP(hipMemcpyAsync(keys, t->d_keys, t->n * 8, hipMemcpyDeviceToHost, ctx->stream));
        MF_HIP(hipMemcpyAsync(values, t->d_vals, t->n * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    MF_HIP(hipStreamSynchronize(ctx->stream));
    return MF_OK;
}

// host pairs, any order, duplicates allowed -> ascending table; the values of a key are added as 64-bit integers, saturating at
// 2^63 - 1 (BigLong2LongHashMap.addAndBound)
static int ctable_from_pairs(mf_ctx *ctx, std::vector<std::pair<uint64_t, uint64_t>> &pr, int k, mf_ctable **out) {
    std::sort(pr.begin(), pr.end());
    const uint64_t VMAX = 0x7FFFFFFFFFFFFFFFull;
    std::vector<uint64_t> keys, vals;
    for (size_t i = 0; i < pr.size(); i++) {
        if (!keys.empty() && keys.back() == pr[i].first) { uint64_t &v = vals.back(); v = v > VMAX - pr[i].second ? VMAX : v + pr[i].second; }
        else { keys.push_back(pr[i].first); vals.push_back(pr[i].second); }
    }
    if (!keys.empty() && k < 32 && (keys.back() >> (2 * k)))
        return mf_set_error("colored k-mers: key %llu does not fit %d-mers (2k = %d bits)", (unsigned long long)keys.back(), k, 2 * k);
    const uint64_t n = keys.size();
    mf_buf<uint64_t> dk, dv;
    MF_TRY(dk.alloc(ctx, n)); MF_TRY(dv.alloc(ctx, n));
    if (n) {
        MF_HIP(hipMemcpyAsync(dk.p, keys.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
        MF_HIP(hipMemcpyAsync(dv.p, vals.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    MF_HIP(hipStreamSynchronize(ctx->stream));
    const size_t kb = dk.bytes(), vb = dv.bytes();
    return mf_ctable_adopt(ctx, k, n, dk.take(), kb, dv.take(), vb, out);
}

extern "C" int mf_ctable_from_host(mf_ctx *ctx, const uint64_t *keys, const uint64_t *values, uint64_t n, int k, mf_ctable **out) {
    if (!ctx || !out || (n && (!keys || !values))) return mf_set_error("mf_ctable_from_host: NULL argument");
    *out = nullptr;
    if (k < 1 || k > 31) return mf_set_error("k must be in [1,31]");
    MF_HIP(hipSetDevice(ctx->device));
    std::vector<std::pair<uint64_t, uint64_t>> pr((size_t)n);
    for (uint64_t i = 0; i < n; i++) {
        if (values[i] >> 63) return mf_set_error("mf_ctable_from_host: value of entry %llu has the sign bit set", (unsigned long long)i);
        pr[(size_t)i] = {keys[i], values[i]};
    }
    return ctable_from_pairs(ctx, pr, k, out);
}

static inline uint64_t be64(const unsigned char *p) {
    uint64_t x = 0;
    for (int i = 0; i < 8; i++) x = (x << 8) | p[i];
    return x;
}
// IOUtils.loadLongKmers (src/io/IOUtils.java:260-281, 403-440): 16-byte big-endian records (key, value); a record is kept iff its value
// is > min_value (signed: one with the sign bit set never is)
extern "C" int mf_ctable_load(mf_ctx *ctx, const char *const *files, int nfiles, int64_t min_value, int k, mf_ctable **out) {
    mf_range rng_("mf:ctable_load");
    if (!ctx || !out || nfiles < 0 || (nfiles && !files)) return mf_set_error("mf_ctable_load: NULL argument");
    *out = nullptr;
    if (k < 1 || k > 31) return mf_set_error("k must be in [1,31]");
    MF_HIP(hipSetDevice(ctx->device));
    std::vector<std::pair<uint64_t, uint64_t>> pr;
    for (int j = 0; j < nfiles; j++) {
        if (!files[j]) return mf_set_error("mf_ctable_load: file %d is NULL", j);
        FILE *f = fopen(files[j], "rb");
        if (!f) return mf_set_error("can't open '%s'", files[j]);
        std::vector<unsigned char> buf(1 << 20);
        size_t got, carry = 0;
        while ((got = fread(buf.data() + carry, 1, buf.size() - carry, f)) > 0) {
            const size_t have = carry + got, whole = have / 16 * 16;
            for (size_t o = 0; o < whole; o += 16) {
                const uint64_t key = be64(&buf[o]); const int64_t v = (int64_t)be64(&buf[o + 8]);
                if (v > min_value && v >= 0) pr.push_back({key, (uint64_t)v});
            }
            carry = have - whole;
            memmove(buf.data(), buf.data() + whole, carry);
        }
        fclose(f);
        if (carry) return mf_set_error("'%s' is not a file of 16-byte (k-mer, value) records: %llu bytes are left over", files[j], (unsigned long long)carry);
    }
    return ctable_from_pairs(ctx, pr, k, out);
}

// the distinct values with the number of k-mers of each, ascending
static int ctable_hist(const mf_ctable *t, std::map<uint64_t, uint64_t> &hist) {
    mf_ctx *ctx = t->ctx;
    if (!t->n) return MF_OK;
    mf_buf<uint64_t> v; MF_TRY(v.alloc(ctx, t->n));
    MF_HIP(hipMemcpyAsync(v.p, t->d_vals, t->n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return kmf_histogram(ctx, v, t->n, hist, 63);
}

extern "C" int mf_ctable_write(const mf_ctable *t, const char *kmers_bin, const char *stat_txt, uint64_t *n_written) {
    mf_range rng_("mf:ctable_write");
    if (!t || !kmers_bin) return mf_set_error("mf_ctable_write: NULL argument");
    MF_TRY(ctable_narrow(t, "mf_ctable_write"));
    mf_ctx *ctx = t->ctx;
    MF_HIP(hipSetDevice(ctx->device));
    std::vector<uint64_t> keys((size_t)t->n), vals((size_t)t->n);
    uint64_t n = 0;
    MF_TRY(mf_ctable_export(t, keys.data(), vals.data(), t->n, &n));
    FILE *f = fopen(kmers_bin, "wb");
    if (!f) return mf_set_error("can't write '%s'", kmers_bin);
    std::vector<unsigned char> buf;
    buf.reserve(1 << 20);
    uint64_t w = 0;
    bool ok = true;
    for (uint64_t i = 0; i < n && ok; i++) {
        if (vals[(size_t)i] == 0) continue;                   // (printKmers writes the entries with value > 0)
        for (int s = 56; s >= 0; s -= 8) buf.push_back((unsigned char)(keys[(size_t)i] >> s));
        for (int s = 56; s >= 0; s -= 8) buf.push_back((unsigned char)(vals[(size_t)i] >> s));
        w++;
        if (buf.size() >= (1 << 20) - 16) { ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); }
    }
    if (ok && !buf.empty()) ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    if (fclose(f) != 0 || !ok) return mf_set_error("can't write '%s'", kmers_bin);
    if (stat_txt) {
        std::map<uint64_t, uint64_t> hist;
        MF_TRY(ctable_hist(t, hist));
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
