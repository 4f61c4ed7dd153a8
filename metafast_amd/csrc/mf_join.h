// mf_join.h -- the join core of the cohort tools ("the join core"; kernels and host helpers: mf_join.hip).
// Every tool streams its samples, once per hash slice of the key space, into an HBM open-addressed union table of 16-byte slots and
// reads the table out again.  A tool brings its union mode and per-sample `add` words, a projection for the read-out, and its own
// post-pass: mf_stats.hip (stats-kmers, stats-kmers-3, specific-kmers-3, kmers-samples-counter, kmers-grouped-counter), mf_specific.hip
// (specific-kmers), mf_kmersets.hip (unique-kmers, unique-kmers-multi, kmers-multiple-filters), mf_color.hip (kmers-color), mf_kps.hip
// (kmers-per-sample).
#pragma once
#include "mf_common.h"
#include <functional>
#include <memory>

#define MF_STATS_KEY_LIMIT (1ull << 62)   // keys of k <= 31; the union table's empty marker lies above
static constexpr uint32_t MF_NO_ROW = 0xFFFFFFFFu;
static constexpr uint64_t MF_JOIN_CURSOR_MAX = 0xFFFFFFFFull;      // the compaction cursors of the join's kernels are 32-bit
static constexpr uint64_t MF_JOIN_NOT_FOUND = ~0ull;
static constexpr uint32_t MF_UKM_KNOCKED = 0x80000000u;            // unique-kmers-multi: bit 31 of the sum word, a filter sample holds the key

struct mf_uslot { uint64_t key; uint32_t cnt; uint32_t row; };

// What a sample's entry adds to its key's slot:
//   MF_UNION_PRESENCE  `add` to the presence word (stats-kmers, stats-kmers-3, kmers-samples-counter, kmers-grouped-counter)
//   MF_UNION_SUM       the entry's value to the second word and 1 to the first (unique-kmers-multi: two words, so that the sum's carry
//                      never reaches the sample count; sum <= 32767 * 65535 < 2^31)
//   MF_UNION_FIELD     the entry's value to the 16-bit field number `add` of the slot (kmers-multiple-filters: cd, uc, nonibd; each
//                      field is written by one table, whose keys are distinct, so no add carries)
//   MF_UNION_COLOR     kmers-color: 1 (or, bit 2 of `add` set, the entry's value) to the 20-bit field number `add & 3` of the 64-bit payload,
//                      saturating at 2^20 - 1 (ColoredKmerOperations.addValue) by a compare-and-swap on the payload word
enum { MF_UNION_PRESENCE = 0, MF_UNION_SUM = 1, MF_UNION_FIELD = 2, MF_UNION_COLOR = 3 };

// ---------------------------------------------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------------------------------------------
// slice of a key: the top 32 bits of fmix64 scaled to [0, S); the slot inside a slice's table comes from the LOW bits
__device__ __forceinline__ uint32_t mf_stats_slice(uint64_t h, uint32_t S) { return (uint32_t)(((h >> 32) * (uint64_t)S) >> 32); }

// what every kernel over a sample's entries asks first: is `key` slice s's business (mine), and what is its hash (h)?  A key >= 2^62
// never is; FLAG: it raises bit 0 of *flags, else it is skipped silently.  (Both come back by value: an out-parameter for h cost
// every caller four registers.)
struct mf_join_key { uint64_t h; bool mine; };
template <bool FLAG>
__device__ __forceinline__ mf_join_key mf_join_mine(uint64_t key, uint32_t S, uint32_t s, unsigned int *flags) {
    if (key >= MF_STATS_KEY_LIMIT) { if (FLAG) atomicOr(flags, 1u); return mf_join_key{0, false}; }
    const uint64_t h = mf_hash64(key);
    return mf_join_key{h, mf_stats_slice(h, S) == s};
}

// read-only probe, one 16-byte load per step: the slot that holds `key` (*raw: its 16 bytes) or MF_JOIN_NOT_FOUND
__device__ __forceinline__ uint64_t mf_join_find(const mf_uslot *__restrict__ slots, uint64_t mask, uint64_t h, uint64_t key, ulonglong2 *raw) {
    uint64_t p = h & mask;
    for (uint64_t probe = 0; probe <= mask; probe++) {
        *raw = *reinterpret_cast<const ulonglong2 *>(&slots[p]);
        if (raw->x == key) return p;
        if (raw->x == MF_EMPTY) break;
        p = (p + 1) & mask;
    }
    return MF_JOIN_NOT_FOUND;
}

// the read-out's projections of a slot (raw.x = key, raw.y = cnt | row << 32): which occupied slots are kept, and their value
struct mf_read_nsamples {          // kmers-samples-counter: every entry -> number of samples
    using value = uint16_t;
    static constexpr bool all = true;
    static constexpr const char *tool = "kmers-samples-counter", *timer = "k_stats_nsamples";
    __device__ __forceinline__ bool keep(ulonglong2) const { return true; }
    __device__ __forceinline__ value val(ulonglong2 raw) const { return (uint16_t)raw.y; }
};
struct mf_read_kps {               // kmers-per-sample: (int)count >= thresh -> the count (thresh may be <= 0: every entry, the ones with count 0 included)
    using value = uint16_t;
    static constexpr bool all = false;
    static constexpr const char *tool = "kmers-per-sample", *timer = "k_kps_select";
    int thresh;
    __device__ __forceinline__ bool keep(ulonglong2 raw) const { return (int)(uint32_t)raw.y >= thresh; }
    __device__ __forceinline__ value val(ulonglong2 raw) const { return (uint16_t)raw.y; }
};
struct mf_read_color {             // kmers-color: every entry -> packed value
    using value = uint64_t;
    static constexpr bool all = true;
    static constexpr const char *tool = "kmers-color", *timer = "k_color_read";
    __device__ __forceinline__ bool keep(ulonglong2) const { return true; }
    __device__ __forceinline__ value val(ulonglong2 raw) const { return raw.y; }
};
struct mf_read_ukm {               // unique-kmers-multi: not knocked out and (short)sum > thr -> (uint16)sum | samples << 16
    using value = uint32_t;
    static constexpr bool all = false;
    static constexpr const char *tool = "unique-kmers-multi", *timer = "k_ukm_select";
    int thr;
    __device__ __forceinline__ bool keep(ulonglong2 raw) const {
        const uint32_t sw = (uint32_t)(raw.y >> 32);
        return !(sw & MF_UKM_KNOCKED) && (int)(int16_t)(uint16_t)sw > thr;
    }
    __device__ __forceinline__ value val(ulonglong2 raw) const { return (uint32_t)((raw.y >> 32) & 0xFFFFu) | ((uint32_t)raw.y << 16); }
};
struct mf_read_uk {                // unique-kmers: every entry -> its pooled value, the sum bounded at 32767 (addAndBound), 0 where knocked out
    using value = uint16_t;
    static constexpr bool all = true;
    static constexpr const char *tool = "unique-kmers", *timer = "k_uk_read";
    __device__ __forceinline__ bool keep(ulonglong2) const { return true; }
    __device__ __forceinline__ value val(ulonglong2 raw) const {
        const uint32_t sw = (uint32_t)(raw.y >> 32);
        return (sw & MF_UKM_KNOCKED) ? (uint16_t)0 : (uint16_t)(sw < 32767u ? sw : 32767u);
    }
};

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
// a sample while a pass reads it: a caller's table (borrowed) or one loaded from its file (owned).  The stream is drained before an
// owned table goes, so no path releases a sample that a kernel still reads, and none leaks one.
struct mf_join_sample {
    mf_ctx *ctx; mf_table *t = nullptr; bool own = false;
    explicit mf_join_sample(mf_ctx *c) : ctx(c) {}
    mf_join_sample(const mf_join_sample &) = delete;
    mf_join_sample &operator=(const mf_join_sample &) = delete;
    ~mf_join_sample() { if (own && t) { (void)hipStreamSynchronize(ctx->stream); mf_table_destroy(t); } }
    int borrow(mf_table *x) { t = x; own = false; return MF_OK; }
    int adopt(mf_table *x) { t = x; own = true; return MF_OK; }      // a table made for this pass: destroyed with the holder
    // entries with count > thr of `nfiles` files; F (may be NULL): mf_table_load_kmers_sum's freq_sum
    int load(const char *const *files, int nfiles, int thr, int k, uint64_t *F = nullptr) {
        own = true;
        return mf_table_load_kmers_sum(ctx, files, nfiles, thr, k, &t, F);
    }
};
using mf_join_get = std::function<int(int j, mf_join_sample &)>;
static inline mf_join_get mf_join_tables(mf_table *const *t) { return [t](int j, mf_join_sample &s) { return s.borrow(t[j]); }; }
static inline mf_join_get mf_join_files(const char *const *files, int thr, int k) {
    return [=](int j, mf_join_sample &s) { return s.load(files + j, 1, thr, k); };
}

// appends device pieces (one per slice) into one buffer
template <typename T>
static int concat(mf_ctx *ctx, const std::vector<std::unique_ptr<mf_buf<T>>> &parts, const std::vector<uint64_t> &ns, mf_buf<T> &out, uint64_t *n) {
    uint64_t tot = 0;
    for (uint64_t x : ns) tot += x;
    MF_TRY(out.alloc(ctx, tot));
    uint64_t at = 0;
    for (size_t i = 0; i < parts.size(); i++) {
        if (ns[i]) MF_HIP(hipMemcpyAsync(out.p + at, parts[i]->p, ns[i] * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
        at += ns[i];
    }
    MF_HIP(hipStreamSynchronize(ctx->stream));
    *n = tot;
    return MF_OK;
}

// the (key, value) pieces a join leaves behind, one per slice
template <typename K, typename V> struct mf_join_parts {
    std::vector<std::unique_ptr<mf_buf<K>>> pk; std::vector<std::unique_ptr<mf_buf<V>>> pv;
    std::vector<uint64_t> ns;
    // a new piece with room for n entries, taken as full until wrote() says otherwise (v == nullptr: a piece of keys alone)
    int add(mf_ctx *ctx, uint64_t n, K **k, V **v) {
        pk.emplace_back(new mf_buf<K>());
        MF_TRY(pk.back()->alloc(ctx, n));
        *k = pk.back()->p;
        if (v) { pv.emplace_back(new mf_buf<V>()); MF_TRY(pv.back()->alloc(ctx, n)); *v = pv.back()->p; }
        ns.push_back(n);
        return MF_OK;
    }
    void wrote(uint64_t m) { ns.back() = m; }
    bool keys_only() const { return pv.empty(); }
    // all pieces in one buffer each (vals stays empty for pieces of keys alone); the pieces are released
    int concat(mf_ctx *ctx, mf_buf<K> &keys, mf_buf<V> &vals, uint64_t *n) {
        MF_TRY(::concat(ctx, pk, ns, keys, n));
        if (!pv.empty()) MF_TRY(::concat(ctx, pv, ns, vals, n));
        pk.clear(); pv.clear(); ns.clear();
        return MF_OK;
    }
};

// a kernel that compacts through nc zeroed 32-bit cursors: launch(cursors) queues it, out[0 .. nc) = where the cursors end.
// what (may be NULL): names the pass in the message when the stream fails
template <typename L>
static int mf_join_cursors(mf_ctx *ctx, int nc, unsigned int *out, const L &launch, const char *what = nullptr) {
    mf_buf<unsigned int> cur; MF_TRY(cur.alloc(ctx, (size_t)nc));
    MF_HIP(hipMemsetAsync(cur.p, 0, 4 * (size_t)nc, ctx->stream));
    launch(cur.p);
    MF_HIP(hipMemcpyAsync(out, cur.p, 4 * (size_t)nc, hipMemcpyDeviceToHost, ctx->stream));
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return mf_set_error("%s failed: %s", what ? what : "hipStreamSynchronize", hipGetErrorString(e));
    return MF_OK;
}

// slices and union-table capacity for an upper bound `total` of the entries that go in
int plan_slices(mf_ctx *ctx, uint64_t total, uint32_t *S_out, uint64_t *cap_out);
unsigned grid_for(mf_ctx *ctx, uint64_t n);
// *total (may be NULL) += the tables' entries; a NULL table or one of another context is an error that names `what`
int tables_total(mf_ctx *ctx, mf_table *const *t, int n, const char *what, uint64_t *total);
// *total = an upper bound of the files' 10-byte records
int file_records(const char *const *files, int n, uint64_t *total);
// reads the flag word a pass left: bit 0 = a key >= 2^62, bit 1 = the union table is full (never with the sizes the host picks; an
// error, never a write out of bounds)
int mf_join_flags(mf_ctx *ctx, const unsigned int *d_flags, const char *what);
// union of slice s of S: `slots` gets `cap` slots; every entry with count > b of the N samples goes in, sample j adding add[j] in `mode`
int mf_join_union(mf_ctx *ctx, const mf_join_get &get, int N, int b, int mode, const uint32_t *add, uint32_t S, uint32_t s, uint64_t cap,
                  mf_buf<mf_uslot> &slots, uint64_t *n_union);
// read-out of a slice's table: the occupied slots that P keeps, as a new piece of `parts`; nu: the union's size (P::all: all of them
// must come out)
template <typename P>
int mf_join_read(mf_ctx *ctx, const mf_uslot *slots, uint64_t cap, uint64_t nu, const P &proj, mf_join_parts<uint64_t, typename P::value> &parts);
// a one-thread-per-entry filter pass of sample j over a slice (queued by launch(t), skipped for an empty sample), then the
// synchronise that the per-sample error message `what` hangs on
template <typename G, typename L>
static int mf_join_pass(mf_ctx *ctx, const G &get, int j, const char *what, const L &launch) {
    mf_join_sample sm(ctx);
    MF_TRY(get(j, sm));
    if (sm.t->n) launch(sm.t);
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return mf_set_error("%s failed: %s", what, hipGetErrorString(e));
    return MF_OK;
}
// (key, value) pairs -> ascending table; the arrays move into the table.  Result tables have k = 31: their keys are any values below
// 2^62 (the union pass rejects larger ones), and the exports / writers order 2k = 62 key bits.
int pairs_to_table(mf_ctx *ctx, mf_buf<uint64_t> &keys, mf_buf<uint16_t> &vals, uint64_t n, mf_table **out);
int empty_table(mf_ctx *ctx, mf_table **out);
// the distinct values of tri[0 .. m) (their low `bits` bits are sorted; tri is overwritten) -> hist[value] += how often
int kmf_histogram(mf_ctx *ctx, mf_buf<uint64_t> &tri, uint64_t m, std::map<uint64_t, uint64_t> &hist, int bits = 48);
