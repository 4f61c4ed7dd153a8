// mf_kmersets.hip -- unique-kmers-multi (src/tools/UniqueKmersMultipleSamplesFinder.java:84-185) and kmers-multiple-filters
// (src/tools/KmersMultipleFilters.java:77-133, IOUtils.MultipleFiltersAndPrintKmers src/io/IOUtils.java:125-213) on the join core
// (mf_join.h).
//   unique-kmers-multi      union (MF_UNION_SUM) of the inputs; the filter samples' keys knock slots out (bit 31 of the sum word);
//                           one read-out of (key, (short)sum, samples) with (short)sum > b; one sort by key; filtered_<i> = the
//                           subsequence with samples >= i, by an order-keeping compaction.
//   unique-kmers            (UniqueKmersFinder.java:73-144) the same union with the sum BOUNDED at 32767 where it is
//                           read: the inputs pooled into one map; one read-out of every slot, knocked-out ones with value 0.
//   kmers-multiple-filters  probe table {key, cd, uc, nonibd} (MF_UNION_FIELD) of the three filter tables; per input sample one
//                           probe per entry: the kept records and every entry's triple packed into 48 bits; the histogram is the
//                           sort of the packed triples and a run-length pass.
#include "mf_join.h"
#include <algorithm>

// a filter sample's entries (count > thr): the slot of a key whose wrapped sum is > thr is knocked out
__global__ __launch_bounds__(256) void k_ukm_knock(mf_uslot *__restrict__ slots, uint64_t mask, const uint64_t *__restrict__ keys,
                                                   const uint16_t *__restrict__ cnts, uint64_t n, int thr, uint32_t S, uint32_t s,
                                                   unsigned int *__restrict__ flags) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if ((int)cnts[i] <= thr) continue;
        const uint64_t key = keys[i];
        const mf_join_key k = mf_join_mine<true>(key, S, s, flags);
        if (!k.mine) continue;
        ulonglong2 raw;
        const uint64_t p = mf_join_find(slots, mask, k.h, key, &raw);
        if (p != MF_JOIN_NOT_FOUND && (int)(int16_t)(uint16_t)(raw.y >> 32) > thr) atomicOr(&slots[p].row, MF_UKM_KNOCKED);
    }
}

// unique-kmers (UniqueKmersFinder.java:91-105): k_ukm_knock's probe with the pooled map's BOUNDED sum in the test where that one wraps --
// the pool is one map filled by addAndBound, so 3 x 20000 is 32767 here and -5536 there
__global__ __launch_bounds__(256) void k_uk_knock(mf_uslot *__restrict__ slots, uint64_t mask, const uint64_t *__restrict__ keys,
                                                  const uint16_t *__restrict__ cnts, uint64_t n, int thr, uint32_t S, uint32_t s,
                                                  unsigned int *__restrict__ flags) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if ((int)cnts[i] <= thr) continue;
        const uint64_t key = keys[i];
        const mf_join_key k = mf_join_mine<true>(key, S, s, flags);
        if (!k.mine) continue;
        ulonglong2 raw;
        const uint64_t p = mf_join_find(slots, mask, k.h, key, &raw);
        if (p == MF_JOIN_NOT_FOUND) continue;
        const uint32_t sum = (uint32_t)(raw.y >> 32) & ~MF_UKM_KNOCKED;
        if ((int)(sum < 32767u ? sum : 32767u) > thr) atomicOr(&slots[p].row, MF_UKM_KNOCKED);
    }
}

// the sorted survivors' payload (uint16)sum | samples << 16 -> two 16-bit arrays (what the order-keeping selection of mf_table.hip takes)
__global__ __launch_bounds__(256) void k_ukm_split(const uint32_t *__restrict__ v, uint64_t n, uint16_t *__restrict__ sums, uint16_t *__restrict__ cnts) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t x = v[i];
        sums[i] = (uint16_t)x; cnts[i] = (uint16_t)(x >> 16);
    }
}

// kmers-multiple-filters: every entry (count > thr) of an input sample in slice s probes {key, cd | uc << 16, nonibd}: its triple, packed
// cd << 32 | uc << 16 | nonibd, goes to tri; the entry itself to (okeys, ovals) when a value of the triple is > 0.
// cursor: [0] kept, [1] found.  (uniform trip count: mf_wave_reserve)
__global__ __launch_bounds__(256) void k_kmf_probe(const mf_uslot *__restrict__ slots, uint64_t mask, const uint64_t *__restrict__ keys,
                                                   const uint16_t *__restrict__ cnts, uint64_t n, int thr, uint32_t S, uint32_t s,
                                                   uint64_t *__restrict__ okeys, uint16_t *__restrict__ ovals, uint64_t *__restrict__ tri,
                                                   unsigned int *__restrict__ cursor, unsigned int *__restrict__ flags) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n; i0 += stride) {
        const uint64_t i = i0 + threadIdx.x;
        bool found = false;
        uint64_t key = 0, t = 0;
        uint16_t c = 0;
        if (i < n) {
            c = cnts[i];
            if ((int)c > thr) {
                key = keys[i];
                const mf_join_key k = mf_join_mine<true>(key, S, s, flags);
                ulonglong2 raw;
                found = k.mine;
                if (found && mf_join_find(slots, mask, k.h, key, &raw) != MF_JOIN_NOT_FOUND)
                    t = ((raw.y & 0xFFFFull) << 32) | (((raw.y >> 16) & 0xFFFFull) << 16) | ((raw.y >> 32) & 0xFFFFull);
            }
        }
        const bool keep = found && t != 0;
        const uint32_t rk = mf_wave_reserve(&cursor[0], keep ? 1u : 0u);
        const uint32_t rf = mf_wave_reserve(&cursor[1], found ? 1u : 0u);
        if (keep) { okeys[rk] = key; ovals[rk] = c; }
        if (found) tri[rf] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
static int ukm_check(int n_in, int max_bad, int min_samples, int max_samples) {
    if (max_bad < 0) return mf_set_error("unique-kmers-multi: maximal-bad-frequence = %d is negative", max_bad);
    if (n_in > 32767) return mf_set_error("unique-kmers-multi: %d input files, at most 32767 (the number of samples is a Java short)", n_in);
    if (min_samples > max_samples) return mf_set_error("--min-samples parameter cannot be greater than --max-samples parameter.");
    return MF_OK;
}

// -> outs: one table per i = min_samples, min_samples + 1, ... up to max_samples or the first empty one (included); counts: their sizes
static int ukm_join(mf_ctx *ctx, const mf_join_get &get_in, int n_in, const mf_join_get &get_f, int n_f, uint64_t total, int b, int min_samples,
                    int max_samples, std::vector<mf_table *> &outs, std::vector<uint64_t> &counts, uint64_t *n_union) {
    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(plan_slices(ctx, total, &S, &cap));
    mf_join_parts<uint64_t, uint32_t> parts;
    mf_buf<unsigned int> flags; MF_TRY(flags.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(flags.p, 0, 4, ctx->stream));
    *n_union = 0;
    const std::vector<uint32_t> add((size_t)n_in, 0u);
    for (uint32_t s = 0; s < S; s++) {
        mf_buf<mf_uslot> slots; uint64_t nu = 0;
        MF_TRY(mf_join_union(ctx, get_in, n_in, b, MF_UNION_SUM, add.data(), S, s, cap, slots, &nu));
        *n_union += nu;
        for (int j = 0; j < n_f; j++)
            MF_TRY(mf_join_pass(ctx, get_f, j, "unique-kmers-multi: filter pass", [&](const mf_table *t) {
                mf_ktimer tm(ctx, "k_ukm_knock");
                k_ukm_knock<<<grid_for(ctx, t->n), 256, 0, ctx->stream>>>(slots.p, cap - 1, t->d_keys, t->d_counts, t->n, b, S, s, flags.p);
            }));
        MF_TRY(mf_join_read(ctx, slots.p, cap, nu, mf_read_ukm{b}, parts));
    }
    MF_TRY(mf_join_flags(ctx, flags.p, "unique-kmers-multi"));
    // one sorted list of the survivors
    mf_buf<uint64_t> keys, sk; mf_buf<uint32_t> vals, sv; uint64_t n = 0;
    MF_TRY(parts.concat(ctx, keys, vals, &n));
    MF_TRY(sk.alloc(ctx, n)); MF_TRY(sv.alloc(ctx, n));
    if (n) MF_TRY(mf_sort_u64_u32(ctx, keys.p, vals.p, n, 62, sk.p, sv.p));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    keys.reset(); vals.reset();
    // filtered_<i>: the subsequence with samples > i - 1 (the order-keeping selection of mf_table.hip)
    mf_buf<uint16_t> sums, scnt;
    MF_TRY(sums.alloc(ctx, n)); MF_TRY(scnt.alloc(ctx, n));
    if (n) {
        mf_ktimer tm(ctx, "k_ukm_split");
        k_ukm_split<<<grid_for(ctx, n), 256, 0, ctx->stream>>>(sv.p, n, sums.p, scnt.p);
    }
    MF_HIP(hipStreamSynchronize(ctx->stream));
    sv.reset();
    for (int64_t i = min_samples; i <= (int64_t)max_samples; i++) {
        mf_buf<uint64_t> ok; mf_buf<uint16_t> ov; uint64_t m = 0;
        // (no key is held by more than n_in samples, and every survivor by at least one)
        if (i > n_in) { MF_TRY(ok.alloc(ctx, 0)); MF_TRY(ov.alloc(ctx, 0)); }
        else MF_TRY(mf_select_by(ctx, sk.p, scnt.p, sums.p, n, (int)std::max<int64_t>(i - 1, -1), ok, ov, &m));
        MF_HIP(hipStreamSynchronize(ctx->stream));
        mf_table *t = nullptr;
        const size_t kb = ok.bytes(), vb = ov.bytes();
        MF_TRY(mf_table_adopt(ctx, 31, m, 0, ok.take(), kb, ov.take(), vb, &t));
        outs.push_back(t);
        counts.push_back(m);
        if (!m) break;
    }
    return MF_OK;
}

static void destroy_all(std::vector<mf_table *> &v) { for (mf_table *t : v) mf_table_destroy(t); v.clear(); }

extern "C" int mf_unique_kmers_multi_tables(mf_ctx *ctx, mf_table *const *inputs, int n_inputs, mf_table *const *filters, int n_filters, int max_bad,
                                            int min_samples, int max_samples, mf_table **out, int *n_out, uint64_t *n_union, uint64_t *counts) {
    mf_range rng_("mf:unique_kmers_multi");
    if (!ctx || !out || !n_out || !n_union || !counts || (n_inputs && !inputs) || (n_filters && !filters) || n_inputs < 0 || n_filters < 0)
        return mf_set_error("mf_unique_kmers_multi_tables: NULL argument");
    *n_out = 0;
    MF_TRY(ukm_check(n_inputs, max_bad, min_samples, max_samples));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    MF_TRY(tables_total(ctx, inputs, n_inputs, "mf_unique_kmers_multi_tables (inputs)", &total));
    MF_TRY(tables_total(ctx, filters, n_filters, "mf_unique_kmers_multi_tables (filters)", nullptr));
    std::vector<mf_table *> outs; std::vector<uint64_t> cs;
    const int rc = ukm_join(ctx, mf_join_tables(inputs), n_inputs, mf_join_tables(filters), n_filters, total, max_bad, min_samples, max_samples, outs, cs, n_union);
    if (rc != MF_OK) { destroy_all(outs); return rc; }
    for (size_t i = 0; i < outs.size(); i++) { out[i] = outs[i]; counts[i] = cs[i]; }
    *n_out = (int)outs.size();
    return MF_OK;
}

extern "C" int mf_unique_kmers_multi(mf_ctx *ctx, const char *const *in_files, int n_inputs, const char *const *filter_files, int n_filters, int max_bad,
                                     int k, int min_samples, int max_samples, const char *out_dir, int *n_out, uint64_t *n_union, uint64_t *counts) {
    mf_range rng_("mf:unique_kmers_multi(files)");
    if (!ctx || !out_dir || !n_out || !n_union || !counts || (n_inputs && !in_files) || (n_filters && !filter_files) || n_inputs < 0 || n_filters < 0)
        return mf_set_error("mf_unique_kmers_multi: NULL argument");
    *n_out = 0;
    if (k < 1 || k > 31) return mf_set_error("k must be in [1,31]");
    MF_TRY(ukm_check(n_inputs, max_bad, min_samples, max_samples));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0, tf = 0;
    MF_TRY(file_records(in_files, n_inputs, &total));
    MF_TRY(file_records(filter_files, n_filters, &tf));
    const mf_join_get gi = mf_join_files(in_files, max_bad, k), gf = mf_join_files(filter_files, max_bad, k);
    std::vector<mf_table *> outs; std::vector<uint64_t> cs;
    int rc = ukm_join(ctx, gi, n_inputs, gf, n_filters, total, max_bad, min_samples, max_samples, outs, cs, n_union);
    for (size_t i = 0; i < outs.size() && rc == MF_OK; i++) {
        uint64_t w = 0;
        rc = mf_table_write_kmers(outs[i], -1, (std::string(out_dir) + "/filtered_" + std::to_string((long long)min_samples + (long long)i) + ".kmers.bin").c_str(), nullptr, &w);
    }
    if (rc == MF_OK) { for (size_t i = 0; i < cs.size(); i++) counts[i] = cs[i]; *n_out = (int)cs.size(); }
    destroy_all(outs);
    return rc;
}

// ---- unique-kmers (UniqueKmersFinder.java:73-144) ----
// The inputs are POOLED: IOUtils.loadKmers(files, b) keeps the RECORDS with a value > b (the threshold is per record, not on the sum:
// a k-mer with count 1 in two files is not there at b = 1) and adds them into one map with addAndBound (the sum stops at 32767).  Every
// filter file, loaded alone at b, zeroes the pooled k-mers it holds.  -> hm: the whole pooled map, the zeroed k-mers with value 0 (what
// printKmers walks: its histogram counts them, its records leave them out)
static int uk_join(mf_ctx *ctx, const mf_join_get &get_in, int n_in, const mf_join_get &get_f, int n_f, uint64_t total, int b, mf_table **hm) {
    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(plan_slices(ctx, total, &S, &cap));
    mf_join_parts<uint64_t, uint16_t> parts;
    mf_buf<unsigned int> flags; MF_TRY(flags.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(flags.p, 0, 4, ctx->stream));
    const std::vector<uint32_t> add((size_t)n_in, 0u);
    for (uint32_t s = 0; s < S; s++) {
        mf_buf<mf_uslot> slots; uint64_t nu = 0;
        MF_TRY(mf_join_union(ctx, get_in, n_in, b, MF_UNION_SUM, add.data(), S, s, cap, slots, &nu));
        for (int j = 0; j < n_f; j++)
            MF_TRY(mf_join_pass(ctx, get_f, j, "unique-kmers: filter pass", [&](const mf_table *t) {
                mf_ktimer tm(ctx, "k_uk_knock");
                k_uk_knock<<<grid_for(ctx, t->n), 256, 0, ctx->stream>>>(slots.p, cap - 1, t->d_keys, t->d_counts, t->n, b, S, s, flags.p);
            }));
        MF_TRY(mf_join_read(ctx, slots.p, cap, nu, mf_read_uk{}, parts));
    }
    MF_TRY(mf_join_flags(ctx, flags.p, "unique-kmers"));
    mf_buf<uint64_t> keys; mf_buf<uint16_t> vals; uint64_t n = 0;
    MF_TRY(parts.concat(ctx, keys, vals, &n));
    return pairs_to_table(ctx, keys, vals, n, hm);
}
static int uk_check(int n_in, int max_bad) {
    if (max_bad < 0) return mf_set_error("unique-kmers: maximal-bad-frequence = %d is negative", max_bad);
    if (n_in > 32767) return mf_set_error("unique-kmers: %d input files, at most 32767 (the pooled sum is kept in 31 bits)", n_in);
    return MF_OK;
}

extern "C" int mf_unique_kmers_tables(mf_ctx *ctx, mf_table *const *inputs, int n_inputs, mf_table *const *filters, int n_filters, int max_bad,
                                      mf_table **out, uint64_t *n_pooled) {
    mf_range rng_("mf:unique_kmers");
    if (!ctx || !out || !n_pooled || (n_inputs && !inputs) || (n_filters && !filters) || n_inputs < 0 || n_filters < 0)
        return mf_set_error("mf_unique_kmers_tables: NULL argument");
    *out = nullptr;
    MF_TRY(uk_check(n_inputs, max_bad));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    MF_TRY(tables_total(ctx, inputs, n_inputs, "mf_unique_kmers_tables (inputs)", &total));
    MF_TRY(tables_total(ctx, filters, n_filters, "mf_unique_kmers_tables (filters)", nullptr));
    mf_table *hm = nullptr;
    MF_TRY(uk_join(ctx, mf_join_tables(inputs), n_inputs, mf_join_tables(filters), n_filters, total, max_bad, &hm));
    *n_pooled = hm->n;
    const int rc = mf_table_filter(hm, max_bad, out);
    mf_table_destroy(hm);
    return rc;
}

extern "C" int mf_unique_kmers(mf_ctx *ctx, const char *const *in_files, int n_inputs, const char *const *filter_files, int n_filters, int max_bad, int k,
                               const char *kmers_bin, const char *stat_txt, uint64_t *n_pooled, uint64_t *n_good) {
    mf_range rng_("mf:unique_kmers(files)");
    if (!ctx || !kmers_bin || (n_inputs && !in_files) || (n_filters && !filter_files) || n_inputs < 0 || n_filters < 0)
        return mf_set_error("mf_unique_kmers: NULL argument");
    if (k < 1 || k > 31) return mf_set_error("k must be in [1,31]");
    MF_TRY(uk_check(n_inputs, max_bad));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0, tf = 0;
    MF_TRY(file_records(in_files, n_inputs, &total));
    MF_TRY(file_records(filter_files, n_filters, &tf));
    mf_table *hm = nullptr;
    MF_TRY(uk_join(ctx, mf_join_files(in_files, max_bad, k), n_inputs, mf_join_files(filter_files, max_bad, k), n_filters, total, max_bad, &hm));
    uint64_t w = 0;
    const int rc = mf_table_write_kmers(hm, max_bad, kmers_bin, stat_txt, &w);
    if (rc == MF_OK) { if (n_pooled) *n_pooled = hm->n; if (n_good) *n_good = w; }
    mf_table_destroy(hm);
    return rc;
}

// ---- kmers-multiple-filters ----
struct kmf_result { mf_table *kept = nullptr; std::vector<uint64_t> triples, counts; uint64_t found = 0; };
using kmf_sink = std::function<int(int j, kmf_result &r)>;          // takes r.kept over (destroys it)

// filter tables 0 = CD, 1 = UC, 2 = NONIBD (threshold 0), `total_f` an upper bound of their entries; inputs at threshold b
static int kmf_join(mf_ctx *ctx, const mf_join_get &get_filter, uint64_t total_f, const mf_join_get &get_in, int n_in, int b, const kmf_sink &sink) {
    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(plan_slices(ctx, total_f, &S, &cap));
    struct per_input { mf_join_parts<uint64_t, uint16_t> parts; std::map<uint64_t, uint64_t> hist; uint64_t found = 0; };
    std::vector<per_input> acc((size_t)n_in);
    mf_buf<unsigned int> flags; MF_TRY(flags.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(flags.p, 0, 4, ctx->stream));
    const uint32_t field[3] = {0u, 1u, 2u};
    for (uint32_t s = 0; s < S; s++) {
        mf_buf<mf_uslot> slots; uint64_t nu = 0;
        MF_TRY(mf_join_union(ctx, get_filter, 3, 0, MF_UNION_FIELD, field, S, s, cap, slots, &nu));
        for (int j = 0; j < n_in; j++) {
            per_input &a = acc[(size_t)j];
            mf_buf<uint64_t> ok, tri; mf_buf<uint16_t> ov;
            unsigned int cc[2] = {0, 0};
            uint64_t n = 0;
            {
                mf_join_sample sm(ctx);
                MF_TRY(get_in(j, sm));
                const mf_table *t = sm.t;
                n = t->n;
                if (n > MF_JOIN_CURSOR_MAX) return mf_set_error("kmers-multiple-filters: input %d has %llu entries, at most 2^32 - 1", j, (unsigned long long)n);
                MF_TRY(ok.alloc(ctx, n)); MF_TRY(ov.alloc(ctx, n)); MF_TRY(tri.alloc(ctx, n));
                MF_TRY(mf_join_cursors(ctx, 2, cc, [&](unsigned int *cur) {
                    if (!n) return;
                    mf_ktimer tm(ctx, "k_kmf_probe");
                    k_kmf_probe<<<grid_for(ctx, n), 256, 0, ctx->stream>>>(slots.p, cap - 1, t->d_keys, t->d_counts, n, b, S, s, ok.p, ov.p, tri.p, cur, flags.p);
                }, "kmers-multiple-filters: probe pass"));
            }
            if (cc[0] > n || cc[1] > n) return mf_set_error("kmers-multiple-filters: %u kept and %u found of %llu entries", cc[0], cc[1], (unsigned long long)n);
            MF_TRY(mf_join_flags(ctx, flags.p, "kmers-multiple-filters"));
            a.found += cc[1];
            MF_TRY(kmf_histogram(ctx, tri, cc[1], a.hist));
            tri.reset();
            // the kept records of this slice, in buffers of their size
            uint64_t *pk = nullptr; uint16_t *pv = nullptr;
            MF_TRY(a.parts.add(ctx, cc[0], &pk, &pv));
            if (cc[0]) {
                MF_HIP(hipMemcpyAsync(pk, ok.p, (size_t)cc[0] * 8, hipMemcpyDeviceToDevice, ctx->stream));
                MF_HIP(hipMemcpyAsync(pv, ov.p, (size_t)cc[0] * 2, hipMemcpyDeviceToDevice, ctx->stream));
                MF_HIP(hipStreamSynchronize(ctx->stream));
            }
            if (s + 1 < S) continue;
            // last slice: this input is complete
            ok.reset(); ov.reset();
            mf_buf<uint64_t> keys; mf_buf<uint16_t> vals; uint64_t nk = 0;
            MF_TRY(a.parts.concat(ctx, keys, vals, &nk));
            kmf_result r;
            MF_TRY(pairs_to_table(ctx, keys, vals, nk, &r.kept));
            r.found = a.found;
            for (auto &kv : a.hist) { r.triples.push_back(kv.first); r.counts.push_back(kv.second); }
            a.hist.clear();
            MF_TRY(sink(j, r));
        }
    }
    return MF_OK;
}

extern "C" int mf_kmers_multiple_filters_tables(mf_ctx *ctx, mf_table *table, mf_table *cd, mf_table *uc, mf_table *nonibd, int max_bad, mf_table **kept,
                                                uint64_t *triples, uint64_t *triple_counts, uint64_t cap, uint64_t *n_triples, uint64_t *found_kept) {
    mf_range rng_("mf:kmers_multiple_filters");
    if (!ctx || !table || !cd || !uc || !nonibd || !kept || !n_triples || !found_kept || (cap && (!triples || !triple_counts)))
        return mf_set_error("mf_kmers_multiple_filters_tables: NULL argument");
    *kept = nullptr;
    if (max_bad < 0) return mf_set_error("kmers-multiple-filters: maximal-bad-frequence = %d is negative", max_bad);
    MF_HIP(hipSetDevice(ctx->device));
    mf_table *all[4] = {cd, uc, nonibd, table};
    uint64_t total = 0;
    MF_TRY(tables_total(ctx, all, 4, "mf_kmers_multiple_filters_tables", &total));
    total -= table->n;
    const kmf_sink sink = [&](int, kmf_result &r) -> int {
        *kept = r.kept;
        *n_triples = r.triples.size();
        for (size_t i = 0; i < r.triples.size() && i < cap; i++) { triples[i] = r.triples[i]; triple_counts[i] = r.counts[i]; }
        found_kept[0] = r.found; found_kept[1] = r.kept->n;
        return MF_OK;
    };
    const int rc = kmf_join(ctx, mf_join_tables(all), total, mf_join_tables(&table), 1, max_bad, sink);
    if (rc != MF_OK && *kept) { mf_table_destroy(*kept); *kept = nullptr; }
    return rc;
}

extern "C" int mf_kmers_multiple_filters(mf_ctx *ctx, const char *const *in_files, int n_inputs, const char *const *cd_files, int n_cd,
                                         const char *const *uc_files, int n_uc, const char *const *nonibd_files, int n_nonibd, int max_bad, int k,
                                         const char *const *out_kmers, const char *const *out_stats, uint64_t *found_kept) {
    mf_range rng_("mf:kmers_multiple_filters(files)");
    if (!ctx || (n_inputs && (!in_files || !out_kmers)) || (n_cd && !cd_files) || (n_uc && !uc_files) || (n_nonibd && !nonibd_files) || n_inputs < 0 ||
        n_cd < 0 || n_uc < 0 || n_nonibd < 0)
        return mf_set_error("mf_kmers_multiple_filters: NULL argument");
    if (k < 1 || k > 31) return mf_set_error("k must be in [1,31]");
    if (max_bad < 0) return mf_set_error("kmers-multiple-filters: maximal-bad-frequence = %d is negative", max_bad);
    MF_HIP(hipSetDevice(ctx->device));
    const char *const *lists[3] = {cd_files, uc_files, nonibd_files};
    const int nl[3] = {n_cd, n_uc, n_nonibd};
    uint64_t total = 0, ti = 0;
    for (int g = 0; g < 3; g++) { uint64_t x = 0; MF_TRY(file_records(lists[g], nl[g], &x)); total += x; }
    MF_TRY(file_records(in_files, n_inputs, &ti));
    for (int j = 0; j < n_inputs; j++) if (!out_kmers[j]) return mf_set_error("mf_kmers_multiple_filters: output path %d is NULL", j);
    const mf_join_get gf = [&](int g, mf_join_sample &sm) -> int {
        if (nl[g]) return sm.load(lists[g], nl[g], 0, k);
        mf_table *none = nullptr;
        MF_TRY(empty_table(ctx, &none));
        return sm.adopt(none);
    };
    const kmf_sink sink = [&](int j, kmf_result &r) -> int {
        uint64_t w = 0;
        int rc = mf_table_write_kmers(r.kept, -1, out_kmers[j], nullptr, &w);
        if (rc == MF_OK && out_stats && out_stats[j]) {
            FILE *f = fopen(out_stats[j], "w");
            if (!f) rc = mf_set_error("can't write '%s'", out_stats[j]);
            else {
                fprintf(f, "# cd k-mer samples\tuc k-mer samples\tnonIBD k-mer samples\tnumber of such k-mers\n");
                for (size_t i = 0; i < r.triples.size(); i++)
                    fprintf(f, "%u\t%u\t%u\t%llu\n", (unsigned)(r.triples[i] >> 32) & 0xFFFFu, (unsigned)(r.triples[i] >> 16) & 0xFFFFu,
                            (unsigned)r.triples[i] & 0xFFFFu, (unsigned long long)r.counts[i]);
                fprintf(f, "\n");
                if (fclose(f) != 0) rc = mf_set_error("can't write '%s'", out_stats[j]);
            }
        }
        if (found_kept) { found_kept[2 * j] = r.found; found_kept[2 * j + 1] = w; }
        mf_table_destroy(r.kept); r.kept = nullptr;
        return rc;
    };
    return kmf_join(ctx, gf, total, mf_join_files(in_files, max_bad, k), n_inputs, max_bad, sink);
}
