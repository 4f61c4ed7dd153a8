// mf_wjoin.hip -- NO-REFERENCE EXTENSION (32 <= k <= 63): unique-kmers-multi and kmers-filter on 2k-bit k-mers (the definitions of
// UniqueKmersMultipleSamplesFinder.java:84-185 and IOUtils.filterAndPrintKmers src/io/IOUtils.java:101-123 carried over to (hi, lo) keys;
// DESIGN.md section 7l).  The join sorts and reduces, it claims nothing (mf_wjoin.h):
//   per slice of the key range   gather the inputs' entries with count > b (k_wj_gather) -> order them (mf_wide_sort_runs: a stable pass on the low
//                                word, one on the high word's 2k - 64 bits, run heads flagged on both words, scan) -> one thread per run reduces
//                                it to (hi, lo, samples, sum mod 2^16) (k_wj_reduce) -> every filter entry with count > b looks its k-mer up in the
//                                slice's ascending distinct k-mers and sets its knocked byte (k_wj_knock) -> the survivors, order kept
//   selection                    filtered_<i> = the survivors with samples >= i, by an order-keeping compaction (k_wj_flag, scan, k_wj_pick)
// Every reduction (a count, a sum mod 2^16, a byte that every writer sets to 1) is independent of the order inside a run: the result is a function of
// the samples alone, for every number of slices.  So is the group word of k_wj_reduce_groups (three counts of a run's entries by their sample's
// group; the callers are the three-group tools of mf_wstats.hip).
#include "mf_wjoin.h"
#include <algorithm>
#include <string>
#include <sys/stat.h>
#include <vector>

#define WJ_CAP_MAX (1ull << 31)        // entries of a slice and of a sample: the gather's cursor is 32-bit, and one sample more may pass it before the host looks
#define WJ_ENTRY_BYTES 112             // HBM a gathered entry stands for while its slice is ordered: 18 gathered, 32 + 10 + 12 in mf_wide_sort_runs, the radix sort's own pair

static unsigned wj_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 0x7FFFFFFFull); }

// the entries with count > b of a sample's piece that belong to slice s -> (ohi, olo, ocnt)[*cursor ...], in any order (the sort comes next); an entry
// past `cap` is counted and not written: the host reads the cursor and reports the slice.  (uniform trip count: mf_wave_reserve)
// weight >= 0: the payload of an entry is the sample's weight, not its count (mf_wjoin_slice_union)
__global__ __launch_bounds__(256) void k_wj_gather(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, const uint16_t *__restrict__ cnt, uint64_t n, int b, int weight,
                                                   int hb, uint32_t S, uint32_t s, uint64_t *__restrict__ ohi, uint64_t *__restrict__ olo, uint16_t *__restrict__ ocnt,
                                                   uint64_t cap, unsigned int *__restrict__ cursor) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n; i0 += stride) {
        const uint64_t i = i0 + threadIdx.x;
        bool keep = false;
        uint64_t h = 0, l = 0; uint16_t c = 0;
        if (i < n) {
            c = cnt[i];
            if ((int)c > b) { h = hi[i]; l = lo[i]; keep = mf_wjoin_slice(h, l, hb, S) == s; }
        }
        const uint32_t r = mf_wave_reserve(cursor, keep ? 1u : 0u);
        if (keep && (uint64_t)r < cap) { ohi[r] = h; olo[r] = l; ocnt[r] = weight >= 0 ? (uint16_t)weight : c; }
    }
}
// the head of a run of equal k-mers (at most one entry per sample: at most 32767 long) -> (hi, lo, entries, the sum of their counts mod 2^16) at the run's number
__global__ __launch_bounds__(256) void k_wj_reduce(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, const uint16_t *__restrict__ cnt,
                                                   const uint32_t *__restrict__ flag, const uint64_t *__restrict__ idx, uint64_t n, uint64_t *__restrict__ ohi,
                                                   uint64_t *__restrict__ olo, uint16_t *__restrict__ ocnt, uint16_t *__restrict__ osum) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    uint32_t c = 1, s = cnt[i];
    for (uint64_t j = i + 1; j < n && !flag[j]; j++) { c++; s += cnt[j]; }
    const uint64_t o = idx[i];
    ohi[o] = hi[i]; olo[o] = lo[i]; ocnt[o] = (uint16_t)c; osum[o] = (uint16_t)s;
}
// k_wj_reduce where the payload of an entry is its sample's group id (0, 1 or 2): the head of a run -> (hi, lo, entries, the run's entries by group as three
// MF_WJOIN_GROUP_BITS-bit fields).  A field is a count: it depends on the run's entries, not on their order (the host has checked that no group
// has more samples than a field holds; an id above 2 would be a shift out of the word and is refused there too)
__global__ __launch_bounds__(256) void k_wj_reduce_groups(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, const uint16_t *__restrict__ grp,
                                                          const uint32_t *__restrict__ flag, const uint64_t *__restrict__ idx, uint64_t n, uint64_t *__restrict__ ohi,
                                                          uint64_t *__restrict__ olo, uint16_t *__restrict__ ocnt, uint32_t *__restrict__ oword) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    uint32_t c = 1, w = 1u << (MF_WJOIN_GROUP_BITS * (uint32_t)(grp[i] & 3u));
    for (uint64_t j = i + 1; j < n && !flag[j]; j++) { c++; w += 1u << (MF_WJOIN_GROUP_BITS * (uint32_t)(grp[j] & 3u)); }
    const uint64_t o = idx[i];
    ohi[o] = hi[i]; olo[o] = lo[i]; ocnt[o] = (uint16_t)c; oword[o] = w;
}
// a filter sample's entries with count > b: a binary search in the slice's ascending distinct k-mers (dhi, dlo)[nd]; the one it finds is knocked out (a plain
// store: every writer writes 1).  A k-mer of another slice, or of no input, is not there.
__global__ __launch_bounds__(256) void k_wj_knock(const uint64_t *__restrict__ fhi, const uint64_t *__restrict__ flo, const uint16_t *__restrict__ fcnt, uint64_t nf, int b,
                                                  const uint64_t *__restrict__ dhi, const uint64_t *__restrict__ dlo, uint64_t nd, uint8_t *__restrict__ knocked) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf || (int)fcnt[i] <= b) return;
    const uint64_t h = fhi[i], l = flo[i];
    uint64_t a = 0, e = nd;
    while (a < e) {
        const uint64_t m = a + (e - a) / 2, mh = dhi[m];
        if (mh < h || (mh == h && dlo[m] < l)) a = m + 1; else e = m;
    }
    if (a < nd && dhi[a] == h && dlo[a] == l) knocked[a] = 1;
}
// the selector of a slice's k-mers: the samples that hold it where (short)sum > b and no filter knocked it out, else 0
__global__ __launch_bounds__(256) void k_wj_mark(const uint16_t *__restrict__ sum, const uint8_t *__restrict__ knocked, uint64_t n, int b, uint16_t *__restrict__ cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (knocked[i] || (int)(int16_t)sum[i] <= b) cnt[i] = 0;
}
__global__ __launch_bounds__(256) void k_wj_flag(const uint16_t *__restrict__ sel, uint64_t n, int thr, uint32_t *__restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = (int)sel[i] > thr ? 1u : 0u;
}
// the flagged entries to their place idx[i], order kept; osel may be NULL
__global__ __launch_bounds__(256) void k_wj_pick(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, const uint16_t *__restrict__ val, const uint16_t *__restrict__ sel,
                                                 const uint32_t *__restrict__ flag, const uint64_t *__restrict__ idx, uint64_t n, uint64_t *__restrict__ ohi,
                                                 uint64_t *__restrict__ olo, uint16_t *__restrict__ oval, uint16_t *__restrict__ osel) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const uint64_t o = idx[i];
    ohi[o] = hi[i]; olo[o] = lo[i]; oval[o] = val[i];
    if (osel) osel[o] = sel[i];
}
// kmers-filter: sel = an entry's count where it is > thr and the filter's value of its k-mer (absent: 0) is > fthr, else 0.  fx.n == 0: an empty filter
__global__ __launch_bounds__(256) void k_wj_keep(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, const uint16_t *__restrict__ cnt, uint64_t n, int thr,
                                                 mf_windex_view fx, int fthr, uint16_t *__restrict__ sel) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint16_t c = cnt[i];
    int fv = 0;
    if ((int)c > thr && fx.n) {
        const uint32_t p = mf_windex_find(fx, hi[i], lo[i]);
        if (p != 0xFFFFFFFFu) fv = (int)fx.cnt[p];
    }
    sel[i] = ((int)c > thr && fv > fthr) ? c : (uint16_t)0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
mf_wjoin_sample::~mf_wjoin_sample() { if (own && t) { (void)hipStreamSynchronize(ctx->stream); mf_wtable_destroy(t); } }

// Slices bound memory: a slice's gathered entries and the sort's buffers (WJ_ENTRY_BYTES each) are to fit in 0.4 of the free HBM, as plan_slices
// (mf_join.hip) allows the narrow union table.  Slices are equal ranges of the key's leading bits, and canonical k-mers are not spread evenly over them
// (a k-mer that starts with A is canonical 7 times in 8, one that starts with T once in 8: up to 7/4 of the mean), so a slice gets room for twice
// the mean -- and all the room the budget has where that is more: a slice that still overflows is an error that names the option, never a write
// out of bounds.
int mf_wjoin_plan(mf_ctx *ctx, uint64_t total, uint32_t *S_out, uint64_t *cap_out) {
    uint32_t S = (uint32_t)std::max<int64_t>(ctx->opt_stats_slices, 0);
    size_t fr = 0, tot = 0;
    MF_HIP(hipMemGetInfo(&fr, &tot));
    const uint64_t budget = (uint64_t)(0.4 * (double)(fr + mf_arena_idle(ctx)) / WJ_ENTRY_BYTES);
    auto room = [&](uint32_t s) { return s == 1 ? total : std::min<uint64_t>(total, 2 * (total / s) + 1024); };
    if (!S) {
        S = 1;
        while (S < 4096 && room(S) > std::min<uint64_t>(budget, WJ_CAP_MAX)) S++;
    }
    const uint64_t cap = std::min<uint64_t>(std::min<uint64_t>(total, std::max<uint64_t>(room(S), budget)), WJ_CAP_MAX);
    if (S == 4096 && room(S) > cap) return mf_set_error("wide join: %llu entries do not fit", (unsigned long long)total);
    *S_out = S;
    *cap_out = std::max<uint64_t>(cap, 1);
    return MF_OK;
}

int mf_wjoin_slice_union(mf_ctx *ctx, int k, const mf_wjoin_get &get, int n_in, int b, uint32_t S, uint32_t s, uint64_t cap, mf_wjoin_union &u,
                         const uint16_t *weight, const uint8_t *group) {
    hipStream_t st = ctx->stream;
    const int hb = 2 * k - 64;
    u.n = 0;
    if (group) {
        if (weight) return mf_set_error("wide join: weights and groups together");
        int per[3] = {0, 0, 0};
        for (int j = 0; j < n_in; j++) {
            if (group[j] > 2) return mf_set_error("wide join: input %d has group %d, at most 2", j, (int)group[j]);
            per[group[j]]++;
        }
        for (int g = 0; g < 3; g++)
            if (per[g] > MF_WJOIN_GROUP_MAX) return mf_set_error("wide join: %d inputs in group %d, at most %d", per[g], g, MF_WJOIN_GROUP_MAX);
    }
    auto payload = [&](int j) { return group ? (int)group[j] : weight ? (int)weight[j] : -1; };
    mf_buf<uint64_t> ghi, glo; mf_buf<uint16_t> gcnt; mf_buf<unsigned int> cur;
    MF_TRY(ghi.alloc(ctx, cap)); MF_TRY(glo.alloc(ctx, cap)); MF_TRY(gcnt.alloc(ctx, cap)); MF_TRY(cur.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(cur.p, 0, 4, st));
    unsigned int m = 0;
    for (int j = 0; j < n_in; j++) {
        mf_wjoin_sample sm(ctx);
        MF_TRY(get(j, sm));
        if (sm.t->n >= WJ_CAP_MAX) return mf_set_error("wide join: input %d has %llu entries, at most 2^31 - 1", j, (unsigned long long)sm.t->n);
        for (auto &pc : sm.t->pieces) {
            if (!pc->n) continue;
            mf_ktimer tm(ctx, "k_wj_gather");
            k_wj_gather<<<wj_grid(pc->n), 256, 0, st>>>(pc->hi.p, pc->lo.p, pc->cnt.p, pc->n, b, payload(j), hb, S, s, ghi.p, glo.p, gcnt.p, cap, cur.p);
        }
        MF_HIP(hipMemcpyAsync(&m, cur.p, 4, hipMemcpyDeviceToHost, st));
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) return mf_set_error("wide join: gather pass failed: %s", hipGetErrorString(e));
        if ((uint64_t)m > cap)
            return mf_set_error("wide join: slice %u of %u holds more than %llu entries (raise option stats_slices)", s, S, (unsigned long long)cap);
    }
    if (!m) return MF_OK;
    mf_wide_runs r;
    MF_TRY(mf_wide_sort_runs(ctx, k, ghi.p, glo.p, gcnt.p, m, r));
    ghi.reset(); glo.reset(); gcnt.reset();
    const uint64_t nd = r.n_runs;
    MF_TRY(u.hi.alloc(ctx, nd)); MF_TRY(u.lo.alloc(ctx, nd)); MF_TRY(u.cnt.alloc(ctx, nd)); MF_TRY(u.knocked.alloc(ctx, nd));
    MF_HIP(hipMemsetAsync(u.knocked.p, 0, nd, st));
    if (group) {
        MF_TRY(u.grp.alloc(ctx, nd));
        mf_ktimer tm(ctx, "k_wj_reduce_groups");
        k_wj_reduce_groups<<<wj_grid(m), 256, 0, st>>>(r.hi.p, r.lo.p, r.cnt.p, r.flag.p, r.idx.p, m, u.hi.p, u.lo.p, u.cnt.p, u.grp.p);
    } else {
        MF_TRY(u.sum.alloc(ctx, nd));
        mf_ktimer tm(ctx, "k_wj_reduce");
        k_wj_reduce<<<wj_grid(m), 256, 0, st>>>(r.hi.p, r.lo.p, r.cnt.p, r.flag.p, r.idx.p, m, u.hi.p, u.lo.p, u.cnt.p, u.sum.p);
    }
    MF_HIP(hipStreamSynchronize(st));
    u.n = nd;
    return MF_OK;
}

int mf_wjoin_knock(mf_ctx *ctx, const mf_wtable *t, int b, mf_wjoin_union &u) {
    if (!u.n) return MF_OK;
    for (auto &pc : t->pieces) {
        if (!pc->n) continue;
        mf_ktimer tm(ctx, "k_wj_knock");
        k_wj_knock<<<wj_grid(pc->n), 256, 0, ctx->stream>>>(pc->hi.p, pc->lo.p, pc->cnt.p, pc->n, b, u.hi.p, u.lo.p, u.n, u.knocked.p);
    }
    return MF_OK;
}

// the entries with sel > thr of (hi, lo, val, sel)[n], order kept -> (ohi, olo, oval[, osel])[*m]
int mf_wjoin_select(mf_ctx *ctx, const uint64_t *hi, const uint64_t *lo, const uint16_t *val, const uint16_t *sel, uint64_t n, int thr, mf_buf<uint64_t> &ohi,
                    mf_buf<uint64_t> &olo, mf_buf<uint16_t> &oval, mf_buf<uint16_t> *osel, uint64_t *m) {
    hipStream_t st = ctx->stream;
    uint64_t keep = 0;
    mf_buf<uint32_t> flag; mf_buf<uint64_t> idx, tot;
    MF_TRY(flag.alloc(ctx, n)); MF_TRY(idx.alloc(ctx, n + 1)); MF_TRY(tot.alloc(ctx, 1));
    if (n) {
        mf_ktimer tm(ctx, "k_wj_flag");
        k_wj_flag<<<wj_grid(n), 256, 0, st>>>(sel, n, thr, flag.p);
    }
    if (n) {
        MF_TRY(mf_scan<1>(ctx, flag.p, idx.p, n, tot.p));
        MF_HIP(hipMemcpyAsync(&keep, tot.p, 8, hipMemcpyDeviceToHost, st));
        MF_HIP(hipStreamSynchronize(st));
    }
    MF_TRY(ohi.alloc(ctx, keep)); MF_TRY(olo.alloc(ctx, keep)); MF_TRY(oval.alloc(ctx, keep));
    if (osel) MF_TRY(osel->alloc(ctx, keep));
    if (keep) {
        mf_ktimer tm(ctx, "k_wj_pick");
        k_wj_pick<<<wj_grid(n), 256, 0, st>>>(hi, lo, val, sel, flag.p, idx.p, n, ohi.p, olo.p, oval.p, osel ? osel->p : nullptr);
    }
    MF_HIP(hipStreamSynchronize(st));
    *m = keep;
    return MF_OK;
}

static int wukm_check(int n_in, int max_bad, int min_samples, int max_samples) {
    if (max_bad < 0) return mf_set_error("unique-kmers-multi: maximal-bad-frequence = %d is negative", max_bad);
    if (n_in > 32767) return mf_set_error("unique-kmers-multi: %d input files, at most 32767 (the number of samples is a Java short)", n_in);
    if (min_samples > max_samples) return mf_set_error("--min-samples parameter cannot be greater than --max-samples parameter.");
    return MF_OK;
}
int mf_wjoin_table(mf_ctx *ctx, int k, int cut, mf_buf<uint64_t> &hi, mf_buf<uint64_t> &lo, mf_buf<uint16_t> &cnt, uint64_t n, mf_wtable **out) {
    auto t = std::make_unique<mf_wtable>();
    t->ctx = ctx; t->k = k; t->n = n; t->n_all = n; t->n_occ = 0; t->cut_thr = cut; t->ascending = true;
    if (n) {
        auto pc = std::make_unique<mf_wtable::piece>();
        pc->hi.swap(hi); pc->lo.swap(lo); pc->cnt.swap(cnt); pc->n = n;
        t->pieces.push_back(std::move(pc));
    }
    *out = t.release();
    return MF_OK;
}
static void wj_destroy_all(std::vector<mf_wtable *> &v) { for (mf_wtable *t : v) mf_wtable_destroy(t); v.clear(); }

// -> outs: one table per i = min_samples, min_samples + 1, ... up to max_samples or the first empty one (included); counts: their sizes
static int wukm_join(mf_ctx *ctx, int k, const mf_wjoin_get &get_in, int n_in, const mf_wjoin_get &get_f, int n_f, uint64_t total, int b, int min_samples,
                     int max_samples, std::vector<mf_wtable *> &outs, std::vector<uint64_t> &counts, uint64_t *n_union) {
    hipStream_t st = ctx->stream;
    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(mf_wjoin_plan(ctx, total, &S, &cap));
    struct part { mf_buf<uint64_t> hi, lo; mf_buf<uint16_t> sum, sel; uint64_t n = 0; };
    std::vector<std::unique_ptr<part>> parts;
    *n_union = 0;
    uint64_t n = 0;
    for (uint32_t s = 0; s < S; s++) {
        mf_wjoin_union u;
        MF_TRY(mf_wjoin_slice_union(ctx, k, get_in, n_in, b, S, s, cap, u));
        if (!u.n) continue;
        *n_union += u.n;
        for (int j = 0; j < n_f; j++) {
            mf_wjoin_sample sm(ctx);
            MF_TRY(get_f(j, sm));
            MF_TRY(mf_wjoin_knock(ctx, sm.t, b, u));
            const hipError_t e = hipStreamSynchronize(st);
            if (e != hipSuccess) return mf_set_error("unique-kmers-multi: filter pass failed: %s", hipGetErrorString(e));
        }
        {
            mf_ktimer tm(ctx, "k_wj_mark");
            k_wj_mark<<<wj_grid(u.n), 256, 0, st>>>(u.sum.p, u.knocked.p, u.n, b, u.cnt.p);
        }
        // the survivors of the slice, in buffers of their size
        auto p = std::make_unique<part>();
        MF_TRY(mf_wjoin_select(ctx, u.hi.p, u.lo.p, u.sum.p, u.cnt.p, u.n, 0, p->hi, p->lo, p->sum, &p->sel, &p->n));
        n += p->n;
        if (p->n) parts.push_back(std::move(p));
    }
    // one ascending list of the survivors: the slices are ranges of the key, in ascending order
    part all;
    if (parts.size() == 1) { all.hi.swap(parts[0]->hi); all.lo.swap(parts[0]->lo); all.sum.swap(parts[0]->sum); all.sel.swap(parts[0]->sel); }
    else {
        MF_TRY(all.hi.alloc(ctx, n)); MF_TRY(all.lo.alloc(ctx, n)); MF_TRY(all.sum.alloc(ctx, n)); MF_TRY(all.sel.alloc(ctx, n));
        uint64_t at = 0;
        for (auto &p : parts) {
            MF_HIP(hipMemcpyAsync(all.hi.p + at, p->hi.p, p->n * 8, hipMemcpyDeviceToDevice, st));
            MF_HIP(hipMemcpyAsync(all.lo.p + at, p->lo.p, p->n * 8, hipMemcpyDeviceToDevice, st));
            MF_HIP(hipMemcpyAsync(all.sum.p + at, p->sum.p, p->n * 2, hipMemcpyDeviceToDevice, st));
            MF_HIP(hipMemcpyAsync(all.sel.p + at, p->sel.p, p->n * 2, hipMemcpyDeviceToDevice, st));
            at += p->n;
        }
        MF_HIP(hipStreamSynchronize(st));
    }
    parts.clear();
    // filtered_<i>: the subsequence with samples > i - 1
    for (int64_t i = min_samples; i <= (int64_t)max_samples; i++) {
        mf_buf<uint64_t> ohi, olo; mf_buf<uint16_t> ov; uint64_t m = 0;
        // (no key is held by more than n_in samples, and every survivor by at least one)
        if (i <= n_in) MF_TRY(mf_wjoin_select(ctx, all.hi.p, all.lo.p, all.sum.p, all.sel.p, n, (int)std::max<int64_t>(i - 1, 0), ohi, olo, ov, nullptr, &m));
        mf_wtable *t = nullptr;
        MF_TRY(mf_wjoin_table(ctx, k, b, ohi, olo, ov, m, &t));
        outs.push_back(t);
        counts.push_back(m);
        if (!m) break;
    }
    return MF_OK;
}

// the k of a list of tables, every one checked: NULL, another context, another k.  *k = 0: no table so far
int mf_wjoin_tables_check(mf_ctx *ctx, mf_wtable *const *t, int n, const char *what, int *k, uint64_t *total) {
    for (int j = 0; j < n; j++) {
        if (!t[j]) return mf_set_error("%s: table %d is NULL", what, j);
        if (t[j]->ctx != ctx) return mf_set_error("%s: table %d belongs to another context", what, j);
        if (t[j]->k < 32 || t[j]->k > 63) return mf_set_error("%s: table %d has k = %d, 32 <= k <= 63", what, j, t[j]->k);
        if (!*k) *k = t[j]->k;
        if (t[j]->k != *k) return mf_set_error("%s: table %d has k = %d, the others k = %d", what, j, t[j]->k, *k);
        if (total) *total += t[j]->n;
    }
    return MF_OK;
}

extern "C" int mf_unique_kmers_multi_wide_tables(mf_ctx *ctx, mf_wtable *const *inputs, int n_inputs, mf_wtable *const *filters, int n_filters, int max_bad,
                                                 int min_samples, int max_samples, mf_wtable **out, int *n_out, uint64_t *n_union, uint64_t *counts) {
    mf_range rng_("mf:unique_kmers_multi_wide");
    if (!ctx || !out || !n_out || !n_union || !counts || (n_inputs && !inputs) || (n_filters && !filters) || n_inputs < 0 || n_filters < 0)
        return mf_set_error("mf_unique_kmers_multi_wide_tables: NULL argument");
    *n_out = 0;
    MF_TRY(wukm_check(n_inputs, max_bad, min_samples, max_samples));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0; int k = 0;
    MF_TRY(mf_wjoin_tables_check(ctx, inputs, n_inputs, "mf_unique_kmers_multi_wide_tables (inputs)", &k, &total));
    MF_TRY(mf_wjoin_tables_check(ctx, filters, n_filters, "mf_unique_kmers_multi_wide_tables (filters)", &k, nullptr));
    if (!k) k = 32;                                         // (no table at all: one empty result)
    const mf_wjoin_get gi = [inputs](int j, mf_wjoin_sample &s) { s.t = inputs[j]; return MF_OK; };
    const mf_wjoin_get gf = [filters](int j, mf_wjoin_sample &s) { s.t = filters[j]; return MF_OK; };
    std::vector<mf_wtable *> outs; std::vector<uint64_t> cs;
    const int rc = wukm_join(ctx, k, gi, n_inputs, gf, n_filters, total, max_bad, min_samples, max_samples, outs, cs, n_union);
    if (rc != MF_OK) { wj_destroy_all(outs); return rc; }
    for (size_t i = 0; i < outs.size(); i++) { out[i] = outs[i]; counts[i] = cs[i]; }
    *n_out = (int)outs.size();
    return MF_OK;
}

int mf_wjoin_file_records(const char *const *files, int n, uint64_t *total) {
    *total = 0;
    for (int j = 0; j < n; j++) {
        if (!files[j]) return mf_set_error("file %d is NULL", j);
        struct stat st;
        if (stat(files[j], &st) != 0) return mf_set_error("can't open '%s'", files[j]);
        *total += (uint64_t)st.st_size / 18;
    }
    return MF_OK;
}

extern "C" int mf_unique_kmers_multi_wide(mf_ctx *ctx, const char *const *in_files, int n_inputs, const char *const *filter_files, int n_filters, int max_bad,
                                          int k, int min_samples, int max_samples, const char *out_dir, int *n_out, uint64_t *n_union, uint64_t *counts) {
    mf_range rng_("mf:unique_kmers_multi_wide(files)");
    if (!ctx || !out_dir || !n_out || !n_union || !counts || (n_inputs && !in_files) || (n_filters && !filter_files) || n_inputs < 0 || n_filters < 0)
        return mf_set_error("mf_unique_kmers_multi_wide: NULL argument");
    *n_out = 0;
    if (k < 32 || k > 63) return mf_set_error("mf_unique_kmers_multi_wide: 32 <= k <= 63 (k <= 31: mf_unique_kmers_multi)");
    MF_TRY(wukm_check(n_inputs, max_bad, min_samples, max_samples));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0, tf = 0;
    MF_TRY(mf_wjoin_file_records(in_files, n_inputs, &total));
    MF_TRY(mf_wjoin_file_records(filter_files, n_filters, &tf));
    // one sample resident at a time, loaded like IOUtils.loadKmers(file, b)
    auto files = [ctx, max_bad, k](const char *const *f) {
        return [=](int j, mf_wjoin_sample &s) { s.own = true; return mf_wtable_load_kmers(ctx, f + j, 1, max_bad, k, &s.t); };
    };
    std::vector<mf_wtable *> outs; std::vector<uint64_t> cs;
    int rc = wukm_join(ctx, k, files(in_files), n_inputs, files(filter_files), n_filters, total, max_bad, min_samples, max_samples, outs, cs, n_union);
    for (size_t i = 0; i < outs.size() && rc == MF_OK; i++) {
        uint64_t w = 0;
        rc = mf_wtable_write_kmers(outs[i], -1, (std::string(out_dir) + "/filtered_" + std::to_string((long long)min_samples + (long long)i) + ".kmers.bin").c_str(), nullptr, &w);
    }
    if (rc == MF_OK) { for (size_t i = 0; i < cs.size(); i++) counts[i] = cs[i]; *n_out = (int)cs.size(); }
    wj_destroy_all(outs);
    return rc;
}

// ---- kmers-filter (IOUtils.filterAndPrintKmers, src/io/IOUtils.java:101-123) ----
extern "C" int mf_wtable_write_kmers_filtered(mf_wtable *t, int threshold, mf_wtable *filter, int filter_threshold, const char *kmers_bin, uint64_t *n_written) {
    mf_range rng_("mf:write_kmers_filtered_wide(file)");
    if (!t || !filter || !kmers_bin) return mf_set_error("mf_wtable_write_kmers_filtered: NULL argument");
    if (t->ctx != filter->ctx) return mf_set_error("mf_wtable_write_kmers_filtered: the filter table belongs to another context");
    if (t->k != filter->k) return mf_set_error("mf_wtable_write_kmers_filtered: tables with different k (%d, %d)", t->k, filter->k);
    mf_ctx *ctx = t->ctx;
    MF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    MF_TRY(mf_wtable_ensure_ascending(t));
    if (filter->n) MF_TRY(mf_wtable_ensure_index(filter));
    const mf_windex_view fx = mf_wtable_view(filter);
    mf_wtable kept;
    kept.ctx = ctx; kept.k = t->k; kept.cut_thr = std::max(threshold, 0); kept.ascending = true;
    for (auto &pc : t->pieces) {
        if (!pc->n) continue;
        mf_buf<uint16_t> sel; MF_TRY(sel.alloc(ctx, pc->n));
        {
            mf_ktimer tm(ctx, "k_wj_keep");
            k_wj_keep<<<wj_grid(pc->n), 256, 0, st>>>(pc->hi.p, pc->lo.p, pc->cnt.p, pc->n, threshold, fx, filter_threshold, sel.p);
        }
        auto kp = std::make_unique<mf_wtable::piece>();
        MF_TRY(mf_wide_compact(ctx, pc->hi.p, pc->lo.p, sel.p, pc->n, 0, *kp));      // (a kept entry's selector is its count, >= 1)
        kept.n += kp->n;
        if (kp->n) kept.pieces.push_back(std::move(kp));
    }
    kept.n_all = kept.n;
    return mf_wtable_write_kmers(&kept, -1, kmers_bin, nullptr, n_written);
}
