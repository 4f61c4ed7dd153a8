// mf_wstats.hip -- NO-REFERENCE EXTENSION (32 <= k <= 63): stats-kmers on 2k-bit k-mers, the definition of mf_stats_kmers_tables
// (StatsKmersFinder.java:89-297) carried over to (hi, lo) keys on the wide join core (mf_wjoin.h),
// and the wide sample counter (KmersSamplesCounter.java:69-140), which is the same union with nothing behind it.
//   union    per slice of the key range, mf_wjoin_slice_union at threshold max_bad with WEIGHTS 1 for the samples of A and 0 for those of B:
//            sum = n1A, cnt - sum = n1B (both <= 1024: the 16-bit sum cannot wrap)
//   select   k_wstats_select: the first five counters and a keep flag from the host's (nA + 1) x (nB + 1) chi-squared table (chisq_keep,
//            mf_stats.h: no floating-point decision on the device); mf_wjoin_select compacts the survivors, order kept -- row r of a slice
//            is its r-th surviving k-mer, ascending
//   gather   the samples again at threshold 0 (k_wstats_gather): one thread per entry with count != 0, a binary search on two words among the
//            slice's m survivors, the count into mat[row * N + j] of a zeroed u16 [m][N] matrix; F_j = the sum of sample j's counts, once
//   rows     the row kernels of mf_stats.hip UNCHANGED (mf_stats_rows_launch), handed the row numbers 0 .. m - 1 as their keys; each group's
//            (row, value) pairs sorted by row (mf_sort_pairs) -- row order is k-mer order -- and turned into (hi, lo) (k_wstats_keys)
// The slices are ascending ranges of the key, so their pieces one after the other are the three ascending tables, for every number of slices.
// A group table's values are Java (short)(int) means: 0 and values >= 0x8000 occur and are kept as the u16 they are.  A group FILE may therefore
// hold records with a value <= 0, which mf_wtable_load_kmers refuses by design (a count is positive); `view --wide-kmers` reads such a file on
// the host.
#include "mf_stats.h"
#include "mf_wjoin.h"
#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

// ---------------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------------
// pass 1 over a slice's union (k_stats_select on (cnt, sum) in place of the presence word): counters [0] n, [1] scarce, [2] in all, [3] unique,
// [4] chi-squared rejected; keep[i] = 1 for a survivor, else 0.  (every lane leaves the loop before the wave sums of mf_stats_add)
__global__ __launch_bounds__(256) void k_wstats_select(const uint16_t *__restrict__ cnt, const uint16_t *__restrict__ sum, uint64_t n, const uint8_t *__restrict__ chi_keep,
                                                       int na, int nb, int scarce_max, uint16_t *__restrict__ keep, unsigned long long *__restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t c_n = 0, c_scarce = 0, c_all = 0, c_uniq = 0, c_rej = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int n1a = (int)sum[i], n1b = (int)cnt[i] - n1a;
        uint16_t kp = 0;
        c_n++;
        if (n1a + n1b <= scarce_max) c_scarce++;
        else if (n1a + n1b == na + nb) c_all++;
        else {
            if (n1a == 0 || n1b == 0) c_uniq++;
            if (chi_keep[(size_t)n1a * (size_t)(nb + 1) + (size_t)n1b]) kp = 1;
            else c_rej++;
        }
        keep[i] = kp;
    }
    mf_stats_add(&ctr[0], c_n); mf_stats_add(&ctr[1], c_scarce); mf_stats_add(&ctr[2], c_all); mf_stats_add(&ctr[3], c_uniq); mf_stats_add(&ctr[4], c_rej);
}

// sample `col`'s entries with count != 0 into its column of the survivors' matrix: mat[row * N + col] = count, row = the k-mer's place in the slice's
// ascending survivors (shi, slo)[m].  A k-mer of another slice, or of no survivor, is not there: the row of one that is lies below m by the search
// itself.  (a sample's k-mers are distinct: plain stores)
__global__ __launch_bounds__(256) void k_wstats_gather(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, const uint16_t *__restrict__ cnt, uint64_t n,
                                                       const uint64_t *__restrict__ shi, const uint64_t *__restrict__ slo, uint64_t m, uint32_t col, uint32_t N,
                                                       uint16_t *__restrict__ mat) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint16_t c = cnt[i];
        if (!c) continue;
        const uint64_t h = hi[i], l = lo[i];
        uint64_t a = 0, e = m;
        while (a < e) {
            const uint64_t mid = a + (e - a) / 2, mh = shi[mid];
            if (mh < h || (mh == h && slo[mid] < l)) a = mid + 1; else e = mid;
        }
        if (a < m && shi[a] == h && slo[a] == l) mat[a * (uint64_t)N + col] = c;
    }
}

// the row numbers 0 .. m - 1: what the row kernels carry through to the group lists in place of a key
__global__ __launch_bounds__(256) void k_wstats_iota(uint64_t *__restrict__ rows, uint64_t m) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) rows[i] = i;
}
// a group's rows, ascending -> their k-mers (a row is below m: the row kernels hand on what k_wstats_iota wrote)
__global__ __launch_bounds__(256) void k_wstats_keys(const uint64_t *__restrict__ rows, uint64_t n, const uint64_t *__restrict__ shi, const uint64_t *__restrict__ slo, uint64_t m,
                                                     uint64_t *__restrict__ ohi, uint64_t *__restrict__ olo) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t r = rows[i];
    if (r < m) { ohi[i] = shi[r]; olo[i] = slo[r]; }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
static unsigned wstats_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 0x7FFFFFFFull); }

// an error of the join core or of a loader, with the tool's name in front
static int wstats_named(const char *tool, int rc) {
    if (rc >= 0) return rc;
    const std::string e = mf_last_error();
    return mf_set_error("%s (--wide-kmers): %s", tool, e.c_str());
}

// the ascending (hi, lo, value) pieces the slices leave, one after the other -> one table
struct wstats_parts {
    struct part { mf_buf<uint64_t> hi, lo; mf_buf<uint16_t> val; uint64_t n = 0; };
    std::vector<std::unique_ptr<part>> parts;
    uint64_t n = 0;
    part *add() { parts.emplace_back(new part()); return parts.back().get(); }
    void wrote(uint64_t m) { parts.back()->n = m; n += m; if (!m) parts.pop_back(); }
    int table(mf_ctx *ctx, int k, int cut, mf_wtable **out) {
        mf_buf<uint64_t> hi, lo; mf_buf<uint16_t> val;
        if (parts.size() == 1) { hi.swap(parts[0]->hi); lo.swap(parts[0]->lo); val.swap(parts[0]->val); }
        else if (n) {
            MF_TRY(hi.alloc(ctx, n)); MF_TRY(lo.alloc(ctx, n)); MF_TRY(val.alloc(ctx, n));
            uint64_t at = 0;
            for (auto &p : parts) {
                MF_HIP(hipMemcpyAsync(hi.p + at, p->hi.p, p->n * 8, hipMemcpyDeviceToDevice, ctx->stream));
                MF_HIP(hipMemcpyAsync(lo.p + at, p->lo.p, p->n * 8, hipMemcpyDeviceToDevice, ctx->stream));
                MF_HIP(hipMemcpyAsync(val.p + at, p->val.p, p->n * 2, hipMemcpyDeviceToDevice, ctx->stream));
                at += p->n;
            }
            MF_HIP(hipStreamSynchronize(ctx->stream));
        }
        parts.clear();
        return mf_wjoin_table(ctx, k, cut, hi, lo, val, n, out);
    }
};

static int wstats_matrix_fits(mf_ctx *ctx, int N, uint64_t m) {
    size_t fr = 0, tot = 0;
    MF_HIP(hipMemGetInfo(&fr, &tot));
    const uint64_t room = (uint64_t)fr + mf_arena_idle(ctx);
    if (m > room / 2 / (uint64_t)N)
        return mf_set_error("stats-kmers (--wide-kmers): the count matrix of %llu k-mers x %d samples x 2 bytes of a slice does not fit the %llu bytes of free "
                            "device memory (raise option stats_slices)", (unsigned long long)m, N, (unsigned long long)room);
    return MF_OK;
}

// the join of na + nb samples, A first; get(j): sample j as it is read in both passes (every entry, the kernels cut at max_bad and at 0)
static int wstats_join(mf_ctx *ctx, int k, const mf_wjoin_get &get, int na, int nb, uint64_t total, int b, double pchi2, double pmw, mf_wtable **chi_out,
                       mf_wtable **ga_out, mf_wtable **gb_out, uint64_t *counters) {
    static const char *tool = "stats-kmers";
    hipStream_t st = ctx->stream;
    const int N = na + nb;
    // the decisions' tables, by the host functions of the narrow tool
    const double q = chi2_1_quantile(pchi2);
    std::vector<uint8_t> chi((size_t)(na + 1) * (nb + 1), 0);
    for (int n1a = 0; n1a <= na; n1a++)
        for (int n1b = 0; n1b <= nb; n1b++)
            chi[(size_t)n1a * (nb + 1) + n1b] = chisq_keep((float)(na - n1a), (float)n1a, (float)(nb - n1b), (float)n1b, q) ? 1 : 0;
    const int scarce_max = (int)std::ceil(N * 0.05);
    const int mw = pmw > 0 ? 1 : 0;
    const uint32_t T = mw ? mw_threshold(na, nb, pmw) : 0u;
    if (ctx->opt_verbose) fprintf(stderr, "[mf] stats (wide): q = %.17g, scarce <= %d, 2*Umin < %u\n", q, scarce_max, T);
    mf_buf<uint8_t> dchi; MF_TRY(dchi.alloc(ctx, chi.size()));
    MF_HIP(hipMemcpyAsync(dchi.p, chi.data(), chi.size(), hipMemcpyHostToDevice, st));
    mf_buf<unsigned long long> ctr; MF_TRY(ctr.alloc(ctx, MF_STATS_COUNTERS));
    MF_HIP(hipMemsetAsync(ctr.p, 0, MF_STATS_COUNTERS * 8, st));
    MF_HIP(hipStreamSynchronize(st));                      // (chi is the host's until here)

    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(wstats_named(tool, mf_wjoin_plan(ctx, total, &S, &cap)));
    std::vector<uint16_t> weight((size_t)N, (uint16_t)0);
    for (int j = 0; j < na; j++) weight[(size_t)j] = 1;
    std::vector<uint64_t> F((size_t)N, 0);
    std::vector<bool> have((size_t)N, false);
    bool have_F = false;
    mf_buf<double> dF; MF_TRY(dF.alloc(ctx, N));
    double M = 0.0;
    wstats_parts p_chi, p_a, p_b;
    for (uint32_t s = 0; s < S; s++) {
        // union and select
        wstats_parts::part *pc = p_chi.add();
        uint64_t m = 0;
        {
            mf_wjoin_union u;
            MF_TRY(wstats_named(tool, mf_wjoin_slice_union(ctx, k, get, N, b, S, s, cap, u, weight.data())));
            if (u.n) {
                mf_buf<uint16_t> keep; MF_TRY(keep.alloc(ctx, u.n));
                {
                    mf_ktimer tm(ctx, "k_wstats_select");
                    const unsigned grid = (unsigned)std::min<uint64_t>((u.n + 255) / 256, (uint64_t)std::max(ctx->n_cu, 1) * 16);
                    k_wstats_select<<<grid, 256, 0, st>>>(u.cnt.p, u.sum.p, u.n, dchi.p, na, nb, scarce_max, keep.p, ctr.p);
                }
                // (the survivors' value is their keep flag: the 1 of the chi-squared list)
                MF_TRY(mf_wjoin_select(ctx, u.hi.p, u.lo.p, keep.p, keep.p, u.n, 0, pc->hi, pc->lo, pc->val, nullptr, &m));
            }
        }
        const uint64_t *shi = pc->hi.p, *slo = pc->lo.p;
        p_chi.wrote(m);                                    // (an empty piece is dropped: shi / slo are not read for m = 0)
        if (!m && have_F) continue;
        // gather
        mf_buf<uint16_t> mat;
        if (m) {
            MF_TRY(wstats_matrix_fits(ctx, N, m));
            MF_TRY(mat.alloc(ctx, m * (uint64_t)N));
            MF_HIP(hipMemsetAsync(mat.p, 0, m * (uint64_t)N * 2, st));
        }
        for (int j = 0; j < N; j++) {
            mf_wjoin_sample sm(ctx);
            MF_TRY(wstats_named(tool, get(j, sm)));
            if (!have[(size_t)j]) {
                for (auto &piece : sm.t->pieces) {
                    uint64_t f = 0;
                    MF_TRY(mf_sum_counts(ctx, piece->cnt.p, piece->n, &f));
                    F[(size_t)j] += f;
                }
                have[(size_t)j] = true;
            }
            if (m)
                for (auto &piece : sm.t->pieces) {
                    if (!piece->n) continue;
                    mf_ktimer tm(ctx, "k_wstats_gather");
                    k_wstats_gather<<<wstats_grid(piece->n), 256, 0, st>>>(piece->hi.p, piece->lo.p, piece->cnt.p, piece->n, shi, slo, m, (uint32_t)j, (uint32_t)N, mat.p);
                }
            const hipError_t e = hipStreamSynchronize(st);
            if (e != hipSuccess) return mf_set_error("stats-kmers (--wide-kmers): gather pass failed: %s", hipGetErrorString(e));
        }
        if (!have_F) {
            uint64_t Fsum = 0;
            for (uint64_t x : F) Fsum += x;
            M = (double)Fsum / N;
            std::vector<double> Fd((size_t)N);
            for (int j = 0; j < N; j++) Fd[(size_t)j] = (double)F[(size_t)j];
            MF_HIP(hipMemcpyAsync(dF.p, Fd.data(), (size_t)N * 8, hipMemcpyHostToDevice, st));
            MF_HIP(hipStreamSynchronize(st));
            have_F = true;
        }
        if (!m) continue;
        // rows: the narrow tool's kernels on row numbers
        mf_buf<uint64_t> rows, ra_k, rb_k; mf_buf<uint16_t> ra_v, rb_v;
        MF_TRY(rows.alloc(ctx, m)); MF_TRY(ra_k.alloc(ctx, m)); MF_TRY(rb_k.alloc(ctx, m)); MF_TRY(ra_v.alloc(ctx, m)); MF_TRY(rb_v.alloc(ctx, m));
        {
            mf_ktimer tm(ctx, "k_wstats_iota");
            k_wstats_iota<<<wstats_grid(m), 256, 0, st>>>(rows.p, m);
        }
        unsigned int cc[2] = {0, 0};
        MF_TRY(mf_join_cursors(ctx, 2, cc, [&](unsigned int *cur) {
            mf_stats_rows_launch(ctx, mf_stats_row_args{mat.p, rows.p, m, na, nb, dF.p, M, mw, T, ra_k.p, rb_k.p, ra_v.p, rb_v.p, cur, ctr.p});
        }, "stats-kmers (--wide-kmers): row pass"));
        mat.reset(); rows.reset();
        int bits = 1;
        while (bits < 63 && (1ull << bits) < m) bits++;
        auto finish = [&](wstats_parts &pg, mf_buf<uint64_t> &rk, mf_buf<uint16_t> &rv, uint64_t ng) -> int {
            wstats_parts::part *o = pg.add();
            if (ng) {
                mf_buf<uint64_t> sk; MF_TRY(sk.alloc(ctx, ng));
                MF_TRY(o->hi.alloc(ctx, ng)); MF_TRY(o->lo.alloc(ctx, ng)); MF_TRY(o->val.alloc(ctx, ng));
                MF_TRY(mf_sort_pairs(ctx, rk.p, rv.p, ng, bits, sk.p, o->val.p));
                {
                    mf_ktimer tm(ctx, "k_wstats_keys");
                    k_wstats_keys<<<wstats_grid(ng), 256, 0, st>>>(sk.p, ng, shi, slo, m, o->hi.p, o->lo.p);
                }
                MF_HIP(hipStreamSynchronize(st));
            }
            pg.wrote(ng);
            return MF_OK;
        };
        MF_TRY(finish(p_a, ra_k, ra_v, cc[0]));
        MF_TRY(finish(p_b, rb_k, rb_v, cc[1]));
    }
    unsigned long long hc[MF_STATS_COUNTERS];
    MF_HIP(hipMemcpyAsync(hc, ctr.p, MF_STATS_COUNTERS * 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < MF_STATS_COUNTERS; i++) counters[i] = hc[i];
    // (the chi-squared list holds counts of 1; a group's values are Java shorts, any 16 bits: "cut" at -1, every record is written)
    MF_TRY(p_chi.table(ctx, k, 0, chi_out));
    MF_TRY(p_a.table(ctx, k, -1, ga_out));
    MF_TRY(p_b.table(ctx, k, -1, gb_out));
    return MF_OK;
}

static int wstats_check(int na, int nb, double p_chi2, int max_bad) {
    MF_TRY(mf_stats_check_groups(na, nb));
    MF_TRY(mf_stats_check_p(p_chi2));
    if (max_bad < 0) return mf_set_error("stats-kmers: maximal-bad-frequence = %d is negative", max_bad);
    return MF_OK;
}
static void wstats_drop(mf_wtable **a, mf_wtable **b, mf_wtable **c) {
    mf_wtable_destroy(*a); mf_wtable_destroy(*b); mf_wtable_destroy(*c);
    *a = *b = *c = nullptr;
}

// n(x) = the samples that hold x with count > b, for every x some sample holds so: the union's cnt, slice after slice
static int wnsamples_join(mf_ctx *ctx, int k, const mf_wjoin_get &get, int n, uint64_t total, int b, mf_wtable **out) {
    static const char *tool = "kmers-samples-counter";
    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(wstats_named(tool, mf_wjoin_plan(ctx, total, &S, &cap)));
    wstats_parts parts;
    for (uint32_t s = 0; s < S && n > 0; s++) {
        mf_wjoin_union u;
        MF_TRY(wstats_named(tool, mf_wjoin_slice_union(ctx, k, get, n, b, S, s, cap, u)));
        wstats_parts::part *p = parts.add();
        p->hi.swap(u.hi); p->lo.swap(u.lo); p->val.swap(u.cnt);
        parts.wrote(u.n);
    }
    return parts.table(ctx, k, 0, out);
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int mf_stats_kmers_wide_tables(mf_ctx *ctx, mf_wtable *const *a, int na, mf_wtable *const *b, int nb, int max_bad, double p_chi2, double p_mw,
                                          mf_wtable **chi, mf_wtable **group_a, mf_wtable **group_b, uint64_t *counters) {
    mf_range rng_("mf:stats_kmers_wide");
    if (!ctx || !chi || !group_a || !group_b || !counters || (na > 0 && !a) || (nb > 0 && !b)) return mf_set_error("mf_stats_kmers_wide_tables: NULL argument");
    *chi = *group_a = *group_b = nullptr;
    MF_TRY(wstats_check(na, nb, p_chi2, max_bad));
    MF_HIP(hipSetDevice(ctx->device));
    std::vector<mf_wtable *> all(a, a + na);
    all.insert(all.end(), b, b + nb);
    uint64_t total = 0; int k = 0;
    MF_TRY(mf_wjoin_tables_check(ctx, all.data(), na + nb, "mf_stats_kmers_wide_tables", &k, &total));
    const mf_wjoin_get get = [&all](int j, mf_wjoin_sample &s) { s.t = all[(size_t)j]; return MF_OK; };
    const int rc = wstats_join(ctx, k, get, na, nb, total, max_bad, p_chi2, p_mw, chi, group_a, group_b, counters);
    if (rc != MF_OK) wstats_drop(chi, group_a, group_b);
    return rc;
}

extern "C" int mf_stats_kmers_wide(mf_ctx *ctx, const char *const *a_files, int na, const char *const *b_files, int nb, int max_bad, int k, double p_chi2,
                                   double p_mw, const char *out_dir, uint64_t *counters) {
    mf_range rng_("mf:stats_kmers_wide(files)");
    if (!ctx || !out_dir || (na > 0 && !a_files) || (nb > 0 && !b_files)) return mf_set_error("mf_stats_kmers_wide: NULL argument");
    if (k < 32 || k > 63) return mf_set_error("mf_stats_kmers_wide: 32 <= k <= 63 (k <= 31: mf_stats_kmers)");
    MF_TRY(wstats_check(na, nb, p_chi2, max_bad));
    MF_HIP(hipSetDevice(ctx->device));
    std::vector<const char *> files(a_files, a_files + na);
    files.insert(files.end(), b_files, b_files + nb);
    uint64_t total = 0;
    MF_TRY(mf_wjoin_file_records(files.data(), na + nb, &total));
    // one sample resident at a time, loaded like IOUtils.loadKmers(file, 0): read twice per slice, for the union and for the gather
    const mf_wjoin_get get = [ctx, &files, k](int j, mf_wjoin_sample &s) { s.own = true; return mf_wtable_load_kmers(ctx, &files[(size_t)j], 1, 0, k, &s.t); };
    mf_wtable *chi = nullptr, *ga = nullptr, *gb = nullptr;
    uint64_t c[MF_STATS_COUNTERS] = {0};
    int rc = wstats_join(ctx, k, get, na, nb, total, max_bad, p_chi2, p_mw, &chi, &ga, &gb, c);
    const std::string d(out_dir);
    uint64_t w = 0;
    if (rc == MF_OK) rc = mf_wtable_write_kmers(chi, 0, (d + "/filtered_chisquared.kmers.bin").c_str(), (d + "/filtered_chisquared.stat.txt").c_str(), &w);
    // (values are Java shorts: every record is written, none is a count the histogram knows)
    if (rc == MF_OK) rc = mf_wtable_write_kmers(ga, -1, (d + "/filtered_groupA.kmers.bin").c_str(), nullptr, &w);
    if (rc == MF_OK) rc = mf_wtable_write_kmers(gb, -1, (d + "/filtered_groupB.kmers.bin").c_str(), nullptr, &w);
    wstats_drop(&chi, &ga, &gb);
    if (rc == MF_OK && counters) memcpy(counters, c, sizeof c);
    return rc;
}

static int wnsamples_check(const char *what, int n) {
    if (n < 0) return mf_set_error("%s: NULL argument", what);
    if (n > 32767) return mf_set_error("kmers-samples-counter: %d input files, at most 32767 (the count is a Java short)", n);
    return MF_OK;
}

extern "C" int mf_kmers_samples_count_wide_tables(mf_ctx *ctx, mf_wtable *const *t, int n, int max_bad, mf_wtable **out) {
    mf_range rng_("mf:kmers_samples_counter_wide");
    if (!ctx || !out || (n > 0 && !t)) return mf_set_error("mf_kmers_samples_count_wide_tables: NULL argument");
    *out = nullptr;
    MF_TRY(wnsamples_check("mf_kmers_samples_count_wide_tables", n));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0; int k = 0;
    MF_TRY(mf_wjoin_tables_check(ctx, t, n, "mf_kmers_samples_count_wide_tables", &k, &total));
    if (!k) k = 32;                                         // (no table at all: one empty result)
    const mf_wjoin_get get = [t](int j, mf_wjoin_sample &s) { s.t = t[j]; return MF_OK; };
    return wnsamples_join(ctx, k, get, n, total, max_bad, out);
}

extern "C" int mf_kmers_samples_count_wide(mf_ctx *ctx, const char *const *files, int n, int max_bad, int k, const char *kmers_bin, const char *stat_txt,
                                           uint64_t *n_kmers) {
    mf_range rng_("mf:kmers_samples_counter_wide(files)");
    if (!ctx || !kmers_bin || (n > 0 && !files)) return mf_set_error("mf_kmers_samples_count_wide: NULL argument");
    if (k < 32 || k > 63) return mf_set_error("mf_kmers_samples_count_wide: 32 <= k <= 63 (k <= 31: mf_kmers_samples_count)");
    MF_TRY(wnsamples_check("mf_kmers_samples_count_wide", n));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    MF_TRY(mf_wjoin_file_records(files, n, &total));
    const mf_wjoin_get get = [ctx, files, k](int j, mf_wjoin_sample &s) { s.own = true; return mf_wtable_load_kmers(ctx, files + j, 1, 0, k, &s.t); };
    mf_wtable *t = nullptr;
    MF_TRY(wnsamples_join(ctx, k, get, n, total, max_bad, &t));
    uint64_t w = 0;
    const int rc = mf_wtable_write_kmers(t, 0, kmers_bin, stat_txt, &w);
    mf_wtable_destroy(t);
    if (rc == MF_OK && n_kmers) *n_kmers = w;
    return rc;
}
