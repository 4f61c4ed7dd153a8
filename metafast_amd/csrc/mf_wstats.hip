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
//
// Three groups: stats-kmers-3 (the definition of mf_stats_kmers3_tables, StatsKmers3GroupsFinder.java:92-377) and
// kmers-grouped-counter (KmersGroupedSamplesCounter.java:82-190) on the same core.  The union is taken with GROUP ids in place of weights: its
// reduce pass leaves one word of three 10-bit per-group sample counts per k-mer (mf_wjoin.h), which three groups need and a 16-bit weighted sum
// cannot hold.  stats-kmers-3 then runs the passes above with k_wstats_select3 (the host's (nA + 1)(nB + 1)(nC + 1) table of chisq3_keep) and
// the three-group row kernels (mf_stats3_rows_launch); the grouped counter looks every -kf k-mer up in the slice's union (k_wstats_probe).
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

// the same pass for three groups (k_stats3_select on the union's group word, mf_wjoin.h): the decision's table indexed by (n1A, n1B, n1C), "unique" = two
// of the three groups hold nothing
__global__ __launch_bounds__(256) void k_wstats_select3(const uint32_t *__restrict__ grp, uint64_t n, const uint8_t *__restrict__ chi_keep, int na, int nb, int nc,
                                                        int scarce_max, uint16_t *__restrict__ keep, unsigned long long *__restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t c_n = 0, c_scarce = 0, c_all = 0, c_uniq = 0, c_rej = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t w = grp[i];
        const int n1a = (int)(w & MF_STATS3_MASK), n1b = (int)((w >> MF_STATS3_BITS) & MF_STATS3_MASK), n1c = (int)((w >> (2 * MF_STATS3_BITS)) & MF_STATS3_MASK);
        uint16_t kp = 0;
        c_n++;
        if (n1a + n1b + n1c <= scarce_max) c_scarce++;
        else if (n1a + n1b + n1c == na + nb + nc) c_all++;
        else {
            if (n1a + n1c == 0 || n1b + n1a == 0 || n1b + n1c == 0) c_uniq++;
            // (n1a <= na, n1b <= nb, n1c <= nc by the union's count of distinct samples: the index is inside the table; a word that broke that is not looked up)
            if (n1a <= na && n1b <= nb && n1c <= nc && chi_keep[((size_t)n1a * (size_t)(nb + 1) + (size_t)n1b) * (size_t)(nc + 1) + (size_t)n1c]) kp = 1;
            else c_rej++;
        }
        keep[i] = kp;
    }
    mf_stats_add(&ctr[0], c_n); mf_stats_add(&ctr[1], c_scarce); mf_stats_add(&ctr[2], c_all); mf_stats_add(&ctr[3], c_uniq); mf_stats_add(&ctr[4], c_rej);
}

// kmers-grouped-counter: one thread per k-mer of the -kf table (khi, klo)[n]; one of slice s is looked up by a binary search on two words in the slice's
// ascending union (dhi, dlo)[nd] and takes its group word.  A k-mer of another slice is skipped, one in no group keeps its 0.
__global__ __launch_bounds__(256) void k_wstats_probe(const uint64_t *__restrict__ khi, const uint64_t *__restrict__ klo, uint64_t n, int hb, uint32_t S, uint32_t s,
                                                      const uint64_t *__restrict__ dhi, const uint64_t *__restrict__ dlo, const uint32_t *__restrict__ dgrp, uint64_t nd,
                                                      uint32_t *__restrict__ words) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t h = khi[i], l = klo[i];
    if (mf_wjoin_slice(h, l, hb, S) != s) return;
    uint64_t a = 0, e = nd;
    while (a < e) {
        const uint64_t mid = a + (e - a) / 2, mh = dhi[mid];
        if (mh < h || (mh == h && dlo[mid] < l)) a = mid + 1; else e = mid;
    }
    if (a < nd && dhi[a] == h && dlo[a] == l) words[i] = dgrp[a];
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

static int wstats_matrix_fits(mf_ctx *ctx, const char *tool, int N, uint64_t m) {
    size_t fr = 0, tot = 0;
    MF_HIP(hipMemGetInfo(&fr, &tot));
    const uint64_t room = (uint64_t)fr + mf_arena_idle(ctx);
    if (m > room / 2 / (uint64_t)N)
        return mf_set_error("%s (--wide-kmers): the count matrix of %llu k-mers x %d samples x 2 bytes of a slice does not fit the %llu bytes of free "
                            "device memory (raise option stats_slices)", tool, (unsigned long long)m, N, (unsigned long long)room);
    return MF_OK;
}

// what the gather pass keeps from slice to slice: F_j = the sum of sample j's counts (summed once, when the sample is first read here), M = their mean
struct wstats_sums {
    std::vector<uint64_t> F; std::vector<bool> have; bool done = false;
    mf_buf<double> dF; double M = 0.0;
    int init(mf_ctx *ctx, int N) { F.assign((size_t)N, 0); have.assign((size_t)N, false); return dF.alloc(ctx, N); }
};
// the gather pass of a slice with m survivors (shi, slo)[m]: the zeroed u16 [m][N] matrix and every sample's column (k_wstats_gather at threshold
// 0); the first time it runs, with or without survivors, it also leaves F_j and M.  Nothing to do: m = 0 and the sums are there.
static int wstats_gather_pass(mf_ctx *ctx, const char *tool, const mf_wjoin_get &get, int N, const uint64_t *shi, const uint64_t *slo, uint64_t m, wstats_sums &sm_,
                              mf_buf<uint16_t> &mat) {
    hipStream_t st = ctx->stream;
    if (!m && sm_.done) return MF_OK;
    if (m) {
        MF_TRY(wstats_matrix_fits(ctx, tool, N, m));
        MF_TRY(mat.alloc(ctx, m * (uint64_t)N));
        MF_HIP(hipMemsetAsync(mat.p, 0, m * (uint64_t)N * 2, st));
    }
    for (int j = 0; j < N; j++) {
        mf_wjoin_sample sm(ctx);
        MF_TRY(wstats_named(tool, get(j, sm)));
        if (!sm_.have[(size_t)j]) {
            for (auto &piece : sm.t->pieces) {
                uint64_t f = 0;
                MF_TRY(mf_sum_counts(ctx, piece->cnt.p, piece->n, &f));
                sm_.F[(size_t)j] += f;
            }
            sm_.have[(size_t)j] = true;
        }
        if (m)
            for (auto &piece : sm.t->pieces) {
                if (!piece->n) continue;
                mf_ktimer tm(ctx, "k_wstats_gather");
                k_wstats_gather<<<wstats_grid(piece->n), 256, 0, st>>>(piece->hi.p, piece->lo.p, piece->cnt.p, piece->n, shi, slo, m, (uint32_t)j, (uint32_t)N, mat.p);
            }
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) return mf_set_error("%s (--wide-kmers): gather pass failed: %s", tool, hipGetErrorString(e));
    }
    if (!sm_.done) {
        uint64_t Fsum = 0;
        for (uint64_t x : sm_.F) Fsum += x;
        sm_.M = (double)Fsum / N;
        std::vector<double> Fd((size_t)N);
        for (int j = 0; j < N; j++) Fd[(size_t)j] = (double)sm_.F[(size_t)j];
        MF_HIP(hipMemcpyAsync(sm_.dF.p, Fd.data(), (size_t)N * 8, hipMemcpyHostToDevice, st));
        MF_HIP(hipStreamSynchronize(st));
        sm_.done = true;
    }
    return MF_OK;
}
// a group's ng (row, value) pairs of a slice with m rows -> a piece of pg: sorted by row (row order is k-mer order), the rows turned into (hi, lo)
static int wstats_finish_group(mf_ctx *ctx, wstats_parts &pg, mf_buf<uint64_t> &rk, mf_buf<uint16_t> &rv, uint64_t ng, const uint64_t *shi, const uint64_t *slo, uint64_t m) {
    int bits = 1;
    while (bits < 63 && (1ull << bits) < m) bits++;
    wstats_parts::part *o = pg.add();
    if (ng) {
        mf_buf<uint64_t> sk; MF_TRY(sk.alloc(ctx, ng));
        MF_TRY(o->hi.alloc(ctx, ng)); MF_TRY(o->lo.alloc(ctx, ng)); MF_TRY(o->val.alloc(ctx, ng));
        MF_TRY(mf_sort_pairs(ctx, rk.p, rv.p, ng, bits, sk.p, o->val.p));
        {
            mf_ktimer tm(ctx, "k_wstats_keys");
            k_wstats_keys<<<wstats_grid(ng), 256, 0, ctx->stream>>>(sk.p, ng, shi, slo, m, o->hi.p, o->lo.p);
        }
        MF_HIP(hipStreamSynchronize(ctx->stream));
    }
    pg.wrote(ng);
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
    wstats_sums sums; MF_TRY(sums.init(ctx, N));
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
        // gather
        mf_buf<uint16_t> mat;
        MF_TRY(wstats_gather_pass(ctx, tool, get, N, shi, slo, m, sums, mat));
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
            mf_stats_rows_launch(ctx, mf_stats_row_args{mat.p, rows.p, m, na, nb, sums.dF.p, sums.M, mw, T, ra_k.p, rb_k.p, ra_v.p, rb_v.p, cur, ctr.p});
        }, "stats-kmers (--wide-kmers): row pass"));
        mat.reset(); rows.reset();
        MF_TRY(wstats_finish_group(ctx, p_a, ra_k, ra_v, cc[0], shi, slo, m));
        MF_TRY(wstats_finish_group(ctx, p_b, rb_k, rb_v, cc[1], shi, slo, m));
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

// ---- three groups ----
// sample j's group id for the union: A (CD) first, then B (UC), then C (nonIBD)
static std::vector<uint8_t> wstats_group_ids(int na, int nb, int nc) {
    std::vector<uint8_t> g((size_t)(na + nb + nc), (uint8_t)0);
    for (int j = na; j < na + nb + nc; j++) g[(size_t)j] = j < na + nb ? 1 : 2;
    return g;
}

// the join of na + nb + nc samples, A first, then B, then C: wstats_join with the union's group word in place of the weighted sum, the
// (nA + 1)(nB + 1)(nC + 1) table of chisq3_keep at the quantile of 2 degrees of freedom, and the three-group row kernels.  grp_out[3]: A, B, C
static int wstats3_join(mf_ctx *ctx, int k, const mf_wjoin_get &get, int na, int nb, int nc, uint64_t total, int b, double pchi2, double pmw, mf_wtable **chi_out,
                        mf_wtable **grp_out, uint64_t *counters) {
    static const char *tool = "stats-kmers-3";
    hipStream_t st = ctx->stream;
    const int N = na + nb + nc;
    const double q = chi2_2_quantile(pchi2);
    std::vector<uint8_t> chi((size_t)(na + 1) * (nb + 1) * (nc + 1), 0);
    for (int n1a = 0; n1a <= na; n1a++)
        for (int n1b = 0; n1b <= nb; n1b++)
            for (int n1c = 0; n1c <= nc; n1c++)
                chi[((size_t)n1a * (nb + 1) + n1b) * (nc + 1) + n1c] =
                    chisq3_keep((float)(na - n1a), (float)n1a, (float)(nb - n1b), (float)n1b, (float)(nc - n1c), (float)n1c, q) ? 1 : 0;
    const int scarce_max = (int)std::ceil(N * 0.05);
    const int mw = pmw > 0 ? 1 : 0;
    const uint32_t Tab = mw ? mw_threshold(na, nb, pmw) : 0u, Tbc = mw ? mw_threshold(nb, nc, pmw) : 0u, Tac = mw ? mw_threshold(na, nc, pmw) : 0u;
    if (ctx->opt_verbose) fprintf(stderr, "[mf] stats3 (wide): q = %.17g, scarce <= %d, 2*Umin < %u (A, B), %u (B, C), %u (A, C)\n", q, scarce_max, Tab, Tbc, Tac);
    mf_buf<uint8_t> dchi; MF_TRY(dchi.alloc(ctx, chi.size()));
    MF_HIP(hipMemcpyAsync(dchi.p, chi.data(), chi.size(), hipMemcpyHostToDevice, st));
    mf_buf<unsigned long long> ctr; MF_TRY(ctr.alloc(ctx, MF_STATS3_COUNTERS));
    MF_HIP(hipMemsetAsync(ctr.p, 0, MF_STATS3_COUNTERS * 8, st));
    MF_HIP(hipStreamSynchronize(st));                      // (chi is the host's until here)

    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(wstats_named(tool, mf_wjoin_plan(ctx, total, &S, &cap)));
    const std::vector<uint8_t> group = wstats_group_ids(na, nb, nc);
    wstats_sums sums; MF_TRY(sums.init(ctx, N));
    wstats_parts p_chi, p_g[3];
    for (uint32_t s = 0; s < S; s++) {
        // union and select
        wstats_parts::part *pc = p_chi.add();
        uint64_t m = 0;
        {
            mf_wjoin_union u;
            MF_TRY(wstats_named(tool, mf_wjoin_slice_union(ctx, k, get, N, b, S, s, cap, u, nullptr, group.data())));
            if (u.n) {
                mf_buf<uint16_t> keep; MF_TRY(keep.alloc(ctx, u.n));
                {
                    mf_ktimer tm(ctx, "k_wstats_select3");
                    const unsigned grid = (unsigned)std::min<uint64_t>((u.n + 255) / 256, (uint64_t)std::max(ctx->n_cu, 1) * 16);
                    k_wstats_select3<<<grid, 256, 0, st>>>(u.grp.p, u.n, dchi.p, na, nb, nc, scarce_max, keep.p, ctr.p);
                }
                MF_TRY(mf_wjoin_select(ctx, u.hi.p, u.lo.p, keep.p, keep.p, u.n, 0, pc->hi, pc->lo, pc->val, nullptr, &m));
            }
        }
        const uint64_t *shi = pc->hi.p, *slo = pc->lo.p;
        p_chi.wrote(m);                                    // (an empty piece is dropped: shi / slo are not read for m = 0)
        // gather
        mf_buf<uint16_t> mat;
        MF_TRY(wstats_gather_pass(ctx, tool, get, N, shi, slo, m, sums, mat));
        if (!m) continue;
        // rows: the narrow tool's kernels on row numbers
        mf_buf<uint64_t> rows, rk[3]; mf_buf<uint16_t> rv[3];
        MF_TRY(rows.alloc(ctx, m));
        for (int g = 0; g < 3; g++) { MF_TRY(rk[g].alloc(ctx, m)); MF_TRY(rv[g].alloc(ctx, m)); }
        {
            mf_ktimer tm(ctx, "k_wstats_iota");
            k_wstats_iota<<<wstats_grid(m), 256, 0, st>>>(rows.p, m);
        }
        unsigned int cc[3] = {0, 0, 0};
        MF_TRY(mf_join_cursors(ctx, 3, cc, [&](unsigned int *cur) {
            mf_stats3_rows_launch(ctx, mf_stats3_row_args{mat.p, rows.p, m, na, nb, nc, sums.dF.p, sums.M, mw, Tab, Tbc, Tac, rk[0].p, rk[1].p, rk[2].p, rv[0].p, rv[1].p,
                                                          rv[2].p, cur, ctr.p});
        }, "stats-kmers-3 (--wide-kmers): row pass"));
        mat.reset(); rows.reset();
        for (int g = 0; g < 3; g++) MF_TRY(wstats_finish_group(ctx, p_g[g], rk[g], rv[g], cc[g], shi, slo, m));
    }
    unsigned long long hc[MF_STATS3_COUNTERS];
    MF_HIP(hipMemcpyAsync(hc, ctr.p, MF_STATS3_COUNTERS * 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < MF_STATS3_COUNTERS; i++) counters[i] = hc[i];
    MF_TRY(p_chi.table(ctx, k, 0, chi_out));
    for (int g = 0; g < 3; g++) MF_TRY(p_g[g].table(ctx, k, -1, &grp_out[g]));
    return MF_OK;
}

static int wstats3_check(int na, int nb, int nc, double p_chi2, int max_bad) {
    MF_TRY(mf_stats_check_groups3(na, nb, nc));
    MF_TRY(mf_stats_check_p(p_chi2));
    if (max_bad < 0) return mf_set_error("stats-kmers-3: maximal-bad-frequence = %d is negative", max_bad);
    return MF_OK;
}

// kmers-grouped-counter: words[i] = the group word of the i-th k-mer of `kmers` (ascending, one piece; n > 0) over the three groups, on the host
static int wgrouped_join(mf_ctx *ctx, int k, const mf_wjoin_get &get, int n_cd, int n_uc, int n_nonibd, uint64_t total, int b, const mf_wtable *kmers,
                         std::vector<uint32_t> &words) {
    static const char *tool = "kmers-grouped-counter";
    hipStream_t st = ctx->stream;
    const int N = n_cd + n_uc + n_nonibd;
    const uint64_t n = kmers->n;
    const mf_wtable::piece &kp = *kmers->pieces[0];
    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(wstats_named(tool, mf_wjoin_plan(ctx, total, &S, &cap)));
    const std::vector<uint8_t> group = wstats_group_ids(n_cd, n_uc, n_nonibd);
    mf_buf<uint32_t> dw; MF_TRY(dw.alloc(ctx, n));
    MF_HIP(hipMemsetAsync(dw.p, 0, n * 4, st));
    for (uint32_t s = 0; s < S && N > 0; s++) {
        mf_wjoin_union u;
        MF_TRY(wstats_named(tool, mf_wjoin_slice_union(ctx, k, get, N, b, S, s, cap, u, nullptr, group.data())));
        if (!u.n) continue;
        {
            mf_ktimer tm(ctx, "k_wstats_probe");
            k_wstats_probe<<<wstats_grid(n), 256, 0, st>>>(kp.hi.p, kp.lo.p, n, 2 * k - 64, S, s, u.hi.p, u.lo.p, u.grp.p, u.n, dw.p);
        }
        const hipError_t e = hipStreamSynchronize(st);     // (the slice's union goes next)
        if (e != hipSuccess) return mf_set_error("kmers-grouped-counter (--wide-kmers): probe pass failed: %s", hipGetErrorString(e));
    }
    words.assign(n, 0);
    MF_HIP(hipMemcpyAsync(words.data(), dw.p, n * 4, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    return MF_OK;
}
// the -kf table as the probe reads it: ascending, in one piece
static int wgrouped_kmers(mf_wtable *kmers) {
    MF_TRY(mf_wtable_ensure_ascending(kmers));
    return mf_wtable_flatten(kmers);
}
static int wgrouped_check(int n_cd, int n_uc, int n_nonibd, int max_bad) {
    MF_TRY(mf_stats_check_grouped(n_cd, n_uc, n_nonibd));
    if (max_bad < 0) return mf_set_error("kmers-grouped-counter: maximal-bad-frequence = %d is negative", max_bad);
    return MF_OK;
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

static void wstats3_drop(mf_wtable **chi, mf_wtable **grp) {
    mf_wtable_destroy(*chi); *chi = nullptr;
    for (int g = 0; g < 3; g++) { mf_wtable_destroy(grp[g]); grp[g] = nullptr; }
}

extern "C" int mf_stats_kmers3_wide_tables(mf_ctx *ctx, mf_wtable *const *a, int na, mf_wtable *const *b, int nb, mf_wtable *const *c, int nc, int max_bad,
                                           double p_chi2, double p_mw, mf_wtable **chi, mf_wtable **group_a, mf_wtable **group_b, mf_wtable **group_c,
                                           uint64_t *counters) {
    mf_range rng_("mf:stats_kmers3_wide");
    if (!ctx || !chi || !group_a || !group_b || !group_c || !counters || (na > 0 && !a) || (nb > 0 && !b) || (nc > 0 && !c))
        return mf_set_error("mf_stats_kmers3_wide_tables: NULL argument");
    *chi = *group_a = *group_b = *group_c = nullptr;
    MF_TRY(wstats3_check(na, nb, nc, p_chi2, max_bad));
    MF_HIP(hipSetDevice(ctx->device));
    std::vector<mf_wtable *> all(a, a + na);
    all.insert(all.end(), b, b + nb);
    all.insert(all.end(), c, c + nc);
    uint64_t total = 0; int k = 0;
    MF_TRY(mf_wjoin_tables_check(ctx, all.data(), na + nb + nc, "mf_stats_kmers3_wide_tables", &k, &total));
    const mf_wjoin_get get = [&all](int j, mf_wjoin_sample &s) { s.t = all[(size_t)j]; return MF_OK; };
    mf_wtable *grp[3] = {nullptr, nullptr, nullptr};
    const int rc = wstats3_join(ctx, k, get, na, nb, nc, total, max_bad, p_chi2, p_mw, chi, grp, counters);
    if (rc != MF_OK) wstats3_drop(chi, grp);
    *group_a = grp[0]; *group_b = grp[1]; *group_c = grp[2];
    return rc;
}

extern "C" int mf_stats_kmers3_wide(mf_ctx *ctx, const char *const *a_files, int na, const char *const *b_files, int nb, const char *const *c_files, int nc,
                                    int max_bad, int k, double p_chi2, double p_mw, const char *out_dir, uint64_t *counters) {
    mf_range rng_("mf:stats_kmers3_wide(files)");
    if (!ctx || !out_dir || (na > 0 && !a_files) || (nb > 0 && !b_files) || (nc > 0 && !c_files)) return mf_set_error("mf_stats_kmers3_wide: NULL argument");
    if (k < 32 || k > 63) return mf_set_error("mf_stats_kmers3_wide: 32 <= k <= 63 (k <= 31: mf_stats_kmers3)");
    MF_TRY(wstats3_check(na, nb, nc, p_chi2, max_bad));
    MF_HIP(hipSetDevice(ctx->device));
    std::vector<const char *> files(a_files, a_files + na);
    files.insert(files.end(), b_files, b_files + nb);
    files.insert(files.end(), c_files, c_files + nc);
    uint64_t total = 0;
    MF_TRY(mf_wjoin_file_records(files.data(), na + nb + nc, &total));
    // one sample resident at a time, loaded like IOUtils.loadKmers(file, 0): read twice per slice, for the union and for the gather
    const mf_wjoin_get get = [ctx, &files, k](int j, mf_wjoin_sample &s) { s.own = true; return mf_wtable_load_kmers(ctx, &files[(size_t)j], 1, 0, k, &s.t); };
    mf_wtable *chi = nullptr, *grp[3] = {nullptr, nullptr, nullptr};
    uint64_t ctr[MF_STATS3_COUNTERS] = {0};
    int rc = wstats3_join(ctx, k, get, na, nb, nc, total, max_bad, p_chi2, p_mw, &chi, grp, ctr);
    const std::string d(out_dir);
    uint64_t w = 0;
    if (rc == MF_OK) rc = mf_wtable_write_kmers(chi, 0, (d + "/filtered_chisquared.kmers.bin").c_str(), (d + "/filtered_chisquared.stat.txt").c_str(), &w);
    // (values are Java shorts: every record is written, none is a count the histogram knows)
    static const char *names[3] = {"/filtered_groupA.kmers.bin", "/filtered_groupB.kmers.bin", "/filtered_groupC.kmers.bin"};
    for (int g = 0; g < 3; g++)
        if (rc == MF_OK) rc = mf_wtable_write_kmers(grp[g], -1, (d + names[g]).c_str(), nullptr, &w);
    wstats3_drop(&chi, grp);
    if (rc == MF_OK && counters) memcpy(counters, ctr, sizeof ctr);
    return rc;
}

// counts[i] = cd << 32 | uc << 16 | nonibd of a group word (the packing of mf_kmers_grouped_count_tables)
static uint64_t wgrouped_pack(uint32_t w) {
    return (uint64_t)(w & MF_STATS3_MASK) << 32 | (uint64_t)((w >> MF_STATS3_BITS) & MF_STATS3_MASK) << 16 | (uint64_t)((w >> (2 * MF_STATS3_BITS)) & MF_STATS3_MASK);
}

extern "C" int mf_kmers_grouped_count_wide_tables(mf_ctx *ctx, mf_wtable *kmers, mf_wtable *const *cd, int n_cd, mf_wtable *const *uc, int n_uc,
                                                  mf_wtable *const *nonibd, int n_nonibd, int max_bad, uint64_t *hi, uint64_t *lo, uint64_t *counts,
                                                  uint64_t cap, uint64_t *n) {
    mf_range rng_("mf:kmers_grouped_counter_wide");
    if (!ctx || !kmers || !n || (cap && (!hi || !lo || !counts)) || (n_cd > 0 && !cd) || (n_uc > 0 && !uc) || (n_nonibd > 0 && !nonibd))
        return mf_set_error("mf_kmers_grouped_count_wide_tables: NULL argument");
    MF_TRY(wgrouped_check(n_cd, n_uc, n_nonibd, max_bad));
    MF_HIP(hipSetDevice(ctx->device));
    std::vector<mf_wtable *> all(cd, cd + n_cd);
    all.insert(all.end(), uc, uc + n_uc);
    all.insert(all.end(), nonibd, nonibd + n_nonibd);
    uint64_t total = 0; int k = 0;
    MF_TRY(mf_wjoin_tables_check(ctx, &kmers, 1, "mf_kmers_grouped_count_wide_tables (kmers)", &k, nullptr));
    MF_TRY(mf_wjoin_tables_check(ctx, all.data(), (int)all.size(), "mf_kmers_grouped_count_wide_tables", &k, &total));
    *n = kmers->n;
    if (cap < kmers->n || !kmers->n) return MF_OK;        // (the number alone: the caller comes again with room; no k-mer: the groups are not read)
    MF_TRY(wgrouped_kmers(kmers));
    const mf_wjoin_get get = [&all](int j, mf_wjoin_sample &s) { s.t = all[(size_t)j]; return MF_OK; };
    std::vector<uint32_t> words;
    MF_TRY(wgrouped_join(ctx, k, get, n_cd, n_uc, n_nonibd, total, max_bad, kmers, words));
    const mf_wtable::piece &kp = *kmers->pieces[0];
    MF_HIP(hipMemcpyAsync(hi, kp.hi.p, kmers->n * 8, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipMemcpyAsync(lo, kp.lo.p, kmers->n * 8, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    for (uint64_t i = 0; i < kmers->n; i++) counts[i] = wgrouped_pack(words[i]);
    return MF_OK;
}

extern "C" int mf_kmers_grouped_count_wide(mf_ctx *ctx, const char *const *kmers_files, int n_kmers_files, const char *const *cd_files, int n_cd,
                                           const char *const *uc_files, int n_uc, const char *const *nonibd_files, int n_nonibd, int max_bad, int k,
                                           const char *out_txt, uint64_t *n_kmers) {
    mf_range rng_("mf:kmers_grouped_counter_wide(files)");
    if (!ctx || !out_txt || (n_kmers_files > 0 && !kmers_files) || (n_cd > 0 && !cd_files) || (n_uc > 0 && !uc_files) || (n_nonibd > 0 && !nonibd_files))
        return mf_set_error("mf_kmers_grouped_count_wide: NULL argument");
    if (k < 32 || k > 63) return mf_set_error("mf_kmers_grouped_count_wide: 32 <= k <= 63 (k <= 31: mf_kmers_grouped_count)");
    MF_TRY(wgrouped_check(n_cd, n_uc, n_nonibd, max_bad));
    MF_HIP(hipSetDevice(ctx->device));
    std::vector<const char *> files(cd_files, cd_files + n_cd);
    files.insert(files.end(), uc_files, uc_files + n_uc);
    files.insert(files.end(), nonibd_files, nonibd_files + n_nonibd);
    uint64_t total = 0;
    MF_TRY(mf_wjoin_file_records(files.data(), (int)files.size(), &total));
    mf_wjoin_sample kf(ctx);                               // IOUtils.loadKmers(kmersFile, 0): a k-mer listed more than once comes once
    kf.own = true;
    MF_TRY(wstats_named("kmers-grouped-counter", mf_wtable_load_kmers(ctx, kmers_files, std::max(n_kmers_files, 0), 0, k, &kf.t)));
    const uint64_t n = kf.t->n;
    std::vector<uint32_t> words;
    std::vector<uint64_t> hi(n), lo(n);
    if (n) {
        MF_TRY(wgrouped_kmers(kf.t));
        // one group file resident at a time, loaded like IOUtils.loadKmers(file, 0); the union cuts at max_bad
        const mf_wjoin_get get = [ctx, &files, k](int j, mf_wjoin_sample &s) { s.own = true; return mf_wtable_load_kmers(ctx, &files[(size_t)j], 1, 0, k, &s.t); };
        MF_TRY(wgrouped_join(ctx, k, get, n_cd, n_uc, n_nonibd, total, max_bad, kf.t, words));
        const mf_wtable::piece &kp = *kf.t->pieces[0];
        MF_HIP(hipMemcpyAsync(hi.data(), kp.hi.p, n * 8, hipMemcpyDeviceToHost, ctx->stream));
        MF_HIP(hipMemcpyAsync(lo.data(), kp.lo.p, n * 8, hipMemcpyDeviceToHost, ctx->stream));
        MF_HIP(hipStreamSynchronize(ctx->stream));
    }
    FILE *f = fopen(out_txt, "w");
    if (!f) return mf_set_error("Couldn't open output file '%s'", out_txt);
    fputs("Kmer\tcd_count\tuc_count\tnonibd_count\n", f);
    char text[64];
    for (uint64_t i = 0; i < n; i++) {
        for (int q = 0; q < k; q++) {                      // (the first base in the highest bits; base q stands at bit 2 (k - 1 - q) of the 2k-bit k-mer)
            const int sh = 2 * (k - 1 - q);
            text[q] = "AGCT"[(sh >= 64 ? hi[i] >> (sh - 64) : lo[i] >> sh) & 3u];
        }
        text[k] = 0;
        const uint32_t w = words[i];
        fprintf(f, "%s\t%u\t%u\t%u\n", text, w & MF_STATS3_MASK, (w >> MF_STATS3_BITS) & MF_STATS3_MASK, (w >> (2 * MF_STATS3_BITS)) & MF_STATS3_MASK);
    }
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) return mf_set_error("can't write '%s'", out_txt);
    if (n_kmers) *n_kmers = n;
    return MF_OK;
}
