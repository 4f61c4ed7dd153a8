// mf_stats.hip -- the multi-sample join of k-mer tables behind stats-kmers (src/tools/StatsKmersFinder.java:89-297) and
// kmers-samples-counter (src/tools/KmersSamplesCounter.java:69-140).
//
// Passes:
//   union   every sample's keys with count > b go into an HBM open-addressed table of 16-byte slots {key, presence, row}; the
//           presence word takes one atomic add per (sample, key): 1 for group A (or for every sample: kmers-samples-counter),
//           1 << 16 for group B.  The key space is cut into S hash slices (top bits of fmix64), one union table per slice, so that
//           the table fits in free HBM; the samples are streamed once per slice.
//   select  the chi-squared decision depends on (n1A, n1B) only: the host evaluates StatsKmersFinder.chisq (float / double, in
//           the reference's order, no contraction) into a (nA+1) x (nB+1) flag table and the kernel looks it up.  Survivors get a
//           row number.
//   gather  the samples again at threshold 0: every entry of a survivor fills its cell of a u16 [rows][N] count matrix.
//   row     v_j = ((double)c_j * M) / F_j, 2 * U1 = sum over pairs of 2 [vA > vB] + [vA == vB] in integers, the Mann-Whitney test
//           as 2 * Umin < T for one integer T the host finds from the p-value formula, the in-order means, the group and Java's
//           (short)(int) cast.  One thread per row up to MF_STATS_THREAD_N samples, one wave per row above.
// No floating point of the decisions but v_j and the means runs on the device, and those are IEEE double operations in the
// reference's order (no contraction in this file).
#pragma clang fp contract(off)
#include "mf_common.h"
#include <algorithm>
#include <cmath>
#include <functional>
#include <memory>
#include <sys/stat.h>

#define MF_STATS_MAX_N 1024          // samples of one stats-kmers run (the row kernels keep a row's values in LDS)
#define MF_STATS_THREAD_N 32         // up to this many samples: one thread per row (values in LDS, 64 KiB per 256 rows), else a wave per row
#define MF_STATS_KEY_LIMIT (1ull << 62)   // keys of k <= 31; the union table's empty marker lies above
static constexpr uint32_t MF_NO_ROW = 0xFFFFFFFFu;

struct mf_uslot { uint64_t key; uint32_t cnt; uint32_t row; };

int mf_sum_counts(mf_ctx *ctx, const uint16_t *d_counts, uint64_t n, uint64_t *total);
int mf_table_load_kmers_sum(mf_ctx *ctx, const char *const *files, int nfiles, int freq_threshold, int k, mf_table **out, uint64_t *freq_sum);

// slice of a key: the top 32 bits of fmix64 scaled to [0, S); the slot inside a slice's table comes from the LOW bits
__device__ __forceinline__ uint32_t mf_stats_slice(uint64_t h, uint32_t S) { return (uint32_t)(((h >> 32) * (uint64_t)S) >> 32); }

// ---------------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void k_stats_init(mf_uslot *__restrict__ slots, uint64_t cap, uint64_t y) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * blockDim.x) {
        ulonglong2 v; v.x = MF_EMPTY; v.y = y;
        *reinterpret_cast<ulonglong2 *>(&slots[i]) = v;
    }
}

// What a sample's entry adds to its key's slot:
//   MF_UNION_PRESENCE  `add` to the presence word (stats-kmers, kmers-samples-counter)
//   MF_UNION_SUM       the entry's value to the second word and 1 to the first (unique-kmers-multi: two words, so that the sum's carry
//                      never reaches the sample count; sum <= 32767 * 65535 < 2^31)
//   MF_UNION_FIELD     the entry's value to the 16-bit field number `add` of the slot (kmers-multiple-filters: cd, uc, nonibd; each
//                      field is written by one table, whose keys are distinct, so no add carries)
//   MF_UNION_COLOR     kmers-color: 1 (or, bit 2 of `add` set, the entry's value) to the 20-bit field number `add & 3` of the 64-bit payload,
//                      saturating at 2^20 - 1 (ColoredKmerOperations.addValue) by a compare-and-swap on the payload word
enum { MF_UNION_PRESENCE = 0, MF_UNION_SUM = 1, MF_UNION_FIELD = 2, MF_UNION_COLOR = 3 };
static constexpr uint64_t MF_COLOR_FIELD_MAX = (1ull << 20) - 1;
// flags: bit 0 = a key >= 2^62, bit 1 = the table is full (never with the sizes the host picks; an error, never a write out of bounds)
template <int MODE>
__global__ __launch_bounds__(256) void k_stats_union(mf_uslot *__restrict__ slots, uint64_t mask, const uint64_t *__restrict__ keys,
                                                     const uint16_t *__restrict__ cnts, uint64_t n, int thr, uint32_t add, uint32_t S, uint32_t s,
                                                     unsigned long long *__restrict__ n_union, unsigned int *__restrict__ flags) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = cnts[i];
        if ((int)c <= thr) continue;
        const uint64_t key = keys[i];
        if (key >= MF_STATS_KEY_LIMIT) { atomicOr(flags, 1u); continue; }
        const uint64_t h = mf_hash64(key);
        if (mf_stats_slice(h, S) != s) continue;
        uint64_t p = h & mask;
        bool done = false;
        for (uint64_t probe = 0; probe <= mask; probe++) {
            const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long *>(&slots[p].key), (unsigned long long)MF_EMPTY,
                                                     (unsigned long long)key);
            if (old == MF_EMPTY || old == key) {
                if (old == MF_EMPTY) atomicAdd(n_union, 1ull);
                if (MODE == MF_UNION_PRESENCE) atomicAdd(&slots[p].cnt, add);
                else if (MODE == MF_UNION_SUM) { atomicAdd(&slots[p].cnt, 1u); atomicAdd(&slots[p].row, c); }
                else if (MODE == MF_UNION_COLOR) {
                    const uint32_t sh = 20u * (add & 3u);
                    const uint64_t inc = (add & 4u) ? (uint64_t)c : 1ull;
                    unsigned long long *w = reinterpret_cast<unsigned long long *>(&slots[p].cnt);
                    unsigned long long cur = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    for (;;) {
                        const uint64_t f = (cur >> sh) & MF_COLOR_FIELD_MAX;
                        const uint64_t nf = f + inc < MF_COLOR_FIELD_MAX ? f + inc : MF_COLOR_FIELD_MAX;
                        const unsigned long long nw = (cur & ~(MF_COLOR_FIELD_MAX << sh)) | (nf << sh);
                        if (nw == cur) break;
                        const unsigned long long old = atomicCAS(w, cur, nw);
                        if (old == cur) break;
                        cur = old;
                    }
                }
                else if (add == 2u) atomicAdd(&slots[p].row, c);
                else atomicAdd(&slots[p].cnt, c << (16u * add));
                done = true;
                break;
            }
            p = (p + 1) & mask;
        }
        if (!done) atomicOr(flags, 2u);
    }
}

// wave sum of a per-lane counter into a 64-bit global counter
__device__ __forceinline__ void mf_stats_add(unsigned long long *ctr, uint32_t x) {
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d, 64);
    if (mf_lane() == 0 && x) atomicAdd(ctr, (unsigned long long)x);
}

// stats-kmers pass 1 over the union (StatsKmersFinder.java:129-162): counters [0] n, [1] scarce, [2] in all, [3] unique, [4] chi-squared
// rejected; survivors get row numbers and their keys go to rkeys.  (uniform trip count: every lane reaches mf_wave_reserve)
__global__ __launch_bounds__(256) void k_stats_select(mf_uslot *__restrict__ slots, uint64_t cap, const uint8_t *__restrict__ chi_keep, int na, int nb,
                                                      int scarce_max, uint64_t *__restrict__ rkeys, unsigned int *__restrict__ cursor,
                                                      unsigned long long *__restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t c_n = 0, c_scarce = 0, c_all = 0, c_uniq = 0, c_rej = 0;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < cap; i0 += stride) {
        const uint64_t i = i0 + threadIdx.x;
        bool keep = false;
        uint64_t key = MF_EMPTY;
        if (i < cap) {
            key = slots[i].key;
            if (key != MF_EMPTY) {
                const uint32_t c = slots[i].cnt;
                const int n1a = (int)(c & 0xFFFFu), n1b = (int)(c >> 16);
                c_n++;
                if (n1a + n1b <= scarce_max) c_scarce++;
                else if (n1a + n1b == na + nb) c_all++;
                else {
                    if (n1a == 0 || n1b == 0) c_uniq++;
                    if (chi_keep[(size_t)n1a * (size_t)(nb + 1) + (size_t)n1b]) keep = true;
                    else c_rej++;
                }
            }
        }
        const uint32_t r = mf_wave_reserve(cursor, keep ? 1u : 0u);
        if (keep) { slots[i].row = r; rkeys[r] = key; }
    }
    mf_stats_add(&ctr[0], c_n); mf_stats_add(&ctr[1], c_scarce); mf_stats_add(&ctr[2], c_all); mf_stats_add(&ctr[3], c_uniq); mf_stats_add(&ctr[4], c_rej);
}

// kmers-samples-counter: every union entry -> (key, number of samples)
__global__ __launch_bounds__(256) void k_stats_nsamples(const mf_uslot *__restrict__ slots, uint64_t cap, uint64_t *__restrict__ okeys,
                                                        uint16_t *__restrict__ ovals, unsigned int *__restrict__ cursor) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < cap; i0 += stride) {
        const uint64_t i = i0 + threadIdx.x;
        const bool here = i < cap && slots[i].key != MF_EMPTY;
        const uint32_t r = mf_wave_reserve(cursor, here ? 1u : 0u);
        if (here) { okeys[r] = slots[i].key; ovals[r] = (uint16_t)slots[i].cnt; }
    }
}

// one sample's entries (count > 0) into its column of the survivors' count matrix
__global__ __launch_bounds__(256) void k_stats_gather(const mf_uslot *__restrict__ slots, uint64_t mask, const uint64_t *__restrict__ keys,
                                                      const uint16_t *__restrict__ cnts, uint64_t n, uint32_t S, uint32_t s, uint32_t col, uint32_t N,
                                                      uint16_t *__restrict__ mat) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint16_t c = cnts[i];
        if (!c) continue;
        const uint64_t key = keys[i];
        if (key >= MF_STATS_KEY_LIMIT) continue;
        const uint64_t h = mf_hash64(key);
        if (mf_stats_slice(h, S) != s) continue;
        uint64_t p = h & mask;
        for (uint64_t probe = 0; probe <= mask; probe++) {
            const ulonglong2 raw = *reinterpret_cast<const ulonglong2 *>(&slots[p]);
            if (raw.x == key) {
                const uint32_t row = (uint32_t)(raw.y >> 32);
                if (row != MF_NO_ROW) mat[(uint64_t)row * N + col] = c;
                break;
            }
            if (raw.x == MF_EMPTY) break;
            p = (p + 1) & mask;
        }
    }
}

struct mf_stats_row_args {
    const uint16_t *mat; const uint64_t *rkeys; uint64_t m;
    int na, nb;
    const double *F; double M;
    int mw; uint32_t T;                                  // mw != 0: keep iff 2 * Umin < T
    uint64_t *ka, *kb; uint16_t *va, *vb;                 // group A / B outputs
    unsigned int *cur;                                    // [0] A, [1] B
    unsigned long long *ctr;                              // [5] MW rejected, [6] |A|, [7] |B|, [8] unique left
};
// Java's (short)(int)x: NaN -> 0, saturation to int, low 16 bits (JLS 5.1.3)
__device__ __forceinline__ uint16_t mf_java_short(double x) {
    int32_t i;
    if (x != x) i = 0;
    else if (x >= 2147483647.0) i = 2147483647;
    else if (x <= -2147483648.0) i = (-2147483647 - 1);
    else i = (int32_t)x;                                  // (in range: truncation toward zero)
    return (uint16_t)(uint32_t)i;
}
// decision + output of one row: group 0 (A) / 1 (B) / -1 (rejected by the Mann-Whitney test) and the value
__device__ __forceinline__ int mf_stats_group(bool pass, double meanA, double meanB, uint16_t *val) {
    if (!pass) return -1;
    if (meanA > meanB) { *val = mf_java_short(meanA); return 0; }
    *val = mf_java_short(meanB);
    return 1;
}
__device__ __forceinline__ void mf_stats_flush(unsigned long long *ctr, uint32_t c_mw, uint32_t c_a, uint32_t c_b, uint32_t c_ul) {
    mf_stats_add(&ctr[5], c_mw); mf_stats_add(&ctr[6], c_a); mf_stats_add(&ctr[7], c_b); mf_stats_add(&ctr[8], c_ul);
}

// one thread per row: the row's N values in LDS, sample j of thread t at v[j * 256 + t] (no bank conflicts)
__global__ __launch_bounds__(256) void k_stats_rows_thread(mf_stats_row_args a) {
    extern __shared__ double vs[];
    const int N = a.na + a.nb;
    uint32_t c_mw = 0, c_a = 0, c_b = 0, c_ul = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r0 = (uint64_t)blockIdx.x * blockDim.x; r0 < a.m; r0 += stride) {   // uniform trip count (mf_wave_reserve)
        const uint64_t r = r0 + threadIdx.x;
        int grp = -1; uint16_t val = 0;
        if (r < a.m) {
            double *v = vs + threadIdx.x;
            const uint16_t *row = a.mat + r * (uint64_t)N;
            bool nan_a = false;
            for (int j = 0; j < N; j++) {
                const double x = ((double)row[j] * a.M) / a.F[j];
                v[(size_t)j * 256] = x;
                if (j < a.na && x != x) nan_a = true;
            }
            bool pass = true;
            if (a.mw) {
                if (nan_a) pass = false;
                else {
                    uint32_t u2 = 0;
                    for (int i = 0; i < a.na; i++) {
                        const double x = v[(size_t)i * 256];
                        for (int j = a.na; j < N; j++) { const double y = v[(size_t)j * 256]; u2 += (x > y ? 2u : 0u) + (x == y ? 1u : 0u); }
                    }
                    const uint32_t tot = 2u * (uint32_t)a.na * (uint32_t)a.nb, u2o = tot - u2;
                    pass = (u2 < u2o ? u2 : u2o) < a.T;
                }
            }
            double sa = 0.0, sb = 0.0;
            for (int j = 0; j < a.na; j++) sa += v[(size_t)j * 256];
            for (int j = a.na; j < N; j++) sb += v[(size_t)j * 256];
            const double meanA = sa / (double)a.na, meanB = sb / (double)a.nb;
            grp = mf_stats_group(pass, meanA, meanB, &val);
            c_mw += grp < 0; c_a += grp == 0; c_b += grp == 1;
            c_ul += grp >= 0 && (meanA == 0.0 || meanB == 0.0);
        }
        const uint32_t ia = mf_wave_reserve(&a.cur[0], grp == 0 ? 1u : 0u);
        const uint32_t ib = mf_wave_reserve(&a.cur[1], grp == 1 ? 1u : 0u);
        if (grp == 0) { a.ka[ia] = a.rkeys[r]; a.va[ia] = val; }
        else if (grp == 1) { a.kb[ib] = a.rkeys[r]; a.vb[ib] = val; }
    }
    mf_stats_flush(a.ctr, c_mw, c_a, c_b, c_ul);
}

// one wave per row (N > MF_STATS_THREAD_N): the lanes compute the row's values into LDS, then share out the A x B pairs
__global__ __launch_bounds__(256) void k_stats_rows_wave(mf_stats_row_args a) {
    __shared__ double vs[4][MF_STATS_MAX_N];
    const int N = a.na + a.nb, w = threadIdx.x >> 6, lane = mf_lane();
    double *v = vs[w];
    uint32_t c_mw = 0, c_a = 0, c_b = 0, c_ul = 0;
    for (uint64_t r0 = (uint64_t)blockIdx.x * 4; r0 < a.m; r0 += (uint64_t)gridDim.x * 4) {   // block-uniform trip count
        const uint64_t r = r0 + (uint64_t)w;
        const bool live = r < a.m;
        bool nan_a = false;
        if (live) {
            const uint16_t *row = a.mat + r * (uint64_t)N;
            for (int j = lane; j < N; j += 64) {
                const double x = ((double)row[j] * a.M) / a.F[j];
                v[j] = x;
                if (j < a.na && x != x) nan_a = true;
            }
        }
        __syncthreads();
        const bool any_nan_a = __any(nan_a);
        bool pass = true;
        if (live && a.mw) {
            if (any_nan_a) pass = false;
            else {
                uint32_t u2 = 0;
                for (int i = 0; i < a.na; i++) {
                    const double x = v[i];
                    for (int j = a.na + lane; j < N; j += 64) { const double y = v[j]; u2 += (x > y ? 2u : 0u) + (x == y ? 1u : 0u); }
                }
                for (int d = 32; d >= 1; d >>= 1) u2 += __shfl_xor(u2, d, 64);
                const uint32_t tot = 2u * (uint32_t)a.na * (uint32_t)a.nb, u2o = tot - u2;
                pass = (u2 < u2o ? u2 : u2o) < a.T;
            }
        }
        if (live && lane == 0) {
            double sa = 0.0, sb = 0.0;
            for (int j = 0; j < a.na; j++) sa += v[j];
            for (int j = a.na; j < N; j++) sb += v[j];
            int grp = -1; uint16_t val = 0;
            const uint64_t key = a.rkeys[r];
            const double meanA = sa / (double)a.na, meanB = sb / (double)a.nb;
            grp = mf_stats_group(pass, meanA, meanB, &val);
            c_mw += grp < 0; c_a += grp == 0; c_b += grp == 1;
            c_ul += grp >= 0 && (meanA == 0.0 || meanB == 0.0);
            if (grp == 0) { const uint32_t i = atomicAdd(&a.cur[0], 1u); a.ka[i] = key; a.va[i] = val; }
            else if (grp == 1) { const uint32_t i = atomicAdd(&a.cur[1], 1u); a.kb[i] = key; a.vb[i] = val; }
        }
        __syncthreads();
    }
    mf_stats_flush(a.ctr, c_mw, c_a, c_b, c_ul);
}

// ---------------------------------------------------------------------------------------------------------------------------
// host: the decisions' tables (StatsKmersFinder.chisq :300-316; commons-math3 3.6.1 MannWhitneyUTest.calculateAsymptoticPValue)
// ---------------------------------------------------------------------------------------------------------------------------
static bool chisq_keep(float c0, float c1, float p0, float p1, double value) {
    float tmp = c0;
    c0 = 100 * c0 / (c0 + c1);
    c1 = 100 * c1 / (tmp + c1);
    tmp = p0;
    p0 = 100 * p0 / (p0 + p1);
    p1 = 100 * p1 / (tmp + p1);
    const float gr_1 = c0 + c1, gr_2 = p0 + p1, all = gr_1 + gr_2;
    const float x1 = gr_1 / all * (p1 + c1), x2 = gr_1 / all * (p0 + c0), x3 = gr_2 / all * (p1 + c1), x4 = gr_2 / all * (p0 + c0);
    const double d1 = (double)std::fabs(p1 - x1) - 0.5, d2 = (double)std::fabs(p0 - x2) - 0.5, d3 = (double)std::fabs(c1 - x3) - 0.5,
                 d4 = (double)std::fabs(c0 - x4) - 0.5;
    double kk = d1 * d1 / (double)x1;
    kk = kk + d2 * d2 / (double)x2;
    kk = kk + d3 * d3 / (double)x3;
    kk = kk + d4 * d4 / (double)x4;
    return value < kk;                                    // (NaN: rejected)
}
// ChiSquaredDistribution(1).inverseCumulativeProbability(1 - p): P(X > q) = erfc(sqrt(q / 2)) = 1 - (1 - p), by bisection
static double chi2_1_quantile(double p_chi2) {
    const double P = 1.0 - p_chi2, tail = 1.0 - P;
    if (P >= 1.0) return INFINITY;
    if (P <= 0.0) return 0.0;
    double lo = 0.0, hi = 1.0;
    while (std::erfc(std::sqrt(hi / 2.0)) > tail && hi < 1e300) hi *= 2.0;
    for (int it = 0; it < 400 && lo < hi; it++) {
        const double mid = lo + (hi - lo) / 2.0;
        if (mid <= lo || mid >= hi) break;
        if (std::erfc(std::sqrt(mid / 2.0)) > tail) lo = mid; else hi = mid;
    }
    return hi;
}
static double mw_pvalue(double umin, int n1, int n2) {
    const long long prod = (long long)n1 * n2;
    const double EU = (double)prod / 2.0, VarU = (double)(prod * (long long)(n1 + n2 + 1)) / 12.0;
    const double z = (umin - EU) / std::sqrt(VarU);
    double cdf;
    if (std::fabs(z) > 40.0) cdf = z < 0 ? 0.0 : 1.0;
    else cdf = 0.5 * std::erfc(-z / std::sqrt(2.0));
    return 2 * cdf;
}
// p grows with Umin: the smallest 2 * Umin in [0, nA nB] whose p is not < pmw (nA nB + 1: every row passes)
static uint32_t mw_threshold(int na, int nb, double pmw) {
    const uint32_t top = (uint32_t)na * (uint32_t)nb;
    for (uint32_t u2 = 0; u2 <= top; u2++)
        if (!(mw_pvalue(u2 / 2.0, na, nb) < pmw)) return u2;
    return top + 1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host: the join
// ---------------------------------------------------------------------------------------------------------------------------
// a sample for a pass: pass 0 = presence (entries with count > b count), pass 1 = counts (threshold 0) + F_j.  *own: destroy after use.
using stats_get = std::function<int(int j, int pass, mf_table **t, bool *own, uint64_t *F)>;

static uint64_t pow2_ge(uint64_t x) { uint64_t p = 1; while (p < x) p <<= 1; return p; }

// slices and union-table capacity for an upper bound `total` of the entries that go in
static int plan_slices(mf_ctx *ctx, uint64_t total, uint32_t *S_out, uint64_t *cap_out) {
    uint32_t S = (uint32_t)std::max<int64_t>(ctx->opt_stats_slices, 0);
    auto cap_of = [&](uint32_t s) {
        const double per = (double)total / s;
        return pow2_ge((uint64_t)(2.0 * (per + 6.0 * std::sqrt(per) + 1024.0)));
    };
    if (!S) {
        size_t fr = 0, tot = 0;
        MF_HIP(hipMemGetInfo(&fr, &tot));
        const double budget = 0.4 * (double)(fr + mf_arena_idle(ctx));
        S = 1;
        while (S < 4096 && (double)cap_of(S) * sizeof(mf_uslot) > budget) S++;
    }
    *S_out = S;
    *cap_out = cap_of(S);
    if (*cap_out >= (1ull << 40)) return mf_set_error("stats join: %llu entries do not fit", (unsigned long long)total);
    return MF_OK;
}

static unsigned grid_for(mf_ctx *ctx, uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->n_cu * 16)); }

// union of one slice: every sample's entries with count > b; adds: add_of(j)
static int union_slice(mf_ctx *ctx, const stats_get &get, int N, int b, uint32_t S, uint32_t s, uint64_t cap, mf_buf<mf_uslot> &slots,
                       const std::function<uint32_t(int)> &add_of, uint64_t *n_union, int mode = MF_UNION_PRESENCE) {
    MF_TRY(slots.alloc(ctx, cap));
    mf_buf<unsigned long long> nu; MF_TRY(nu.alloc(ctx, 1));
    mf_buf<unsigned int> flags; MF_TRY(flags.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(nu.p, 0, 8, ctx->stream));
    MF_HIP(hipMemsetAsync(flags.p, 0, 4, ctx->stream));
    {
        mf_ktimer tm(ctx, "k_stats_init");
        k_stats_init<<<grid_for(ctx, cap), 256, 0, ctx->stream>>>(slots.p, cap, mode == MF_UNION_PRESENCE ? (uint64_t)MF_NO_ROW << 32 : 0ull);
    }
    for (int j = 0; j < N; j++) {
        mf_table *t = nullptr; bool own = false; uint64_t F = 0;
        MF_TRY(get(j, 0, &t, &own, &F));
        if (t->n) {
            mf_ktimer tm(ctx, "k_stats_union");
            const unsigned g = grid_for(ctx, t->n);
            const uint32_t add = add_of(j);
            if (mode == MF_UNION_PRESENCE) k_stats_union<MF_UNION_PRESENCE><<<g, 256, 0, ctx->stream>>>(slots.p, cap - 1, t->d_keys, t->d_counts, t->n, b, add, S, s, nu.p, flags.p);
            else if (mode == MF_UNION_SUM) k_stats_union<MF_UNION_SUM><<<g, 256, 0, ctx->stream>>>(slots.p, cap - 1, t->d_keys, t->d_counts, t->n, b, add, S, s, nu.p, flags.p);
            else if (mode == MF_UNION_COLOR) k_stats_union<MF_UNION_COLOR><<<g, 256, 0, ctx->stream>>>(slots.p, cap - 1, t->d_keys, t->d_counts, t->n, b, add, S, s, nu.p, flags.p);
            else k_stats_union<MF_UNION_FIELD><<<g, 256, 0, ctx->stream>>>(slots.p, cap - 1, t->d_keys, t->d_counts, t->n, b, add, S, s, nu.p, flags.p);
        }
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (own) mf_table_destroy(t);
        if (e != hipSuccess) return mf_set_error("stats join: union pass failed: %s", hipGetErrorString(e));
    }
    unsigned int fl = 0; unsigned long long n = 0;
    MF_HIP(hipMemcpyAsync(&fl, flags.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipMemcpyAsync(&n, nu.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    if (fl & 1u) return mf_set_error("stats join: a k-mer key >= 2^62 (k-mers files hold k <= 31)");
    if (fl & 2u) return mf_set_error("stats join: the union table of a slice is full (raise option stats_slices)");
    *n_union = n;
    return MF_OK;
}

// (key, value) pairs -> ascending table; the arrays move into the table.  Result tables have k = 31: their keys are any values below
// 2^62 (the union pass rejects larger ones), and the exports / writers order 2k = 62 key bits.
static int pairs_to_table(mf_ctx *ctx, mf_buf<uint64_t> &keys, mf_buf<uint16_t> &vals, uint64_t n, mf_table **out) {
    const int k = 31;
    mf_buf<uint64_t> sk; mf_buf<uint16_t> sv;
    MF_TRY(sk.alloc(ctx, n)); MF_TRY(sv.alloc(ctx, n));
    if (n) MF_TRY(mf_sort_pairs(ctx, keys.p, vals.p, n, 2 * k, sk.p, sv.p));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    const size_t kb = sk.bytes(), vb = sv.bytes();
    return mf_table_adopt(ctx, k, n, 0, sk.take(), kb, sv.take(), vb, out);
}

// appends device pieces (one per slice) into one buffer
template <typename T>
static int concat(mf_ctx *ctx, std::vector<mf_buf<T> *> &parts, const std::vector<uint64_t> &ns, mf_buf<T> &out, uint64_t *n) {
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

static int stats_join(mf_ctx *ctx, const stats_get &get, int na, int nb, uint64_t total, int b, double pchi2, double pmw, mf_table **chi_out,
                      mf_table **a_out, mf_table **b_out, uint64_t *counters) {
    const int N = na + nb;
    // the decisions' tables
    const double q = chi2_1_quantile(pchi2);
    std::vector<uint8_t> chi((size_t)(na + 1) * (nb + 1), 0);
    for (int n1a = 0; n1a <= na; n1a++)
        for (int n1b = 0; n1b <= nb; n1b++) chi[(size_t)n1a * (nb + 1) + n1b] = chisq_keep((float)(na - n1a), (float)n1a, (float)(nb - n1b), (float)n1b, q) ? 1 : 0;
    const int scarce_max = (int)std::ceil(N * 0.05);
    const int mw = pmw > 0 ? 1 : 0;
    const uint32_t T = mw ? mw_threshold(na, nb, pmw) : 0u;
    if (ctx->opt_verbose) fprintf(stderr, "[mf] stats: q = %.17g, scarce <= %d, 2*Umin < %u\n", q, scarce_max, T);
    mf_buf<uint8_t> dchi; MF_TRY(dchi.alloc(ctx, chi.size()));
    MF_HIP(hipMemcpyAsync(dchi.p, chi.data(), chi.size(), hipMemcpyHostToDevice, ctx->stream));
    mf_buf<unsigned long long> ctr; MF_TRY(ctr.alloc(ctx, 9));
    MF_HIP(hipMemsetAsync(ctr.p, 0, 9 * 8, ctx->stream));

    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(plan_slices(ctx, total, &S, &cap));
    std::vector<std::unique_ptr<mf_buf<uint64_t>>> pk_chi, pk_a, pk_b;
    std::vector<std::unique_ptr<mf_buf<uint16_t>>> pv_a, pv_b;
    std::vector<uint64_t> n_chi, n_a, n_b;
    std::vector<uint64_t> F((size_t)N, 0);
    bool have_F = false;
    for (uint32_t s = 0; s < S; s++) {
        mf_buf<mf_uslot> slots; uint64_t nu = 0;
        MF_TRY(union_slice(ctx, get, N, b, S, s, cap, slots, [&](int j) { return j < na ? 1u : (1u << 16); }, &nu));
        // select
        pk_chi.emplace_back(new mf_buf<uint64_t>()); mf_buf<uint64_t> &rkeys = *pk_chi.back();
        MF_TRY(rkeys.alloc(ctx, nu));
        mf_buf<unsigned int> cur; MF_TRY(cur.alloc(ctx, 2));
        MF_HIP(hipMemsetAsync(cur.p, 0, 8, ctx->stream));
        {
            mf_ktimer tm(ctx, "k_stats_select");
            k_stats_select<<<grid_for(ctx, cap), 256, 0, ctx->stream>>>(slots.p, cap, dchi.p, na, nb, scarce_max, rkeys.p, cur.p, ctr.p);
        }
        unsigned int m32 = 0;
        MF_HIP(hipMemcpyAsync(&m32, cur.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        MF_HIP(hipStreamSynchronize(ctx->stream));
        const uint64_t m = m32;
        n_chi.push_back(m);
        // gather
        mf_buf<uint16_t> mat; MF_TRY(mat.alloc(ctx, m * (uint64_t)N));
        if (m) MF_HIP(hipMemsetAsync(mat.p, 0, mat.bytes(), ctx->stream));
        const bool need_counts = m > 0 || !have_F;
        for (int j = 0; j < N && need_counts; j++) {
            mf_table *t = nullptr; bool own = false; uint64_t Fj = 0;
            MF_TRY(get(j, 1, &t, &own, &Fj));
            F[(size_t)j] = Fj;
            if (m && t->n) {
                mf_ktimer tm(ctx, "k_stats_gather");
                k_stats_gather<<<grid_for(ctx, t->n), 256, 0, ctx->stream>>>(slots.p, cap - 1, t->d_keys, t->d_counts, t->n, S, s, (uint32_t)j, (uint32_t)N, mat.p);
            }
            const hipError_t e = hipStreamSynchronize(ctx->stream);
            if (own) mf_table_destroy(t);
            if (e != hipSuccess) return mf_set_error("stats join: gather pass failed: %s", hipGetErrorString(e));
        }
        have_F = true;
        slots.reset();
        // rows
        uint64_t Fsum = 0;
        for (uint64_t x : F) Fsum += x;
        const double M = (double)Fsum / N;
        std::vector<double> Fd((size_t)N);
        for (int j = 0; j < N; j++) Fd[(size_t)j] = (double)F[(size_t)j];
        mf_buf<double> dF; MF_TRY(dF.alloc(ctx, N));
        MF_HIP(hipMemcpyAsync(dF.p, Fd.data(), (size_t)N * 8, hipMemcpyHostToDevice, ctx->stream));
        pk_a.emplace_back(new mf_buf<uint64_t>()); pk_b.emplace_back(new mf_buf<uint64_t>());
        pv_a.emplace_back(new mf_buf<uint16_t>()); pv_b.emplace_back(new mf_buf<uint16_t>());
        MF_TRY(pk_a.back()->alloc(ctx, m)); MF_TRY(pk_b.back()->alloc(ctx, m)); MF_TRY(pv_a.back()->alloc(ctx, m)); MF_TRY(pv_b.back()->alloc(ctx, m));
        MF_HIP(hipMemsetAsync(cur.p, 0, 8, ctx->stream));
        if (m) {
            mf_stats_row_args ra{mat.p, rkeys.p, m, na, nb, dF.p, M, mw, T, pk_a.back()->p, pk_b.back()->p, pv_a.back()->p, pv_b.back()->p, cur.p, ctr.p};
            if (N <= MF_STATS_THREAD_N) {
                mf_ktimer tm(ctx, "k_stats_rows_thread");
                k_stats_rows_thread<<<(unsigned)std::min<uint64_t>((m + 255) / 256, (uint64_t)ctx->n_cu * 8), 256, (size_t)N * 256 * sizeof(double), ctx->stream>>>(ra);
            } else {
                mf_ktimer tm(ctx, "k_stats_rows_wave");
                k_stats_rows_wave<<<(unsigned)std::min<uint64_t>((m + 3) / 4, (uint64_t)ctx->n_cu * 16), 256, 0, ctx->stream>>>(ra);
            }
        }
        unsigned int cc[2] = {0, 0};
        MF_HIP(hipMemcpyAsync(cc, cur.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        MF_HIP(hipStreamSynchronize(ctx->stream));
        n_a.push_back(cc[0]); n_b.push_back(cc[1]);
    }
    unsigned long long hc[9];
    MF_HIP(hipMemcpyAsync(hc, ctr.p, 9 * 8, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 9; i++) counters[i] = hc[i];
    // the three lists: concatenated over the slices, sorted, as tables
    auto finish = [&](std::vector<std::unique_ptr<mf_buf<uint64_t>>> &pk, std::vector<std::unique_ptr<mf_buf<uint16_t>>> *pv, std::vector<uint64_t> &ns,
                      mf_table **out) -> int {
        std::vector<mf_buf<uint64_t> *> kp;
        for (auto &x : pk) kp.push_back(x.get());
        mf_buf<uint64_t> keys; mf_buf<uint16_t> vals; uint64_t n = 0;
        MF_TRY(concat(ctx, kp, ns, keys, &n));
        if (pv) {
            std::vector<mf_buf<uint16_t> *> vp;
            for (auto &x : *pv) vp.push_back(x.get());
            uint64_t n2 = 0;
            MF_TRY(concat(ctx, vp, ns, vals, &n2));
        } else {
            MF_TRY(vals.alloc(ctx, n));
            std::vector<uint16_t> ones(std::max<uint64_t>(n, 1), 1);
            if (n) MF_HIP(hipMemcpyAsync(vals.p, ones.data(), n * 2, hipMemcpyHostToDevice, ctx->stream));
            MF_HIP(hipStreamSynchronize(ctx->stream));
        }
        for (auto &x : pk) x->reset();
        if (pv) for (auto &x : *pv) x->reset();
        return pairs_to_table(ctx, keys, vals, n, out);
    };
    MF_TRY(finish(pk_chi, nullptr, n_chi, chi_out));
    MF_TRY(finish(pk_a, &pv_a, n_a, a_out));
    return finish(pk_b, &pv_b, n_b, b_out);
}

static int nsamples_join(mf_ctx *ctx, const stats_get &get, int N, uint64_t total, int b, mf_table **out) {
    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(plan_slices(ctx, total, &S, &cap));
    std::vector<std::unique_ptr<mf_buf<uint64_t>>> pk;
    std::vector<std::unique_ptr<mf_buf<uint16_t>>> pv;
    std::vector<uint64_t> ns;
    for (uint32_t s = 0; s < S; s++) {
        mf_buf<mf_uslot> slots; uint64_t nu = 0;
        MF_TRY(union_slice(ctx, get, N, b, S, s, cap, slots, [](int) { return 1u; }, &nu));
        pk.emplace_back(new mf_buf<uint64_t>()); pv.emplace_back(new mf_buf<uint16_t>());
        MF_TRY(pk.back()->alloc(ctx, nu)); MF_TRY(pv.back()->alloc(ctx, nu));
        mf_buf<unsigned int> cur; MF_TRY(cur.alloc(ctx, 1));
        MF_HIP(hipMemsetAsync(cur.p, 0, 4, ctx->stream));
        {
            mf_ktimer tm(ctx, "k_stats_nsamples");
            k_stats_nsamples<<<grid_for(ctx, cap), 256, 0, ctx->stream>>>(slots.p, cap, pk.back()->p, pv.back()->p, cur.p);
        }
        unsigned int m = 0;
        MF_HIP(hipMemcpyAsync(&m, cur.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        MF_HIP(hipStreamSynchronize(ctx->stream));
        if (m != nu) return mf_set_error("kmers-samples-counter: %u union entries written, %llu claimed", m, (unsigned long long)nu);
        ns.push_back(m);
    }
    std::vector<mf_buf<uint64_t> *> kp; std::vector<mf_buf<uint16_t> *> vp;
    for (auto &x : pk) kp.push_back(x.get());
    for (auto &x : pv) vp.push_back(x.get());
    mf_buf<uint64_t> keys; mf_buf<uint16_t> vals; uint64_t n = 0, n2 = 0;
    MF_TRY(concat(ctx, kp, ns, keys, &n));
    MF_TRY(concat(ctx, vp, ns, vals, &n2));
    pk.clear(); pv.clear();
    return pairs_to_table(ctx, keys, vals, n, out);
}

static int check_groups(int na, int nb) {
    if (na < 1 || nb < 1) return mf_set_error("stats-kmers: both groups need at least one sample (|A| = %d, |B| = %d)", na, nb);
    if (na + nb > MF_STATS_MAX_N)
        return mf_set_error("stats-kmers: %d samples, this build supports at most %d (|A| + |B|)", na + nb, MF_STATS_MAX_N);
    return MF_OK;
}
static int check_p(double pchi2) {
    if (!(pchi2 >= 0.0 && pchi2 <= 1.0)) return mf_set_error("Error calculating chi-squared value! (p-value-chi2 = %g is not in [0, 1])", pchi2);
    return MF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int mf_stats_kmers_tables(mf_ctx *ctx, mf_table *const *a, int na, mf_table *const *b, int nb, int max_bad, double p_chi2, double p_mw,
                                     mf_table **chi, mf_table **group_a, mf_table **group_b, uint64_t *counters) {
    mf_range rng_("mf:stats_kmers");
    if (!ctx || !chi || !group_a || !group_b || !counters || (na && !a) || (nb && !b)) return mf_set_error("mf_stats_kmers_tables: NULL argument");
    *chi = *group_a = *group_b = nullptr;
    MF_TRY(check_groups(na, nb));
    MF_TRY(check_p(p_chi2));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    for (int j = 0; j < na + nb; j++) {
        const mf_table *t = j < na ? a[j] : b[j - na];
        if (!t) return mf_set_error("mf_stats_kmers_tables: table %d is NULL", j);
        if (t->ctx != ctx) return mf_set_error("mf_stats_kmers_tables: table %d belongs to another context", j);
        total += t->n;
    }
    std::vector<uint64_t> F((size_t)(na + nb), 0);
    std::vector<bool> have((size_t)(na + nb), false);
    stats_get get = [&](int j, int pass, mf_table **t, bool *own, uint64_t *Fj) -> int {
        *t = j < na ? a[j] : b[j - na];
        *own = false;
        if (pass == 1) {
            if (!have[(size_t)j]) { MF_TRY(mf_sum_counts(ctx, (*t)->d_counts, (*t)->n, &F[(size_t)j])); have[(size_t)j] = true; }
            *Fj = F[(size_t)j];
        }
        return MF_OK;
    };
    return stats_join(ctx, get, na, nb, total, max_bad, p_chi2, p_mw, chi, group_a, group_b, counters);
}

static int file_records(const char *const *files, int n, uint64_t *total) {
    *total = 0;
    for (int j = 0; j < n; j++) {
        if (!files[j]) return mf_set_error("file %d is NULL", j);
        struct stat st;
        if (stat(files[j], &st) != 0) return mf_set_error("can't open '%s'", files[j]);
        *total += (uint64_t)st.st_size / 10;
    }
    return MF_OK;
}

extern "C" int mf_stats_kmers(mf_ctx *ctx, const char *const *a_files, int na, const char *const *b_files, int nb, int max_bad, double p_chi2,
                              double p_mw, const char *out_dir, uint64_t *counters) {
    mf_range rng_("mf:stats_kmers(files)");
    if (!ctx || !out_dir || (na && !a_files) || (nb && !b_files)) return mf_set_error("mf_stats_kmers: NULL argument");
    MF_TRY(check_groups(na, nb));
    MF_TRY(check_p(p_chi2));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t ta = 0, tb = 0;
    MF_TRY(file_records(a_files, na, &ta));
    MF_TRY(file_records(b_files, nb, &tb));
    // (the join keys on the 64-bit values the files hold: k = 31 only picks the loader's internal partitioning, which changes no result;
    // every key of a k <= 31 file is below 2^62, a larger one is an error)
    stats_get get = [&](int j, int pass, mf_table **t, bool *own, uint64_t *Fj) -> int {
        const char *one[1] = {j < na ? a_files[j] : b_files[j - na]};
        *own = true;
        return mf_table_load_kmers_sum(ctx, one, 1, pass == 0 ? max_bad : 0, 31, t, pass == 1 ? Fj : nullptr);
    };
    mf_table *chi = nullptr, *ga = nullptr, *gb = nullptr;
    uint64_t c[9] = {0};
    int rc = stats_join(ctx, get, na, nb, ta + tb, max_bad, p_chi2, p_mw, &chi, &ga, &gb, c);
    const std::string d(out_dir);
    uint64_t w = 0;
    if (rc == MF_OK) rc = mf_table_write_kmers(chi, 0, (d + "/filtered_chisquared.kmers.bin").c_str(), (d + "/filtered_chisquared.stat.txt").c_str(), &w);
    // (values are Java shorts: every record is written, none is a count the histogram knows)
    if (rc == MF_OK) rc = mf_table_write_kmers(ga, -1, (d + "/filtered_groupA.kmers.bin").c_str(), nullptr, &w);
    if (rc == MF_OK) rc = mf_table_write_kmers(gb, -1, (d + "/filtered_groupB.kmers.bin").c_str(), nullptr, &w);
    mf_table_destroy(chi); mf_table_destroy(ga); mf_table_destroy(gb);
    if (rc == MF_OK && counters) memcpy(counters, c, sizeof c);
    return rc;
}

extern "C" int mf_kmers_samples_count_tables(mf_ctx *ctx, mf_table *const *t, int n, int max_bad, mf_table **out) {
    mf_range rng_("mf:kmers_samples_counter");
    if (!ctx || !out || (n && !t)) return mf_set_error("mf_kmers_samples_count_tables: NULL argument");
    *out = nullptr;
    if (n > 32767) return mf_set_error("kmers-samples-counter: %d input files, at most 32767 (the count is a Java short)", n);
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    for (int j = 0; j < n; j++) {
        if (!t[j]) return mf_set_error("mf_kmers_samples_count_tables: table %d is NULL", j);
        if (t[j]->ctx != ctx) return mf_set_error("mf_kmers_samples_count_tables: table %d belongs to another context", j);
        total += t[j]->n;
    }
    stats_get get = [&](int j, int, mf_table **tt, bool *own, uint64_t *) -> int { *tt = t[j]; *own = false; return MF_OK; };
    return nsamples_join(ctx, get, n, total, max_bad, out);
}

extern "C" int mf_kmers_samples_count(mf_ctx *ctx, const char *const *files, int n, int max_bad, int k, const char *kmers_bin, const char *stat_txt,
                                      uint64_t *n_kmers) {
    mf_range rng_("mf:kmers_samples_counter(files)");
    if (!ctx || !kmers_bin || (n && !files)) return mf_set_error("mf_kmers_samples_count: NULL argument");
    if (k < 1 || k > 31) return mf_set_error("k must be in [1,31]");
    if (n > 32767) return mf_set_error("kmers-samples-counter: %d input files, at most 32767 (the count is a Java short)", n);
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    MF_TRY(file_records(files, n, &total));
    stats_get get = [&](int j, int, mf_table **tt, bool *own, uint64_t *) -> int {
        const char *one[1] = {files[j]};
        *own = true;
        return mf_table_load_kmers_sum(ctx, one, 1, max_bad, k, tt, nullptr);
    };
    mf_table *t = nullptr;
    MF_TRY(nsamples_join(ctx, get, n, total, max_bad, &t));
    uint64_t w = 0;
    const int rc = mf_table_write_kmers(t, 0, kmers_bin, stat_txt, &w);
    mf_table_destroy(t);
    if (rc == MF_OK && n_kmers) *n_kmers = w;
    return rc;
}

// ===========================================================================================================================
// unique-kmers-multi (src/tools/UniqueKmersMultipleSamplesFinder.java:84-185) and kmers-multiple-filters
// (src/tools/KmersMultipleFilters.java:77-133, IOUtils.MultipleFiltersAndPrintKmers src/io/IOUtils.java:125-213) on the same union
// table.
//   unique-kmers-multi      union (MF_UNION_SUM) of the inputs; the filter samples' keys knock slots out (bit 31 of the sum word);
//                           one select of (key, (short)sum, samples) with (short)sum > b; one sort by key; filtered_<i> = the
//                           subsequence with samples >= i, by an order-keeping compaction.
//   kmers-multiple-filters  probe table {key, cd, uc, nonibd} (MF_UNION_FIELD) of the three filter tables; per input sample one
//                           probe per entry: the kept records and every entry's triple packed into 48 bits; the histogram is the
//                           sort of the packed triples and a run-length pass.
// ===========================================================================================================================
int mf_sort_u64_u32(mf_ctx *ctx, const uint64_t *d_keys_in, const uint32_t *d_vals_in, uint64_t n, int bits, uint64_t *d_keys_out, uint32_t *d_vals_out);
int mf_select_by(mf_ctx *ctx, const uint64_t *keys, const uint16_t *sel, const uint16_t *vals, uint64_t n, int thr, mf_buf<uint64_t> &ok,
                 mf_buf<uint16_t> &oc, uint64_t *n_out);
static constexpr uint64_t MF_JOIN_CURSOR_MAX = 0xFFFFFFFFull;      // the compaction cursors of the join's kernels are 32-bit

static constexpr uint32_t MF_UKM_KNOCKED = 0x80000000u;

// a filter sample's entries (count > thr): the slot of a key whose wrapped sum is > thr is knocked out
__global__ __launch_bounds__(256) void k_ukm_knock(mf_uslot *__restrict__ slots, uint64_t mask, const uint64_t *__restrict__ keys,
                                                   const uint16_t *__restrict__ cnts, uint64_t n, int thr, uint32_t S, uint32_t s,
                                                   unsigned int *__restrict__ flags) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if ((int)cnts[i] <= thr) continue;
        const uint64_t key = keys[i];
        if (key >= MF_STATS_KEY_LIMIT) { atomicOr(flags, 1u); continue; }
        const uint64_t h = mf_hash64(key);
        if (mf_stats_slice(h, S) != s) continue;
        uint64_t p = h & mask;
        for (uint64_t probe = 0; probe <= mask; probe++) {
            const ulonglong2 raw = *reinterpret_cast<const ulonglong2 *>(&slots[p]);
            if (raw.x == key) {
                if ((int)(int16_t)(uint16_t)(raw.y >> 32) > thr) atomicOr(&slots[p].row, MF_UKM_KNOCKED);
                break;
            }
            if (raw.x == MF_EMPTY) break;
            p = (p + 1) & mask;
        }
    }
}

// survivors: not knocked out and (short)sum > thr -> (key, (uint16)sum | samples << 16)   (uniform trip count: mf_wave_reserve)
__global__ __launch_bounds__(256) void k_ukm_select(const mf_uslot *__restrict__ slots, uint64_t cap, int thr, uint64_t *__restrict__ okeys,
                                                    uint32_t *__restrict__ ovals, unsigned int *__restrict__ cursor) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < cap; i0 += stride) {
        const uint64_t i = i0 + threadIdx.x;
        bool keep = false;
        ulonglong2 raw; raw.x = MF_EMPTY; raw.y = 0;
        if (i < cap) {
            raw = *reinterpret_cast<const ulonglong2 *>(&slots[i]);
            const uint32_t sw = (uint32_t)(raw.y >> 32);
            keep = raw.x != MF_EMPTY && !(sw & MF_UKM_KNOCKED) && (int)(int16_t)(uint16_t)sw > thr;
        }
        const uint32_t r = mf_wave_reserve(cursor, keep ? 1u : 0u);
        if (keep) { okeys[r] = raw.x; ovals[r] = (uint32_t)((raw.y >> 32) & 0xFFFFu) | ((uint32_t)raw.y << 16); }
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
                if (key >= MF_STATS_KEY_LIMIT) atomicOr(flags, 1u);
                else {
                    const uint64_t h = mf_hash64(key);
                    if (mf_stats_slice(h, S) == s) {
                        found = true;
                        uint64_t p = h & mask;
                        for (uint64_t probe = 0; probe <= mask; probe++) {
                            const ulonglong2 raw = *reinterpret_cast<const ulonglong2 *>(&slots[p]);
                            if (raw.x == key) { t = ((raw.y & 0xFFFFull) << 32) | (((raw.y >> 16) & 0xFFFFull) << 16) | ((raw.y >> 32) & 0xFFFFull); break; }
                            if (raw.x == MF_EMPTY) break;
                            p = (p + 1) & mask;
                        }
                    }
                }
            }
        }
        const bool keep = found && t != 0;
        const uint32_t rk = mf_wave_reserve(&cursor[0], keep ? 1u : 0u);
        const uint32_t rf = mf_wave_reserve(&cursor[1], found ? 1u : 0u);
        if (keep) { okeys[rk] = key; ovals[rk] = c; }
        if (found) tri[rf] = t;
    }
}

// run heads of the sorted packed triples -> (triple, index of its first occurrence), in any order
__global__ __launch_bounds__(256) void k_kmf_runs(const uint64_t *__restrict__ tri, uint64_t n, uint64_t *__restrict__ vals, uint64_t *__restrict__ starts,
                                                  unsigned int *__restrict__ cursor) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n; i0 += stride) {
        const uint64_t i = i0 + threadIdx.x;
        const bool head = i < n && (i == 0 || tri[i] != tri[i - 1]);
        const uint32_t r = mf_wave_reserve(cursor, head ? 1u : 0u);
        if (head) { vals[r] = tri[i]; starts[r] = i; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
// a sample for a pass over a slice: *own: destroy after use
using set_get = std::function<int(int j, mf_table **t, bool *own)>;

static int read_flags(mf_ctx *ctx, mf_buf<unsigned int> &flags, const char *what) {
    unsigned int fl = 0;
    MF_HIP(hipMemcpyAsync(&fl, flags.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    if (fl & 1u) return mf_set_error("%s: a k-mer key >= 2^62 (k-mers files hold k <= 31)", what);
    return MF_OK;
}

static int ukm_check(int n_in, int max_bad, int min_samples, int max_samples) {
    if (max_bad < 0) return mf_set_error("unique-kmers-multi: maximal-bad-frequence = %d is negative", max_bad);
    if (n_in > 32767) return mf_set_error("unique-kmers-multi: %d input files, at most 32767 (the number of samples is a Java short)", n_in);
    if (min_samples > max_samples) return mf_set_error("--min-samples parameter cannot be greater than --max-samples parameter.");
    return MF_OK;
}

// -> outs: one table per i = min_samples, min_samples + 1, ... up to max_samples or the first empty one (included); counts: their sizes
static int ukm_join(mf_ctx *ctx, const set_get &get_in, int n_in, const set_get &get_f, int n_f, uint64_t total, int b, int min_samples, int max_samples,
                    std::vector<mf_table *> &outs, std::vector<uint64_t> &counts, uint64_t *n_union) {
    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(plan_slices(ctx, total, &S, &cap));
    std::vector<std::unique_ptr<mf_buf<uint64_t>>> pk;
    std::vector<std::unique_ptr<mf_buf<uint32_t>>> pv;
    std::vector<uint64_t> ns;
    mf_buf<unsigned int> flags; MF_TRY(flags.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(flags.p, 0, 4, ctx->stream));
    *n_union = 0;
    const stats_get in_pass = [&](int j, int, mf_table **t, bool *own, uint64_t *) -> int { return get_in(j, t, own); };
    for (uint32_t s = 0; s < S; s++) {
        mf_buf<mf_uslot> slots; uint64_t nu = 0;
        MF_TRY(union_slice(ctx, in_pass, n_in, b, S, s, cap, slots, [](int) { return 0u; }, &nu, MF_UNION_SUM));
        *n_union += nu;
        for (int j = 0; j < n_f; j++) {
            mf_table *t = nullptr; bool own = false;
            MF_TRY(get_f(j, &t, &own));
            if (t->n) {
                mf_ktimer tm(ctx, "k_ukm_knock");
                k_ukm_knock<<<grid_for(ctx, t->n), 256, 0, ctx->stream>>>(slots.p, cap - 1, t->d_keys, t->d_counts, t->n, b, S, s, flags.p);
            }
            const hipError_t e = hipStreamSynchronize(ctx->stream);
            if (own) mf_table_destroy(t);
            if (e != hipSuccess) return mf_set_error("unique-kmers-multi: filter pass failed: %s", hipGetErrorString(e));
        }
        if (nu > MF_JOIN_CURSOR_MAX)
            return mf_set_error("unique-kmers-multi: %llu union k-mers in one slice, at most 2^32 - 1 (raise option stats_slices)", (unsigned long long)nu);
        pk.emplace_back(new mf_buf<uint64_t>()); pv.emplace_back(new mf_buf<uint32_t>());
        MF_TRY(pk.back()->alloc(ctx, nu)); MF_TRY(pv.back()->alloc(ctx, nu));
        mf_buf<unsigned int> cur; MF_TRY(cur.alloc(ctx, 1));
        MF_HIP(hipMemsetAsync(cur.p, 0, 4, ctx->stream));
        {
            mf_ktimer tm(ctx, "k_ukm_select");
            k_ukm_select<<<grid_for(ctx, cap), 256, 0, ctx->stream>>>(slots.p, cap, b, pk.back()->p, pv.back()->p, cur.p);
        }
        unsigned int m = 0;
        MF_HIP(hipMemcpyAsync(&m, cur.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        MF_HIP(hipStreamSynchronize(ctx->stream));
        if (m > nu) return mf_set_error("unique-kmers-multi: %u survivors of %llu union entries", m, (unsigned long long)nu);
        ns.push_back(m);
    }
    MF_TRY(read_flags(ctx, flags, "unique-kmers-multi"));
    // one sorted list of the survivors
    mf_buf<uint64_t> keys, sk; mf_buf<uint32_t> vals, sv; uint64_t n = 0, n2 = 0;
    {
        std::vector<mf_buf<uint64_t> *> kp; std::vector<mf_buf<uint32_t> *> vp;
        for (auto &x : pk) kp.push_back(x.get());
        for (auto &x : pv) vp.push_back(x.get());
        MF_TRY(concat(ctx, kp, ns, keys, &n));
        MF_TRY(concat(ctx, vp, ns, vals, &n2));
        pk.clear(); pv.clear();
    }
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

static int tables_total(mf_ctx *ctx, mf_table *const *t, int n, const char *what, uint64_t *total) {
    for (int j = 0; j < n; j++) {
        if (!t[j]) return mf_set_error("%s: table %d is NULL", what, j);
        if (t[j]->ctx != ctx) return mf_set_error("%s: table %d belongs to another context", what, j);
        if (total) *total += t[j]->n;
    }
    return MF_OK;
}

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
    const set_get gi = [&](int j, mf_table **t, bool *own) -> int { *t = inputs[j]; *own = false; return MF_OK; };
    const set_get gf = [&](int j, mf_table **t, bool *own) -> int { *t = filters[j]; *own = false; return MF_OK; };
    std::vector<mf_table *> outs; std::vector<uint64_t> cs;
    const int rc = ukm_join(ctx, gi, n_inputs, gf, n_filters, total, max_bad, min_samples, max_samples, outs, cs, n_union);
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
    auto loader = [&](const char *const *files) {
        return [=](int j, mf_table **t, bool *own) -> int {
            const char *one[1] = {files[j]};
            *own = true;
            return mf_table_load_kmers_sum(ctx, one, 1, max_bad, k, t, nullptr);
        };
    };
    const set_get gi = loader(in_files), gf = loader(filter_files);
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

// ---- kmers-multiple-filters ----
struct kmf_result { mf_table *kept = nullptr; std::vector<uint64_t> triples, counts; uint64_t found = 0; };
using kmf_sink = std::function<int(int j, kmf_result &r)>;          // takes r.kept over (destroys it)

// the packed triples of one (input, slice) -> added to hist
static int kmf_histogram(mf_ctx *ctx, mf_buf<uint64_t> &tri, uint64_t m, std::map<uint64_t, uint64_t> &hist, int bits = 48) {
    if (!m) return MF_OK;
    mf_buf<uint64_t> st; mf_buf<uint16_t> d0, d1;
    MF_TRY(st.alloc(ctx, m)); MF_TRY(d0.alloc(ctx, m)); MF_TRY(d1.alloc(ctx, m));
    MF_HIP(hipMemsetAsync(d0.p, 0, d0.bytes(), ctx->stream));
    MF_TRY(mf_sort_pairs(ctx, tri.p, d0.p, m, bits, st.p, d1.p));
    d0.reset(); d1.reset();
    mf_buf<unsigned int> cur; MF_TRY(cur.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(cur.p, 0, 4, ctx->stream));
    // (the run heads reuse tri: it has been sorted into st)
    mf_buf<uint64_t> starts; MF_TRY(starts.alloc(ctx, m));
    {
        mf_ktimer tm(ctx, "k_kmf_runs");
        k_kmf_runs<<<grid_for(ctx, m), 256, 0, ctx->stream>>>(st.p, m, tri.p, starts.p, cur.p);
    }
    unsigned int r = 0;
    MF_HIP(hipMemcpyAsync(&r, cur.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    if (r > m) return mf_set_error("kmers-multiple-filters: %u runs in %llu triples", r, (unsigned long long)m);
    std::vector<uint64_t> hv(r), hs(r);
    if (r) {
        MF_HIP(hipMemcpyAsync(hv.data(), tri.p, (size_t)r * 8, hipMemcpyDeviceToHost, ctx->stream));
        MF_HIP(hipMemcpyAsync(hs.data(), starts.p, (size_t)r * 8, hipMemcpyDeviceToHost, ctx->stream));
        MF_HIP(hipStreamSynchronize(ctx->stream));
    }
    std::vector<uint32_t> order(r);
    for (uint32_t i = 0; i < r; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return hs[x] < hs[y]; });
    for (uint32_t i = 0; i < r; i++) {
        const uint64_t end = i + 1 < r ? hs[order[i + 1]] : m;
        hist[hv[order[i]]] += end - hs[order[i]];
    }
    return MF_OK;
}

// filter tables 0 = CD, 1 = UC, 2 = NONIBD (threshold 0), `total_f` an upper bound of their entries; inputs at threshold b
static int kmf_join(mf_ctx *ctx, const set_get &get_filter, uint64_t total_f, const set_get &get_in, int n_in, int b, const kmf_sink &sink) {
    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(plan_slices(ctx, total_f, &S, &cap));
    struct per_input {
        std::vector<std::unique_ptr<mf_buf<uint64_t>>> pk; std::vector<std::unique_ptr<mf_buf<uint16_t>>> pv; std::vector<uint64_t> ns;
        std::map<uint64_t, uint64_t> hist; uint64_t found = 0;
    };
    std::vector<per_input> acc((size_t)n_in);
    mf_buf<unsigned int> flags; MF_TRY(flags.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(flags.p, 0, 4, ctx->stream));
    const stats_get f_pass = [&](int j, int, mf_table **t, bool *own, uint64_t *) -> int { return get_filter(j, t, own); };
    for (uint32_t s = 0; s < S; s++) {
        mf_buf<mf_uslot> slots; uint64_t nu = 0;
        MF_TRY(union_slice(ctx, f_pass, 3, 0, S, s, cap, slots, [](int j) { return (uint32_t)j; }, &nu, MF_UNION_FIELD));
        for (int j = 0; j < n_in; j++) {
            per_input &a = acc[(size_t)j];
            mf_table *t = nullptr; bool own = false;
            MF_TRY(get_in(j, &t, &own));
            const uint64_t n = t->n;
            mf_buf<uint64_t> ok, tri; mf_buf<uint16_t> ov; mf_buf<unsigned int> cur;
            int rc = n > MF_JOIN_CURSOR_MAX ? mf_set_error("kmers-multiple-filters: input %d has %llu entries, at most 2^32 - 1", j, (unsigned long long)n) : MF_OK;
            if (rc == MF_OK) rc = ok.alloc(ctx, n);
            if (rc == MF_OK) rc = ov.alloc(ctx, n);
            if (rc == MF_OK) rc = tri.alloc(ctx, n);
            if (rc == MF_OK) rc = cur.alloc(ctx, 2);
            unsigned int cc[2] = {0, 0};
            if (rc == MF_OK) {
                hipError_t e = hipMemsetAsync(cur.p, 0, 8, ctx->stream);
                if (e == hipSuccess && n) {
                    mf_ktimer tm(ctx, "k_kmf_probe");
                    k_kmf_probe<<<grid_for(ctx, n), 256, 0, ctx->stream>>>(slots.p, cap - 1, t->d_keys, t->d_counts, n, b, S, s, ok.p, ov.p, tri.p, cur.p, flags.p);
                }
                if (e == hipSuccess) e = hipMemcpyAsync(cc, cur.p, 8, hipMemcpyDeviceToHost, ctx->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
                if (e != hipSuccess) rc = mf_set_error("kmers-multiple-filters: probe pass failed: %s", hipGetErrorString(e));
            }
            if (own) mf_table_destroy(t);
            MF_TRY(rc);
            if (cc[0] > n || cc[1] > n) return mf_set_error("kmers-multiple-filters: %u kept and %u found of %llu entries", cc[0], cc[1], (unsigned long long)n);
            MF_TRY(read_flags(ctx, flags, "kmers-multiple-filters"));
            a.found += cc[1];
            MF_TRY(kmf_histogram(ctx, tri, cc[1], a.hist));
            tri.reset();
            // the kept records of this slice, in buffers of their size
            a.pk.emplace_back(new mf_buf<uint64_t>()); a.pv.emplace_back(new mf_buf<uint16_t>());
            MF_TRY(a.pk.back()->alloc(ctx, cc[0])); MF_TRY(a.pv.back()->alloc(ctx, cc[0]));
            if (cc[0]) {
                MF_HIP(hipMemcpyAsync(a.pk.back()->p, ok.p, (size_t)cc[0] * 8, hipMemcpyDeviceToDevice, ctx->stream));
                MF_HIP(hipMemcpyAsync(a.pv.back()->p, ov.p, (size_t)cc[0] * 2, hipMemcpyDeviceToDevice, ctx->stream));
                MF_HIP(hipStreamSynchronize(ctx->stream));
            }
            a.ns.push_back(cc[0]);
            if (s + 1 < S) continue;
            // last slice: this input is complete
            std::vector<mf_buf<uint64_t> *> kp; std::vector<mf_buf<uint16_t> *> vp;
            for (auto &x : a.pk) kp.push_back(x.get());
            for (auto &x : a.pv) vp.push_back(x.get());
            ok.reset(); ov.reset();
            mf_buf<uint64_t> keys; mf_buf<uint16_t> vals; uint64_t nk = 0, nk2 = 0;
            MF_TRY(concat(ctx, kp, a.ns, keys, &nk));
            MF_TRY(concat(ctx, vp, a.ns, vals, &nk2));
            a.pk.clear(); a.pv.clear();
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

static int empty_table(mf_ctx *ctx, mf_table **out) {
    mf_buf<uint64_t> k; mf_buf<uint16_t> v;
    MF_TRY(k.alloc(ctx, 0)); MF_TRY(v.alloc(ctx, 0));
    return pairs_to_table(ctx, k, v, 0, out);
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
    const set_get gf = [&](int j, mf_table **t, bool *own) -> int { *t = all[j]; *own = false; return MF_OK; };
    const set_get gi = [&](int, mf_table **t, bool *own) -> int { *t = table; *own = false; return MF_OK; };
    const kmf_sink sink = [&](int, kmf_result &r) -> int {
        *kept = r.kept;
        *n_triples = r.triples.size();
        for (size_t i = 0; i < r.triples.size() && i < cap; i++) { triples[i] = r.triples[i]; triple_counts[i] = r.counts[i]; }
        found_kept[0] = r.found; found_kept[1] = r.kept->n;
        return MF_OK;
    };
    const int rc = kmf_join(ctx, gf, total, gi, 1, max_bad, sink);
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
    const set_get gf = [&](int g, mf_table **t, bool *own) -> int {
        *own = true;
        if (!nl[g]) return empty_table(ctx, t);
        return mf_table_load_kmers_sum(ctx, lists[g], nl[g], 0, k, t, nullptr);
    };
    const set_get gi = [&](int j, mf_table **t, bool *own) -> int {
        const char *one[1] = {in_files[j]};
        *own = true;
        return mf_table_load_kmers_sum(ctx, one, 1, max_bad, k, t, nullptr);
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
    return kmf_join(ctx, gf, total, gi, n_inputs, max_bad, sink);
}

// ===========================================================================================================================
// kmers-color (src/tools/ColorKmersMain.java:89-136, src/algo/ColoredKmerOperations.java) on the same union table (DESIGN.md
// section 7c): the slot's 64-bit payload IS the packed value -- three 20-bit fields, class c in bits 20c .. 20c + 19 -- and a sample's
// entry adds 1 (or its value, -val) to its class's field with the reference's saturation (MF_UNION_COLOR).  Read-out, one sort by
// key, and the distinct-value histogram for the .stat.txt.  The result is an mf_ctable: ascending keys with 64-bit values.
// ===========================================================================================================================
#define MF_COLOR_MAX_N 1024

// every union entry -> (key, packed value)   (uniform trip count: mf_wave_reserve)
__global__ __launch_bounds__(256) void k_color_read(const mf_uslot *__restrict__ slots, uint64_t cap, uint64_t *__restrict__ okeys,
                                                    uint64_t *__restrict__ ovals, unsigned int *__restrict__ cursor) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < cap; i0 += stride) {
        const uint64_t i = i0 + threadIdx.x;
        ulonglong2 raw; raw.x = MF_EMPTY; raw.y = 0;
        if (i < cap) raw = *reinterpret_cast<const ulonglong2 *>(&slots[i]);
        const bool here = raw.x != MF_EMPTY;
        const uint32_t r = mf_wave_reserve(cursor, here ? 1u : 0u);
        if (here) { okeys[r] = raw.x; ovals[r] = raw.y; }
    }
}
int mf_sort_u64_u64(mf_ctx *ctx, const uint64_t *d_keys_in, const uint64_t *d_vals_in, uint64_t n, int bits, uint64_t *d_keys_out, uint64_t *d_vals_out);

int mf_ctable_adopt(mf_ctx *ctx, int k, uint64_t n, uint64_t *d_keys, size_t kb, uint64_t *d_vals, size_t vb, mf_ctable **out) {
    mf_ctable *t = new mf_ctable();
    t->ctx = ctx; t->k = k; t->n = n; t->d_keys = d_keys; t->keys_bytes = kb; t->d_vals = d_vals; t->vals_bytes = vb;
    *out = t;
    return MF_OK;
}
extern "C" void mf_ctable_destroy(mf_ctable *t) {
    if (!t) return;
    if (t->d_keys) mf_release(t->ctx, t->d_keys, t->keys_bytes);
    if (t->d_vals) mf_release(t->ctx, t->d_vals, t->vals_bytes);
    delete t;
}
extern "C" int mf_ctable_stats(const mf_ctable *t, uint64_t *n, int *k) {
    if (!t) return mf_set_error("mf_ctable_stats: NULL table");
    if (n) *n = t->n;
    if (k) *k = t->k;
    return MF_OK;
}
extern "C" int mf_ctable_export(const mf_ctable *t, uint64_t *keys, uint64_t *values, uint64_t cap, uint64_t *n) {
    if (!t || !n) return mf_set_error("mf_ctable_export: NULL argument");
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

static int color_check(int n, const int *classes, int max_bad) {
    if (n > MF_COLOR_MAX_N) return mf_set_error("kmers-color: %d samples, at most %d (a field of the packed value holds 20 bits)", n, MF_COLOR_MAX_N);
    if (max_bad < 0) return mf_set_error("kmers-color: maximal-bad-frequency = %d is negative", max_bad);
    for (int j = 0; j < n; j++)
        if (classes[j] < 0 || classes[j] > 2) return mf_set_error("kmers-color: sample %d has class %d (the classes are 0, 1 and 2)", j, classes[j]);
    return MF_OK;
}

static int color_join(mf_ctx *ctx, const stats_get &get, int N, const int *classes, uint64_t total, int b, int count_values, int k, mf_ctable **out) {
    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(plan_slices(ctx, total, &S, &cap));
    std::vector<std::unique_ptr<mf_buf<uint64_t>>> pk, pv;
    std::vector<uint64_t> ns;
    for (uint32_t s = 0; s < S; s++) {
        mf_buf<mf_uslot> slots; uint64_t nu = 0;
        MF_TRY(union_slice(ctx, get, N, b, S, s, cap, slots, [&](int j) { return (uint32_t)classes[j] | (count_values ? 4u : 0u); }, &nu, MF_UNION_COLOR));
        if (nu > MF_JOIN_CURSOR_MAX) return mf_set_error("kmers-color: %llu union k-mers in one slice, at most 2^32 - 1 (raise option stats_slices)", (unsigned long long)nu);
        pk.emplace_back(new mf_buf<uint64_t>()); pv.emplace_back(new mf_buf<uint64_t>());
        MF_TRY(pk.back()->alloc(ctx, nu)); MF_TRY(pv.back()->alloc(ctx, nu));
        mf_buf<unsigned int> cur; MF_TRY(cur.alloc(ctx, 1));
        MF_HIP(hipMemsetAsync(cur.p, 0, 4, ctx->stream));
        {
            mf_ktimer tm(ctx, "k_color_read");
            k_color_read<<<grid_for(ctx, cap), 256, 0, ctx->stream>>>(slots.p, cap, pk.back()->p, pv.back()->p, cur.p);
        }
        unsigned int m = 0;
        MF_HIP(hipMemcpyAsync(&m, cur.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        MF_HIP(hipStreamSynchronize(ctx->stream));
        if (m != nu) return mf_set_error("kmers-color: %u union entries written, %llu claimed", m, (unsigned long long)nu);
        ns.push_back(m);
    }
    std::vector<mf_buf<uint64_t> *> kp, vp;
    for (auto &x : pk) kp.push_back(x.get());
    for (auto &x : pv) vp.push_back(x.get());
    mf_buf<uint64_t> keys, vals; uint64_t n = 0, n2 = 0;
    MF_TRY(concat(ctx, kp, ns, keys, &n));
    MF_TRY(concat(ctx, vp, ns, vals, &n2));
    pk.clear(); pv.clear();
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
    stats_get get = [&](int j, int, mf_table **tt, bool *own, uint64_t *) -> int { *tt = t[j]; *own = false; return MF_OK; };
    return color_join(ctx, get, n, classes, total, max_bad, count_values, k, out);
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
    stats_get get = [&](int j, int, mf_table **tt, bool *own, uint64_t *) -> int {
        const char *one[1] = {files[j]};
        *own = true;
        return mf_table_load_kmers_sum(ctx, one, 1, max_bad, k, tt, nullptr);
    };
    mf_ctable *t = nullptr;
    MF_TRY(color_join(ctx, get, n, classes, total, max_bad, count_values, k, &t));
    uint64_t w = 0;
    const int rc = mf_ctable_write(t, kmers_bin, stat_txt, &w);
    mf_ctable_destroy(t);
    if (rc == MF_OK && n_kmers) *n_kmers = w;
    return rc;
}
