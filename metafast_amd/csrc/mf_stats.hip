// mf_stats.hip -- stats-kmers (src/tools/StatsKmersFinder.java:89-297), stats-kmers-3 (src/tools/StatsKmers3GroupsFinder.java:92-377),
// kmers-samples-counter (src/tools/KmersSamplesCounter.java:69-140) and kmers-grouped-counter
// (src/tools/KmersGroupedSamplesCounter.java:82-190) on the join core (mf_join.h); specific-kmers-3
// (src/tools/SpecificKmers3GroupsFinder.java:70-313) is a mode of the three-group join.
//
// Passes:
//   union   every sample's keys with count > b go into an HBM open-addressed table of 16-byte slots {key, presence, row}; the
//           presence word takes one atomic add per (sample, key): 1 for group A (or for every sample: kmers-samples-counter),
//           1 << 16 for group B; with three groups (stats-kmers-3, kmers-grouped-counter) three 10-bit fields, 1, 1 << 10 and
//           1 << 20 (at most 1022 samples in a group).  The key space is cut into S hash slices (top bits of fmix64), one union table per slice, so that
//           the table fits in free HBM; the samples are streamed once per slice.  (mf_join.hip)
//   select  the chi-squared decision depends on (n1A, n1B) only: the host evaluates StatsKmersFinder.chisq (float / double, in
//           the reference's order, no contraction) into a (nA+1) x (nB+1) flag table and the kernel looks it up.  Survivors get a
//           row number.
//   gather  the samples again at threshold 0: every entry of a survivor fills its cell of a u16 [rows][N] count matrix.
//   row     v_j = ((double)c_j * M) / F_j, 2 * U1 = sum over pairs of 2 [vA > vB] + [vA == vB] in integers, the Mann-Whitney test
//           as 2 * Umin < T for one integer T the host finds from the p-value formula, the in-order means, the group and Java's
//           (short)(int) cast.  One thread per row up to MF_STATS_THREAD_N samples, one wave per row above.  Three groups: the
//           three pairwise statistics (A, B), (B, C), (A, C), each against its own T; a row passes when any pair does.
// No floating point of the decisions but v_j and the means runs on the device, and those are IEEE double operations in the
// reference's order (no contraction in this file).
#pragma clang fp contract(off)
#include "mf_stats.h"
#include <algorithm>
#include <cmath>


// ---------------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------------
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

// (the three per-group sample counts of a presence word of stats-kmers-3 / kmers-grouped-counter: MF_STATS3_BITS each, mf_stats.h)
// stats-kmers-3 pass 1 (StatsKmers3GroupsFinder.java:135-170): as k_stats_select, the decision's table indexed by (n1A, n1B, n1C)
__global__ __launch_bounds__(256) void k_stats3_select(mf_uslot *__restrict__ slots, uint64_t cap, const uint8_t *__restrict__ chi_keep, int na, int nb, int nc,
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
                const int n1a = (int)(c & MF_STATS3_MASK), n1b = (int)((c >> MF_STATS3_BITS) & MF_STATS3_MASK), n1c = (int)((c >> (2 * MF_STATS3_BITS)) & MF_STATS3_MASK);
                c_n++;
                if (n1a + n1b + n1c <= scarce_max) c_scarce++;
                else if (n1a + n1b + n1c == na + nb + nc) c_all++;
                else {
                    if (n1a + n1c == 0 || n1b + n1a == 0 || n1b + n1c == 0) c_uniq++;
                    if (chi_keep[((size_t)n1a * (size_t)(nb + 1) + (size_t)n1b) * (size_t)(nc + 1) + (size_t)n1c]) keep = true;
                    else c_rej++;
                }
            }
        }
        const uint32_t r = mf_wave_reserve(cursor, keep ? 1u : 0u);
        if (keep) { slots[i].row = r; rkeys[r] = key; }
    }
    mf_stats_add(&ctr[0], c_n); mf_stats_add(&ctr[1], c_scarce); mf_stats_add(&ctr[2], c_all); mf_stats_add(&ctr[3], c_uniq); mf_stats_add(&ctr[4], c_rej);
}

// one sample's entries (count > 0) into its column of the survivors' count matrix
__global__ __launch_bounds__(256) void k_stats_gather(const mf_uslot *__restrict__ slots, uint64_t mask, const uint64_t *__restrict__ keys,
                                                      const uint16_t *__restrict__ cnts, uint64_t n, uint32_t S, uint32_t s, uint32_t col, uint32_t N,
                                                      uint16_t *__restrict__ mat) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint16_t c = cnts[i];
        if (!c) continue;
        const uint64_t key = keys[i];
        const mf_join_key k = mf_join_mine<false>(key, S, s, nullptr);  // (a key >= 2^62 is in no union: skipped, the union pass has said so)
        ulonglong2 raw;
        if (!k.mine || mf_join_find(slots, mask, k.h, key, &raw) == MF_JOIN_NOT_FOUND) continue;
        const uint32_t row = (uint32_t)(raw.y >> 32);
        if (row != MF_NO_ROW) mat[(uint64_t)row * N + col] = c;
    }
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

// ---- three groups (StatsKmers3GroupsFinder.java:256-312; the launch's arguments: mf_stats3_row_args, mf_stats.h) ----
// group 0 (A) / 1 (B) / 2 (C) / -1 (rejected) and the value (:290-304: a mean that is not greater than both others, a NaN included, loses)
__device__ __forceinline__ int mf_stats3_group(bool pass, double meanA, double meanB, double meanC, uint16_t *val) {
    if (!pass) return -1;
    if (meanA > meanB && meanA > meanC) { *val = mf_java_short(meanA); return 0; }
    if (meanB > meanA && meanB > meanC) { *val = mf_java_short(meanB); return 1; }
    *val = mf_java_short(meanC);
    return 2;
}
__device__ __forceinline__ bool mf_stats3_unique_left(double meanA, double meanB, double meanC) {
    return meanA + meanB == 0.0 || meanA + meanC == 0.0 || meanB + meanC == 0.0;
}
__device__ __forceinline__ void mf_stats3_flush(unsigned long long *ctr, uint32_t c_mw, uint32_t c_a, uint32_t c_b, uint32_t c_c, uint32_t c_ul) {
    mf_stats_add(&ctr[5], c_mw); mf_stats_add(&ctr[6], c_a); mf_stats_add(&ctr[7], c_b); mf_stats_add(&ctr[8], c_c); mf_stats_add(&ctr[9], c_ul);
}
// one pair of groups, X = v[x0 .. x0 + nx) against Y = v[y0 .. y0 + ny) (element j at v[j * STRIDE]): a NaN in X fails the pair, a NaN
// in Y adds nothing; the lanes of a wave (LANES = 64) share out Y, one thread (LANES = 1) takes it all
template <int STRIDE, int LANES>
__device__ __forceinline__ bool mf_stats3_pair(const double *v, int x0, int nx, int y0, int ny, bool nan_x, uint32_t T, int lane) {
    if (nan_x) return false;
    uint32_t u2 = 0;
    for (int i = x0; i < x0 + nx; i++) {
        const double x = v[(size_t)i * STRIDE];
        for (int j = y0 + lane; j < y0 + ny; j += LANES) { const double y = v[(size_t)j * STRIDE]; u2 += (x > y ? 2u : 0u) + (x == y ? 1u : 0u); }
    }
    if (LANES > 1) for (int d = 32; d >= 1; d >>= 1) u2 += __shfl_xor(u2, d, 64);
    const uint32_t tot = 2u * (uint32_t)nx * (uint32_t)ny, u2o = tot - u2;
    return (u2 < u2o ? u2 : u2o) < T;
}

// one thread per row, the layout of k_stats_rows_thread
__global__ __launch_bounds__(256) void k_stats3_rows_thread(mf_stats3_row_args a) {
    extern __shared__ double vs[];
    const int nab = a.na + a.nb, N = nab + a.nc;
    uint32_t c_mw = 0, c_a = 0, c_b = 0, c_c = 0, c_ul = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r0 = (uint64_t)blockIdx.x * blockDim.x; r0 < a.m; r0 += stride) {   // uniform trip count (mf_wave_reserve)
        const uint64_t r = r0 + threadIdx.x;
        int grp = -1; uint16_t val = 0;
        if (r < a.m) {
            double *v = vs + threadIdx.x;
            const uint16_t *row = a.mat + r * (uint64_t)N;
            bool nan_a = false, nan_b = false;
            for (int j = 0; j < N; j++) {
                const double x = ((double)row[j] * a.M) / a.F[j];
                v[(size_t)j * 256] = x;
                if (x != x) { if (j < a.na) nan_a = true; else if (j < nab) nan_b = true; }
            }
            const bool pass = !a.mw || mf_stats3_pair<256, 1>(v, 0, a.na, a.na, a.nb, nan_a, a.Tab, 0) ||
                              mf_stats3_pair<256, 1>(v, a.na, a.nb, nab, a.nc, nan_b, a.Tbc, 0) ||
                              mf_stats3_pair<256, 1>(v, 0, a.na, nab, a.nc, nan_a, a.Tac, 0);
            double sa = 0.0, sb = 0.0, sc = 0.0;
            for (int j = 0; j < a.na; j++) sa += v[(size_t)j * 256];
            for (int j = a.na; j < nab; j++) sb += v[(size_t)j * 256];
            for (int j = nab; j < N; j++) sc += v[(size_t)j * 256];
            const double meanA = sa / (double)a.na, meanB = sb / (double)a.nb, meanC = sc / (double)a.nc;
            grp = mf_stats3_group(pass, meanA, meanB, meanC, &val);
            c_mw += grp < 0; c_a += grp == 0; c_b += grp == 1; c_c += grp == 2;
            c_ul += grp >= 0 && mf_stats3_unique_left(meanA, meanB, meanC);
        }
        const uint32_t ia = mf_wave_reserve(&a.cur[0], grp == 0 ? 1u : 0u);
        const uint32_t ib = mf_wave_reserve(&a.cur[1], grp == 1 ? 1u : 0u);
        const uint32_t ic = mf_wave_reserve(&a.cur[2], grp == 2 ? 1u : 0u);
        if (grp == 0) { a.ka[ia] = a.rkeys[r]; a.va[ia] = val; }
        else if (grp == 1) { a.kb[ib] = a.rkeys[r]; a.vb[ib] = val; }
        else if (grp == 2) { a.kc[ic] = a.rkeys[r]; a.vc[ic] = val; }
    }
    mf_stats3_flush(a.ctr, c_mw, c_a, c_b, c_c, c_ul);
}

// one wave per row, the layout of k_stats_rows_wave (32 KiB of LDS a block).  `live`, the NaN flags and every pair's result are the
// same in all lanes of a wave, so the waves of a block part only between the two barriers.
__global__ __launch_bounds__(256) void k_stats3_rows_wave(mf_stats3_row_args a) {
    __shared__ double vs[4][MF_STATS_MAX_N];
    const int nab = a.na + a.nb, N = nab + a.nc, w = threadIdx.x >> 6, lane = mf_lane();
    double *v = vs[w];
    uint32_t c_mw = 0, c_a = 0, c_b = 0, c_c = 0, c_ul = 0;
    for (uint64_t r0 = (uint64_t)blockIdx.x * 4; r0 < a.m; r0 += (uint64_t)gridDim.x * 4) {   // block-uniform trip count
        const uint64_t r = r0 + (uint64_t)w;
        const bool live = r < a.m;
        bool nan_a = false, nan_b = false;
        if (live) {
            const uint16_t *row = a.mat + r * (uint64_t)N;
            for (int j = lane; j < N; j += 64) {
                const double x = ((double)row[j] * a.M) / a.F[j];
                v[j] = x;
                if (x != x) { if (j < a.na) nan_a = true; else if (j < nab) nan_b = true; }
            }
        }
        __syncthreads();
        const bool any_nan_a = __any(nan_a), any_nan_b = __any(nan_b);
        bool pass = true;
        if (live && a.mw)
            pass = mf_stats3_pair<1, 64>(v, 0, a.na, a.na, a.nb, any_nan_a, a.Tab, lane) ||
                   mf_stats3_pair<1, 64>(v, a.na, a.nb, nab, a.nc, any_nan_b, a.Tbc, lane) ||
                   mf_stats3_pair<1, 64>(v, 0, a.na, nab, a.nc, any_nan_a, a.Tac, lane);
        if (live && lane == 0) {
            double sa = 0.0, sb = 0.0, sc = 0.0;
            for (int j = 0; j < a.na; j++) sa += v[j];
            for (int j = a.na; j < nab; j++) sb += v[j];
            for (int j = nab; j < N; j++) sc += v[j];
            uint16_t val = 0;
            const uint64_t key = a.rkeys[r];
            const double meanA = sa / (double)a.na, meanB = sb / (double)a.nb, meanC = sc / (double)a.nc;
            const int grp = mf_stats3_group(pass, meanA, meanB, meanC, &val);
            c_mw += grp < 0; c_a += grp == 0; c_b += grp == 1; c_c += grp == 2;
            c_ul += grp >= 0 && mf_stats3_unique_left(meanA, meanB, meanC);
            if (grp == 0) { const uint32_t i = atomicAdd(&a.cur[0], 1u); a.ka[i] = key; a.va[i] = val; }
            else if (grp == 1) { const uint32_t i = atomicAdd(&a.cur[1], 1u); a.kb[i] = key; a.vb[i] = val; }
            else if (grp == 2) { const uint32_t i = atomicAdd(&a.cur[2], 1u); a.kc[i] = key; a.vc[i] = val; }
        }
        __syncthreads();
    }
    mf_stats3_flush(a.ctr, c_mw, c_a, c_b, c_c, c_ul);
}

// ---- specific-kmers-3 (SpecificKmers3GroupsFinder.java:166-254): the rows of k_stats3_rows_*, decided its way ----
// A sample that does not hold the k-mer contributes 0, not 0 * M / F_j (:173-199): an empty sample (F_j = 0) gives no NaN, so no pair has
// a NaN rule to apply.  Unique left is the presence test of :207 on the gathered row (a count of 0 = absent: every load is at threshold
// 0), not a test of the means -- M may be 0 (truncated), and then every mean is.
__device__ __forceinline__ double mf_specific3_value(uint16_t c, double M, double F) { return c ? ((double)c * M) / F : 0.0; }
__device__ __forceinline__ bool mf_specific3_unique(uint32_t n1a, uint32_t n1b, uint32_t n1c) { return n1a + n1c == 0 || n1b + n1a == 0 || n1b + n1c == 0; }

// one thread per row, the layout of k_stats_rows_thread
__global__ __launch_bounds__(256) void k_specific3_rows_thread(mf_stats3_row_args a) {
    extern __shared__ double vs[];
    const int nab = a.na + a.nb, N = nab + a.nc;
    uint32_t c_mw = 0, c_a = 0, c_b = 0, c_c = 0, c_ul = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r0 = (uint64_t)blockIdx.x * blockDim.x; r0 < a.m; r0 += stride) {   // uniform trip count (mf_wave_reserve)
        const uint64_t r = r0 + threadIdx.x;
        int grp = -1; uint16_t val = 0;
        if (r < a.m) {
            double *v = vs + threadIdx.x;
            const uint16_t *row = a.mat + r * (uint64_t)N;
            uint32_t n1a = 0, n1b = 0, n1c = 0;
            for (int j = 0; j < N; j++) {
                const uint16_t c = row[j];
                v[(size_t)j * 256] = mf_specific3_value(c, a.M, a.F[j]);
                if (c) { if (j < a.na) n1a++; else if (j < nab) n1b++; else n1c++; }
            }
            const bool pass = !a.mw || mf_stats3_pair<256, 1>(v, 0, a.na, a.na, a.nb, false, a.Tab, 0) ||
                              mf_stats3_pair<256, 1>(v, a.na, a.nb, nab, a.nc, false, a.Tbc, 0) ||
                              mf_stats3_pair<256, 1>(v, 0, a.na, nab, a.nc, false, a.Tac, 0);
            double sa = 0.0, sb = 0.0, sc = 0.0;
            for (int j = 0; j < a.na; j++) sa += v[(size_t)j * 256];
            for (int j = a.na; j < nab; j++) sb += v[(size_t)j * 256];
            for (int j = nab; j < N; j++) sc += v[(size_t)j * 256];
            grp = mf_stats3_group(pass, sa / (double)a.na, sb / (double)a.nb, sc / (double)a.nc, &val);
            c_mw += grp < 0; c_a += grp == 0; c_b += grp == 1; c_c += grp == 2;
            c_ul += grp >= 0 && mf_specific3_unique(n1a, n1b, n1c);
        }
        const uint32_t ia = mf_wave_reserve(&a.cur[0], grp == 0 ? 1u : 0u);
        const uint32_t ib = mf_wave_reserve(&a.cur[1], grp == 1 ? 1u : 0u);
        const uint32_t ic = mf_wave_reserve(&a.cur[2], grp == 2 ? 1u : 0u);
        if (grp == 0) { a.ka[ia] = a.rkeys[r]; a.va[ia] = val; }
        else if (grp == 1) { a.kb[ib] = a.rkeys[r]; a.vb[ib] = val; }
        else if (grp == 2) { a.kc[ic] = a.rkeys[r]; a.vc[ic] = val; }
    }
    mf_stats3_flush(a.ctr, c_mw, c_a, c_b, c_c, c_ul);
}

// one wave per row, the layout of k_stats3_rows_wave (32 KiB of LDS a block); the holders of a row are counted by the lanes and summed
__global__ __launch_bounds__(256) void k_specific3_rows_wave(mf_stats3_row_args a) {
    __shared__ double vs[4][MF_STATS_MAX_N];
    const int nab = a.na + a.nb, N = nab + a.nc, w = threadIdx.x >> 6, lane = mf_lane();
    double *v = vs[w];
    uint32_t c_mw = 0, c_a = 0, c_b = 0, c_c = 0, c_ul = 0;
    for (uint64_t r0 = (uint64_t)blockIdx.x * 4; r0 < a.m; r0 += (uint64_t)gridDim.x * 4) {   // block-uniform trip count
        const uint64_t r = r0 + (uint64_t)w;
        const bool live = r < a.m;
        uint32_t n1 = 0;                                  // holders this lane saw: A | B << 10 | C << 20 (at most 1024 in all)
        if (live) {
            const uint16_t *row = a.mat + r * (uint64_t)N;
            for (int j = lane; j < N; j += 64) {
                const uint16_t c = row[j];
                v[j] = mf_specific3_value(c, a.M, a.F[j]);
                if (c) n1 += j < a.na ? 1u : j < nab ? 1u << 10 : 1u << 20;
            }
        }
        __syncthreads();
        for (int d = 32; d >= 1; d >>= 1) n1 += __shfl_xor(n1, d, 64);
        bool pass = true;
        if (live && a.mw)
            pass = mf_stats3_pair<1, 64>(v, 0, a.na, a.na, a.nb, false, a.Tab, lane) ||
                   mf_stats3_pair<1, 64>(v, a.na, a.nb, nab, a.nc, false, a.Tbc, lane) ||
                   mf_stats3_pair<1, 64>(v, 0, a.na, nab, a.nc, false, a.Tac, lane);
        if (live && lane == 0) {
            double sa = 0.0, sb = 0.0, sc = 0.0;
            for (int j = 0; j < a.na; j++) sa += v[j];
            for (int j = a.na; j < nab; j++) sb += v[j];
            for (int j = nab; j < N; j++) sc += v[j];
            uint16_t val = 0;
            const uint64_t key = a.rkeys[r];
            const int grp = mf_stats3_group(pass, sa / (double)a.na, sb / (double)a.nb, sc / (double)a.nc, &val);
            c_mw += grp < 0; c_a += grp == 0; c_b += grp == 1; c_c += grp == 2;
            c_ul += grp >= 0 && mf_specific3_unique(n1 & 0x3FFu, (n1 >> 10) & 0x3FFu, n1 >> 20);
            if (grp == 0) { const uint32_t i = atomicAdd(&a.cur[0], 1u); a.ka[i] = key; a.va[i] = val; }
            else if (grp == 1) { const uint32_t i = atomicAdd(&a.cur[1], 1u); a.kb[i] = key; a.vb[i] = val; }
            else if (grp == 2) { const uint32_t i = atomicAdd(&a.cur[2], 1u); a.kc[i] = key; a.vc[i] = val; }
        }
        __syncthreads();
    }
    mf_stats3_flush(a.ctr, c_mw, c_a, c_b, c_c, c_ul);
}

// kmers-grouped-counter: the presence word of every key of the -kf table that slice s holds (a key in no group keeps its 0)
__global__ __launch_bounds__(256) void k_grouped_probe(const mf_uslot *__restrict__ slots, uint64_t mask, const uint64_t *__restrict__ keys, uint64_t n,
                                                       uint32_t S, uint32_t s, uint32_t *__restrict__ words, unsigned int *__restrict__ flags) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[i];
        const mf_join_key k = mf_join_mine<true>(key, S, s, flags);
        ulonglong2 raw;
        if (!k.mine || mf_join_find(slots, mask, k.h, key, &raw) == MF_JOIN_NOT_FOUND) continue;
        words[i] = (uint32_t)raw.y;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host: the decisions' tables (StatsKmersFinder.chisq :300-316; commons-math3 3.6.1 MannWhitneyUTest.calculateAsymptoticPValue)
// ---------------------------------------------------------------------------------------------------------------------------
bool chisq_keep(float c0, float c1, float p0, float p1, double value) {
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
double chi2_1_quantile(double p_chi2) {
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
// StatsKmers3GroupsFinder.chisq :346-369 (c = A, p = B, q = C; Math.pow(x, 2) = x * x)
bool chisq3_keep(float c0, float c1, float p0, float p1, float q0, float q1, double value) {
    float tmp = c0;
    c0 = 100 * c0 / (c0 + c1);
    c1 = 100 * c1 / (tmp + c1);
    tmp = p0;
    p0 = 100 * p0 / (p0 + p1);
    p1 = 100 * p1 / (tmp + p1);
    tmp = q0;
    q0 = 100 * q0 / (q0 + q1);
    q1 = 100 * q1 / (tmp + q1);
    const float gr_1 = c0 + c1, gr_2 = p0 + p1, gr_3 = q0 + q1, all = gr_1 + gr_2 + gr_3;
    const float x1 = gr_1 / all * (p1 + c1 + q1), x2 = gr_1 / all * (p0 + c0 + q0), x3 = gr_2 / all * (p1 + c1 + q1), x4 = gr_2 / all * (p0 + c0 + q0),
                x5 = gr_3 / all * (p1 + c1 + q1), x6 = gr_3 / all * (p0 + c0 + q0);
    const double d1 = (double)std::fabs(p1 - x1) - 0.5, d2 = (double)std::fabs(p0 - x2) - 0.5, d3 = (double)std::fabs(c1 - x3) - 0.5,
                 d4 = (double)std::fabs(c0 - x4) - 0.5, d5 = (double)std::fabs(q1 - x5) - 0.5, d6 = (double)std::fabs(q0 - x6) - 0.5;
    double stat = d1 * d1 / (double)x1;
    stat = stat + d2 * d2 / (double)x2;
    stat = stat + d3 * d3 / (double)x3;
    stat = stat + d4 * d4 / (double)x4;
    stat = stat + d5 * d5 / (double)x5;
    stat = stat + d6 * d6 / (double)x6;
    return value < stat;                                  // (NaN: rejected)
}
// ChiSquaredDistribution(2).inverseCumulativeProbability(1 - p): P(X > q) = exp(-q / 2), so q = -2 ln p (the reference's solver agrees
// to its accuracy of 1e-15, not to the last bit)
double chi2_2_quantile(double p_chi2) {
    if (p_chi2 <= 0.0) return INFINITY;
    if (p_chi2 >= 1.0) return 0.0;
    return -2.0 * std::log(p_chi2);
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
// (or_equal: the smallest whose p is > pmw -- specific-kmers keeps a row unless p > pmw, SpecificKmersFinder.java:166-170)
uint32_t mw_threshold(int na, int nb, double pmw, bool or_equal) {
    const uint32_t top = (uint32_t)na * (uint32_t)nb;
    for (uint32_t u2 = 0; u2 <= top; u2++) {
        const double p = mw_pvalue(u2 / 2.0, na, nb);
        if (or_equal ? p > pmw : !(p < pmw)) return u2;
    }
    return top + 1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host: the join
// ---------------------------------------------------------------------------------------------------------------------------
// the two-group row kernels over a.m rows (nothing is queued for none): one thread per row up to MF_STATS_THREAD_N samples, one wave per row
// above.  The launcher of stats_join (below) and of the wide tool (mf_wstats.hip), which hands in row numbers as rkeys.
void mf_stats_rows_launch(mf_ctx *ctx, const mf_stats_row_args &ra) {
    if (!ra.m) return;
    const int N = ra.na + ra.nb;
    if (N <= MF_STATS_THREAD_N) {
        const unsigned g_thread = (unsigned)std::min<uint64_t>((ra.m + 255) / 256, (uint64_t)ctx->n_cu * 8);
        mf_ktimer tm(ctx, "k_stats_rows_thread");
        k_stats_rows_thread<<<g_thread, 256, (size_t)N * 256 * sizeof(double), ctx->stream>>>(ra);
    } else {
        const unsigned g_wave = (unsigned)std::min<uint64_t>((ra.m + 3) / 4, (uint64_t)ctx->n_cu * 16);
        mf_ktimer tm(ctx, "k_stats_rows_wave");
        k_stats_rows_wave<<<g_wave, 256, 0, ctx->stream>>>(ra);
    }
}
// the three-group row kernels over a.m rows, the same grids: stats-kmers-3's, or (specific) specific-kmers-3's.  The launcher of stats_join
// (below) and of the wide three-group tool (mf_wstats.hip), which hands in row numbers as rkeys.
void mf_stats3_rows_launch(mf_ctx *ctx, const mf_stats3_row_args &ra, bool specific) {
    if (!ra.m) return;
    const int N = ra.na + ra.nb + ra.nc;
    const unsigned g_thread = (unsigned)std::min<uint64_t>((ra.m + 255) / 256, (uint64_t)ctx->n_cu * 8);
    const unsigned g_wave = (unsigned)std::min<uint64_t>((ra.m + 3) / 4, (uint64_t)ctx->n_cu * 16);
    const size_t lds = (size_t)N * 256 * sizeof(double);
    if (specific && N <= MF_STATS_THREAD_N) {
        mf_ktimer tm(ctx, "k_specific3_rows_thread");
        k_specific3_rows_thread<<<g_thread, 256, lds, ctx->stream>>>(ra);
    } else if (specific) {
        mf_ktimer tm(ctx, "k_specific3_rows_wave");
        k_specific3_rows_wave<<<g_wave, 256, 0, ctx->stream>>>(ra);
    } else if (N <= MF_STATS_THREAD_N) {
        mf_ktimer tm(ctx, "k_stats3_rows_thread");
        k_stats3_rows_thread<<<g_thread, 256, lds, ctx->stream>>>(ra);
    } else {
        mf_ktimer tm(ctx, "k_stats3_rows_wave");
        k_stats3_rows_wave<<<g_wave, 256, 0, ctx->stream>>>(ra);
    }
}

// sample j for the gather pass: its entries at threshold 0, and F_j = the sum of its counts
using stats_get_counts = std::function<int(int j, mf_join_sample &, uint64_t *F)>;

// the join of G = 2 (stats-kmers) or 3 (stats-kmers-3) groups of ng[0 .. G) samples, numbered group by group; grp_out[0 .. G) get the
// groups' tables, counters MF_STATS_COUNTERS (G = 2) or MF_STATS3_COUNTERS values.  specific (G = 3 only): the decision of specific-kmers-3
// (SpecificKmers3GroupsFinder.java:70-280) -- the quantile of 1 degree of freedom, M truncated to a long, an absent sample's value 0
// whatever its F_j, unique-left by presence (k_specific3_rows_*); chi_out may then be NULL: the tool writes no chi-squared list
static int stats_join(mf_ctx *ctx, const mf_join_get &get, const stats_get_counts &get_counts, const int *ng, int G, uint64_t total, int b, double pchi2,
                      double pmw, mf_table **chi_out, mf_table **grp_out, uint64_t *counters, bool specific = false) {
    const int na = ng[0], nb = ng[1], nc = G == 3 ? ng[2] : 0, N = na + nb + nc;
    const int n_ctr = G == 3 ? MF_STATS3_COUNTERS : MF_STATS_COUNTERS;
    // the decisions' tables (three groups: one byte per (n1A, n1B, n1C), at most 342^3 = 4 * 10^7 of them)
    const double q = G == 3 && !specific ? chi2_2_quantile(pchi2) : chi2_1_quantile(pchi2);
    std::vector<uint8_t> chi((size_t)(na + 1) * (nb + 1) * (nc + 1), 0);
    for (int n1a = 0; n1a <= na; n1a++)
        for (int n1b = 0; n1b <= nb; n1b++) {
            if (G == 2) { chi[(size_t)n1a * (nb + 1) + n1b] = chisq_keep((float)(na - n1a), (float)n1a, (float)(nb - n1b), (float)n1b, q) ? 1 : 0; continue; }
            for (int n1c = 0; n1c <= nc; n1c++)
                chi[((size_t)n1a * (nb + 1) + n1b) * (nc + 1) + n1c] =
                    chisq3_keep((float)(na - n1a), (float)n1a, (float)(nb - n1b), (float)n1b, (float)(nc - n1c), (float)n1c, q) ? 1 : 0;
        }
    const int scarce_max = (int)std::ceil(N * 0.05);
    const int mw = pmw > 0 ? 1 : 0;
    const uint32_t T = mw ? mw_threshold(na, nb, pmw) : 0u;                                   // (A, B)
    const uint32_t Tbc = mw && G == 3 ? mw_threshold(nb, nc, pmw) : 0u, Tac = mw && G == 3 ? mw_threshold(na, nc, pmw) : 0u;
    if (ctx->opt_verbose && G == 2) fprintf(stderr, "[mf] stats: q = %.17g, scarce <= %d, 2*Umin < %u\n", q, scarce_max, T);
    if (ctx->opt_verbose && G == 3) fprintf(stderr, "[mf] stats3: q = %.17g, scarce <= %d, 2*Umin < %u (A, B), %u (B, C), %u (A, C)\n", q, scarce_max, T, Tbc, Tac);
    mf_buf<uint8_t> dchi; MF_TRY(dchi.alloc(ctx, chi.size()));
    MF_HIP(hipMemcpyAsync(dchi.p, chi.data(), chi.size(), hipMemcpyHostToDevice, ctx->stream));
    mf_buf<unsigned long long> ctr; MF_TRY(ctr.alloc(ctx, (size_t)n_ctr));
    MF_HIP(hipMemsetAsync(ctr.p, 0, (size_t)n_ctr * 8, ctx->stream));

    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(plan_slices(ctx, total, &S, &cap));
    std::vector<uint32_t> add((size_t)N);
    for (int j = 0; j < N; j++) {
        const int g = j < na ? 0 : j < na + nb ? 1 : 2;
        add[(size_t)j] = 1u << ((G == 3 ? MF_STATS3_BITS : 16) * g);
    }
    mf_join_parts<uint64_t, uint16_t> p_chi, p_g[3];         // (the chi-squared list: keys alone)
    std::vector<uint64_t> F((size_t)N, 0);
    bool have_F = false;
    for (uint32_t s = 0; s < S; s++) {
        mf_buf<mf_uslot> slots; uint64_t nu = 0;
        MF_TRY(mf_join_union(ctx, get, N, b, MF_UNION_PRESENCE, add.data(), S, s, cap, slots, &nu));
        // select
        uint64_t *rkeys = nullptr;
        MF_TRY(p_chi.add(ctx, nu, &rkeys, nullptr));
        unsigned int m32 = 0;
        MF_TRY(mf_join_cursors(ctx, 1, &m32, [&](unsigned int *cur) {
            if (G == 2) {
                mf_ktimer tm(ctx, "k_stats_select");
                k_stats_select<<<grid_for(ctx, cap), 256, 0, ctx->stream>>>(slots.p, cap, dchi.p, na, nb, scarce_max, rkeys, cur, ctr.p);
            } else {
                mf_ktimer tm(ctx, "k_stats3_select");
                k_stats3_select<<<grid_for(ctx, cap), 256, 0, ctx->stream>>>(slots.p, cap, dchi.p, na, nb, nc, scarce_max, rkeys, cur, ctr.p);
            }
        }));
        const uint64_t m = m32;
        p_chi.wrote(m);
        // gather
        mf_buf<uint16_t> mat; MF_TRY(mat.alloc(ctx, m * (uint64_t)N));
        if (m) MF_HIP(hipMemsetAsync(mat.p, 0, mat.bytes(), ctx->stream));
        const bool need_counts = m > 0 || !have_F;
        for (int j = 0; j < N && need_counts; j++)
            MF_TRY(mf_join_pass(ctx, [&](int jj, mf_join_sample &sm) { return get_counts(jj, sm, &F[(size_t)jj]); }, j, "stats join: gather pass",
                                [&](const mf_table *t) {
                                    if (!m) return;
                                    mf_ktimer tm(ctx, "k_stats_gather");
                                    k_stats_gather<<<grid_for(ctx, t->n), 256, 0, ctx->stream>>>(slots.p, cap - 1, t->d_keys, t->d_counts, t->n, S, s, (uint32_t)j, (uint32_t)N, mat.p);
                                }));
        have_F = true;
        slots.reset();
        // rows
        uint64_t Fsum = 0;
        for (uint64_t x : F) Fsum += x;
        const double M = specific ? (double)(Fsum / (uint64_t)N) : (double)Fsum / N;   // (specific: meanSumKmers is a long, :147-151)
        std::vector<double> Fd((size_t)N);
        for (int j = 0; j < N; j++) Fd[(size_t)j] = (double)F[(size_t)j];
        mf_buf<double> dF; MF_TRY(dF.alloc(ctx, N));
        MF_HIP(hipMemcpyAsync(dF.p, Fd.data(), (size_t)N * 8, hipMemcpyHostToDevice, ctx->stream));
        uint64_t *kg[3] = {nullptr, nullptr, nullptr}; uint16_t *vg[3] = {nullptr, nullptr, nullptr};
        for (int g = 0; g < G; g++) MF_TRY(p_g[g].add(ctx, m, &kg[g], &vg[g]));
        unsigned int cc[3] = {0, 0, 0};
        MF_TRY(mf_join_cursors(ctx, G, cc, [&](unsigned int *cur) {
            if (G == 2)
                mf_stats_rows_launch(ctx, mf_stats_row_args{mat.p, rkeys, m, na, nb, dF.p, M, mw, T, kg[0], kg[1], vg[0], vg[1], cur, ctr.p});
            else
                mf_stats3_rows_launch(ctx, mf_stats3_row_args{mat.p, rkeys, m, na, nb, nc, dF.p, M, mw, T, Tbc, Tac, kg[0], kg[1], kg[2], vg[0], vg[1], vg[2], cur, ctr.p},
                                      specific);
        }));
        for (int g = 0; g < G; g++) p_g[g].wrote(cc[g]);
    }
    unsigned long long hc[MF_STATS3_COUNTERS];
    MF_HIP(hipMemcpyAsync(hc, ctr.p, (size_t)n_ctr * 8, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n_ctr; i++) counters[i] = hc[i];
    // the lists: concatenated over the slices, sorted, as tables
    auto finish = [&](mf_join_parts<uint64_t, uint16_t> &p, mf_table **out) -> int {
        mf_buf<uint64_t> keys; mf_buf<uint16_t> vals; uint64_t n = 0;
        const bool ones_for_values = p.keys_only();            // (the chi-squared list: every value is 1)
        MF_TRY(p.concat(ctx, keys, vals, &n));
        if (ones_for_values) {
            MF_TRY(vals.alloc(ctx, n));
            std::vector<uint16_t> ones(std::max<uint64_t>(n, 1), 1);
            if (n) MF_HIP(hipMemcpyAsync(vals.p, ones.data(), n * 2, hipMemcpyHostToDevice, ctx->stream));
            MF_HIP(hipStreamSynchronize(ctx->stream));
        }
        return pairs_to_table(ctx, keys, vals, n, out);
    };
    if (chi_out) MF_TRY(finish(p_chi, chi_out));
    for (int g = 0; g < G; g++) MF_TRY(finish(p_g[g], &grp_out[g]));
    return MF_OK;
}

static int nsamples_join(mf_ctx *ctx, const mf_join_get &get, int N, uint64_t total, int b, mf_table **out) {
    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(plan_slices(ctx, total, &S, &cap));
    const std::vector<uint32_t> add((size_t)N, 1u);
    mf_join_parts<uint64_t, uint16_t> parts;
    for (uint32_t s = 0; s < S; s++) {
        mf_buf<mf_uslot> slots; uint64_t nu = 0;
        MF_TRY(mf_join_union(ctx, get, N, b, MF_UNION_PRESENCE, add.data(), S, s, cap, slots, &nu));
        MF_TRY(mf_join_read(ctx, slots.p, cap, nu, mf_read_nsamples{}, parts));
    }
    mf_buf<uint64_t> keys; mf_buf<uint16_t> vals; uint64_t n = 0;
    MF_TRY(parts.concat(ctx, keys, vals, &n));
    return pairs_to_table(ctx, keys, vals, n, out);
}

int mf_stats_check_groups(int na, int nb) {
    if (na < 1 || nb < 1) return mf_set_error("stats-kmers: both groups need at least one sample (|A| = %d, |B| = %d)", na, nb);
    if (na + nb > MF_STATS_MAX_N)
        return mf_set_error("stats-kmers: %d samples, this build supports at most %d (|A| + |B|)", na + nb, MF_STATS_MAX_N);
    return MF_OK;
}
int mf_stats_check_groups3(int na, int nb, int nc) {
    if (na < 1 || nb < 1 || nc < 1)
        return mf_set_error("stats-kmers-3: every group needs at least one sample (|A| = %d, |B| = %d, |C| = %d)", na, nb, nc);
    if ((int64_t)na + nb + nc > MF_STATS_MAX_N)
        return mf_set_error("stats-kmers-3: %lld samples, this build supports at most %d (|A| + |B| + |C|)", (long long)na + nb + nc, MF_STATS_MAX_N);
    return MF_OK;
}
int mf_stats_check_p(double pchi2) {
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
    MF_TRY(mf_stats_check_groups(na, nb));
    MF_TRY(mf_stats_check_p(p_chi2));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    std::vector<mf_table *> all(a, a + na);
    all.insert(all.end(), b, b + nb);
    MF_TRY(tables_total(ctx, all.data(), na + nb, "mf_stats_kmers_tables", &total));
    std::vector<uint64_t> F((size_t)(na + nb), 0);
    std::vector<bool> have((size_t)(na + nb), false);
    const stats_get_counts get_counts = [&](int j, mf_join_sample &sm, uint64_t *Fj) -> int {
        sm.borrow(all[(size_t)j]);
        if (!have[(size_t)j]) { MF_TRY(mf_sum_counts(ctx, sm.t->d_counts, sm.t->n, &F[(size_t)j])); have[(size_t)j] = true; }
        *Fj = F[(size_t)j];
        return MF_OK;
    };
    const int ng[2] = {na, nb};
    mf_table *grp[2] = {nullptr, nullptr};
    const int rc = stats_join(ctx, mf_join_tables(all.data()), get_counts, ng, 2, total, max_bad, p_chi2, p_mw, chi, grp, counters);
    *group_a = grp[0]; *group_b = grp[1];
    return rc;
}

extern "C" int mf_stats_kmers(mf_ctx *ctx, const char *const *a_files, int na, const char *const *b_files, int nb, int max_bad, double p_chi2,
                              double p_mw, const char *out_dir, uint64_t *counters) {
    mf_range rng_("mf:stats_kmers(files)");
    if (!ctx || !out_dir || (na && !a_files) || (nb && !b_files)) return mf_set_error("mf_stats_kmers: NULL argument");
    MF_TRY(mf_stats_check_groups(na, nb));
    MF_TRY(mf_stats_check_p(p_chi2));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t ta = 0, tb = 0;
    MF_TRY(file_records(a_files, na, &ta));
    MF_TRY(file_records(b_files, nb, &tb));
    // (the join keys on the 64-bit values the files hold: k = 31 only picks the loader's internal partitioning, which changes no result;
    // every key of a k <= 31 file is below 2^62, a larger one is an error)
    std::vector<const char *> files(a_files, a_files + na);
    files.insert(files.end(), b_files, b_files + nb);
    const stats_get_counts get_counts = [&](int j, mf_join_sample &sm, uint64_t *Fj) -> int { return sm.load(&files[(size_t)j], 1, 0, 31, Fj); };
    mf_table *chi = nullptr, *grp[2] = {nullptr, nullptr};
    uint64_t c[MF_STATS_COUNTERS] = {0};
    const int ng[2] = {na, nb};
    int rc = stats_join(ctx, mf_join_files(files.data(), max_bad, 31), get_counts, ng, 2, ta + tb, max_bad, p_chi2, p_mw, &chi, grp, c);
    mf_table *ga = grp[0], *gb = grp[1];
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

extern "C" int mf_stats_kmers3_tables(mf_ctx *ctx, mf_table *const *a, int na, mf_table *const *b, int nb, mf_table *const *c, int nc, int max_bad,
                                      double p_chi2, double p_mw, mf_table **chi, mf_table **group_a, mf_table **group_b, mf_table **group_c,
                                      uint64_t *counters) {
    mf_range rng_("mf:stats_kmers3");
    if (!ctx || !chi || !group_a || !group_b || !group_c || !counters || (na && !a) || (nb && !b) || (nc && !c))
        return mf_set_error("mf_stats_kmers3_tables: NULL argument");
    *chi = *group_a = *group_b = *group_c = nullptr;
    MF_TRY(mf_stats_check_groups3(na, nb, nc));
    MF_TRY(mf_stats_check_p(p_chi2));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    std::vector<mf_table *> all(a, a + na);
    all.insert(all.end(), b, b + nb);
    all.insert(all.end(), c, c + nc);
    const int N = na + nb + nc;
    MF_TRY(tables_total(ctx, all.data(), N, "mf_stats_kmers3_tables", &total));
    std::vector<uint64_t> F((size_t)N, 0);
    std::vector<bool> have((size_t)N, false);
    const stats_get_counts get_counts = [&](int j, mf_join_sample &sm, uint64_t *Fj) -> int {
        sm.borrow(all[(size_t)j]);
        if (!have[(size_t)j]) { MF_TRY(mf_sum_counts(ctx, sm.t->d_counts, sm.t->n, &F[(size_t)j])); have[(size_t)j] = true; }
        *Fj = F[(size_t)j];
        return MF_OK;
    };
    const int ng[3] = {na, nb, nc};
    mf_table *grp[3] = {nullptr, nullptr, nullptr};
    const int rc = stats_join(ctx, mf_join_tables(all.data()), get_counts, ng, 3, total, max_bad, p_chi2, p_mw, chi, grp, counters);
    *group_a = grp[0]; *group_b = grp[1]; *group_c = grp[2];
    return rc;
}

extern "C" int mf_stats_kmers3(mf_ctx *ctx, const char *const *a_files, int na, const char *const *b_files, int nb, const char *const *c_files, int nc,
                               int max_bad, double p_chi2, double p_mw, const char *out_dir, uint64_t *counters) {
    mf_range rng_("mf:stats_kmers3(files)");
    if (!ctx || !out_dir || (na && !a_files) || (nb && !b_files) || (nc && !c_files)) return mf_set_error("mf_stats_kmers3: NULL argument");
    MF_TRY(mf_stats_check_groups3(na, nb, nc));
    MF_TRY(mf_stats_check_p(p_chi2));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t ta = 0, tb = 0, tc = 0;
    MF_TRY(file_records(a_files, na, &ta));
    MF_TRY(file_records(b_files, nb, &tb));
    MF_TRY(file_records(c_files, nc, &tc));
    std::vector<const char *> files(a_files, a_files + na);   // (keys and k as in mf_stats_kmers)
    files.insert(files.end(), b_files, b_files + nb);
    files.insert(files.end(), c_files, c_files + nc);
    const stats_get_counts get_counts = [&](int j, mf_join_sample &sm, uint64_t *Fj) -> int { return sm.load(&files[(size_t)j], 1, 0, 31, Fj); };
    mf_table *chi = nullptr, *grp[3] = {nullptr, nullptr, nullptr};
    uint64_t c[MF_STATS3_COUNTERS] = {0};
    const int ng[3] = {na, nb, nc};
    int rc = stats_join(ctx, mf_join_files(files.data(), max_bad, 31), get_counts, ng, 3, ta + tb + tc, max_bad, p_chi2, p_mw, &chi, grp, c);
    const std::string d(out_dir);
    uint64_t w = 0;
    if (rc == MF_OK) rc = mf_table_write_kmers(chi, 0, (d + "/filtered_chisquared.kmers.bin").c_str(), (d + "/filtered_chisquared.stat.txt").c_str(), &w);
    static const char *names[3] = {"/filtered_groupA.kmers.bin", "/filtered_groupB.kmers.bin", "/filtered_groupC.kmers.bin"};
    for (int g = 0; g < 3; g++)
        if (rc == MF_OK) rc = mf_table_write_kmers(grp[g], -1, (d + names[g]).c_str(), nullptr, &w);
    mf_table_destroy(chi);
    for (int g = 0; g < 3; g++) mf_table_destroy(grp[g]);
    if (rc == MF_OK && counters) memcpy(counters, c, sizeof c);
    return rc;
}

// ---- specific-kmers-3: the three-group join in its `specific` mode; every load is at threshold 0, F_j = the sum of the loaded map's values
// (:103-114: the saturated sums, not the records' sum of loadKmersFreq)
static int specific3_run(mf_ctx *ctx, const mf_join_get &get, int na, int nb, int nc, uint64_t total, double p_chi2, double p_mw, mf_table **grp,
                         uint64_t *counters) {
    const int N = na + nb + nc;
    std::vector<uint64_t> F((size_t)N, 0);
    std::vector<bool> have((size_t)N, false);
    const stats_get_counts get_counts = [&](int j, mf_join_sample &sm, uint64_t *Fj) -> int {
        MF_TRY(get(j, sm));
        if (!have[(size_t)j]) { MF_TRY(mf_sum_counts(ctx, sm.t->d_counts, sm.t->n, &F[(size_t)j])); have[(size_t)j] = true; }
        *Fj = F[(size_t)j];
        return MF_OK;
    };
    const int ng[3] = {na, nb, nc};
    return stats_join(ctx, get, get_counts, ng, 3, total, 0, p_chi2, p_mw, nullptr, grp, counters, true);
}
static int check_specific3(int na, int nb, int nc) {
    if (na < 1 || nb < 1 || nc < 1)
        return mf_set_error("specific-kmers-3: every group needs at least one sample (|A| = %d, |B| = %d, |C| = %d)", na, nb, nc);
    if ((int64_t)na + nb + nc > MF_STATS_MAX_N)
        return mf_set_error("specific-kmers-3: %lld samples, this build supports at most %d (|A| + |B| + |C|)", (long long)na + nb + nc, MF_STATS_MAX_N);
    return MF_OK;
}

extern "C" int mf_specific_kmers3_tables(mf_ctx *ctx, mf_table *const *a, int na, mf_table *const *b, int nb, mf_table *const *c, int nc, double p_chi2,
                                         double p_mw, mf_table **group_a, mf_table **group_b, mf_table **group_c, uint64_t *counters) {
    mf_range rng_("mf:specific_kmers3");
    if (!ctx || !group_a || !group_b || !group_c || !counters || (na && !a) || (nb && !b) || (nc && !c))
        return mf_set_error("mf_specific_kmers3_tables: NULL argument");
    *group_a = *group_b = *group_c = nullptr;
    MF_TRY(check_specific3(na, nb, nc));
    MF_TRY(mf_stats_check_p(p_chi2));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    std::vector<mf_table *> all(a, a + na);
    all.insert(all.end(), b, b + nb);
    all.insert(all.end(), c, c + nc);
    MF_TRY(tables_total(ctx, all.data(), na + nb + nc, "mf_specific_kmers3_tables", &total));
    mf_table *grp[3] = {nullptr, nullptr, nullptr};
    const int rc = specific3_run(ctx, mf_join_tables(all.data()), na, nb, nc, total, p_chi2, p_mw, grp, counters);
    *group_a = grp[0]; *group_b = grp[1]; *group_c = grp[2];
    return rc;
}

extern "C" int mf_specific_kmers3(mf_ctx *ctx, const char *const *a_files, int na, const char *const *b_files, int nb, const char *const *c_files, int nc,
                                  double p_chi2, double p_mw, const char *out_dir, uint64_t *counters) {
    mf_range rng_("mf:specific_kmers3(files)");
    if (!ctx || !out_dir || (na && !a_files) || (nb && !b_files) || (nc && !c_files)) return mf_set_error("mf_specific_kmers3: NULL argument");
    MF_TRY(check_specific3(na, nb, nc));
    MF_TRY(mf_stats_check_p(p_chi2));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t ta = 0, tb = 0, tc = 0;
    MF_TRY(file_records(a_files, na, &ta));
    MF_TRY(file_records(b_files, nb, &tb));
    MF_TRY(file_records(c_files, nc, &tc));
    std::vector<const char *> files(a_files, a_files + na);   // (keys and k as in mf_stats_kmers)
    files.insert(files.end(), b_files, b_files + nb);
    files.insert(files.end(), c_files, c_files + nc);
    mf_table *grp[3] = {nullptr, nullptr, nullptr};
    uint64_t c[MF_SPECIFIC3_COUNTERS] = {0};
    int rc = specific3_run(ctx, mf_join_files(files.data(), 0, 31), na, nb, nc, ta + tb + tc, p_chi2, p_mw, grp, c);
    const std::string d(out_dir);
    uint64_t w = 0;
    static const char *names[3] = {"/filtered_groupA.kmers.bin", "/filtered_groupB.kmers.bin", "/filtered_groupC.kmers.bin"};
    for (int g = 0; g < 3; g++)
        if (rc == MF_OK) rc = mf_table_write_kmers(grp[g], -1, (d + names[g]).c_str(), nullptr, &w);
    for (int g = 0; g < 3; g++) mf_table_destroy(grp[g]);
    if (rc == MF_OK && counters) memcpy(counters, c, sizeof c);
    return rc;
}

// kmers-grouped-counter: keys = the keys of `kmers` in ascending order (a table keeps them partition by partition), words[i] = the presence
// word of keys[i] over the three groups, both on the host
static int grouped_join(mf_ctx *ctx, const mf_join_get &get, const int *ng, uint64_t total, int b, const mf_table *kmers, std::vector<uint64_t> &keys,
                        std::vector<uint32_t> &words) {
    const int N = ng[0] + ng[1] + ng[2];
    const uint64_t n = kmers->n;
    keys.assign(n, 0); words.assign(n, 0);
    if (!n) return MF_OK;                                  // (no key to look up: the groups' files are not streamed at all)
    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(plan_slices(ctx, total, &S, &cap));
    std::vector<uint32_t> add((size_t)N);
    for (int j = 0; j < N; j++) add[(size_t)j] = 1u << (MF_STATS3_BITS * (j < ng[0] ? 0 : j < ng[0] + ng[1] ? 1 : 2));
    mf_buf<uint64_t> sk; MF_TRY(sk.alloc(ctx, n));
    {   // the library's radix sort moves (key, 16-bit value) pairs and has no keys-only form: the table's own counts ride along as the
        // payload and are dropped (2 n bytes of output that nothing reads, next to the 8 n of the keys, in each of its passes)
        mf_buf<uint16_t> unused; MF_TRY(unused.alloc(ctx, n));
        MF_TRY(mf_sort_pairs(ctx, kmers->d_keys, kmers->d_counts, n, 64, sk.p, unused.p));
    }
    mf_buf<uint32_t> dw; MF_TRY(dw.alloc(ctx, n));
    mf_buf<unsigned int> flags; MF_TRY(flags.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(dw.p, 0, n * 4, ctx->stream));
    MF_HIP(hipMemsetAsync(flags.p, 0, 4, ctx->stream));
    for (uint32_t s = 0; s < S; s++) {
        mf_buf<mf_uslot> slots; uint64_t nu = 0;
        MF_TRY(mf_join_union(ctx, get, N, b, MF_UNION_PRESENCE, add.data(), S, s, cap, slots, &nu));
        {
            mf_ktimer tm(ctx, "k_grouped_probe");
            k_grouped_probe<<<grid_for(ctx, n), 256, 0, ctx->stream>>>(slots.p, cap - 1, sk.p, n, S, s, dw.p, flags.p);
        }
        MF_TRY(mf_join_flags(ctx, flags.p, "kmers-grouped-counter"));       // (synchronises: the slice's table goes next)
    }
    MF_HIP(hipMemcpyAsync(keys.data(), sk.p, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipMemcpyAsync(words.data(), dw.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    return MF_OK;
}
int mf_stats_check_grouped(int n_cd, int n_uc, int n_nonibd) {
    if (n_cd < 0 || n_uc < 0 || n_nonibd < 0 || n_cd > 1022 || n_uc > 1022 || n_nonibd > 1022)
        return mf_set_error("kmers-grouped-counter: %d, %d and %d files, at most 1022 in a group", n_cd, n_uc, n_nonibd);
    return MF_OK;
}
static uint64_t grouped_pack(uint32_t w) {
    return (uint64_t)(w & MF_STATS3_MASK) << 32 | (uint64_t)((w >> MF_STATS3_BITS) & MF_STATS3_MASK) << 16 | (uint64_t)((w >> (2 * MF_STATS3_BITS)) & MF_STATS3_MASK);
}

extern "C" int mf_kmers_grouped_count_tables(mf_ctx *ctx, mf_table *kmers, mf_table *const *cd, int n_cd, mf_table *const *uc, int n_uc,
                                             mf_table *const *nonibd, int n_nonibd, int max_bad, uint64_t *keys, uint64_t *counts, uint64_t cap,
                                             uint64_t *n) {
    mf_range rng_("mf:kmers_grouped_counter");
    if (!ctx || !kmers || !n || (cap && (!keys || !counts)) || (n_cd > 0 && !cd) || (n_uc > 0 && !uc) || (n_nonibd > 0 && !nonibd))
        return mf_set_error("mf_kmers_grouped_count_tables: NULL argument");
    MF_TRY(mf_stats_check_grouped(n_cd, n_uc, n_nonibd));
    MF_HIP(hipSetDevice(ctx->device));
    std::vector<mf_table *> all(cd, cd + n_cd);
    all.insert(all.end(), uc, uc + n_uc);
    all.insert(all.end(), nonibd, nonibd + n_nonibd);
    uint64_t total = 0;
    MF_TRY(tables_total(ctx, &kmers, 1, "mf_kmers_grouped_count_tables", nullptr));
    MF_TRY(tables_total(ctx, all.data(), (int)all.size(), "mf_kmers_grouped_count_tables", &total));
    *n = kmers->n;
    if (cap < kmers->n) return MF_OK;                     // (the number alone: the caller comes again with room)
    const int ng[3] = {n_cd, n_uc, n_nonibd};
    std::vector<uint64_t> hk; std::vector<uint32_t> words;
    MF_TRY(grouped_join(ctx, mf_join_tables(all.data()), ng, total, max_bad, kmers, hk, words));
    for (uint64_t i = 0; i < kmers->n; i++) { keys[i] = hk[i]; counts[i] = grouped_pack(words[i]); }
    return MF_OK;
}

extern "C" int mf_kmers_grouped_count(mf_ctx *ctx, const char *const *kmers_files, int n_kmers_files, const char *const *cd_files, int n_cd,
                                      const char *const *uc_files, int n_uc, const char *const *nonibd_files, int n_nonibd, int max_bad, int k,
                                      const char *out_txt, uint64_t *n_kmers) {
    mf_range rng_("mf:kmers_grouped_counter(files)");
    if (!ctx || !out_txt || (n_kmers_files > 0 && !kmers_files) || (n_cd > 0 && !cd_files) || (n_uc > 0 && !uc_files) || (n_nonibd > 0 && !nonibd_files))
        return mf_set_error("mf_kmers_grouped_count: NULL argument");
    if (k < 1 || k > 31) return mf_set_error("k must be in [1,31]");
    MF_TRY(mf_stats_check_grouped(n_cd, n_uc, n_nonibd));
    MF_HIP(hipSetDevice(ctx->device));
    std::vector<const char *> files(cd_files, cd_files + n_cd);
    files.insert(files.end(), uc_files, uc_files + n_uc);
    files.insert(files.end(), nonibd_files, nonibd_files + n_nonibd);
    uint64_t total = 0;
    MF_TRY(file_records(files.data(), (int)files.size(), &total));
    mf_join_sample kf(ctx);                               // IOUtils.loadKmers(kmersFile, 0): a k-mer listed more than once comes once
    MF_TRY(kf.load(kmers_files, std::max(n_kmers_files, 0), 0, k));
    const int ng[3] = {n_cd, n_uc, n_nonibd};
    std::vector<uint64_t> keys; std::vector<uint32_t> words;
    MF_TRY(grouped_join(ctx, mf_join_files(files.data(), max_bad, k), ng, total, max_bad, kf.t, keys, words));
    FILE *f = fopen(out_txt, "w");
    if (!f) return mf_set_error("Couldn't open output file '%s'", out_txt);
    fputs("Kmer\tcd_count\tuc_count\tnonibd_count\n", f);
    char text[32];
    for (size_t i = 0; i < keys.size(); i++) {
        for (int q = 0; q < k; q++) text[q] = "AGCT"[(keys[i] >> (2 * (k - 1 - q))) & 3u];       // ShortKmer.toString
        text[k] = 0;
        const uint32_t w = words[i];
        fprintf(f, "%s\t%u\t%u\t%u\n", text, w & MF_STATS3_MASK, (w >> MF_STATS3_BITS) & MF_STATS3_MASK, (w >> (2 * MF_STATS3_BITS)) & MF_STATS3_MASK);
    }
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) return mf_set_error("can't write '%s'", out_txt);
    if (n_kmers) *n_kmers = keys.size();
    return MF_OK;
}

extern "C" int mf_kmers_samples_count_tables(mf_ctx *ctx, mf_table *const *t, int n, int max_bad, mf_table **out) {
    mf_range rng_("mf:kmers_samples_counter");
    if (!ctx || !out || (n && !t)) return mf_set_error("mf_kmers_samples_count_tables: NULL argument");
    *out = nullptr;
    if (n > 32767) return mf_set_error("kmers-samples-counter: %d input files, at most 32767 (the count is a Java short)", n);
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    MF_TRY(tables_total(ctx, t, n, "mf_kmers_samples_count_tables", &total));
    return nsamples_join(ctx, mf_join_tables(t), n, total, max_bad, out);
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
    mf_table *t = nullptr;
    MF_TRY(nsamples_join(ctx, mf_join_files(files, max_bad, k), n, total, max_bad, &t));
    uint64_t w = 0;
    const int rc = mf_table_write_kmers(t, 0, kmers_bin, stat_txt, &w);
    mf_table_destroy(t);
    if (rc == MF_OK && n_kmers) *n_kmers = w;
    return rc;
}
