// mf_stats.h -- what the group-comparison tools share beside the join core: the limits of a row, the wave counter, Java's cast, and the
// host's decision tables (defined in mf_stats.hip; used there and by mf_specific.hip).
#pragma once
#include "mf_join.h"

#define MF_STATS_MAX_N 1024          // samples of one stats-kmers run (the row kernels keep a row's values in LDS)
#define MF_STATS_THREAD_N 32         // up to this many samples: one thread per row (values in LDS, 64 KiB per 256 rows), else a wave per row

// wave sum of a per-lane counter into a 64-bit global counter
__device__ __forceinline__ void mf_stats_add(unsigned long long *ctr, uint32_t x) {
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d, 64);
    if (mf_lane() == 0 && x) atomicAdd(ctr, (unsigned long long)x);
}
// Java's (short)(int)x: NaN -> 0, saturation to int, low 16 bits (JLS 5.1.3)
__device__ __forceinline__ uint16_t mf_java_short(double x) {
    int32_t i;
    if (x != x) i = 0;
    else if (x >= 2147483647.0) i = 2147483647;
    else if (x <= -2147483648.0) i = (-2147483647 - 1);
    else i = (int32_t)x;                                  // (in range: truncation toward zero)
    return (uint16_t)(uint32_t)i;
}

// the two-group chi-squared decision (StatsKmersFinder.chisq = SpecificKmersFinder.chisq) and the quantile with 1 degree of freedom
bool chisq_keep(float c0, float c1, float p0, float p1, double value);
double chi2_1_quantile(double p_chi2);
// the smallest 2 * Umin in [0, nA nB] whose p is not < pmw (or_equal: whose p is > pmw); nA nB + 1: every row passes
uint32_t mw_threshold(int na, int nb, double pmw, bool or_equal = false);
int mf_stats_check_p(double pchi2);
// 1 <= |A|, 1 <= |B|, |A| + |B| <= MF_STATS_MAX_N
int mf_stats_check_groups(int na, int nb);

// a launch of the two-group row kernels (k_stats_rows_thread / k_stats_rows_wave, mf_stats.hip: compiled there, without contraction)
struct mf_stats_row_args {
    const uint16_t *mat; const uint64_t *rkeys; uint64_t m;
    int na, nb;
    const double *F; double M;
    int mw; uint32_t T;                                  // mw != 0: keep iff 2 * Umin < T
    uint64_t *ka, *kb; uint16_t *va, *vb;                 // group A / B outputs: a kept row's rkeys word and its value
    unsigned int *cur;                                    // [0] A, [1] B
    unsigned long long *ctr;                              // [5] MW rejected, [6] |A|, [7] |B|, [8] unique left
};
void mf_stats_rows_launch(mf_ctx *ctx, const mf_stats_row_args &ra);

// ---- three groups (stats-kmers-3, kmers-grouped-counter, specific-kmers-3) ----
// the three per-group sample counts of a presence word: 10 bits each (at most 1022 samples in a group)
#define MF_STATS3_BITS 10
#define MF_STATS3_MASK 0x3FFu
// the three-group chi-squared decision (StatsKmers3GroupsFinder.chisq; c = A, p = B, q = C) and the quantile with 2 degrees of freedom
bool chisq3_keep(float c0, float c1, float p0, float p1, float q0, float q1, double value);
double chi2_2_quantile(double p_chi2);
// 1 <= |A|, |B|, |C|, |A| + |B| + |C| <= MF_STATS_MAX_N
int mf_stats_check_groups3(int na, int nb, int nc);
// kmers-grouped-counter: 0 ... 1022 samples in each group
int mf_stats_check_grouped(int n_cd, int n_uc, int n_nonibd);
// a launch of the three-group row kernels (k_stats3_rows_thread / k_stats3_rows_wave, or specific-kmers-3's k_specific3_rows_*; mf_stats.hip)
struct mf_stats3_row_args {
    const uint16_t *mat; const uint64_t *rkeys; uint64_t m;
    int na, nb, nc;
    const double *F; double M;
    int mw; uint32_t Tab, Tbc, Tac;                       // mw != 0: keep iff 2 * Umin < T for (A, B), (B, C) or (A, C)
    uint64_t *ka, *kb, *kc; uint16_t *va, *vb, *vc;       // group A / B / C outputs
    unsigned int *cur;                                    // [0] A, [1] B, [2] C
    unsigned long long *ctr;                              // [5] MW rejected, [6] |A|, [7] |B|, [8] |C|, [9] unique left
};
void mf_stats3_rows_launch(mf_ctx *ctx, const mf_stats3_row_args &ra, bool specific = false);
