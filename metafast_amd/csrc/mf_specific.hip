// mf_specific.hip -- specific-kmers (src/tools/SpecificKmersFinder.java:65-245) on the join core (mf_join.h).  Its
// three-group sibling, specific-kmers-3, is a mode of the three-group join of mf_stats.hip; unique-kmers is in mf_kmersets.hip.
//
// The tool decides on RAW counts, and its "scarce" cut compares the count of the FIRST sample (A's in order, then B's) that holds the
// k-mer with ceil(N * 0.05).  Passes per hash slice:
//   union   as stats-kmers at threshold 0: the presence word holds n1A | n1B << 16.
//   select  total and unique are counted; a k-mer that the chi-squared table keeps, or that every sample holds, gets a row; the others'
//           row word becomes MF_SPEC_REJECTED: whether they count as scarce or as skipped by chi-squared hangs on the first holder's count.
//   gather  the samples again, IN ORDER, one kernel per sample with a synchronise between them: an entry of a row's k-mer fills its cell
//           of the u16 count matrix; the first entry to reach a rejected k-mer is its first holder's -- it swaps the mark for MF_NO_ROW
//           and counts the k-mer as scarce or as skipped.
//   rows    first holder = the first non-zero cell in sample order; scarce rows end there.  Mann-Whitney on the raw counts as integers
//           (2 * U1 over the pairs; a count is exact as a double, so is the comparison), kept unless p > pmw, i.e. 2 * Umin < T with T the
//           smallest 2 * Umin whose p is > pmw; the means are integer sums divided as doubles (sums below 2^53 are exact in any order).
// No floating point but the two divisions of a row's means runs on the device.
#pragma clang fp contract(off)
#include "mf_stats.h"
#include <algorithm>
#include <cmath>

static constexpr uint32_t MF_SPEC_REJECTED = 0xFFFFFFFEu;          // row word: rejected by chi-squared, first holder not yet seen
static constexpr uint64_t MF_SPEC_ROWS_MAX = 0xFFFFFFF0ull;        // row numbers stay below the marks

// counters of mf_specific_kmers* (MF_SPECIFIC_COUNTERS of them), in the order of the reference's log lines
enum { SPEC_TOTAL = 0, SPEC_UNIQUE, SPEC_SCARCE, SPEC_SKIP_CHI2, SPEC_SKIP_MW, SPEC_UNIQUE_LEFT, SPEC_GROUP_A, SPEC_GROUP_B };
static_assert(SPEC_GROUP_B + 1 == MF_SPECIFIC_COUNTERS, "counters of specific-kmers");

// ---------------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------------
// pass 1 over the union (:119-162 without the scarce cut).  (uniform trip count: every lane reaches mf_wave_reserve)
__global__ __launch_bounds__(256) void k_specific_select(mf_uslot *__restrict__ slots, uint64_t cap, const uint8_t *__restrict__ chi_keep, int na, int nb,
                                                         uint64_t *__restrict__ rkeys, unsigned int *__restrict__ cursor,
                                                         unsigned long long *__restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t c_n = 0, c_uniq = 0;
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
                if (n1a == 0 || n1b == 0) c_uniq++;
                keep = n1a + n1b == na + nb || chi_keep[(size_t)n1a * (size_t)(nb + 1) + (size_t)n1b];   // (in all files: kept, :160-162)
                if (!keep) slots[i].row = MF_SPEC_REJECTED;
            }
        }
        const uint32_t r = mf_wave_reserve(cursor, keep ? 1u : 0u);
        if (keep) { slots[i].row = r; rkeys[r] = key; }
    }
    mf_stats_add(&ctr[SPEC_TOTAL], c_n); mf_stats_add(&ctr[SPEC_UNIQUE], c_uniq);
}

// one sample's entries (count > 0): a cell of the count matrix, or -- the first holder of a rejected k-mer -- the scarce / skipped count
__global__ __launch_bounds__(256) void k_specific_gather(mf_uslot *__restrict__ slots, uint64_t mask, const uint64_t *__restrict__ keys,
                                                         const uint16_t *__restrict__ cnts, uint64_t n, uint32_t S, uint32_t s, uint32_t col, uint32_t N,
                                                         uint32_t bound, uint16_t *__restrict__ mat, unsigned long long *__restrict__ ctr) {
    uint32_t c_scarce = 0, c_rej = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint16_t c = cnts[i];
        if (!c) continue;
        const uint64_t key = keys[i];
        const mf_join_key k = mf_join_mine<false>(key, S, s, nullptr);  // (a key >= 2^62 is in no union: skipped, the union pass has said so)
        ulonglong2 raw;
        if (!k.mine) continue;
        const uint64_t p = mf_join_find(slots, mask, k.h, key, &raw);
        if (p == MF_JOIN_NOT_FOUND) continue;
        const uint32_t row = (uint32_t)(raw.y >> 32);
        if (row == MF_SPEC_REJECTED) {
            if (atomicCAS(&slots[p].row, MF_SPEC_REJECTED, MF_NO_ROW) == MF_SPEC_REJECTED) { if (c <= bound) c_scarce++; else c_rej++; }
        } else if (row != MF_NO_ROW) mat[(uint64_t)row * N + col] = c;
    }
    mf_stats_add(&ctr[SPEC_SCARCE], c_scarce); mf_stats_add(&ctr[SPEC_SKIP_CHI2], c_rej);
}

struct mf_spec_row_args {
    const uint16_t *mat; const uint64_t *rkeys; uint64_t m;
    int na, nb;
    uint32_t bound;                                       // scarce: first holder's count <= bound
    int mw; uint32_t T;                                   // mw != 0: keep iff 2 * Umin < T
    uint64_t *ka, *kb; uint16_t *va, *vb;                 // group A / B outputs
    unsigned int *cur;                                    // [0] A, [1] B
    unsigned long long *ctr;
};
// the decision of a row that is not scarce: 0 (A) / 1 (B) / -1 (rejected by the Mann-Whitney test) and the value; u2 = 2 * U1
__device__ __forceinline__ int mf_spec_group(const mf_spec_row_args &a, uint32_t u2, uint32_t sa, uint32_t sb, uint16_t *val) {
    if (a.mw) {
        const uint32_t tot = 2u * (uint32_t)a.na * (uint32_t)a.nb, u2o = tot - u2;
        if (!((u2 < u2o ? u2 : u2o) < a.T)) return -1;
    }
    const double meanA = (double)sa / (double)a.na, meanB = (double)sb / (double)a.nb;
    if (meanA > meanB) { *val = mf_java_short(meanA); return 0; }
    *val = mf_java_short(meanB);                          // (a tie goes to B)
    return 1;
}
__device__ __forceinline__ void mf_spec_flush(unsigned long long *ctr, uint32_t c_sc, uint32_t c_mw, uint32_t c_ul, uint32_t c_a, uint32_t c_b) {
    mf_stats_add(&ctr[SPEC_SCARCE], c_sc); mf_stats_add(&ctr[SPEC_SKIP_MW], c_mw); mf_stats_add(&ctr[SPEC_UNIQUE_LEFT], c_ul);
    mf_stats_add(&ctr[SPEC_GROUP_A], c_a); mf_stats_add(&ctr[SPEC_GROUP_B], c_b);
}

// one thread per row (N <= MF_STATS_THREAD_N): the row's N counts in LDS, sample j of thread t at v[j * 256 + t] -- 2-byte cells, two
// threads to a bank word, 16 KiB a block at N = 32 (a quarter of k_stats_rows_thread's doubles)
__global__ __launch_bounds__(256) void k_specific_rows_thread(mf_spec_row_args a) {
    extern __shared__ uint16_t cs[];
    const int N = a.na + a.nb;
    uint32_t c_sc = 0, c_mw = 0, c_ul = 0, c_a = 0, c_b = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r0 = (uint64_t)blockIdx.x * blockDim.x; r0 < a.m; r0 += stride) {   // uniform trip count (mf_wave_reserve)
        const uint64_t r = r0 + threadIdx.x;
        int grp = -1; uint16_t val = 0;
        if (r < a.m) {
            uint16_t *v = cs + threadIdx.x;
            const uint16_t *row = a.mat + r * (uint64_t)N;
            uint32_t first = 0, sa = 0, sb = 0, n1a = 0, n1b = 0;
            for (int j = 0; j < N; j++) {
                const uint16_t c = row[j];
                v[(size_t)j * 256] = c;
                if (c && !first) first = c;
                if (j < a.na) { sa += c; n1a += c != 0; } else { sb += c; n1b += c != 0; }
            }
            if (first <= a.bound) c_sc++;
            else {
                uint32_t u2 = 0;
                if (a.mw)
                    for (int i = 0; i < a.na; i++) {
                        const uint16_t x = v[(size_t)i * 256];
                        for (int j = a.na; j < N; j++) { const uint16_t y = v[(size_t)j * 256]; u2 += (x > y ? 2u : 0u) + (x == y ? 1u : 0u); }
                    }
                grp = mf_spec_group(a, u2, sa, sb, &val);
                c_mw += grp < 0; c_a += grp == 0; c_b += grp == 1;
                c_ul += grp >= 0 && (n1a == 0 || n1b == 0);
            }
        }
        const uint32_t ia = mf_wave_reserve(&a.cur[0], grp == 0 ? 1u : 0u);
        const uint32_t ib = mf_wave_reserve(&a.cur[1], grp == 1 ? 1u : 0u);
        if (grp == 0) { a.ka[ia] = a.rkeys[r]; a.va[ia] = val; }
        else if (grp == 1) { a.kb[ib] = a.rkeys[r]; a.vb[ib] = val; }
    }
    mf_spec_flush(a.ctr, c_sc, c_mw, c_ul, c_a, c_b);
}

// one wave per row (N > MF_STATS_THREAD_N): the lanes bring the row's counts into LDS (2 KiB a wave, 8 KiB a block) with their sums,
// holders and the first holder's place, then share out the A x B pairs.  `live` and every reduced value are the same in all lanes of a
// wave, so the waves of a block part only between the two barriers.
__global__ __launch_bounds__(256) void k_specific_rows_wave(mf_spec_row_args a) {
    __shared__ uint16_t cs[4][MF_STATS_MAX_N];
    const int N = a.na + a.nb, w = threadIdx.x >> 6, lane = mf_lane();
    uint16_t *v = cs[w];
    uint32_t c_sc = 0, c_mw = 0, c_ul = 0, c_a = 0, c_b = 0;
    for (uint64_t r0 = (uint64_t)blockIdx.x * 4; r0 < a.m; r0 += (uint64_t)gridDim.x * 4) {   // block-uniform trip count
        const uint64_t r = r0 + (uint64_t)w;
        const bool live = r < a.m;
        uint32_t sa = 0, sb = 0, n1 = 0, jf = (uint32_t)N;  // n1: holders A | B << 16; jf: the first holder this lane saw
        if (live) {
            const uint16_t *row = a.mat + r * (uint64_t)N;
            for (int j = lane; j < N; j += 64) {
                const uint16_t c = row[j];
                v[j] = c;
                if (c && jf == (uint32_t)N) jf = (uint32_t)j;
                if (j < a.na) { sa += c; n1 += c != 0; } else { sb += c; n1 += c != 0 ? 1u << 16 : 0u; }
            }
        }
        __syncthreads();
        for (int d = 32; d >= 1; d >>= 1) {
            sa += __shfl_xor(sa, d, 64); sb += __shfl_xor(sb, d, 64); n1 += __shfl_xor(n1, d, 64);
            const uint32_t o = __shfl_xor(jf, d, 64);
            jf = o < jf ? o : jf;
        }
        const bool scarce = live && (jf >= (uint32_t)N || v[jf] <= a.bound);
        uint32_t u2 = 0;
        if (live && !scarce && a.mw) {
            for (int i = 0; i < a.na; i++) {
                const uint16_t x = v[i];
                for (int j = a.na + lane; j < N; j += 64) { const uint16_t y = v[j]; u2 += (x > y ? 2u : 0u) + (x == y ? 1u : 0u); }
            }
            for (int d = 32; d >= 1; d >>= 1) u2 += __shfl_xor(u2, d, 64);
        }
        if (live && lane == 0) {
            if (scarce) c_sc++;
            else {
                uint16_t val = 0;
                const uint64_t key = a.rkeys[r];
                const int grp = mf_spec_group(a, u2, sa, sb, &val);
                c_mw += grp < 0; c_a += grp == 0; c_b += grp == 1;
                c_ul += grp >= 0 && ((n1 & 0xFFFFu) == 0 || (n1 >> 16) == 0);
                if (grp == 0) { const uint32_t i = atomicAdd(&a.cur[0], 1u); a.ka[i] = key; a.va[i] = val; }
                else if (grp == 1) { const uint32_t i = atomicAdd(&a.cur[1], 1u); a.kb[i] = key; a.vb[i] = val; }
            }
        }
        __syncthreads();
    }
    mf_spec_flush(a.ctr, c_sc, c_mw, c_ul, c_a, c_b);
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
// the join of nA + nB samples (A first), every pass at threshold 0; grp_out[2] get the groups' tables, counters MF_SPECIFIC_COUNTERS values
static int specific_join(mf_ctx *ctx, const mf_join_get &get, int na, int nb, uint64_t total, double pchi2, double pmw, mf_table **grp_out,
                         uint64_t *counters) {
    const int N = na + nb;
    const double q = chi2_1_quantile(pchi2);
    std::vector<uint8_t> chi((size_t)(na + 1) * (nb + 1), 0);
    for (int n1a = 0; n1a <= na; n1a++)
        for (int n1b = 0; n1b <= nb; n1b++)
            chi[(size_t)n1a * (nb + 1) + n1b] = chisq_keep((float)(na - n1a), (float)n1a, (float)(nb - n1b), (float)n1b, q) ? 1 : 0;
    const uint32_t bound = (uint32_t)std::ceil(N * 0.05);
    const int mw = pmw > 0 ? 1 : 0;
    const uint32_t T = mw ? mw_threshold(na, nb, pmw, true) : 0u;
    if (ctx->opt_verbose) fprintf(stderr, "[mf] specific: q = %.17g, first holder's count <= %u is scarce, 2*Umin < %u\n", q, bound, T);
    mf_buf<uint8_t> dchi; MF_TRY(dchi.alloc(ctx, chi.size()));
    MF_HIP(hipMemcpyAsync(dchi.p, chi.data(), chi.size(), hipMemcpyHostToDevice, ctx->stream));
    mf_buf<unsigned long long> ctr; MF_TRY(ctr.alloc(ctx, (size_t)MF_SPECIFIC_COUNTERS));
    MF_HIP(hipMemsetAsync(ctr.p, 0, (size_t)MF_SPECIFIC_COUNTERS * 8, ctx->stream));

    uint32_t S = 1; uint64_t cap = 0;
    MF_TRY(plan_slices(ctx, total, &S, &cap));
    std::vector<uint32_t> add((size_t)N);
    for (int j = 0; j < N; j++) add[(size_t)j] = j < na ? 1u : 1u << 16;
    mf_join_parts<uint64_t, uint16_t> p_g[2];
    for (uint32_t s = 0; s < S; s++) {
        mf_buf<mf_uslot> slots; uint64_t nu = 0;
        MF_TRY(mf_join_union(ctx, get, N, 0, MF_UNION_PRESENCE, add.data(), S, s, cap, slots, &nu));
        if (nu > MF_SPEC_ROWS_MAX)
            return mf_set_error("specific-kmers: %llu union k-mers in one slice, at most 2^32 - 16 (raise option stats_slices)", (unsigned long long)nu);
        // select
        mf_buf<uint64_t> rkeys; MF_TRY(rkeys.alloc(ctx, nu));
        unsigned int m32 = 0;
        MF_TRY(mf_join_cursors(ctx, 1, &m32, [&](unsigned int *cur) {
            mf_ktimer tm(ctx, "k_specific_select");
            k_specific_select<<<grid_for(ctx, cap), 256, 0, ctx->stream>>>(slots.p, cap, dchi.p, na, nb, rkeys.p, cur, ctr.p);
        }));
        const uint64_t m = m32;
        if (m > nu) return mf_set_error("specific-kmers: %llu rows of %llu union k-mers", (unsigned long long)m, (unsigned long long)nu);
        // gather: in sample order, each sample's kernel done before the next one's starts (the first holder is the first to come)
        mf_buf<uint16_t> mat; MF_TRY(mat.alloc(ctx, m * (uint64_t)N));
        if (m) MF_HIP(hipMemsetAsync(mat.p, 0, mat.bytes(), ctx->stream));
        for (int j = 0; j < N && nu; j++)
            MF_TRY(mf_join_pass(ctx, get, j, "specific-kmers: gather pass", [&](const mf_table *t) {
                mf_ktimer tm(ctx, "k_specific_gather");
                k_specific_gather<<<grid_for(ctx, t->n), 256, 0, ctx->stream>>>(slots.p, cap - 1, t->d_keys, t->d_counts, t->n, S, s, (uint32_t)j, (uint32_t)N,
                                                                               bound, mat.p, ctr.p);
            }));
        slots.reset();
        // rows
        uint64_t *kg[2] = {nullptr, nullptr}; uint16_t *vg[2] = {nullptr, nullptr};
        for (int g = 0; g < 2; g++) MF_TRY(p_g[g].add(ctx, m, &kg[g], &vg[g]));
        unsigned int cc[2] = {0, 0};
        MF_TRY(mf_join_cursors(ctx, 2, cc, [&](unsigned int *cur) {
            if (!m) return;
            const mf_spec_row_args ra{mat.p, rkeys.p, m, na, nb, bound, mw, T, kg[0], kg[1], vg[0], vg[1], cur, ctr.p};
            if (N <= MF_STATS_THREAD_N) {
                mf_ktimer tm(ctx, "k_specific_rows_thread");
                const unsigned g_thread = (unsigned)std::min<uint64_t>((m + 255) / 256, (uint64_t)ctx->n_cu * 8);
                k_specific_rows_thread<<<g_thread, 256, (size_t)N * 256 * sizeof(uint16_t), ctx->stream>>>(ra);
            } else {
                mf_ktimer tm(ctx, "k_specific_rows_wave");
                const unsigned g_wave = (unsigned)std::min<uint64_t>((m + 3) / 4, (uint64_t)ctx->n_cu * 16);
                k_specific_rows_wave<<<g_wave, 256, 0, ctx->stream>>>(ra);
            }
        }));
        if (cc[0] > m || cc[1] > m) return mf_set_error("specific-kmers: %u + %u survivors of %llu rows", cc[0], cc[1], (unsigned long long)m);
        for (int g = 0; g < 2; g++) p_g[g].wrote(cc[g]);
    }
    unsigned long long hc[MF_SPECIFIC_COUNTERS];
    MF_HIP(hipMemcpyAsync(hc, ctr.p, sizeof hc, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < MF_SPECIFIC_COUNTERS; i++) counters[i] = hc[i];
    for (int g = 0; g < 2; g++) {
        mf_buf<uint64_t> keys; mf_buf<uint16_t> vals; uint64_t n = 0;
        MF_TRY(p_g[g].concat(ctx, keys, vals, &n));
        MF_TRY(pairs_to_table(ctx, keys, vals, n, &grp_out[g]));
    }
    return MF_OK;
}

static int check_groups(int na, int nb) {
    if (na < 1 || nb < 1) return mf_set_error("specific-kmers: both groups need at least one sample (|A| = %d, |B| = %d)", na, nb);
    if ((int64_t)na + nb > MF_STATS_MAX_N)
        return mf_set_error("specific-kmers: %lld samples, this build supports at most %d (|A| + |B|)", (long long)na + nb, MF_STATS_MAX_N);
    return MF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int mf_specific_kmers_tables(mf_ctx *ctx, mf_table *const *a, int na, mf_table *const *b, int nb, double p_chi2, double p_mw,
                                        mf_table **group_a, mf_table **group_b, uint64_t *counters) {
    mf_range rng_("mf:specific_kmers");
    if (!ctx || !group_a || !group_b || !counters || (na && !a) || (nb && !b)) return mf_set_error("mf_specific_kmers_tables: NULL argument");
    *group_a = *group_b = nullptr;
    MF_TRY(check_groups(na, nb));
    MF_TRY(mf_stats_check_p(p_chi2));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t total = 0;
    std::vector<mf_table *> all(a, a + na);
    all.insert(all.end(), b, b + nb);
    MF_TRY(tables_total(ctx, all.data(), na + nb, "mf_specific_kmers_tables", &total));
    mf_table *grp[2] = {nullptr, nullptr};
    const int rc = specific_join(ctx, mf_join_tables(all.data()), na, nb, total, p_chi2, p_mw, grp, counters);
    if (rc != MF_OK) { mf_table_destroy(grp[0]); mf_table_destroy(grp[1]); return rc; }
    *group_a = grp[0]; *group_b = grp[1];
    return MF_OK;
}

extern "C" int mf_specific_kmers(mf_ctx *ctx, const char *const *a_files, int na, const char *const *b_files, int nb, double p_chi2, double p_mw,
                                 const char *out_dir, uint64_t *counters) {
    mf_range rng_("mf:specific_kmers(files)");
    if (!ctx || !out_dir || (na && !a_files) || (nb && !b_files)) return mf_set_error("mf_specific_kmers: NULL argument");
    MF_TRY(check_groups(na, nb));
    MF_TRY(mf_stats_check_p(p_chi2));
    MF_HIP(hipSetDevice(ctx->device));
    uint64_t ta = 0, tb = 0;
    MF_TRY(file_records(a_files, na, &ta));
    MF_TRY(file_records(b_files, nb, &tb));
    std::vector<const char *> files(a_files, a_files + na);   // (keys and k as in mf_stats_kmers)
    files.insert(files.end(), b_files, b_files + nb);
    mf_table *grp[2] = {nullptr, nullptr};
    uint64_t c[MF_SPECIFIC_COUNTERS] = {0};
    int rc = specific_join(ctx, mf_join_files(files.data(), 0, 31), na, nb, ta + tb, p_chi2, p_mw, grp, c);
    const std::string d(out_dir);
    uint64_t w = 0;
    // (values are Java shorts: every record is written)
    if (rc == MF_OK) rc = mf_table_write_kmers(grp[0], -1, (d + "/filtered_groupA.kmers.bin").c_str(), nullptr, &w);
    if (rc == MF_OK) rc = mf_table_write_kmers(grp[1], -1, (d + "/filtered_groupB.kmers.bin").c_str(), nullptr, &w);
    mf_table_destroy(grp[0]); mf_table_destroy(grp[1]);
    if (rc == MF_OK && counters) memcpy(counters, c, sizeof c);
    return rc;
}
