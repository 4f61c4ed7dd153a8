// mf_skm.hip -- k-mer counting through SUPER-K-MERS (minimizer partitions), the default path for k >= MF_SKM_MIN_K.
//
// Same job as mf_count.hip (IOUtils.loadReads, src/io/IOUtils.java:756-768: every k-mer of every read ->
// BigLong2ShortHashMap.addAndBound(canonical, 1)), same result (dense (key,count) arrays), different traffic: the
// one-record-per-k-mer path moves 8 bytes per k-mer OCCURRENCE through two radix passes and the count pass (3 x 96 GB
// at 1.2e10 occurrences).  Here a read is cut into runs of consecutive k-mers that share their minimizer (mf_common.h),
// and a run of r k-mers travels as ONE 16-byte record holding its r+k-1 bases (about 7 k-mers per record at k=31):
//
//   S1 k_skm_hist     ASCII -> 2-bit -> M-mer hashes -> sliding-window minimum -> runs; per-block histogram of the
//                     records' level-1 digit (top bits of the partition hash of the run's minimizer).  On large inputs it
//                     runs over every 16th tile only and just SIZES the digit regions
//      k_scan         region starts / exact output ranges (padded to whole 64-byte lines)
//   S2 k_skm_scatter  the minimizer scan (again, where S1 ran over everything), records built and radix-partitioned through
//                     64-byte LDS staging lines; one-pass form: regions reserved chunk by chunk during the scatter
//      skm_pilot      (reads) a few hundred would-be units of level 1 are copied out and counted: distinct k-mers per occurrence
//                     and the share that survives the cut decide the bits of the following levels and the table partitions per
//                     unit -- the plan assumes no sequencing depth
//   S3 k_skm_split    further levels: the digit is read from the record (22 digit bits travel with it)
//   S4 k_skm_count    one counting unit per 512-thread workgroup at a time, units claimed from a counter three ahead: identical
//                     records are told apart first (a pass of the records through the empty table: the k-mers of a record that
//                     occurs n times are inserted once, with weight n); every wave deals the surviving records out as items of
//                     <= 2 k-mers -> open-addressed count table in LDS -> compacted (key,count) slices; a batch of units at a time
//      k_gather       slices of the batch -> dense arrays, every unit cut into 2^s table partitions by the next bits of the
//                     partition hash (the HBM index is built partition by partition, mf_table.hip)
//
// A partition holds ALL occurrences of its k-mers, so the counts are exact; only the grouping of the dense table
// differs from mf_count.hip (by minimizer partition instead of by hash partition).  If a partition has more distinct
// k-mers than the LDS table holds, the caller falls back to mf_count.hip's path.
//
// One translation unit, stage by stage in headers (included below in this order):
//   mf_skm_scan.h     the record, and the minimizer scan S1 and S2 share
//   mf_skm_scatter.h  S1 k_skm_hist, S2 k_skm_scatter with its staging lines and run list, the directory kernels of level 1
//   mf_skm_split.h    S3 k_skm_split
//   mf_skm_count.h    S4 k_skm_count, k_gather_split / k_gather_split_n
//   mf_skm.hip        the host: the pilot, a slice step by step (skm_slice), a run (skm_run), the streamed level 1, the entry points, the debug snapshot
#include "mf_common.h"
#include "mf_count_dev.h"
#include <algorithm>
#include <memory>
#include <vector>
#include "mf_skm_scan.h"
#include "mf_skm_scatter.h"
#include "mf_skm_split.h"
#include "mf_skm_count.h"

// =============================================================================================
// host orchestration
// =============================================================================================
template <typename KF> static int skm_set_lds(KF kern, size_t bytes) {
    MF_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return MF_OK;
}

// =============================================================================================
// The PILOT (round 4): distinct k-mers per occurrence, measured before the levels after the first are planned.
// What a counting unit costs is decided by its DISTINCT k-mers (the LDS table takes C2_FILL claims; a unit beyond that is
// counted again in 4, 16, 64 passes), and a plan made from the number of occurrences alone has one sequencing depth in mind: with
// the benchmark's 7.4 occurrences per distinct k-mer built in, the same 100 M reads drawn from a pool sixteen times as large
// (5-fold instead of 83-fold depth, 3.4 occurrences per distinct k-mer) had every second unit counted in four passes -- 362 ms
// instead of 32.  The reference's map does not care: it doubles when it is full (Long2ShortHashMap.java:191-214).
// Once level 1 stands, the records of a few of its digit regions whose NEXT digits are among the smallest `nsel` values -- that
// is: a few hundred would-be units an eighth of the planned size, each with ALL the occurrences of its k-mers -- are copied out
// (two small passes over <= 8 regions: histogram, scatter) and counted with the counting kernel itself; nothing is kept but the
// number of distinct k-mers.  ~2 M occurrences, five small launches and one round trip to the host (0.2 ms at 100 M reads).
// =============================================================================================
#define SKM_PILOT_CH 8192          // records of a region per workgroup
__global__ __launch_bounds__(256) void k_skm_pilot(const skm_rec *__restrict__ recs, const uint64_t *__restrict__ pstart, const uint32_t *__restrict__ plen,
                                                   const uint32_t *__restrict__ regions, int shift, uint32_t nsel, uint32_t *__restrict__ cnt,
                                                   uint32_t *__restrict__ occ, const uint64_t *__restrict__ ostart, uint32_t *__restrict__ cur,
                                                   skm_rec *__restrict__ out) {
    // ostart == nullptr: histogram pass (cnt / occ [region][digit]: records, k-mers); else: the records go to out[ostart[bin] + ...]
    extern __shared__ uint32_t sh[];                                    // [2 * nsel] (histogram pass)
    const uint32_t rg = blockIdx.y, d1 = regions[rg];
    const uint64_t start = pstart[d1];
    const uint32_t len = plen[d1];
    const uint32_t j0 = blockIdx.x * (uint32_t)SKM_PILOT_CH;
    if (j0 >= len) return;
    const uint32_t j1 = min(len, j0 + (uint32_t)SKM_PILOT_CH);
    const bool hist = ostart == nullptr;
    if (hist) { for (uint32_t i = threadIdx.x; i < 2u * nsel; i += blockDim.x) sh[i] = 0; __syncthreads(); }
    for (uint32_t j = j0 + threadIdx.x; j < j1; j += blockDim.x) {
        const skm_rec v = recs[start + j];
        if (!skm_rec_valid(v)) continue;
        const uint32_t d = skm_rec_digits(v) >> shift;
        if (d >= nsel) continue;
        if (hist) { atomicAdd(&sh[d], 1u); atomicAdd(&sh[nsel + d], skm_rec_n(v)); }
        else { const uint32_t at = atomicAdd(&cur[rg * nsel + d], 1u); out[ostart[rg * nsel + d] + at] = v; }
    }
    if (hist) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nsel; i += blockDim.x) {
            if (sh[i]) { atomicAdd(&cnt[rg * nsel + i], sh[i]); atomicAdd(&occ[rg * nsel + i], sh[nsel + i]); }
        }
    }
}
__global__ void k_skm_pilot_dir(const uint32_t *__restrict__ cnt, uint32_t n, uint32_t *__restrict__ plen) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) plen[i] = (cnt[i] + 3u) & ~3u;
}
// -> *rho = distinct k-mers per occurrence among the sampled units (< 0: nothing sampled); bufA / pstart / plen: level 1 (indexed by digit)
template <int K>
static int skm_pilot(mf_ctx *ctx, const skm_rec *bufA, const uint64_t *pstart, const uint32_t *plen, uint32_t dlo, uint32_t dhi, uint64_t n_occ, int nd1,
                     int bits_planned, int kthr, double *rho, double *kept, double *rec_per_occ) {
    hipStream_t st = ctx->stream;
    *rho = -1.0; *kept = -1.0; *rec_per_occ = 0.0;
    if (dhi <= dlo) return MF_OK;
    const uint32_t R = std::min<uint32_t>(8u, dhi - dlo);
    const int pb = std::min((int)SKM_DIGIT_BITS, bits_planned + 3);                       // would-be units an eighth of the planned size
    const double per_unit = (double)n_occ / (double)nd1 / (double)(1u << pb);            // occurrences of one of them
    uint32_t nsel = (uint32_t)std::min<double>((double)(1u << pb), std::max(1.0, std::ceil(2.5e6 / (per_unit * R))));
    if (nsel > 2048u) nsel = 2048u;
    const uint32_t nb = R * nsel;
    std::vector<uint32_t> h_reg(R);
    for (uint32_t i = 0; i < R; i++) h_reg[i] = dlo + (uint32_t)(((uint64_t)(2 * i + 1) * (dhi - dlo)) / (2 * R));      // spread over the slice's digits
    std::vector<uint32_t> h_len(nd1);
    mf_buf<uint32_t> reg, cnt, occ, cur, uplen, dcount; mf_buf<uint64_t> ostart, toff; mf_buf<unsigned long long> ps;
    MF_TRY(reg.alloc(ctx, R)); MF_TRY(cnt.alloc(ctx, (size_t)3 * nb)); MF_TRY(uplen.alloc(ctx, nb)); MF_TRY(dcount.alloc(ctx, nb));
    MF_TRY(ostart.alloc(ctx, (size_t)nb + 1)); MF_TRY(toff.alloc(ctx, (size_t)nb + 1)); MF_TRY(ps.alloc(ctx, 24));
    uint32_t *const d_cnt = cnt.p, *const d_occ = cnt.p + nb, *const d_cur = cnt.p + 2 * (size_t)nb;
    MF_HIP(hipMemcpyAsync(reg.p, h_reg.data(), (size_t)R * 4, hipMemcpyHostToDevice, st));
    MF_HIP(hipMemsetAsync(cnt.p, 0, (size_t)3 * nb * 4, st));
    MF_HIP(hipMemsetAsync(ps.p, 0, 24 * 8, st));
    // (a region's length is not known on the host: the grid covers the longest a region can be, 4 x the mean)
    const uint64_t mean_len = std::max<uint64_t>(1, n_occ / (uint64_t)nd1 / 4);          // (records >= occurrences / 20; 4 is generous)
    const unsigned gx = (unsigned)std::min<uint64_t>(65535, (4 * mean_len + SKM_PILOT_CH - 1) / SKM_PILOT_CH + 1);
    const int shift = SKM_DIGIT_BITS - pb;
    mf_ktimer tm(ctx, "k_skm_pilot");
    k_skm_pilot<<<dim3(gx, R), 256, (size_t)2 * nsel * 4, st>>>(bufA, pstart, plen, reg.p, shift, nsel, d_cnt, d_occ, nullptr, nullptr, nullptr);
    k_skm_pilot_dir<<<(nb + 255) / 256, 256, 0, st>>>(d_cnt, nb, uplen.p);
    MF_TRY(mf_scan<1>(ctx, uplen.p, ostart.p, nb, (uint64_t *)&ps.p[0]));
    MF_TRY(mf_scan<1>(ctx, d_occ, toff.p, nb, (uint64_t *)&ps.p[1]));
    unsigned long long tot[2] = {0, 0};
    MF_HIP(hipMemcpyAsync(tot, ps.p, 16, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    if (!tot[0] || !tot[1]) return MF_OK;
    mf_buf<skm_rec> pr; mf_buf<uint64_t> tkeys; mf_buf<uint16_t> tcnt;
    if (pr.alloc(ctx, tot[0] + 4) != MF_OK || tkeys.alloc(ctx, tot[1]) != MF_OK || tcnt.alloc(ctx, tot[1]) != MF_OK) return MF_OK;      // (no room: no pilot)
    MF_HIP(hipMemsetAsync(pr.p, 0xFF, (tot[0] + 4) * sizeof(skm_rec), st));               // padding = sentinels
    k_skm_pilot<<<dim3(gx, R), 256, 0, st>>>(bufA, pstart, plen, reg.p, shift, nsel, nullptr, nullptr, ostart.p, d_cur, pr.p);
    {
        const unsigned grid = (unsigned)std::min<uint64_t>(nb, (uint64_t)ctx->n_cu * C2_WG_PER_CU);
        // ps: [2] overflow [3] distinct before the cut [4] units redone [8..24) diagnostics
        k_skm_count<K><<<grid, SKM_CT, C2_LDS, st>>>(pr.p, ostart.p, uplen.p, nb, toff.p, tkeys.p, tcnt.p, dcount.p, (unsigned int *)&ps.p[2], 0u, (uint64_t)0, kthr,
                                                         &ps.p[3], (unsigned int *)&ps.p[4], nullptr, &ps.p[8], (uint64_t)tot[1], (uint32_t)ctx->opt_skm_dedupe, nullptr);
    }
    MF_TRY(mf_scan<1>(ctx, dcount.p, ostart.p, nb, (uint64_t *)&ps.p[5]));                // [5] k-mers that survive the cut
    unsigned long long res[4] = {0, 0, 0, 0};
    MF_HIP(hipMemcpyAsync(res, &ps.p[2], 32, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    MF_HIP(hipGetLastError());
    const bool over = (res[0] & 0xFFFFFFFFull) != 0;
    *rho = over ? 1.0 : (double)res[1] / (double)tot[1];              // (a unit beyond 64 passes at an eighth of the size: plan as fine as it gets)
    if (!over) *kept = (double)res[3] / (double)tot[1];
    *rec_per_occ = (double)tot[0] / (double)tot[1];                    // (padded to fours per would-be unit: a few per cent high)
    if (ctx->opt_verbose)
        fprintf(stderr, "[mf] skm pilot: %u would-be units of %u regions (2^%d per region): %llu records, %llu occurrences, %llu distinct k-mers = %.4f per occurrence (%llu kept), %llu unit(s) redone\n",
                nb, R, pb, tot[0], tot[1], res[1], *rho, res[3], res[2] & 0xFFFFFFFFull);
    return MF_OK;
}

// =============================================================================================
// a run, its slices, and what they hand to each other
// =============================================================================================
// What mf_debug_skm_records (the end of this file) takes out of a run: the state of every slice at the point where count + gather would begin
struct skm_snap_slice {
    std::vector<uint64_t> rec;             // the record buffer over [0, cap): x, y of record 0, x, y of record 1, ...
    std::vector<uint64_t> pstart, l1_pstart; std::vector<uint32_t> plen, pocc, l1_plen;      // the final directory; the slice's level-1 directory
    std::vector<int> lv;                   // the levels' bits as they were run (after the pilot)
    uint64_t cap = 0, wpb = 0, n_valid = 0; uint32_t dlo = 0, dhi = 0; int G = 0, one_pass = 0, repeated = 0, fast = 0;
};
struct mf_skm_snap { std::vector<skm_snap_slice> slices; };
#define MF_SKM_SNAPPED 3           /* skm_run: the records went to ctx->skm_snap, nothing was counted */
// what the slices of one run add up to: the dense table (grouped by partition, slice after slice = partition order), the
// partition offsets, the tallies
struct skm_acc {
    mf_skm_snap *snap = nullptr;           // (null in production)
    mf_buf<uint64_t> dk; mf_buf<uint16_t> dc; uint64_t dused = 0, dcap = 0;
    mf_buf<uint64_t> doff;                 // [np_total + 1]: the TABLE's partitions (two per counting partition, k_gather_split)
    mf_buf<unsigned long long> dhist, c2p;
    unsigned long long n_records = 0, cap_l1 = 0;
    uint32_t np_total = 0;
    int split_bits = 1;                    // table partitions per counting partition = 2^split_bits (k_gather_split / k_gather_split_n)
    int table_bits = 0;                    // the caller's wish for the table (0: one bit more than the counting plan)
};
#define MF_SKM_NOMEM 2             /* skm_slice: a record buffer did not fit -- the caller tries again with more slices */
// Level 1 of a run that is counted in slices, done ONCE for all the run's digits (round 3): round 2's slices each scanned the reads
// again for their own digits because two sliced record buffers were budgeted -- at 380 M reads k_skm_scatter was 412 ms of a
// 970 ms sample.  One full level-1 buffer + one slice-sized buffer for the following levels fit as well (57 GB of reads +
// 87 GB + 87 / S GB), and the reads are scanned once; the slices then differ only in which level-1 partitions they split and count.
struct skm_shared {
    uint32_t lo = 0, hi = 0;           // the run's level-1 digits
    bool ready = false;
    mf_buf<skm_rec> buf; mf_buf<uint64_t> pstart; mf_buf<uint32_t> plen, pocc;
    std::vector<uint64_t> h_pstart;    // (host copy: where the digit regions start, for the slices' buffer sizes)
    unsigned long long cap = 0;
    void clear() { buf.reset(); pstart.reset(); plen.reset(); pocc.reset(); h_pstart.clear(); ready = false; cap = 0; }
};
// the reads of a run, as every scan of them is given them
struct skm_reads { const uint8_t *bases; uint64_t n_bases; const uint32_t *vmask; uint64_t n_words; };
// what a run gives every one of its slices
struct skm_job { skm_reads in; uint64_t n_occ; unsigned long long *scal; int kthr; };
// the launch form of level 1: what k_skm_hist and k_skm_scatter are both given ([lo, hi): the level-1 digits the launch keeps)
struct skm_l1 { skm_reads in; uint64_t wpb; int bits1, G; uint32_t lo, hi; size_t fast_lds; };
// what a slice carries from step to step (skm_slice)
struct skm_slice_state {
    std::vector<int> &lv; int total_bits;                 // the levels' bits and their sum: the pilot may change lv[1..], once
    uint32_t dlo, dhi;                                    // the slice's level-1 digits
    skm_l1 l1;
    uint32_t np; mf_buf<uint64_t> pstart; mf_buf<uint32_t> plen, pocc;      // the directory of the level that stands
    mf_buf<skm_rec> bufA; unsigned long long cap = 0;     // ... and its records
    uint64_t rebase = 0;                                  // where the slice's records start in a shared level-1 buffer
    int snap_one_pass = 0, snap_repeated = 0;             // (what A.snap reports: level 1 in the one-pass form / again with exact ranges after an overflow)
};
// a step of a slice or of a run: anything but MF_OK (an error, MF_SKM_NOMEM, MF_SKM_FALLBACK) ends the caller with it
#define SKM_STEP(call) do { const int rc__ = (call); if (rc__ != MF_OK) return rc__; } while (0)

// the scatter's run redistribution needs LDS behind the staging lines: levels of up to 10 bits (option scatter_fast = 0: never)
static size_t skm_fast_lds(const mf_ctx *ctx, int nd1) {
    const size_t fast_lds = ((skm_stage_bytes(nd1) + 15) & ~(size_t)15) + (size_t)16 * SKM_FAST_WAVE_BYTES;
    return fast_lds > (size_t)160 * 1024 || ctx->opt_scatter_fast == 0 ? 0 : fast_lds;
}
// S2, one launch: with exact ranges (blockstart) or in the one-pass form (DYN: Dy), the FAST form where its LDS fits
template <int K, bool DYN>
static int skm_scatter(mf_ctx *ctx, const skm_l1 &L, const uint64_t *blockstart, skm_rec *out, const skm_dyn &Dy) {
    hipStream_t st = ctx->stream;
    mf_ktimer t(ctx, "k_skm_scatter");
    if (L.fast_lds) {
        MF_TRY(skm_set_lds(k_skm_scatter<K, DYN, true>, L.fast_lds));
        k_skm_scatter<K, DYN, true><<<L.G, 1024, L.fast_lds, st>>>(L.in.bases, L.in.n_bases, L.in.vmask, L.in.n_words, L.wpb, L.bits1, blockstart, L.G, out, Dy, L.lo, L.hi);
    } else {
        const size_t lds = skm_stage_bytes(1 << L.bits1);
        MF_TRY(skm_set_lds(k_skm_scatter<K, DYN, false>, lds));
        k_skm_scatter<K, DYN, false><<<L.G, 1024, lds, st>>>(L.in.bases, L.in.n_bases, L.in.vmask, L.in.n_words, L.wpb, L.bits1, blockstart, L.G, out, Dy, L.lo, L.hi);
    }
    return MF_OK;
}
// Three or more levels ping-pong between record buffers: all of them get the size of the LAST level's (every level
// adds padding), so the third level re-uses the first level's buffer instead of asking for a third one that is a few
// megabytes too large for it (at 200 M reads, k = 21 a buffer is 125 GB: there is no room for three, and a second
// sample would find the arena's idle regions just too small again).
static unsigned long long skm_final_cap(const std::vector<int> &lv, uint64_t n_occ, unsigned long long c1, bool headroom) {
    const int nd1 = 1 << lv[0];
    // (plan still open: room for the padding of whatever the pilot decides -- at most 2 x n_occ / 1100 partitions of 4 records each)
    if (headroom) return c1 + n_occ / 128 + (unsigned long long)nd1 * SKM_LINE * (1ull << MF_MAX_DIGIT_BITS);
    if (lv.size() < 3) return c1;
    unsigned long long c = c1, p = (unsigned long long)nd1;
    for (size_t li = 1; li < lv.size(); li++) { c += p * SKM_LINE * (1ull << lv[li]); p <<= lv[li]; }
    return c;
}

// ---- level 1 (S1, S2): histogram, region sizes, the record buffer, scatter, directory.  own: the buffer is this slice's alone and
// has to do for the following levels too (skm_final_cap; headroom: their plan is still open); else it is the run's shared level 1.
// Level 1 in ONE pass over the reads where it pays (large inputs, a split level follows): the digit regions are sized
// from a histogram of a sixteenth of the input and handed out chunk-wise during the scatter, instead of a full
// minimizer pass just to count (k_skm_hist over everything costs 17 ms of 300 at 100 M reads).  If a region turns out
// too small the level is repeated with exact ranges.  skm_dyn: 0 never, 1 auto, 2 always (tests).
template <int K>
static int skm_level1(mf_ctx *ctx, const skm_job &J, skm_slice_state &T, bool own, bool headroom) {
    hipStream_t st = ctx->stream;
    unsigned long long *const scal = J.scal;
    const skm_l1 &L = T.l1;
    const int bits1 = L.bits1, nd1 = 1 << bits1, G = L.G;
    const uint32_t np = T.np;
    const bool l1_only = T.lv.size() == 1;
    auto final_cap = [&](unsigned long long c1) { return skm_final_cap(T.lv, J.n_occ, c1, headroom); };
    unsigned long long &cap = T.cap;
    bool dyn = !l1_only && (ctx->opt_skm_dyn == 2 || (ctx->opt_skm_dyn == 1 && L.in.n_words >= (1ull << 24)));
    for (int attempt = dyn ? 0 : 1; attempt < 2; attempt++) {
        const bool D = attempt == 0;
        const int stride = D ? (ctx->opt_skm_dyn == 2 ? 3 : 16) : 1;
        mf_buf<uint32_t> blockhist; MF_TRY(blockhist.alloc(ctx, (size_t)nd1 * G));
        mf_buf<uint32_t> blockocc; if (l1_only) MF_TRY(blockocc.alloc(ctx, (size_t)nd1 * G));
        {
            mf_ktimer t(ctx, D ? "k_skm_hist_sample" : "k_skm_hist");
            k_skm_hist<K><<<G, 1024, (size_t)nd1 * 8, st>>>(L.in.bases, L.in.n_bases, L.in.vmask, L.in.n_words, L.wpb, bits1, blockhist.p, blockocc.p, G, stride, L.lo, L.hi);
        }
        MF_DBG(ctx, "k_skm_hist");
        if (D) {
            mf_buf<uint32_t> rsize; MF_TRY(rsize.alloc(ctx, np));
            mf_buf<uint64_t> rstart; MF_TRY(rstart.alloc(ctx, (size_t)np + 1));
            mf_buf<unsigned long long> gcur; MF_TRY(gcur.alloc(ctx, np));
            k_skm_region_sizes<<<(nd1 + 255) / 256, 256, 0, st>>>(blockhist.p, G, nd1, (uint32_t)stride, rsize.p, L.lo, L.hi);
            MF_TRY(mf_scan<1>(ctx, rsize.p, rstart.p, np, (uint64_t *)&scal[1]));
            MF_HIP(hipMemcpyAsync(gcur.p, rstart.p, (size_t)np * 8, hipMemcpyDeviceToDevice, st));
            MF_HIP(hipMemsetAsync(&scal[5], 0, 8, st));
            MF_HIP(hipMemcpyAsync(&cap, &scal[1], 8, hipMemcpyDeviceToHost, st));
            MF_HIP(hipStreamSynchronize(st));
            if (T.bufA.alloc(ctx, std::max<unsigned long long>(cap + (uint64_t)G * SKM_CH, own ? final_cap(cap) : 0ull)) != MF_OK) return MF_SKM_NOMEM;
            skm_dyn Dy; Dy.gcur = gcur.p; Dy.rend = rstart.p + 1; Dy.overflow = (unsigned int *)&scal[5]; Dy.dump = cap; Dy.save = nullptr;
            MF_TRY((skm_scatter<K, true>(ctx, L, nullptr, T.bufA.p, Dy)));
            MF_DBG(ctx, "k_skm_scatter");
            k_skm_dir_dyn<<<(nd1 + 255) / 256, 256, 0, st>>>(rstart.p, gcur.p, nd1, T.pstart.p, T.plen.p);
            unsigned long long ovf = 0;
            MF_HIP(hipMemcpyAsync(&ovf, &scal[5], 8, hipMemcpyDeviceToHost, st));
            MF_HIP(hipStreamSynchronize(st));
            if (!ovf) { T.snap_one_pass = 1; break; }
            T.snap_repeated = 1;
            if (ctx->opt_verbose) fprintf(stderr, "[mf] skm: a sampled digit region was too small, level 1 again with exact ranges\n");
            T.bufA.reset();
            continue;
        }
        mf_buf<uint64_t> blockstart; MF_TRY(blockstart.alloc(ctx, (size_t)nd1 * G + 1));
        MF_TRY(mf_scan<SKM_LINE>(ctx, blockhist.p, blockstart.p, (uint64_t)nd1 * G, (uint64_t *)&scal[1]));
        MF_HIP(hipMemcpyAsync(&cap, &scal[1], 8, hipMemcpyDeviceToHost, st));
        MF_HIP(hipStreamSynchronize(st));                       // padded number of records
        if (T.bufA.alloc(ctx, own ? final_cap(cap) : cap) != MF_OK) return MF_SKM_NOMEM;
        MF_TRY((skm_scatter<K, false>(ctx, L, blockstart.p, T.bufA.p, skm_dyn())));
        MF_DBG(ctx, "k_skm_scatter");
        k_skm_dir<<<(nd1 + 255) / 256, 256, 0, st>>>(blockstart.p, blockocc.p, G, nd1, T.pstart.p, T.plen.p, T.pocc.p);
    }
    return MF_OK;
}

// ---- a level 1 for all the run's slices: the first slice publishes the one it has made, every slice takes its view of it
template <int K>
static int skm_share_level1(mf_ctx *ctx, skm_slice_state &T, skm_shared *SH, uint64_t n_occ) {
    hipStream_t st = ctx->stream;
    const int nd1 = 1 << T.l1.bits1;
    if (!SH->ready) {
        // the first slice has made level 1 for all of them
        SH->buf.swap(T.bufA); SH->pstart.swap(T.pstart); SH->plen.swap(T.plen); SH->pocc.swap(T.pocc);
        SH->cap = T.cap;
        SH->h_pstart.resize(nd1);
        MF_HIP(hipMemcpyAsync(SH->h_pstart.data(), SH->pstart.p, (size_t)nd1 * 8, hipMemcpyDeviceToHost, st));
        MF_HIP(hipStreamSynchronize(st));
        SH->ready = true;
        if (T.l1.lo == 0 && T.l1.hi == (uint32_t)nd1 && n_occ) { ctx->last_l1_per_occ = (double)SH->cap / (double)n_occ; ctx->last_l1_k = K; }
    }
    // this slice's view: the shared buffer, its own copy of the directory (the levels swap it away), and as many records
    // as its digit regions span
    T.bufA.borrow(ctx, SH->buf.p, SH->buf.n);
    MF_TRY(T.pstart.alloc(ctx, T.np)); MF_TRY(T.plen.alloc(ctx, T.np)); MF_TRY(T.pocc.alloc(ctx, T.np));
    MF_HIP(hipMemcpyAsync(T.pstart.p, SH->pstart.p, (size_t)nd1 * 8, hipMemcpyDeviceToDevice, st));
    MF_HIP(hipMemcpyAsync(T.plen.p, SH->plen.p, (size_t)nd1 * 4, hipMemcpyDeviceToDevice, st));
    T.rebase = SH->h_pstart[T.dlo];
    T.cap = (T.dhi < (uint32_t)nd1 ? SH->h_pstart[T.dhi] : SH->cap) - T.rebase;
    return MF_OK;
}

// ---- the pilot: distinct k-mers per occurrence -> the levels after the first (T.lv[1..]) and, where the cut is made in the
// counting kernel, the table partitions per counting unit (A.split_bits, *split_from_pilot)
template <int K>
static int skm_replan_from_pilot(mf_ctx *ctx, const skm_job &J, skm_slice_state &T, skm_acc &A, bool *split_from_pilot) {
    const uint64_t n_occ = J.n_occ;
    const int kthr = J.kthr, bits1 = T.l1.bits1, nd1 = 1 << bits1;
    std::vector<int> &lv = T.lv;
    int &total_bits = T.total_bits;
    double rho = -1.0, kept = -1.0, rpo = 0.0;
    MF_TRY(skm_pilot<K>(ctx, T.bufA.p, T.pstart.p, T.plen.p, T.dlo, T.dhi, n_occ, nd1, total_bits - bits1, kthr, &rho, &kept, &rpo));
    ctx->last_pilot_rho = rho; ctx->n_pilots++;
    if (rho > 0.0) {
        double want_units = (double)n_occ * rho / (double)std::max<int64_t>(64, ctx->opt_skm_unit_distinct);
        // ... and a unit's RECORDS should fit the search for identical ones (its first C2_DD * SKM_CT = 2048 records go through the
        // table as records, the rest is inserted as it comes): 380 M reads at 315-fold depth planned by distinct k-mers alone had
        // 3170 records per unit and lost 6 % of k_skm_count to the records the search did not see
        // (round 5: a record of short k-mers holds few of them -- 4.8 per record at k = 21, 8.4 at k = 31 -- and 2000 such records are a small unit:
        // more than half of k_skm_count is per-unit overhead (profiles/r05k_count_phase_cycles.txt).  50 M reads, k_skm_count / the whole step in
        // ms with 2000 and with 4000 records: k = 21 20.2 -> 16.5 / 129.9 -> 125.7, k = 23 19.8 -> 15.7 / 118.0 -> 114.2, 200 M reads at k = 21
        // 87.1 -> 70.0 / 375.9 -> 358.7; k = 25, 27, 31: no difference -- the distinct k-mers bound those.  profiles/r05t_unit_records_sweep.txt)
        const int64_t unit_records = ctx->opt_skm_unit_records > 0 ? ctx->opt_skm_unit_records : (K >= 25 ? 2000 : 4000) * SKM_CT / 512;
        if (ctx->opt_skm_dedupe) want_units = std::max(want_units, (double)n_occ * rpo / (double)unit_records);
        int Bc = 0; while (Bc < 30 && (double)(1ull << Bc) < want_units) Bc++;
        const int r = std::max(1, std::min(Bc - bits1, std::min((int)SKM_DIGIT_BITS, 30 - bits1)));
        if (ctx->opt_verbose) fprintf(stderr, "[mf] skm pilot: %.4f distinct k-mers per occurrence -> %d bits after level 1 (planned from the occurrences alone: %d)\n", rho, r, total_bits - bits1);
        lv.resize(1);
        if (r <= MF_MAX_DIGIT_BITS) lv.push_back(r); else { lv.push_back((r + 1) / 2); lv.push_back(r / 2); }
        total_bits = 0; for (int b : lv) total_bits += b;
        if (kthr >= 0 && kept >= 0.0 && !A.doff.p) {
            // the table holds the k-mers that survive the cut: as many table partitions per counting unit as keep a partition
            // within the graph kernels' LDS lookup table (mf_nbr.h: 352 keys; 100 M reads of the benchmark: 343 per unit -> 2 x 172)
            const double per_unit = (double)n_occ * kept / (double)(1ull << total_bits);
            int sb = 0; while (sb < 4 && per_unit / (double)(1 << sb) > (double)ctx->opt_part_good) sb++;
            A.split_bits = sb; *split_from_pilot = true;
            if (ctx->opt_verbose) fprintf(stderr, "[mf] skm pilot: %.4f k-mers per occurrence survive the cut: %.0f per counting unit -> %d table partition(s) per unit\n", kept, per_unit, 1 << sb);
        }
    }
    return MF_OK;
}

// ---- the table's partitions, once per run (the first slice, now that the plan stands): 2^split_bits per counting partition
static int skm_plan_table(mf_ctx *ctx, int total_bits, bool split_from_pilot, skm_acc &A) {
    if (!split_from_pilot) A.split_bits = A.table_bits > 0 ? std::max(0, std::min(4, A.table_bits - total_bits)) : 1;
    if (total_bits + A.split_bits > 30) A.split_bits = 30 - total_bits;
    A.np_total = (uint32_t)(1ull << (total_bits + A.split_bits));      // partitions of the table: 2^split_bits per counting partition
    MF_TRY(A.doff.alloc(ctx, (size_t)A.np_total + 1));
    return MF_OK;
}

// ---- the slice's digits only: the directory of the following levels starts at digit dlo
static int skm_restrict_to_slice(mf_ctx *ctx, skm_slice_state &T) {
    hipStream_t st = ctx->stream;
    const uint32_t dlo = T.dlo, np = T.dhi - T.dlo;
    T.np = np;
    mf_buf<uint64_t> ps; MF_TRY(ps.alloc(ctx, np)); mf_buf<uint32_t> pl, po; MF_TRY(pl.alloc(ctx, np)); MF_TRY(po.alloc(ctx, np));
    MF_HIP(hipMemcpyAsync(ps.p, T.pstart.p + dlo, (size_t)np * 8, hipMemcpyDeviceToDevice, st));
    MF_HIP(hipMemcpyAsync(pl.p, T.plen.p + dlo, (size_t)np * 4, hipMemcpyDeviceToDevice, st));
    MF_HIP(hipMemcpyAsync(po.p, T.pocc.p + dlo, (size_t)np * 4, hipMemcpyDeviceToDevice, st));
    T.pstart.swap(ps); T.plen.swap(pl); T.pocc.swap(po);
    return MF_OK;
}

// ---- A.snap (mf_debug_skm_records), in two steps: the slice's level-1 directory before the split levels swap it away ...
static int skm_snapshot_level1(mf_ctx *ctx, const skm_slice_state &T, skm_snap_slice &snap) {
    hipStream_t st = ctx->stream;
    const uint32_t np = T.np;
    snap.l1_pstart.resize(np); snap.l1_plen.resize(np);
    MF_HIP(hipMemcpyAsync(snap.l1_pstart.data(), T.pstart.p, (size_t)np * 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipMemcpyAsync(snap.l1_plen.data(), T.plen.p, (size_t)np * 4, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    return MF_OK;
}
// ... and the records and the directory as they stand in front of count + gather: the slice goes to A.snap and ends here
static int skm_snapshot(mf_ctx *ctx, const skm_job &J, const skm_slice_state &T, skm_snap_slice &snap, mf_skm_snap *to) {
    hipStream_t st = ctx->stream;
    const uint32_t np = T.np;
    // (pocc of a shared level 1 without a split level does not exist: S > 1 needs two levels)
    snap.cap = std::min<unsigned long long>(T.cap, T.bufA.n); snap.lv = T.lv; snap.dlo = T.dlo; snap.dhi = T.dhi; snap.G = T.l1.G; snap.wpb = T.l1.wpb;
    snap.one_pass = T.snap_one_pass; snap.repeated = T.snap_repeated; snap.fast = T.l1.fast_lds != 0;
    snap.rec.resize((size_t)snap.cap * 2); snap.pstart.resize(np); snap.plen.resize(np); snap.pocc.resize(np);
    unsigned long long nv = 0;
    if (snap.cap) MF_HIP(hipMemcpyAsync(snap.rec.data(), T.bufA.p, (size_t)snap.cap * sizeof(skm_rec), hipMemcpyDeviceToHost, st));
    MF_HIP(hipMemcpyAsync(snap.pstart.data(), T.pstart.p, (size_t)np * 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipMemcpyAsync(snap.plen.data(), T.plen.p, (size_t)np * 4, hipMemcpyDeviceToHost, st));
    MF_HIP(hipMemcpyAsync(snap.pocc.data(), T.pocc.p, (size_t)np * 4, hipMemcpyDeviceToHost, st));
    MF_HIP(hipMemcpyAsync(&nv, &J.scal[6], 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    MF_HIP(hipGetLastError());
    snap.n_valid = nv;
    to->slices.push_back(std::move(snap));
    return MF_OK;
}

// (verbose >= 2) What a ONE-pass split would have to cope with ("measure, do not argue"): its sub-partitions would be sized from a
// SAMPLE of the records (every 16th tile, as level 1 is) plus slack, and a record that finds its sub-partition full goes to an overflow
// list.  From the exact sizes at hand: the records that overflow, in expectation over the sample (n' ~ Binomial(n, 1/16) as a normal
// deviate, capacity = 16 n' (1 + slack) + 64), at 6 / 12 / 25 / 50 % slack.
static int skm_split_whatif(mf_ctx *ctx, const uint32_t *olen, uint64_t np2) {
    hipStream_t st = ctx->stream;
    std::vector<uint32_t> h(np2);
    MF_HIP(hipMemcpyAsync(h.data(), olen, np2 * 4, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    double tot = 0, tot2 = 0, mx = 0;
    for (uint32_t v : h) { tot += v; tot2 += (double)v * v; mx = std::max(mx, (double)v); }
    const double mean = tot / (double)np2, sd = std::sqrt(std::max(0.0, tot2 / (double)np2 - mean * mean));
    const double slack[4] = {0.06, 0.12, 0.25, 0.50};
    double over[4] = {0, 0, 0, 0}, parts[4] = {0, 0, 0, 0}, room[4] = {0, 0, 0, 0};
    for (uint32_t v : h) {
        const double n = v, mu = n / 16.0, sg = std::sqrt(n / 16.0 * 15.0 / 16.0);
        for (int q = 0; q < 4; q++) {
            // overflow = n - cap(n') where cap = 16 n' (1 + s) + 64; integrate over n' = mu + z sg on a grid of z
            double e = 0, pr = 0, rm = 0;
            for (int zi = -40; zi <= 40; zi++) {
                const double z = zi * 0.1, w = std::exp(-0.5 * z * z) * 0.1 / 2.5066282746;
                const double cap = std::max(0.0, 16.0 * (mu + z * sg) * (1.0 + slack[q]) + 64.0);
                if (n > cap) { e += w * (n - cap); pr += w; }
                rm += w * cap;
            }
            over[q] += e; parts[q] += pr; room[q] += rm;
        }
    }
    fprintf(stderr, "[mf] skm split, one-pass what-if: %llu sub-partitions of %.0f records on average (sd %.0f, largest %.0f); sized from a 1/16 sample + slack:\n", (unsigned long long)np2, mean, sd, mx);
    for (int q = 0; q < 4; q++)
        fprintf(stderr, "[mf]     slack %2.0f %%: %.3f %% of the records overflow (%.0f records in %.0f sub-partitions), the regions take %.2f x the records\n", slack[q] * 100.0,
                100.0 * over[q] / std::max(tot, 1.0), over[q], parts[q], room[q] / std::max(tot, 1.0));
    return MF_OK;
}

// ---- the levels after the first (S3), ping-pong between two record buffers: T.bufA and the directory end as the last level's.
// cap_last: the size every buffer of the ping-pong gets (skm_final_cap); last_of_shared: the run's last slice behind a shared level 1
static int skm_split_levels(mf_ctx *ctx, const skm_job &J, skm_slice_state &T, skm_shared *SH, bool last_of_shared, unsigned long long cap_last) {
    hipStream_t st = ctx->stream;
    unsigned long long *const scal = J.scal;
    const std::vector<int> &lv = T.lv;
    uint32_t &np = T.np; unsigned long long &cap = T.cap;
    mf_buf<uint64_t> &pstart = T.pstart; mf_buf<uint32_t> &plen = T.plen, &pocc = T.pocc; mf_buf<skm_rec> &bufA = T.bufA;
    int used = 0;
    mf_buf<skm_rec> spare;                                // the buffer a level has read from: the next level writes into it
    for (size_t li = 1; li < lv.size(); li++) {
        const int bits = lv[li], nd = 1 << bits;
        const uint64_t cap2 = cap + (uint64_t)np * SKM_LINE * nd;
        const uint64_t np2 = (uint64_t)np * nd;
        if (np2 > 0xFFFFFFF0ull) return mf_set_error("too many partitions");
        const bool last = li + 1 == lv.size();
        mf_buf<skm_rec> bufB;
        if (spare.p && spare.n >= cap2) bufB.swap(spare);
        else if (bufB.alloc(ctx, std::max<unsigned long long>(cap2, cap_last)) != MF_OK) {
            if (ctx->opt_verbose) fprintf(stderr, "[mf] skm: no room for %.1f GB of level-%zu records (arena %.1f GB): %s\n", cap2 * 16 / 1e9, li + 1, ctx->arena_bytes / 1e9, mf_last_error());
            return MF_SKM_NOMEM;
        }
        mf_buf<uint64_t> ostart; MF_TRY(ostart.alloc(ctx, np2));
        mf_buf<uint32_t> olen; MF_TRY(olen.alloc(ctx, np2));
        mf_buf<uint32_t> oocc; if (last) MF_TRY(oocc.alloc(ctx, np2));
        const size_t lds = skm_stage_bytes(nd);
        const unsigned grid = (unsigned)std::min<uint64_t>(np, (uint64_t)ctx->n_cu * (lds > 72 * 1024 ? 1 : 2));
        {
            MF_TRY(skm_set_lds(k_skm_split, lds));
            mf_ktimer t(ctx, "k_skm_split");
            k_skm_split<<<grid, 1024, lds, st>>>(bufA.p, pstart.p, plen.p, np, SKM_DIGIT_BITS - used - bits, bits, bufB.p, ostart.p, olen.p, oocc.p,
                                                 li == 1 ? &scal[6] : nullptr, li == 1 ? T.rebase : 0);
        }
        MF_DBG(ctx, "k_skm_split");
        if (ctx->opt_verbose >= 2 && last) MF_TRY(skm_split_whatif(ctx, olen.p, np2));
        bufA.swap(bufB);
        if (!last && bufB.owned) { spare.reset(); spare.swap(bufB); }        // (a borrowed level-1 buffer is the other slices' input too ...
        else if (!last && SH && last_of_shared && bufB.p == SH->buf.p) {    // ... unless this is the run's last slice: its third level writes there)
            bufB.reset(); spare.reset(); spare.swap(SH->buf); SH->ready = false;
        }
        pstart.swap(ostart); plen.swap(olen);
        if (last) pocc.swap(oocc);
        cap = cap2; np = (uint32_t)np2; used += bits;
    }
    return MF_OK;
}

// the dense table does not hold `need` entries: a larger one.  Everything still to come is bounded by the slices of the remaining batches
// (rest_cap); expect the ratio seen so far (`need` entries out of done_cap)
static int skm_grow_table(mf_ctx *ctx, skm_acc &A, uint64_t need, uint64_t done_cap, uint64_t rest_cap) {
    hipStream_t st = ctx->stream;
    const double ratio = done_cap ? (double)need / (double)done_cap : 1.0;
    uint64_t want = need + (uint64_t)std::min<double>((double)rest_cap, (double)rest_cap * ratio * 1.12 + 4096.0);
    if (want < need) want = need;
    mf_buf<uint64_t> nk; mf_buf<uint16_t> nc;
    if (nk.alloc(ctx, want) != MF_OK || nc.alloc(ctx, want) != MF_OK) return MF_SKM_NOMEM;
    if (A.dused) {
        ctx->n_table_regrown++;                                 // (mf_ctx_stat "skm_table_regrown")
        MF_HIP(hipMemcpyAsync(nk.p, A.dk.p, A.dused * 8, hipMemcpyDeviceToDevice, st));
        MF_HIP(hipMemcpyAsync(nc.p, A.dc.p, A.dused * 2, hipMemcpyDeviceToDevice, st));
        MF_HIP(hipStreamSynchronize(st));
    }
    A.dk.swap(nk); A.dc.swap(nc);
    A.dcap = want;
    return MF_OK;
}

// ---- count + gather (S4), a batch of partitions at a time.  A partition's (key,count) slice is sized by its k-mer count
// (it cannot hold more distinct k-mers than it has k-mers, nor more than the LDS table), i.e. all slices together
// are as large as the k-mer stream itself: the buffer holds ONE batch of slices and is redused, the dense table grows
// batch by batch (sized from the first batch's distinct / k-mer ratio; re-allocated if that was too optimistic).
// slices_to_come: the run's slices after this one (taken to be like this one where the table grows)
template <int K>
static int skm_count_batches(mf_ctx *ctx, const skm_job &J, skm_slice_state &T, skm_acc &A, uint32_t slices_to_come) {
    hipStream_t st = ctx->stream;
    unsigned long long *const scal = J.scal;
    const uint64_t n_occ = J.n_occ;
    const int kthr = J.kthr, bits1 = T.l1.bits1, total_bits = T.total_bits;
    const uint32_t np = T.np, dlo = T.dlo;
    mf_buf<uint64_t> &pstart = T.pstart; mf_buf<uint32_t> &plen = T.plen, &pocc = T.pocc; mf_buf<skm_rec> &bufA = T.bufA;
    mf_buf<uint32_t> pcap; MF_TRY(pcap.alloc(ctx, np));
    mf_buf<uint64_t> toff; MF_TRY(toff.alloc(ctx, (size_t)np + 1));
    k_skm_cap<<<(np + 255) / 256, 256, 0, st>>>(pocc.p, np, pcap.p, kthr >= 0 ? (uint32_t)kthr + 1u : 1u);
    MF_TRY(mf_scan<1>(ctx, pcap.p, toff.p, np, (uint64_t *)&scal[4]));
    // As few batches as the memory allows (every batch is a launch, a scan, a gather and a round trip to the host: 8 -> 2
    // batches took 4 ms off a 200 ms step): the temporary lists of one batch may take a fifth of the device.
    uint32_t nbatch = 1;
    if (ctx->opt_skm_batches > 0) nbatch = (uint32_t)std::min<int64_t>(ctx->opt_skm_batches, np);
    else {
        unsigned long long tall = 0;
        MF_HIP(hipMemcpyAsync(&tall, &scal[4], 8, hipMemcpyDeviceToHost, st));
        MF_HIP(hipStreamSynchronize(st));
        size_t fr = 0, tot = 0;
        MF_HIP(hipMemGetInfo(&fr, &tot));
        double budget = (ctx->opt_arena_cap_gb > 0 ? (double)ctx->opt_arena_cap_gb * 1e9 : (double)tot) * 0.22;
        if (ctx->opt_arena_cap_gb <= 0) budget = std::min(budget, ((double)fr + (double)mf_arena_idle(ctx)) * 0.5);      // ... and half of what is free right now
        // (a small sample -- the drop-in's 20 M reads -- in one batch asked for 12 GB of lists beside 10 GB of records: memory a short process
        // pays 35 ms per GiB for when the driver has to clear it first; a batch more costs 0.7 ms)
        if (n_occ < (1ull << 32)) budget = std::min(budget, 3e9);
        while (nbatch < 64 && nbatch * 2 <= np && (double)tall * 10.0 / nbatch > budget) nbatch *= 2;
    }
    const uint32_t PB = (np + nbatch - 1) / nbatch;
    std::vector<unsigned long long> tb(nbatch + 1);
    for (uint32_t b = 0; b <= nbatch; b++)
        MF_HIP(hipMemcpyAsync(&tb[b], &toff.p[std::min<uint64_t>((uint64_t)b * PB, np)], 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    pcap.reset(); pocc.reset();
    const unsigned long long tcap = tb[nbatch];
    unsigned long long tmax = 0;
    for (uint32_t b = 0; b < nbatch; b++) tmax = std::max(tmax, tb[b + 1] - tb[b]);
    mf_buf<uint64_t> tkeys; mf_buf<uint16_t> tcnt;
    if (tkeys.alloc(ctx, tmax) != MF_OK || tcnt.alloc(ctx, tmax) != MF_OK) {
        if (ctx->opt_verbose) fprintf(stderr, "[mf] skm: no room for %.1f GB of temporary lists\n", tmax * 10 / 1e9);
        return MF_SKM_NOMEM;
    }
    mf_buf<uint32_t> dcount; MF_TRY(dcount.alloc(ctx, np));
    mf_buf<uint64_t> coff; MF_TRY(coff.alloc(ctx, (size_t)np + 1));      // offsets of the counting partitions inside their batch
    // this slice's partitions in the numbering of the whole run (A.np_total, doffp: the table's partitions, two per counting partition)
    const uint32_t pbase = (uint32_t)(((uint64_t)dlo * A.np_total) >> bits1);
    uint64_t *const doffp = A.doff.p + pbase;
    mf_buf<uint64_t> &dk = A.dk; mf_buf<uint16_t> &dc = A.dc;
    uint64_t &dused = A.dused, &dcap = A.dcap;
    mf_buf<unsigned long long> &dhist = A.dhist, &c2p = A.c2p;
    for (uint32_t b = 0; b < nbatch; b++) {
        const uint32_t p0 = (uint32_t)std::min<uint64_t>((uint64_t)b * PB, np), p1 = (uint32_t)std::min<uint64_t>((uint64_t)(b + 1) * PB, np);
        if (p0 == p1) continue;
        {
            const unsigned grid = (unsigned)std::min<uint64_t>(p1 - p0, (uint64_t)ctx->n_cu * C2_WG_PER_CU);      // resident workgroups
            MF_HIP(hipMemsetAsync(&scal[8], 0, 16, st));                     // ([8] units redone, [9] the unit counter)
            mf_ktimer t(ctx, "k_skm_count");
            k_skm_count<K><<<grid, SKM_CT, C2_LDS, st>>>(bufA.p, pstart.p, plen.p, p1, toff.p, tkeys.p, tcnt.p, dcount.p, (unsigned int *)&scal[2], p0, (uint64_t)tb[b], kthr, &scal[7],
                                                         (unsigned int *)&scal[8], dhist.p, c2p.p, (uint64_t)tmax, (uint32_t)ctx->opt_skm_dedupe, (ctx->opt_skm_dynq ? (unsigned int *)&scal[9] : nullptr));
        }
        MF_DBG(ctx, "k_skm_count");
        MF_TRY(mf_scan<1>(ctx, dcount.p + p0, coff.p + p0, p1 - p0, (uint64_t *)&scal[3]));      // offsets inside the batch
        unsigned long long res[2];
        MF_HIP(hipMemcpyAsync(res, &scal[2], 16, hipMemcpyDeviceToHost, st));
        MF_HIP(hipStreamSynchronize(st));
        if (ctx->opt_verbose) {
            unsigned long long nr = 0;
            MF_HIP(hipMemcpy(&nr, &scal[8], 8, hipMemcpyDeviceToHost));
            if (nr & 0xFFFFFFFFull) fprintf(stderr, "[mf] skm: batch %u: %llu partition(s) counted in several passes\n", b, nr & 0xFFFFFFFFull);
        }
        if (ctx->opt_verbose) {
            unsigned long long bad = 0;
            MF_HIP(hipMemcpy(&bad, &c2p.p[7], 8, hipMemcpyDeviceToHost));
            if (bad) fprintf(stderr, "[mf] skm: batch %u: %llu counter(s) found non-zero under an empty key so far\n", b, bad);
        }
        if (res[0]) {
            if (ctx->opt_verbose) fprintf(stderr, "[mf] skm: a minimizer partition overflows the LDS table (code %llu), using the k-mer path\n", res[0]);
            if (ctx->opt_verbose && res[0] == 2) {
                unsigned long long h[16];
                MF_HIP(hipMemcpy(h, c2p.p, 128, hipMemcpyDeviceToHost));
                fprintf(stderr, "[mf]   p=%llu o=%llu room=%llu wb=%llu nkeep=%llu tcap=%llu p0=%llu np=%llu (batch %u: tb=%llu..%llu)\n", h[8], h[9], h[10], h[11], h[12], h[13], h[14], h[15], b, tb[b], tb[b + 1]);
            }
            MF_HIP(hipMemsetAsync(&scal[2], 0, 8, st));
            return MF_SKM_FALLBACK;
        }
        const uint64_t d_b = res[1];
        // (what is still to come: the remaining batches + the slices still to come, taken to be like this one)
        if (dused + d_b > dcap) SKM_STEP(skm_grow_table(ctx, A, dused + d_b, tb[b + 1], tcap - tb[b + 1] + (uint64_t)slices_to_come * tcap));
        {
            const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)(p1 - p0) + 3) / 4, (uint64_t)ctx->n_cu * 32);
            mf_ktimer t(ctx, "k_gather");
            if (A.split_bits == 1)
                k_gather_split<K><<<grid, 256, 0, st>>>(tkeys.p, tcnt.p, toff.p, dcount.p, coff.p, p1, dk.p + dused, dc.p + dused, p0, (uint64_t)tb[b],
                                                        doffp, dused, 31 - total_bits);
            else
                k_gather_split_n<K><<<grid, 256, 0, st>>>(tkeys.p, tcnt.p, toff.p, dcount.p, coff.p, p1, dk.p + dused, dc.p + dused, p0, (uint64_t)tb[b],
                                                          doffp, dused, std::min(31, 32 - total_bits - A.split_bits), A.split_bits);
        }
        MF_DBG(ctx, "k_gather");
        dused += d_b;
    }
    MF_HIP(hipGetLastError());
    return MF_OK;
}

// One SLICE of the run: the records whose level-1 digit lies in [dlo, dhi) go through scatter, split and count.  A run is one
// slice unless the records do not fit next to the reads (300 M reads and more): then the reads are scanned once per slice
// and only a 1 / S share of the records exists at any time.  Partitions are numbered by digit, so slice after slice fills
// the dense table in the same order as a single pass would.
// SH: level 1 covers all of the run's digits and is done by the first slice; dlo / dhi then only say which regions this slice takes.
// *plan_open: the levels after the first are still to be planned (skm_pilot): lv[1..] may change in here, once
template <int K>
static int skm_slice(mf_ctx *ctx, const skm_job &J, std::vector<int> &lv, uint32_t dlo, uint32_t dhi, uint32_t slice, uint32_t n_slices, skm_acc &A,
                     skm_shared *SH, bool *plan_open) {
    hipStream_t st = ctx->stream;
    const int bits1 = lv[0], nd1 = 1 << bits1;
    skm_slice_state T{lv};
    T.total_bits = 0; for (int b : lv) T.total_bits += b;
    T.dlo = dlo; T.dhi = dhi;
    int G = ctx->opt_l1_blocks > 0 ? (int)ctx->opt_l1_blocks : ctx->n_cu;
    {
        uint64_t maxG = (J.in.n_words + 1023) / 1024;
        if ((uint64_t)G > maxG) G = (int)maxG;
        if (G < 1) G = 1;
    }
    T.l1 = skm_l1{J.in, (J.in.n_words + G - 1) / G, bits1, G, SH ? SH->lo : dlo, SH ? SH->hi : dhi, skm_fast_lds(ctx, nd1)};
    T.np = (uint32_t)nd1;
    MF_TRY(T.pstart.alloc(ctx, T.np)); MF_TRY(T.plen.alloc(ctx, T.np)); MF_TRY(T.pocc.alloc(ctx, T.np));
    const bool open = plan_open && *plan_open;
    if (A.snap && SH && SH->ready && !A.snap->slices.empty()) { T.snap_one_pass = A.snap->slices.back().one_pass; T.snap_repeated = A.snap->slices.back().repeated; }   // (the first slice's level 1)

    // S1, S2: level 1 -- unless the run's first slice has made it for all of them; then this slice's view of the shared one
    if (!(SH && SH->ready)) SKM_STEP(skm_level1<K>(ctx, J, T, !SH, open));
    if (SH) SKM_STEP(skm_share_level1<K>(ctx, T, SH, J.n_occ));
    // the plan: the following levels from the pilot (once per run), the table's partitions (the first slice of the run)
    bool split_from_pilot = false;
    if (open) {
        *plan_open = false;
        SKM_STEP(skm_replan_from_pilot<K>(ctx, J, T, A, &split_from_pilot));
    }
    if (!A.doff.p) SKM_STEP(skm_plan_table(ctx, T.total_bits, split_from_pilot, A));
    MF_HIP(hipMemsetAsync(&J.scal[6], 0, 8, st));         // [6] records without padding ([7] distinct k-mers before the cut: whole run)
    const unsigned long long cap_l1 = T.cap, cap_last = skm_final_cap(lv, J.n_occ, T.cap, false);
    // the directory cut to the slice's digits
    if (dlo != 0 || dhi != (uint32_t)nd1) SKM_STEP(skm_restrict_to_slice(ctx, T));
    skm_snap_slice snap;
    if (A.snap) SKM_STEP(skm_snapshot_level1(ctx, T, snap));
    // S3: the split levels
    SKM_STEP(skm_split_levels(ctx, J, T, SH, slice + 1 == n_slices, cap_last));
    if (A.snap) return skm_snapshot(ctx, J, T, snap, A.snap);
    // S4: count + gather, batch by batch into the run's table
    SKM_STEP(skm_count_batches<K>(ctx, J, T, A, n_slices - 1 - slice));
    T.bufA.reset();
    {
        unsigned long long nv = 0;
        MF_HIP(hipMemcpyAsync(&nv, &J.scal[6], 8, hipMemcpyDeviceToHost, st));
        MF_HIP(hipStreamSynchronize(st));
        A.n_records += nv ? nv : cap_l1;                  // (plans without a split level: the padded level-1 count)
    }
    if (ctx->opt_verbose)
        fprintf(stderr, "[mf] count(skm): slice %u/%u digits [%u,%u): records=%llu levels=%zu bits=%d np=%u distinct so far=%llu\n", slice + 1, n_slices, dlo, dhi,
                (unsigned long long)T.cap, lv.size(), T.total_bits, T.np, (unsigned long long)A.dused);
    return MF_OK;
}

// Slices (HBM budget): the records of a run are about a third of the reads' bytes per radix level, two levels ping-pong.
// Reads, table and index have to fit beside them.  Option skm_slices forces a number (tests); arena_cap_gb stands in for
// a smaller device.
// *shared: the slices share ONE level 1 over all digits (skm_shared) instead of scanning the reads once each.  It needs
// the whole level-1 buffer + the slice-sized buffers of the following levels beside the growing table, which is tried
// when what is free right now says so (option skm_shared: 0 never, 1 auto, 2 whenever there are slices); if it then
// does not fit after all, the level-1 buffer is kept for a second try with twice the slices before the run goes back
// to slices that scan for themselves (skm_run).
template <int K>
static int skm_plan_slices(mf_ctx *ctx, const skm_job &J, const std::vector<int> &lv, uint32_t *n_slices, bool *share) {
    const uint64_t n_bases = J.in.n_bases, n_occ = J.n_occ;
    const int kthr = J.kthr, nd1 = 1 << lv[0];
    uint32_t S = 1;
    bool shared = false;
    if (lv.size() >= 2) {
        size_t fr = 0, tot = 0;
        MF_HIP(hipMemGetInfo(&fr, &tot));
        if (ctx->opt_skm_slices > 0) S = (uint32_t)ctx->opt_skm_slices;
        else {
            double budget = (ctx->opt_arena_cap_gb > 0 ? (double)ctx->opt_arena_cap_gb * 1e9 : (double)tot * 0.92) - (double)n_bases * 1.15 - 8e9;
            const double table = (double)n_occ * 0.14 * 26.0;       // (distinct k-mers that survive ~ a seventh of the occurrences) x (entry + index)
            budget -= std::min(table, budget * 0.5);
            const double recs = (double)n_occ / 5.5 * 16.0 * 2.3;    // two buffers + slices' padding
            while (S < 64 && recs / S > budget) S *= 2;
        }
        while (S > 1 && (uint32_t)nd1 / S < 4) S /= 2;
        if (S > 1 && ctx->opt_skm_shared == 2) shared = true;
        else if (S > 1 && ctx->opt_skm_shared == 1 && ctx->opt_arena_cap_gb <= 0) {
            // free now (the reads are already resident) - the table (the k-mers that survive the cut; it is sized from the first
            // batch's ratio, so it rarely grows twice) - room for a batch of temporary lists (they adapt: more batches)
            const double avail = ((double)fr + (double)mf_arena_idle(ctx)) * 0.96 - (double)n_occ * (kthr >= 1 ? 0.04 : 0.10) * 10.0 * 1.3 - (double)tot * 0.05;
            // records: a minimizer run is (K - M + 2) / 2 k-mers long where reads and the record format do not cut it shorter
            const double run = std::min<double>((K - mf_skm_m(K) + 2) / 2.0, (double)skm_word<K>::RMAX) * 0.78;
            const double full = (double)n_occ / run * 16.0 * 1.10;
            const double nb = lv.size() >= 3 ? 2.0 : 1.0;
            auto need = [&](uint32_t s2) { return full * (1.0 + nb * 1.15 / s2); };
            uint32_t S2 = ctx->opt_skm_slices > 0 ? S : 2;                   // (a forced number of slices stays)
            // (beyond 16 slices a split launch has too few partitions to fill the device: then the slices scan for themselves)
            while (ctx->opt_skm_slices <= 0 && S2 < 16 && need(S2) > avail) S2 *= 2;
            while (S2 > 1 && (uint32_t)nd1 / S2 < 4) S2 /= 2;
            if (S2 > 1 && need(S2) <= avail) { shared = true; S = S2; }
            if (ctx->opt_verbose)
                fprintf(stderr, "[mf] skm: free %.1f GB + idle %.1f GB -> %.1f GB for records; one level 1 = %.1f GB + %.1f GB per slice at %u slices: %s\n", fr / 1e9,
                        mf_arena_idle(ctx) / 1e9, avail / 1e9, full / 1e9, (need(S2) - full) / 1e9, S2, shared ? "shared" : "every slice scans");
        }
    }
    *n_slices = S; *share = shared;
    return MF_OK;
}

// A shard of the table (the level-1 digits [own_lo, own_hi) of a rank): the other ranks' partitions are empty here: offsets 0 before the
// owner's range, the table's size after it
static int skm_shard_offsets(mf_ctx *ctx, skm_acc &A, int bits1, uint32_t own_lo, uint32_t own_hi) {
    hipStream_t st = ctx->stream;
    const uint32_t pb0 = (uint32_t)(((uint64_t)own_lo * A.np_total) >> bits1), pb1 = (uint32_t)(((uint64_t)own_hi * A.np_total) >> bits1);
    if (pb0) MF_HIP(hipMemsetAsync(A.doff.p, 0, (size_t)pb0 * 8, st));
    if (A.np_total > pb1) {
        MF_HIP(hipMemsetAsync(A.doff.p + pb1 + 1, 0, (size_t)(A.np_total - pb1) * 8, st));
        k_skm_add_base<<<(A.np_total - pb1 + 255) / 256, 256, 0, st>>>(A.doff.p + pb1 + 1, (uint64_t)(A.np_total - pb1), A.dused);
    }
    if (!A.dused) MF_HIP(hipMemsetAsync(A.doff.p, 0, ((size_t)A.np_total + 1) * 8, st));
    return MF_OK;
}

// The end of a run: what its slices added up to (A) becomes the table -- the dense arrays, n_all, the counts the cut dropped, the partition offsets
static int skm_make_table(mf_ctx *ctx, int k, const skm_job &J, skm_acc &A, int total_bits, uint64_t *n_all, mf_table **out) {
    hipStream_t st = ctx->stream;
    const int kthr = J.kthr;
    const uint64_t n_dist = A.dused;
    const size_t kb = A.dk.bytes(), cb = A.dc.bytes();       // (capacity: may be a little larger than n_dist)
    MF_TRY(mf_table_adopt(ctx, k, n_dist, J.n_occ, A.dk.take(), kb, A.dc.take(), cb, out));
    {
        unsigned long long na = 0;
        MF_HIP(hipMemcpyAsync(&na, &J.scal[7], 8, hipMemcpyDeviceToHost, st));
        MF_HIP(hipStreamSynchronize(st));
        if (n_all) *n_all = na;
        (*out)->n_records = A.n_records;
        (*out)->cut_thr = kthr;
        if (kthr >= 0) {
            (*out)->dropped_hist.assign((size_t)kthr + 1, 0);
            MF_HIP(hipMemcpyAsync((*out)->dropped_hist.data(), A.dhist.p, ((size_t)kthr + 1) * 8, hipMemcpyDeviceToHost, st));
            MF_HIP(hipStreamSynchronize(st));
        }
        (*out)->record_bytes = 16;
    }
    if (total_bits + A.split_bits <= 30) {
        (*out)->part_bits = total_bits + A.split_bits;
        (*out)->part_skm = 1;
        (*out)->part_off_bytes = A.doff.bytes();
        (*out)->d_part_off = A.doff.take();
    }
    return MF_OK;
}

// lv: digit bits per level (lv[0] = level 1).  Returns MF_OK and *out, or MF_SKM_FALLBACK (nothing allocated) when the
// input does not suit this path (a partition too rich for the LDS table, too many levels, not enough memory).
template <int K>
static int skm_run(mf_ctx *ctx, const uint8_t *d_bases, uint64_t n_bases, const uint32_t *vmask, uint64_t n_words,
                   uint64_t n_occ, const std::vector<int> &lv0, bool adaptive, int table_bits, unsigned long long *scal, int thr, uint64_t *n_all, mf_table **out,
                   skm_shared *pre = nullptr) {
    // pre: level 1 stands already (a STREAMED one, skm_stream_* below: the reads are gone, d_bases == nullptr) -- whatever would scan them again
    // ends the run with MF_SKM_FALLBACK and the caller starts over from the files
    hipStream_t st = ctx->stream;
    std::vector<int> lv = lv0;                 // (the levels after the first may change once the pilot has measured the reads' depth)
    const int bits1 = lv[0], nd1 = 1 << bits1;
    int total_bits = 0; for (int b : lv) total_bits += b;
    if (total_bits > 30 || total_bits - bits1 > SKM_DIGIT_BITS) return MF_SKM_FALLBACK;      // (the table gets total_bits + 1 partition bits)
    // counts of the entries the cut drops (the .stat.txt histogram needs them): drop_hist[c], c <= thr.  The kernel tallies
    // them in a small LDS histogram: a cut above C2_LH - 1 is made afterwards (mf_count_skm)
    const int kthr = thr < C2_LH ? thr : -1;
    const skm_job J{{d_bases, n_bases, vmask, n_words}, n_occ, scal, kthr};
    MF_TRY(skm_set_lds(k_skm_count<K>, C2_LDS));
    uint32_t S = 1; bool shared = false;
    MF_TRY(skm_plan_slices<K>(ctx, J, lv, &S, &shared));
    // a shard of the table only (mf_count_device_shard): the owner's digits, sliced like a whole run
    const uint32_t W = (uint32_t)std::max(ctx->own_world, 1);
    if (W > 1 && (uint32_t)nd1 < W) return mf_set_error("count (shard): %d level-1 digits for %u ranks", nd1, W);
    const uint32_t own_lo = (uint32_t)((uint64_t)nd1 * (uint32_t)ctx->own_rank / W), own_hi = (uint32_t)((uint64_t)nd1 * ((uint32_t)ctx->own_rank + 1) / W);
    while (S > 1 && (own_hi - own_lo) / S < 1) S /= 2;
    if (S == 1) shared = false;
    skm_shared SH; SH.lo = own_lo; SH.hi = own_hi;
    if (pre) {
        if (W != 1 || lv.size() < 2 || !pre->ready) return MF_SKM_FALLBACK;
        shared = true;
        SH.buf.swap(pre->buf); SH.pstart.swap(pre->pstart); SH.plen.swap(pre->plen); SH.pocc.swap(pre->pocc); SH.h_pstart.swap(pre->h_pstart);
        SH.cap = pre->cap; SH.ready = true; pre->ready = false;
    }
    const uint32_t S_own = S;
    int shared_tries = 0;
    // ---- the PILOT (round 4, skm_pilot above): the plan the caller made sizes the counting units by OCCURRENCES; what a unit costs
    // is decided by its DISTINCT k-mers.  The first slice measures them once its level 1 stands and re-plans the later levels.
    bool plan_open = adaptive && ctx->opt_skm_pilot != 0 && lv.size() >= 2 && W == 1;
    for (;;) {
        if (pre && !(shared && SH.ready)) return MF_SKM_FALLBACK;
        skm_acc A;                                              // (A.np_total, A.doff: set by the first slice, once the plan stands)
        A.table_bits = table_bits;
        A.snap = ctx->skm_snap;
        if (A.snap) A.snap->slices.clear();
        if (kthr >= 0) { MF_TRY(A.dhist.alloc(ctx, (size_t)MF_MAX_COUNT + 1)); MF_HIP(hipMemsetAsync(A.dhist.p, 0, A.dhist.bytes(), st)); }
        MF_TRY(A.c2p.alloc(ctx, 16)); MF_HIP(hipMemsetAsync(A.c2p.p, 0, 128, st));     // [7] counters found non-zero under an empty key (verbose), [8,16) overflow diagnostics
        MF_HIP(hipMemsetAsync(&scal[7], 0, 8, st));
        int rc = MF_OK;
        for (uint32_t sl = 0; sl < S && rc == MF_OK; sl++)
            rc = skm_slice<K>(ctx, J, lv, own_lo + (uint32_t)((uint64_t)(own_hi - own_lo) * sl / S), own_lo + (uint32_t)((uint64_t)(own_hi - own_lo) * (sl + 1) / S),
                              sl, S, A, shared ? &SH : nullptr, &plan_open);
        if (rc == MF_OK && A.snap) { SH.clear(); return MF_SKM_SNAPPED; }
        total_bits = 0; for (int b : lv) total_bits += b;
        if (rc == MF_OK && W > 1) MF_TRY(skm_shard_offsets(ctx, A, bits1, own_lo, own_hi));
        if (rc == MF_SKM_NOMEM) {
            ctx->n_slice_restarts++;                             // (what was counted so far is thrown away: mf_ctx_stat "slice_restarts", bench.py reports it)
            const bool can_double = lv.size() >= 2 && S < 64 && (own_hi - own_lo) / (2 * S) >= 1 && (W > 1 || (uint32_t)nd1 / (2 * S) >= 4);
            if (shared && SH.ready && can_double && shared_tries++ < 2) {
                if (ctx->opt_verbose) fprintf(stderr, "[mf] skm: %u slice(s) behind a shared level 1 do not fit, trying %u\n", S, 2 * S);
                S *= 2;
                continue;
            }
            if (shared) {
                if (ctx->opt_verbose) fprintf(stderr, "[mf] skm: a shared level 1 does not fit, every slice scans for itself\n");
                shared = false; SH.clear(); S = S_own;
                continue;
            }
            if (can_double) {
                if (ctx->opt_verbose) fprintf(stderr, "[mf] skm: %u slice(s) do not fit, trying %u\n", S, 2 * S);
                S *= 2;
                continue;
            }
            return MF_SKM_FALLBACK;
        }
        if (rc != MF_OK) return rc;
        SH.clear();
        // (the record buffers stay in the arena for the next sample: hipMalloc costs 35 ms per GiB, 5 s for a 150 GiB level 1;
        // a host that needs the memory asks with mf_ctx_trim_bytes)
        if (ctx->opt_verbose)
            fprintf(stderr, "[mf] count(skm): n_occ=%llu records=%llu slices=%u%s levels=%zu bits=%d distinct=%llu\n", (unsigned long long)n_occ,
                    A.n_records, S, shared ? " (one level 1)" : "", lv.size(), total_bits, (unsigned long long)A.dused);
        return skm_make_table(ctx, K, J, A, total_bits, n_all, out);
    }
}

// (a k-mer length whose window of M-mers the scan is not built for -- 3 <= k - M + 1 <= 17: the sliding minimum and the halo of 16 M-mers a
// lane takes from the next one -- goes to the one-record-per-k-mer path)
template <int K, typename... A> static int skm_run_if(A &&... a) {
    if constexpr (K - mf_skm_m(K) + 1 >= 3 && K - mf_skm_m(K) + 1 <= 17) return skm_run<K>(std::forward<A>(a)...);
    else return MF_SKM_FALLBACK;
}
// =============================================================================================
// STREAMED level 1 (round 6; the driver is mf_stream.hip): the reads of a library arrive piece by piece while the rest of the file is still crossing
// PCIe.  begin: the digit regions are sized from a SAMPLE of the files (chunks spread evenly over them, parsed like a small file) and the record
// buffer is made; piece: one launch of the one-pass scatter per piece, all pieces filling the same regions through the same cursors; finish: the
// directory, and the run goes on behind a level 1 that "the first slice has made" (skm_shared).  A region that turns out too small, a plan without
// a split level, anything else that would need the reads again: MF_SKM_FALLBACK, and the caller loads the files whole.
// =============================================================================================
struct mf_skm_stream {
    mf_ctx *ctx = nullptr; int k = 0;
    std::vector<int> lv; bool adaptive = false; int table_bits = 0;
    int G = 0; size_t fast_lds = 0;
    mf_buf<unsigned long long> scal, gcur, save;
    mf_buf<uint64_t> rstart;
    mf_buf<skm_rec> buf; unsigned long long cap = 0;
    uint64_t pieces = 0;
};
__global__ void k_skm_region_sizes_stream(const uint32_t *__restrict__ blockhist, int Gs, int nd, double scale, uint32_t G, uint32_t pct, uint32_t *__restrict__ rsize) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= nd) return;
    uint64_t t = 0;
    for (int b = 0; b < Gs; b++) t += blockhist[(size_t)d * Gs + b];
    const double e = (double)t * scale;
    // an eighth + four standard deviations of the sample's count, scaled; a partly used chunk per workgroup; the runs a piece border cuts
    uint64_t r = (uint64_t)(e + e / 8.0 + 4.0 * sqrt((double)t + 1.0) * scale) + (uint64_t)G * SKM_CH + 16384;
    if (pct != 100u) r = r * pct / 100u;                 // (tests: regions that overflow)
    r = (r + SKM_CH - 1) & ~(uint64_t)(SKM_CH - 1);
    rsize[d] = r > 0xFFFFFF00ull ? 0xFFFFFF00u : (uint32_t)r;
}
template <int K>
static int skm_stream_begin(mf_skm_stream *S, const uint8_t *s_bases, uint64_t s_nbases, const uint32_t *s_vmask, uint64_t s_nwords, double scale) {
    mf_ctx *ctx = S->ctx; hipStream_t st = ctx->stream;
    const int bits1 = S->lv[0], nd1 = 1 << bits1;
    int total_bits = 0; for (int b : S->lv) total_bits += b;
    if (S->lv.size() < 2 || total_bits > 30 || total_bits - bits1 > SKM_DIGIT_BITS) return MF_SKM_FALLBACK;
    S->G = ctx->opt_l1_blocks > 0 ? (int)ctx->opt_l1_blocks : ctx->n_cu;
    S->fast_lds = skm_fast_lds(ctx, nd1);
    int Gs = S->G;
    { const uint64_t maxG = (s_nwords + 1023) / 1024; if ((uint64_t)Gs > maxG) Gs = (int)std::max<uint64_t>(maxG, 1); }
    const uint64_t wpb = (s_nwords + Gs - 1) / Gs;
    mf_buf<uint32_t> blockhist; MF_TRY(blockhist.alloc(ctx, (size_t)nd1 * Gs));
    {
        mf_ktimer t(ctx, "k_skm_hist_sample");
        k_skm_hist<K><<<Gs, 1024, (size_t)nd1 * 8, st>>>(s_bases, s_nbases, s_vmask, s_nwords, wpb, bits1, blockhist.p, nullptr, Gs, 1, 0u, (uint32_t)nd1);
    }
    MF_TRY(S->scal.alloc(ctx, 12)); MF_HIP(hipMemsetAsync(S->scal.p, 0, S->scal.bytes(), st));
    mf_buf<uint32_t> rsize; MF_TRY(rsize.alloc(ctx, (size_t)nd1));
    MF_TRY(S->rstart.alloc(ctx, (size_t)nd1 + 1)); MF_TRY(S->gcur.alloc(ctx, (size_t)nd1)); MF_TRY(S->save.alloc(ctx, (size_t)S->G * nd1));
    k_skm_region_sizes_stream<<<(nd1 + 255) / 256, 256, 0, st>>>(blockhist.p, Gs, nd1, scale, (uint32_t)S->G, (uint32_t)std::max<int64_t>(ctx->opt_stream_count_test_pct, 1), rsize.p);
    MF_TRY(mf_scan<1>(ctx, rsize.p, S->rstart.p, (uint64_t)nd1, (uint64_t *)&S->scal.p[1]));
    MF_HIP(hipMemcpyAsync(S->gcur.p, S->rstart.p, (size_t)nd1 * 8, hipMemcpyDeviceToDevice, st));
    MF_HIP(hipMemsetAsync(S->save.p, 0xFF, S->save.bytes(), st));
    MF_HIP(hipMemcpyAsync(&S->cap, &S->scal.p[1], 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    if (S->buf.alloc(ctx, S->cap + (uint64_t)S->G * SKM_CH) != MF_OK) return MF_SKM_FALLBACK;
    if (ctx->opt_verbose) fprintf(stderr, "[mf] skm (streamed): level 1 of %d bits, regions for %.2f G records (%.1f GB) from a sample of %.1f M bases x %.1f\n", bits1, S->cap / 1e9, S->cap * 16 / 1e9, s_nbases / 1e6, scale);
    return MF_OK;
}
template <int K>
static int skm_stream_piece(mf_skm_stream *S, const uint8_t *d_bases, uint64_t n_bases, const uint32_t *vmask, uint64_t n_words) {
    mf_ctx *ctx = S->ctx;
    const int bits1 = S->lv[0], nd1 = 1 << bits1, G = S->G;
    const skm_l1 L{{d_bases, n_bases, vmask, n_words}, (n_words + G - 1) / G, bits1, G, 0u, (uint32_t)nd1, S->fast_lds};
    skm_dyn Dy; Dy.gcur = S->gcur.p; Dy.rend = S->rstart.p + 1; Dy.overflow = (unsigned int *)&S->scal.p[5]; Dy.dump = S->cap; Dy.save = S->save.p;
    MF_TRY((skm_scatter<K, true>(ctx, L, nullptr, S->buf.p, Dy)));
    S->pieces++;
    MF_HIP(hipGetLastError());
    return MF_OK;
}
static int skm_cut_above(int rc, int thr, mf_table **out) {
    if (rc == MF_OK && thr >= 0 && (*out)->cut_thr < thr) {
        // a cut the counting kernel does not make itself (thr >= C2_LH): as a pass over the finished table
        mf_table *all = *out, *good = nullptr;
        rc = mf_table_filter(all, thr, &good);
        if (rc == MF_OK) { good->n_occ = all->n_occ; good->n_records = all->n_records; good->record_bytes = all->record_bytes; }
        mf_table_destroy(all);
        *out = good;
    }
    return rc;
}
template <int K>
static int skm_stream_finish(mf_skm_stream *S, uint64_t n_occ, uint64_t n_bases, int thr, uint64_t *n_all, mf_table **out) {
    mf_ctx *ctx = S->ctx; hipStream_t st = ctx->stream;
    const int nd1 = 1 << S->lv[0];
    k_skm_close_chunks<<<(unsigned)(((uint64_t)S->G * nd1 + 255) / 256), 256, 0, st>>>(S->save.p, (uint64_t)S->G * nd1, S->cap, S->buf.p);
    skm_shared pre; pre.lo = 0; pre.hi = (uint32_t)nd1;
    MF_TRY(pre.pstart.alloc(ctx, (size_t)nd1)); MF_TRY(pre.plen.alloc(ctx, (size_t)nd1)); MF_TRY(pre.pocc.alloc(ctx, (size_t)nd1));
    k_skm_dir_dyn<<<(nd1 + 255) / 256, 256, 0, st>>>(S->rstart.p, S->gcur.p, nd1, pre.pstart.p, pre.plen.p);
    unsigned long long ovf = 0;
    pre.h_pstart.resize((size_t)nd1);
    MF_HIP(hipMemcpyAsync(&ovf, &S->scal.p[5], 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipMemcpyAsync(pre.h_pstart.data(), pre.pstart.p, (size_t)nd1 * 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    if (ovf) {
        if (ctx->opt_verbose) fprintf(stderr, "[mf] skm (streamed): a digit region sized from the sample was too small\n");
        return MF_SKM_FALLBACK;
    }
    pre.buf.swap(S->buf); pre.cap = S->cap; pre.ready = true;
    S->gcur.reset(); S->save.reset(); S->rstart.reset();
    MF_HIP(hipMemsetAsync(S->scal.p, 0, S->scal.bytes(), st));
    const int rc = skm_run<K>(ctx, nullptr, n_bases, nullptr, (n_bases + 31) / 32, n_occ, S->lv, S->adaptive, S->table_bits, S->scal.p, thr, n_all, out, &pre);
    return skm_cut_above(rc, thr, out);
}
template <int K, typename... A> static int skm_stream_begin_if(A &&... a) {
    if constexpr (K - mf_skm_m(K) + 1 >= 3 && K - mf_skm_m(K) + 1 <= 17) return skm_stream_begin<K>(std::forward<A>(a)...); else return MF_SKM_FALLBACK;
}
template <int K, typename... A> static int skm_stream_piece_if(A &&... a) {
    if constexpr (K - mf_skm_m(K) + 1 >= 3 && K - mf_skm_m(K) + 1 <= 17) return skm_stream_piece<K>(std::forward<A>(a)...); else return MF_SKM_FALLBACK;
}
template <int K, typename... A> static int skm_stream_finish_if(A &&... a) {
    if constexpr (K - mf_skm_m(K) + 1 >= 3 && K - mf_skm_m(K) + 1 <= 17) return skm_stream_finish<K>(std::forward<A>(a)...); else return MF_SKM_FALLBACK;
}
#ifndef MF_SKM_ONLY_K31
#define SKM_STREAM_SWITCH(FN, ...) switch (S->k) { \
        case 20: return FN<20>(__VA_ARGS__); case 21: return FN<21>(__VA_ARGS__); case 22: return FN<22>(__VA_ARGS__); case 23: return FN<23>(__VA_ARGS__); \
        case 24: return FN<24>(__VA_ARGS__); case 25: return FN<25>(__VA_ARGS__); case 26: return FN<26>(__VA_ARGS__); case 27: return FN<27>(__VA_ARGS__); \
        case 28: return FN<28>(__VA_ARGS__); case 29: return FN<29>(__VA_ARGS__); case 30: return FN<30>(__VA_ARGS__); case 31: return FN<31>(__VA_ARGS__); \
        default: return MF_SKM_FALLBACK; }
#else
#define SKM_STREAM_SWITCH(FN, ...) switch (S->k) { case 31: return FN<31>(__VA_ARGS__); default: return MF_SKM_FALLBACK; }
#endif
// lv / adaptive / table_bits: the counting plan (mf_count_plan) made from an ESTIMATE of the occurrences; MF_SKM_FALLBACK: not this way
int mf_skm_stream_begin(mf_ctx *ctx, int k, const std::vector<int> &lv, bool adaptive, int table_bits, const uint8_t *s_bases, uint64_t s_nbases,
                        const uint32_t *s_vmask, uint64_t s_nwords, double scale, mf_skm_stream **out) {
    *out = nullptr;
    if (!ctx->opt_skm || k < MF_SKM_MIN_K || k > 31 || ctx->own_world > 1) return MF_SKM_FALLBACK;
    std::unique_ptr<mf_skm_stream> U(new mf_skm_stream());
    mf_skm_stream *S = U.get();
    S->ctx = ctx; S->k = k; S->lv = lv; S->adaptive = adaptive; S->table_bits = table_bits;
    auto go = [&]() -> int { SKM_STREAM_SWITCH(skm_stream_begin_if, S, s_bases, s_nbases, s_vmask, s_nwords, scale) };
    const int rc = go();
    if (rc == MF_OK) *out = U.release();
    return rc;
}
int mf_skm_stream_piece(mf_skm_stream *S, const uint8_t *d_bases, uint64_t n_bases, const uint32_t *vmask, uint64_t n_words) {
    SKM_STREAM_SWITCH(skm_stream_piece_if, S, d_bases, n_bases, vmask, n_words)
}
int mf_skm_stream_finish(mf_skm_stream *S, uint64_t n_occ, uint64_t n_bases, int thr, uint64_t *n_all, mf_table **out) {
    SKM_STREAM_SWITCH(skm_stream_finish_if, S, n_occ, n_bases, thr, n_all, out)
}
void mf_skm_stream_free(mf_skm_stream *S) { delete S; }

// adaptive: the plan was made from the number of occurrences alone -- the levels after the first may be re-planned from a pilot
// table_bits: partition bits the caller wants the TABLE to have (0: one more than the counting plan's)
int mf_count_skm(mf_ctx *ctx, const uint8_t *d_bases, uint64_t n_bases, const uint32_t *vmask, uint64_t n_words, uint64_t n_occ,
                 int k, const std::vector<int> &lv, bool adaptive, int table_bits, unsigned long long *scal, int thr, uint64_t *n_all, mf_table **out) {
    int rc = MF_SKM_FALLBACK;
    switch (k) {
#define SKM_CASE(KK) case KK: rc = skm_run_if<KK>(ctx, d_bases, n_bases, vmask, n_words, n_occ, lv, adaptive, table_bits, scal, thr, n_all, out); break;
#ifndef MF_SKM_ONLY_K31              /* (a quick look at one instantiation's code: hipcc -DMF_SKM_ONLY_K31 -S) */
        SKM_CASE(20) SKM_CASE(21) SKM_CASE(22) SKM_CASE(23) SKM_CASE(24) SKM_CASE(25)
        SKM_CASE(26) SKM_CASE(27) SKM_CASE(28) SKM_CASE(29) SKM_CASE(30)
#endif
        SKM_CASE(31)
#undef SKM_CASE
        default: return MF_SKM_FALLBACK;
    }
    return skm_cut_above(rc, thr, out);
}

// =============================================================================================
// Debugging aid of tests/test_skm_records_gpu.py (not part of the C-ABI): the records of a counting run as they stand in front of k_skm_count.
// The call is mf_count_device's own (mask, plan, S1, S2, the pilot, every S3 level: mf_count_core with the context's options) with ctx->skm_snap set, which makes
// skm_slice copy its record buffer and directory to the host where count + gather would start, and end there.  A call that would not take this path
// (k < MF_SKM_MIN_K, option skm = 0, an input the path hands back) is an error.
//   mf_debug_skm_records  -> *out: the snapshot (mf_debug_skm_free)
//   mf_debug_skm_info     slice < 0: info[0] = number of slices; else info[0..10) = cap, partitions, dlo, dhi, G, words per block, one-pass level 1 (0 / 1),
//                         level 1 repeated with exact ranges after an overflow, the valid-record counter (scal[6]), number of levels; info[10..18) = the
//                         levels' bits; info[18] = FAST form of the scatter (0 / 1); info[19] = partitions of the slice's level 1
//   mf_debug_skm_copy     rec[2 cap] (x, y of every record), pstart / plen / pocc [partitions], l1_pstart / l1_plen [level-1 partitions]; null: not wanted
// =============================================================================================
int mf_count_core(mf_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases, int k, int min_len, mf_table **out, int thr,
                  uint64_t *n_all);
extern "C" void mf_debug_skm_free(mf_skm_snap *s) { delete s; }
extern "C" int mf_debug_skm_records(mf_ctx *ctx, const void *d_bases, const void *d_offsets, uint64_t n_reads, uint64_t n_bases, int k, int min_len, mf_skm_snap **out) {
    if (!ctx || !out) return mf_set_error("mf_debug_skm_records: NULL argument");
    *out = nullptr;
    if (k < MF_SKM_MIN_K || k > 31 || !ctx->opt_skm)
        return mf_set_error("mf_debug_skm_records: k = %d, option skm = %d: the call would not take the super-k-mer path", k, (int)ctx->opt_skm);
    std::unique_ptr<mf_skm_snap> S(new mf_skm_snap());
    mf_table *t = nullptr;
    ctx->skm_snap = S.get();
    const int rc = mf_count_core(ctx, (const uint8_t *)d_bases, (const uint64_t *)d_offsets, n_reads, n_bases, k, min_len, &t, -1, nullptr);
    ctx->skm_snap = nullptr;
    if (rc < 0) return rc;
    if (rc != MF_SKM_SNAPPED) {
        const bool empty = t && t->n_occ == 0;
        if (t) mf_table_destroy(t);
        if (!empty) return mf_set_error("mf_debug_skm_records: the input did not go through the super-k-mer path");
        S->slices.clear();                                 // (no k-mer occurrence at all: no records)
    }
    *out = S.release();
    return MF_OK;
}
extern "C" int mf_debug_skm_info(const mf_skm_snap *s, int slice, uint64_t *info) {
    if (!s || !info) return mf_set_error("mf_debug_skm_info: NULL argument");
    if (slice < 0) { info[0] = s->slices.size(); return MF_OK; }
    if ((size_t)slice >= s->slices.size()) return mf_set_error("mf_debug_skm_info: slice %d of %zu", slice, s->slices.size());
    const skm_snap_slice &x = s->slices[(size_t)slice];
    if (x.lv.size() > 8) return mf_set_error("mf_debug_skm_info: %zu levels", x.lv.size());
    const uint64_t v[10] = {x.cap, x.pstart.size(), x.dlo, x.dhi, (uint64_t)x.G, x.wpb, (uint64_t)x.one_pass, (uint64_t)x.repeated, x.n_valid, x.lv.size()};
    for (int i = 0; i < 10; i++) info[i] = v[i];
    for (size_t i = 0; i < 8; i++) info[10 + i] = i < x.lv.size() ? (uint64_t)x.lv[i] : 0;
    info[18] = (uint64_t)x.fast; info[19] = x.l1_pstart.size();
    return MF_OK;
}
extern "C" int mf_debug_skm_copy(const mf_skm_snap *s, int slice, uint64_t *rec, uint64_t *pstart, uint32_t *plen, uint32_t *pocc, uint64_t *l1_pstart, uint32_t *l1_plen) {
    if (!s || slice < 0 || (size_t)slice >= s->slices.size()) return mf_set_error("mf_debug_skm_copy: no such slice");
    const skm_snap_slice &x = s->slices[(size_t)slice];
    if (rec) std::copy(x.rec.begin(), x.rec.end(), rec);
    if (pstart) std::copy(x.pstart.begin(), x.pstart.end(), pstart);
    if (plen) std::copy(x.plen.begin(), x.plen.end(), plen);
    if (pocc) std::copy(x.pocc.begin(), x.pocc.end(), pocc);
    if (l1_pstart) std::copy(x.l1_pstart.begin(), x.l1_pstart.end(), l1_pstart);
    if (l1_plen) std::copy(x.l1_plen.begin(), x.l1_plen.end(), l1_plen);
    return MF_OK;
}

// =============================================================================================
// Debugging aid of tests/test_skm_count_units_gpu.py (not part of the C-ABI; host code only, no kernel of its own): S4 on records the test supplies.
// The record buffer and the directory come from the host, the launches are skm_count_batches' own (k_skm_count<K> with C2_LDS dynamic LDS through
// skm_set_lds, the units split into batches by the same rule, a scan of the batch's dcount, k_gather_split for 2 table partitions per unit and
// k_gather_split_n otherwise), and everything the stage writes goes back to the host.
//   mf_debug_skm_count       rec[2 n_rec] (x, y of every record), pstart / plen [np]; k 20 .. 31; thr -1 .. C2_LH - 1; dedupe: the option's raw value; dyn 1: as
//                            skm_count_batches launches it (a unit counter, drop_hist when thr >= 0), 0: as skm_pilot does (neither); grid 1 .. 2 CUs; n_batches >= 1;
//                            room[np] or null: entries a unit's slice of the lists takes (null: its occurrences / (thr + 1), k_skm_cap); split_bits < 0: no gather,
//                            else 0 .. 4 table partitions bits per unit, from bit `bit` of the partition hash.
//                            A directory that is not well formed is refused before anything is allocated or launched: regions ascending, disjoint, inside the buffer,
//                            plen a multiple of 4; a record with n = 63 is all ones; any other has 1 <= n <= RMAX and zero bits behind its last base.
//                            The lists are allocated at the units' occurrences (>= the sum of `room`) and filled with 0xA5 before every batch: what a unit
//                            writes beyond its room stays inside them and shows.  A batch that raises `overflow` is the last one, and nothing is gathered.
//   mf_debug_skm_count_info  info[0..10) = np, length of the lists, overflow, n_all, n_redo (summed over the batches), gathered (0 / 1), entries of dk / dc, length of
//                            dfine, batches launched, CUs of the device
//   mf_debug_skm_count_copy  dcount [np] (0xFFFFFFFF: never written), toff [np + 1], tkeys / tcnt [length of the lists]: unit p's slice starts at toff[p]
//                            (a batch's lists as the batch left them; behind the last unit, up to the end of the allocation, the last batch's), drop_hist [C2_LH]
//                            (dyn = 1 and thr >= 0, else zeros), dk / dc, dfine [(np << split_bits) + 1]; null: not wanted
// =============================================================================================
struct mf_skm_count_dbg {
    std::vector<uint32_t> dcount; std::vector<uint64_t> toff, tkeys, drop_hist, dk, dfine; std::vector<uint16_t> tcnt, dc;
    uint64_t overflow = 0, n_all = 0, n_redo = 0, gathered = 0, launches = 0, n_cu = 0;
};
// the directory and the records of its regions, as k_skm_count takes them for granted; occ[p]: the k-mers of unit p
static int skm_debug_check_units(const uint64_t *rec, uint64_t n_rec, const uint64_t *pstart, const uint32_t *plen, uint32_t np, int k, std::vector<uint32_t> &occ) {
    const uint32_t rmax = (uint32_t)std::min(MF_SKM_BASES - (k - 1), 20);
    uint64_t end = 0;
    occ.assign(np, 0);
    for (uint32_t p = 0; p < np; p++) {
        if (plen[p] % 4u) return mf_set_error("mf_debug_skm_count: plen[%u] = %u is not a multiple of 4", p, plen[p]);
        if (pstart[p] < end) return mf_set_error("mf_debug_skm_count: region %u starts at %llu, inside or in front of the region before it (which ends at %llu)", p, (unsigned long long)pstart[p], (unsigned long long)end);
        if (pstart[p] > n_rec || plen[p] > n_rec - pstart[p]) return mf_set_error("mf_debug_skm_count: region %u = [%llu, + %u) leaves the buffer of %llu records", p, (unsigned long long)pstart[p], plen[p], (unsigned long long)n_rec);
        end = pstart[p] + plen[p];
        uint64_t o = 0;
        for (uint64_t j = pstart[p]; j < end; j++) {
            const uint64_t x = rec[2 * j], y = rec[2 * j + 1];
            const uint32_t n = (uint32_t)y & 63u;
            if (x == ~0ull && y == ~0ull) continue;
            if (n < 1u || n > rmax) return mf_set_error("mf_debug_skm_count: record %llu of region %u has n = %u (1 .. %u, or an all-ones sentinel)", (unsigned long long)j, p, n, rmax);
            const int nb = (int)n + k - 1;                                       // bases: 0 .. 31 in x, 32 .. 49 in the top 36 bits of y
            const uint64_t jx = nb >= 32 ? 0ull : x & ((1ull << (64 - 2 * nb)) - 1ull);
            const uint64_t jy = (nb <= 32 ? y : y & ((1ull << (64 - 2 * (nb - 32))) - 1ull)) & ~((1ull << 28) - 1ull);
            if (jx || jy) return mf_set_error("mf_debug_skm_count: record %llu of region %u has bits set behind its last base (%d bases)", (unsigned long long)j, p, nb);
            o += n;
        }
        if (o > 0xFFFFFFFFull) return mf_set_error("mf_debug_skm_count: region %u holds %llu k-mers", p, (unsigned long long)o);
        occ[p] = (uint32_t)o;
    }
    return MF_OK;
}
template <int K>
static int skm_debug_count(mf_ctx *ctx, const uint64_t *rec, uint64_t n_rec, const uint64_t *pstart, const uint32_t *plen, uint32_t np, int thr, uint32_t dedupe, int dyn,
                           unsigned grid, uint32_t nbatch, const std::vector<uint64_t> &h_toff, uint64_t t_alloc, int S, int bit, mf_skm_count_dbg &D) {
    hipStream_t st = ctx->stream;
    MF_TRY(skm_set_lds(k_skm_count<K>, C2_LDS));
    mf_buf<skm_rec> buf; MF_TRY(buf.alloc(ctx, n_rec + 4));
    mf_buf<uint64_t> ps, toff, coff, tkeys, dk, dfine; mf_buf<uint32_t> pl, dcount; mf_buf<uint16_t> tcnt, dc; mf_buf<unsigned long long> scal, dhist, c2p;
    MF_TRY(ps.alloc(ctx, np)); MF_TRY(pl.alloc(ctx, np)); MF_TRY(toff.alloc(ctx, (size_t)np + 1)); MF_TRY(coff.alloc(ctx, (size_t)np + 1)); MF_TRY(dcount.alloc(ctx, np));
    MF_TRY(tkeys.alloc(ctx, t_alloc)); MF_TRY(tcnt.alloc(ctx, t_alloc));
    MF_TRY(scal.alloc(ctx, 16)); MF_TRY(c2p.alloc(ctx, 16)); MF_TRY(dhist.alloc(ctx, (size_t)MF_MAX_COUNT + 1));
    const uint64_t d_alloc = h_toff[np];                                          // (no overflow: dcount[p] <= the room of p)
    if (S >= 0) { MF_TRY(dk.alloc(ctx, d_alloc)); MF_TRY(dc.alloc(ctx, d_alloc)); MF_TRY(dfine.alloc(ctx, ((size_t)np << S) + 1)); }
    MF_HIP(hipMemsetAsync(buf.p, 0xFF, (n_rec + 4) * sizeof(skm_rec), st));        // padding = sentinels
    if (n_rec) MF_HIP(hipMemcpyAsync(buf.p, rec, n_rec * sizeof(skm_rec), hipMemcpyHostToDevice, st));
    MF_HIP(hipMemcpyAsync(ps.p, pstart, (size_t)np * 8, hipMemcpyHostToDevice, st));
    MF_HIP(hipMemcpyAsync(pl.p, plen, (size_t)np * 4, hipMemcpyHostToDevice, st));
    MF_HIP(hipMemcpyAsync(toff.p, h_toff.data(), ((size_t)np + 1) * 8, hipMemcpyHostToDevice, st));
    MF_HIP(hipMemsetAsync(dcount.p, 0xFF, (size_t)np * 4, st));
    MF_HIP(hipMemsetAsync(scal.p, 0, 16 * 8, st)); MF_HIP(hipMemsetAsync(c2p.p, 0, 16 * 8, st)); MF_HIP(hipMemsetAsync(dhist.p, 0, dhist.bytes(), st));
    if (S >= 0) MF_HIP(hipMemsetAsync(dfine.p, 0xFF, dfine.bytes(), st));
    // the batches of skm_count_batches
    const uint32_t PB = (np + nbatch - 1) / nbatch;
    std::vector<uint64_t> tb(nbatch + 1);
    for (uint32_t b = 0; b <= nbatch; b++) tb[b] = h_toff[std::min<uint64_t>((uint64_t)b * PB, np)];
    uint64_t tmax = 0;
    for (uint32_t b = 0; b < nbatch; b++) tmax = std::max(tmax, tb[b + 1] - tb[b]);
    D.tkeys.assign(t_alloc, 0xA5A5A5A5A5A5A5A5ull); D.tcnt.assign(t_alloc, (uint16_t)0xA5A5);
    uint64_t dused = 0;
    for (uint32_t b = 0; b < nbatch; b++) {
        const uint32_t p0 = (uint32_t)std::min<uint64_t>((uint64_t)b * PB, np), p1 = (uint32_t)std::min<uint64_t>((uint64_t)(b + 1) * PB, np);
        if (p0 == p1) continue;
        MF_HIP(hipMemsetAsync(tkeys.p, 0xA5, t_alloc * 8, st)); MF_HIP(hipMemsetAsync(tcnt.p, 0xA5, t_alloc * 2, st));
        MF_HIP(hipMemsetAsync(&scal.p[8], 0, 16, st));                           // ([8] units redone, [9] the unit counter)
        {
            const unsigned g = std::min<unsigned>(grid, p1 - p0);
            mf_ktimer t(ctx, "k_skm_count");
            k_skm_count<K><<<g, SKM_CT, C2_LDS, st>>>(buf.p, ps.p, pl.p, p1, toff.p, tkeys.p, tcnt.p, dcount.p, (unsigned int *)&scal.p[2], p0, (uint64_t)tb[b], thr, &scal.p[7],
                                                      (unsigned int *)&scal.p[8], dyn && thr >= 0 ? dhist.p : nullptr, c2p.p, (uint64_t)tmax, dedupe, dyn ? (unsigned int *)&scal.p[9] : nullptr);
        }
        D.launches++;
        MF_TRY(mf_scan<1>(ctx, dcount.p + p0, coff.p + p0, p1 - p0, (uint64_t *)&scal.p[3]));
        unsigned long long res[2], nr = 0;
        MF_HIP(hipMemcpyAsync(res, &scal.p[2], 16, hipMemcpyDeviceToHost, st));
        MF_HIP(hipMemcpyAsync(&nr, &scal.p[8], 8, hipMemcpyDeviceToHost, st));
        // this batch's lists: its units' slices, and (the last batch) what lies behind them
        const uint64_t span = p1 == np ? t_alloc - tb[b] : tb[b + 1] - tb[b];
        if (span) {
            MF_HIP(hipMemcpyAsync(D.tkeys.data() + tb[b], tkeys.p, span * 8, hipMemcpyDeviceToHost, st));
            MF_HIP(hipMemcpyAsync(D.tcnt.data() + tb[b], tcnt.p, span * 2, hipMemcpyDeviceToHost, st));
        }
        MF_HIP(hipStreamSynchronize(st));
        MF_HIP(hipGetLastError());
        D.n_redo += nr & 0xFFFFFFFFull;
        if (res[0]) { D.overflow = res[0] & 0xFFFFFFFFull; break; }
        if (S < 0) continue;
        const uint64_t d_b = res[1];
        if (dused + d_b > d_alloc) return mf_set_error("mf_debug_skm_count: batch %u keeps %llu entries, its units' rooms add up to less", b, (unsigned long long)d_b);
        {
            const unsigned g = (unsigned)std::min<uint64_t>(((uint64_t)(p1 - p0) + 3) / 4, (uint64_t)ctx->n_cu * 32);
            mf_ktimer t(ctx, "k_gather");
            if (S == 1)
                k_gather_split<K><<<g, 256, 0, st>>>(tkeys.p, tcnt.p, toff.p, dcount.p, coff.p, p1, dk.p + dused, dc.p + dused, p0, (uint64_t)tb[b], dfine.p, dused, bit);
            else
                k_gather_split_n<K><<<g, 256, 0, st>>>(tkeys.p, tcnt.p, toff.p, dcount.p, coff.p, p1, dk.p + dused, dc.p + dused, p0, (uint64_t)tb[b], dfine.p, dused, bit, S);
        }
        dused += d_b;
        if (p1 == np) D.gathered = 1;
    }
    D.dcount.resize(np); D.drop_hist.assign(C2_LH, 0);
    unsigned long long na = 0;
    MF_HIP(hipMemcpyAsync(D.dcount.data(), dcount.p, (size_t)np * 4, hipMemcpyDeviceToHost, st));
    MF_HIP(hipMemcpyAsync(D.drop_hist.data(), dhist.p, (size_t)C2_LH * 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipMemcpyAsync(&na, &scal.p[7], 8, hipMemcpyDeviceToHost, st));
    if (D.gathered) {
        D.dk.resize(dused); D.dc.resize(dused); D.dfine.resize(((size_t)np << S) + 1);
        if (dused) { MF_HIP(hipMemcpyAsync(D.dk.data(), dk.p, dused * 8, hipMemcpyDeviceToHost, st)); MF_HIP(hipMemcpyAsync(D.dc.data(), dc.p, dused * 2, hipMemcpyDeviceToHost, st)); }
        MF_HIP(hipMemcpyAsync(D.dfine.data(), dfine.p, D.dfine.size() * 8, hipMemcpyDeviceToHost, st));
    }
    MF_HIP(hipStreamSynchronize(st));
    MF_HIP(hipGetLastError());
    D.n_all = na;
    return MF_OK;
}
extern "C" void mf_debug_skm_count_free(mf_skm_count_dbg *d) { delete d; }
extern "C" int mf_debug_skm_count(mf_ctx *ctx, const uint64_t *rec, uint64_t n_rec, const uint64_t *pstart, const uint32_t *plen, uint32_t np, int k, int thr, int dedupe, int dyn,
                                  int grid, int n_batches, const uint32_t *room, int split_bits, int bit, mf_skm_count_dbg **out) {
    if (!ctx || !out || !pstart || !plen || (n_rec && !rec)) return mf_set_error("mf_debug_skm_count: NULL argument");
    *out = nullptr;
    if (k < MF_SKM_MIN_K || k > 31) return mf_set_error("mf_debug_skm_count: k = %d (%d .. 31)", k, MF_SKM_MIN_K);
    if (thr < -1 || thr >= C2_LH) return mf_set_error("mf_debug_skm_count: thr = %d (-1 .. %d: a higher cut is made after the kernel)", thr, C2_LH - 1);
    if (dedupe < 0 || (dyn != 0 && dyn != 1)) return mf_set_error("mf_debug_skm_count: dedupe = %d, dyn = %d", dedupe, dyn);
    if (grid < 1 || grid > ctx->n_cu * C2_WG_PER_CU) return mf_set_error("mf_debug_skm_count: grid = %d (1 .. %d)", grid, ctx->n_cu * C2_WG_PER_CU);
    if (n_batches < 1) return mf_set_error("mf_debug_skm_count: n_batches = %d", n_batches);
    if (np < 1 || np > (1u << 20) || n_rec > (1ull << 24)) return mf_set_error("mf_debug_skm_count: %u units, %llu records (1 .. 2^20 units, at most 2^24 records)", np, (unsigned long long)n_rec);
    if (split_bits > 4 || (split_bits >= 0 && (bit < 0 || bit > 31 || bit + split_bits > 32))) return mf_set_error("mf_debug_skm_count: split_bits = %d from bit %d", split_bits, bit);
    std::vector<uint32_t> occ;
    MF_TRY(skm_debug_check_units(rec, n_rec, pstart, plen, np, k, occ));
    std::vector<uint64_t> toff((size_t)np + 1, 0);
    uint64_t t_alloc = 0;                                     // (a unit that ran past its room would still end in front of its slice's start + its occurrences)
    for (uint32_t p = 0; p < np; p++) {
        const uint32_t r = room ? room[p] : occ[p] / (thr >= 0 ? (uint32_t)thr + 1u : 1u);
        toff[p + 1] = toff[p] + r; t_alloc += std::max(r, occ[p]);
    }
    std::unique_ptr<mf_skm_count_dbg> D(new mf_skm_count_dbg());
    D->toff = toff; D->n_cu = (uint64_t)ctx->n_cu;
    const uint32_t nbatch = (uint32_t)std::min<int64_t>(n_batches, np);
    int rc = MF_ERR;
    switch (k) {
#define SKM_CASE(KK) case KK: rc = skm_debug_count<KK>(ctx, rec, n_rec, pstart, plen, np, thr, (uint32_t)dedupe, dyn, (unsigned)grid, nbatch, toff, t_alloc, split_bits, bit, *D); break;
#ifndef MF_SKM_ONLY_K31
        SKM_CASE(20) SKM_CASE(21) SKM_CASE(22) SKM_CASE(23) SKM_CASE(24) SKM_CASE(25)
        SKM_CASE(26) SKM_CASE(27) SKM_CASE(28) SKM_CASE(29) SKM_CASE(30)
#endif
        SKM_CASE(31)
#undef SKM_CASE
        default: return mf_set_error("mf_debug_skm_count: k = %d is not compiled in", k);
    }
    if (rc < 0) return rc;
    *out = D.release();
    return MF_OK;
}
extern "C" int mf_debug_skm_count_info(const mf_skm_count_dbg *d, uint64_t *info) {
    if (!d || !info) return mf_set_error("mf_debug_skm_count_info: NULL argument");
    const uint64_t v[10] = {d->dcount.size(), d->tkeys.size(), d->overflow, d->n_all, d->n_redo, d->gathered, d->dk.size(), d->dfine.size(), d->launches, d->n_cu};
    for (int i = 0; i < 10; i++) info[i] = v[i];
    return MF_OK;
}
extern "C" int mf_debug_skm_count_copy(const mf_skm_count_dbg *d, uint32_t *dcount, uint64_t *toff, uint64_t *tkeys, uint16_t *tcnt, uint64_t *drop_hist, uint64_t *dk, uint16_t *dc,
                                       uint64_t *dfine) {
    if (!d) return mf_set_error("mf_debug_skm_count_copy: NULL argument");
    if (dcount) std::copy(d->dcount.begin(), d->dcount.end(), dcount);
    if (toff) std::copy(d->toff.begin(), d->toff.end(), toff);
    if (tkeys) std::copy(d->tkeys.begin(), d->tkeys.end(), tkeys);
    if (tcnt) std::copy(d->tcnt.begin(), d->tcnt.end(), tcnt);
    if (drop_hist) std::copy(d->drop_hist.begin(), d->drop_hist.end(), drop_hist);
    if (dk) std::copy(d->dk.begin(), d->dk.end(), dk);
    if (dc) std::copy(d->dc.begin(), d->dc.end(), dc);
    if (dfine) std::copy(d->dfine.begin(), d->dfine.end(), dfine);
    return MF_OK;
}
