// mf_wfeatures.hip -- NO-REFERENCE EXTENSION (32 <= k <= 63): features-calculator on wide components, all three inputs of the reference's tool.
// The definitions are those of the k <= 31 entry points (mf_cc.hip: mf_features_device_selected, mf_features_reads_device_selected) word for
// word on 2k-bit canonical k-mers; the checker is the test suite's CPU restatement compiled for 128-bit keys:
//   hm        every member k-mer of every component once, value 0
//   k-mers    the sample table's count is the value (k_w_features: a thread per LISTING probes the sample's index)
//   reads     every position of every read of >= k bases whose canonical k-mer is in hm adds 1 to it: 64-bit, no saturation
//   result    per component over its member LISTINGS (a k-mer listed by two components is read once per listing); with a selected table only
//             the listings whose k-mer has a value > 0 there take part -- in the sum, in found and in the denominator (0.0 / 0.0 = NaN)
// The reads branch in three launches:
//   k_wf_index     insert-or-find of ALL listings into an index of 8-byte slots (position | tag, load <= 0.5, hashed by mf_whash_key: the layout
//                  mf_windex_find probes).  mf_windex_build assumes distinct keys; a components.bin of seq2comp lists a shared k-mer several
//                  times.  A lane claims an empty slot with one 64-bit CAS; a lane that meets an occupied slot with its own tag compares both
//                  words with the occupant's listing (hi[] / lo[] are input, never written) and on equality records rep[j] = occupant, else
//                  probes on.  The only transition of a slot is empty -> listing, so a value read as occupied IS the occupant, and a stale
//                  "empty" is corrected by the CAS's return value.  No lane waits for another; every probe ends at an empty slot.  Which of
//                  several equal listings wins does not matter: the occurrences live at occ[rep] and every listing reads them there.
//   k_wf_presence  one thread per run of WF_RUN positions of ONE read (the launch shape of k_ws2c_pairs / k_cp_mark: the read by binary search
//                  in the scanned runs per read), ws2c_roll for the canonical k-mers, mf_windex_find, atomicAdd(&occ[idx], 1) on a hit.  A run
//                  reads exactly its count + k - 1 bases: never a byte outside its read.
//   k_wf_occ       k_features_occ of mf_cc.hip reading occ[rep[j]]: wave-level sum where a wave sits in one component.
#include "mf_wide.h"
#include "mf_roll.h"
#include <algorithm>
#include <memory>

#ifndef WF_RUN
#define WF_RUN 32                     // positions per thread of k_wf_presence (a run decodes k - 1 lead-in bases on top of them: DESIGN 7)
#endif
int mf_wf_run() { return WF_RUN; }

#define WF_NONE 0xFFFFFFFFu

// ---- the member index with duplicates ----
__global__ __launch_bounds__(256) void k_wf_index(unsigned long long *__restrict__ slots, uint64_t mask, const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo,
                                                  uint64_t n, int k, uint32_t *__restrict__ rep) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t mh = hi[j], ml = lo[j];
    const uint64_t h = mf_whash_key(((mf_u128)mh << 64) | (mf_u128)ml, k);
    const uint32_t tag = (uint32_t)(h >> 32);
    const unsigned long long ent = (h & 0xFFFFFFFF00000000ull) | (unsigned long long)(uint32_t)j;      // (j < 2^32 - 1: never MF_WIDX_EMPTY)
    uint64_t s = h & mask;
    for (;;) {
        unsigned long long v = slots[s];
        if (v == MF_WIDX_EMPTY) {
            v = atomicCAS(&slots[s], MF_WIDX_EMPTY, ent);
            if (v == MF_WIDX_EMPTY) { rep[j] = (uint32_t)j; return; }
        }
        if ((uint32_t)(v >> 32) == tag) {                  // v: the listing that holds the slot, for good
            const uint32_t p = (uint32_t)v;
            if (lo[p] == ml && hi[p] == mh) { rep[j] = p; return; }
        }
        s = (s + 1) & mask;
    }
}

// ---- presence ----
// runs[i] = the threads read i takes: ceil(max(0, len - k + 1) / WF_RUN); offsets that go backwards or a read of 2^31 or more k-mers raise *bad
__global__ void k_wf_sizes(const uint64_t *__restrict__ off, uint64_t n, int k, uint32_t *__restrict__ runs, unsigned int *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = off[i], b = off[i + 1];
    uint64_t ni = 0;
    if (b < a) atomicOr(bad, 1u);
    else if (b - a >= (uint64_t)k) ni = b - a - (uint64_t)k + 1;
    if (ni >= 0x80000000ull) { atomicOr(bad, 1u); ni = 0; }
    runs[i] = (uint32_t)((ni + WF_RUN - 1) / WF_RUN);
}
// (mf_scan sums a tile in 32 bits: above one workgroup's worth the run counts are scanned as two 16-bit halves, as cp_scan of mf_comppaths.hip)
__global__ void k_wf_split(const uint32_t *__restrict__ in, uint64_t n, uint32_t *__restrict__ lo, uint32_t *__restrict__ hi) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const uint32_t v = in[i]; lo[i] = v & 0xFFFFu; hi[i] = v >> 16; }
}
__global__ void k_wf_join(const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi, uint64_t n1, uint64_t *__restrict__ out, uint64_t *__restrict__ total) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n1) return;
    const uint64_t v = lo[i] + (hi[i] << 16);
    out[i] = v;
    if (i == n1 - 1) *total = v;
}
// thread r: its run of WF_RUN positions belongs to the last read s with srun[s] <= r (reads without positions take no run: they are skipped)
__global__ __launch_bounds__(256) void k_wf_presence(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ off, const uint64_t *__restrict__ srun, uint64_t n_reads,
                                                     uint64_t n_runs, int k, mf_windex_view ix, unsigned long long *__restrict__ occ) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs) return;
    uint64_t a = 0, b = n_reads;
    while (b - a > 1u) { const uint64_t m = a + (b - a) / 2u; if (srun[m] <= r) a = m; else b = m; }
    const uint64_t o = off[a];
    const uint64_t ni = off[a + 1] - o - (uint64_t)k + 1u, p0 = (r - srun[a]) * WF_RUN;          // (p0 < ni: the read has ceil(ni / WF_RUN) runs)
    const uint32_t count = (uint32_t)(ni - p0 < WF_RUN ? ni - p0 : WF_RUN);
    ws2c_roll(bases + o + p0, count, k, [&](uint32_t, uint64_t h, uint64_t l) {
        const uint32_t idx = mf_windex_find(ix, h, l);
        if (idx != WF_NONE) atomicAdd(&occ[idx], 1ull);
    });
}

// ---- selection and reduction: k_features_select / k_features_occ / k_features_rev of mf_cc.hip on two words ----
// sel[j] = 1 iff listing j's k-mer has a value > 0 in the selected table; selcnt[c] = such listings of component c (the breadth's denominator)
__global__ __launch_bounds__(256) void k_wf_select(mf_windex_view ix, const uint64_t *__restrict__ chi, const uint64_t *__restrict__ clo, const uint32_t *__restrict__ comp_of,
                                                   uint64_t nk, uint8_t *__restrict__ sel, unsigned int *__restrict__ selcnt) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t comp = 0xFFFFFFFFu, hit = 0;
    if (j < nk) {
        comp = comp_of[j];
        const uint32_t p = mf_windex_find(ix, chi[j], clo[j]);
        hit = p != WF_NONE && ix.cnt[p] > 0;
        sel[j] = (uint8_t)hit;
    }
    const uint32_t first = __shfl(comp, 0, 64);
    if (__ballot(comp != first) == 0ull) {
        const uint32_t tot = (uint32_t)__popcll(__ballot(hit != 0));
        if (mf_lane() == 0 && tot) atomicAdd(&selcnt[first], tot);
    } else if (hit) atomicAdd(&selcnt[comp], 1u);
}
// reads branch: the occurrences of listing j's k-mer stand at occ[rep[j]]
__global__ __launch_bounds__(256) void k_wf_occ(const unsigned long long *__restrict__ occ, const uint32_t *__restrict__ rep, const uint32_t *__restrict__ comp_of, uint64_t nk,
                                                int threshold, const uint8_t *__restrict__ sel, unsigned long long *__restrict__ vec, unsigned int *__restrict__ found) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t comp = 0xFFFFFFFFu, hit = 0; unsigned long long val = 0;
    if (j < nk) {
        comp = comp_of[j];
        if (!sel || sel[j]) {
            const unsigned long long v = occ[rep[j]];
            if ((long long)v > (long long)threshold) { val = v; hit = 1; }
        }
    }
    const uint32_t first = __shfl(comp, 0, 64);
    if (__ballot(comp != first) == 0ull) {
        for (int d = 32; d >= 1; d >>= 1) { val += __shfl_down(val, d, 64); hit += __shfl_down(hit, d, 64); }
        if (mf_lane() == 0 && hit) { atomicAdd(&vec[first], val); atomicAdd(&found[first], hit); }
    } else if (hit) {
        atomicAdd(&vec[comp], val);
        atomicAdd(&found[comp], 1u);
    }
}
// k-mers branch: a thread per listing probes the sample's index (sel == nullptr: every listing takes part)
__global__ __launch_bounds__(256) void k_w_features(mf_windex_view ix, const uint64_t *__restrict__ chi, const uint64_t *__restrict__ clo, const uint32_t *__restrict__ comp_of,
                                                    uint64_t nk, int threshold, const uint8_t *__restrict__ sel, unsigned long long *__restrict__ vec,
                                                    unsigned int *__restrict__ found) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t comp = 0xFFFFFFFFu, val = 0, hit = 0;
    if (j < nk) {
        comp = comp_of[j];
        if (!sel || sel[j]) {
            const uint32_t p = mf_windex_find(ix, chi[j], clo[j]);
            if (p != WF_NONE) { const uint32_t v = ix.cnt[p]; if ((int)v > threshold) { val = v; hit = 1; } }
        }
    }
    const uint32_t first = __shfl(comp, 0, 64);
    if (__ballot(comp != first) == 0ull) {
        for (int d = 32; d >= 1; d >>= 1) { val += __shfl_down(val, d, 64); hit += __shfl_down(hit, d, 64); }
        if (mf_lane() == 0 && hit) { atomicAdd(&vec[first], (unsigned long long)val); atomicAdd(&found[first], hit); }
    } else if (hit) {
        atomicAdd(&vec[comp], (unsigned long long)val);
        atomicAdd(&found[comp], 1u);
    }
}

static inline unsigned wf_grid(uint64_t n, unsigned bs = 256) { return (unsigned)((n + bs - 1) / bs); }

static int wf_check_k(const char *who, const char *narrow, int k) {
    if (k < 32 || k > 63) return mf_set_error("%s: 32 <= k <= 63 (k <= 31: %s)", who, narrow);
    return MF_OK;
}
// what every device form checks of its handles (vec and the reads' pointers: the callers)
static int wf_check(const char *who, const char *narrow, mf_ctx *ctx, const mf_wcomps *c, const mf_wtable *sample, const mf_wtable *selected) {
    if (c->ctx != ctx || (sample && sample->ctx != ctx) || (selected && selected->ctx != ctx)) return mf_set_error("%s: a handle belongs to another context", who);
    MF_TRY(wf_check_k(who, narrow, c->k));
    if (sample && sample->k != c->k) return mf_set_error("%s: components of %d-mers, sample of %d-mers", who, c->k, sample->k);
    if (selected && selected->k != c->k) return mf_set_error("%s: components of %d-mers, selected k-mers of %d-mers", who, c->k, selected->k);
    if (c->n_kmers >= 0xFFFFFFFFull) return mf_set_error("%s: %llu members (fewer than 2^32 - 1)", who, (unsigned long long)c->n_kmers);
    return MF_OK;
}
static int wf_scan(mf_ctx *ctx, const uint32_t *in, uint64_t *out, uint64_t n, uint64_t *total) {
    if (n <= 65536) return mf_scan<1>(ctx, in, out, n, total);               // (one workgroup, 64-bit sums)
    mf_buf<uint32_t> lo, hi; mf_buf<uint64_t> olo, ohi;
    MF_TRY(lo.alloc(ctx, n)); MF_TRY(hi.alloc(ctx, n)); MF_TRY(olo.alloc(ctx, n + 1)); MF_TRY(ohi.alloc(ctx, n + 1));
    k_wf_split<<<wf_grid(n), 256, 0, ctx->stream>>>(in, n, lo.p, hi.p);
    MF_TRY(mf_scan<1>(ctx, lo.p, olo.p, n, total));
    MF_TRY(mf_scan<1>(ctx, hi.p, ohi.p, n, total));
    k_wf_join<<<wf_grid(n + 1), 256, 0, ctx->stream>>>(olo.p, ohi.p, n + 1, out, total);
    MF_HIP(hipGetLastError());
    MF_HIP(hipStreamSynchronize(ctx->stream));             // (the halves go back to the arena)
    return MF_OK;
}
// the selection on the listings: mask per listing + count per component (host); selected == NULL: no mask
static int wf_selection(mf_ctx *ctx, mf_wcomps *c, mf_wtable *selected, mf_buf<uint8_t> &mask, std::vector<unsigned int> &selcnt) {
    if (!selected) return MF_OK;
    hipStream_t st = ctx->stream;
    mf_buf<unsigned int> dcnt;
    MF_TRY(mask.alloc(ctx, c->n_kmers)); MF_TRY(dcnt.alloc(ctx, c->n));
    MF_HIP(hipMemsetAsync(mask.p, 0, c->n_kmers ? c->n_kmers : 1, st));
    MF_HIP(hipMemsetAsync(dcnt.p, 0, c->n * 4, st));
    if (selected->n && c->n_kmers) {
        MF_TRY(mf_wtable_ensure_index(selected));
        mf_ktimer tm(ctx, "k_wf_select");
        k_wf_select<<<wf_grid(c->n_kmers), 256, 0, st>>>(mf_wtable_view(selected), c->hi.p, c->lo.p, c->comp.p, c->n_kmers, mask.p, dcnt.p);
    }
    MF_HIP(hipGetLastError());
    selcnt.resize(c->n);
    MF_HIP(hipMemcpyAsync(selcnt.data(), dcnt.p, c->n * 4, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    return MF_OK;
}
// vec and found to the host; breadth[i] = found / cnt as features_breadth of mf_cc.hip: cnt counts the selected listings only, a component
// without any gives 0.0 / 0.0 = NaN, and a negative threshold makes absent k-mers (value 0) count as found (value > threshold)
static int wf_finish(mf_ctx *ctx, const mf_wcomps *c, const unsigned long long *dvec, const unsigned int *dfound, const std::vector<unsigned int> *selcnt, int threshold,
                     int64_t *vec, double *breadth) {
    hipStream_t st = ctx->stream;
    const uint64_t nc = c->n;
    std::vector<unsigned int> hf(nc);
    MF_HIP(hipMemcpyAsync(vec, dvec, nc * 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipMemcpyAsync(hf.data(), dfound, nc * 4, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    if (breadth)
        for (uint64_t i = 0; i < nc; i++) {
            const uint64_t cnt = selcnt ? (uint64_t)(*selcnt)[i] : c->sizes[i];
            const double f = threshold < 0 ? (double)cnt : (double)hf[i];
            breadth[i] = f / (double)cnt;
        }
    return MF_OK;
}

// ---- the k-mers branch ----
static int wf_kmers(const char *who, mf_ctx *ctx, mf_wcomps *c, mf_wtable *sample, mf_wtable *selected, int threshold, int64_t *vec, double *breadth) {
    if (!ctx || !c || !sample || !vec) return mf_set_error("%s: NULL argument", who);
    MF_TRY(wf_check(who, "mf_features_device", ctx, c, sample, selected));
    MF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t nc = c->n;
    if (!nc) return MF_OK;
    mf_buf<uint8_t> mask; std::vector<unsigned int> selcnt;
    MF_TRY(wf_selection(ctx, c, selected, mask, selcnt));
    mf_buf<unsigned long long> dvec; mf_buf<unsigned int> dfound;
    MF_TRY(dvec.alloc(ctx, nc)); MF_TRY(dfound.alloc(ctx, nc));
    MF_HIP(hipMemsetAsync(dvec.p, 0, nc * 8, st));
    MF_HIP(hipMemsetAsync(dfound.p, 0, nc * 4, st));
    if (sample->n && c->n_kmers) {
        MF_TRY(mf_wtable_ensure_index(sample));
        mf_ktimer tm(ctx, "k_features");
        k_w_features<<<wf_grid(c->n_kmers), 256, 0, st>>>(mf_wtable_view(sample), c->hi.p, c->lo.p, c->comp.p, c->n_kmers, threshold, mask.p, dvec.p, dfound.p);
    }
    MF_HIP(hipGetLastError());
    return wf_finish(ctx, c, dvec.p, dfound.p, selected ? &selcnt : nullptr, threshold, vec, breadth);
}
extern "C" int mf_features_wide_device_selected(mf_ctx *ctx, mf_wcomps *c, mf_wtable *sample, mf_wtable *selected, int threshold, int64_t *vec, double *breadth) {
    mf_range rng_("mf:features_wide");
    return wf_kmers("mf_features_wide_device_selected", ctx, c, sample, selected, threshold, vec, breadth);
}
extern "C" int mf_features_wide_device(mf_ctx *ctx, mf_wcomps *c, mf_wtable *sample, int threshold, int64_t *vec, double *breadth) {
    mf_range rng_("mf:features_wide");
    return wf_kmers("mf_features_wide_device", ctx, c, sample, nullptr, threshold, vec, breadth);
}

// ---- the reads branch ----
static int wf_reads(const char *who, mf_ctx *ctx, mf_wcomps *c, const void *d_bases, const void *d_offsets, uint64_t n_reads, uint64_t n_bases, mf_wtable *selected,
                    int threshold, int64_t *vec, double *breadth) {
    if (!ctx || !c || !vec || (n_reads && (!d_bases || !d_offsets))) return mf_set_error("%s: NULL argument", who);
    MF_TRY(wf_check(who, "mf_features_reads_device", ctx, c, nullptr, selected));
    MF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t nc = c->n, nk = c->n_kmers;
    if (!nc) return MF_OK;
    const uint8_t *bases = (const uint8_t *)d_bases;
    const uint64_t *off = (const uint64_t *)d_offsets;
    const int k = c->k;
    // the reads' runs first: what is wrong with the offsets is said before anything is built
    mf_buf<uint64_t> srun; uint64_t n_runs = 0;
    if (n_reads) {
        mf_buf<uint32_t> runs; mf_buf<uint64_t> tot; mf_buf<unsigned int> bad;
        MF_TRY(runs.alloc(ctx, n_reads)); MF_TRY(srun.alloc(ctx, n_reads + 1)); MF_TRY(tot.alloc(ctx, 1)); MF_TRY(bad.alloc(ctx, 1));
        MF_HIP(hipMemsetAsync(bad.p, 0, 4, st));
        k_wf_sizes<<<wf_grid(n_reads), 256, 0, st>>>(off, n_reads, k, runs.p, bad.p);
        MF_HIP(hipGetLastError());
        MF_TRY(wf_scan(ctx, runs.p, srun.p, n_reads, tot.p));
        unsigned int h_bad = 0; uint64_t h_end = 0;
        MF_HIP(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, st));
        MF_HIP(hipMemcpyAsync(&h_end, off + n_reads, 8, hipMemcpyDeviceToHost, st));
        MF_HIP(hipMemcpyAsync(&n_runs, tot.p, 8, hipMemcpyDeviceToHost, st));
        MF_HIP(hipStreamSynchronize(st));
        if (h_bad) return mf_set_error("%s: offsets that go backwards, or a read of 2^31 or more k-mers", who);
        if (h_end != n_bases) return mf_set_error("%s: the offsets end at %llu, n_bases = %llu", who, (unsigned long long)h_end, (unsigned long long)n_bases);
    }
    mf_buf<uint8_t> mask; std::vector<unsigned int> selcnt;
    MF_TRY(wf_selection(ctx, c, selected, mask, selcnt));
    mf_buf<unsigned long long> dvec; mf_buf<unsigned int> dfound;
    MF_TRY(dvec.alloc(ctx, nc)); MF_TRY(dfound.alloc(ctx, nc));
    MF_HIP(hipMemsetAsync(dvec.p, 0, nc * 8, st));
    MF_HIP(hipMemsetAsync(dfound.p, 0, nc * 4, st));
    if (nk) {
        mf_buf<unsigned long long> index, occ; mf_buf<uint32_t> rep;
        uint64_t cap = 1024;
        while (cap < 2 * nk) cap <<= 1;
        MF_TRY(index.alloc(ctx, cap)); MF_TRY(occ.alloc(ctx, nk)); MF_TRY(rep.alloc(ctx, nk));
        MF_HIP(hipMemsetAsync(index.p, 0xFF, cap * 8, st));
        MF_HIP(hipMemsetAsync(occ.p, 0, nk * 8, st));
        {
            mf_ktimer tm(ctx, "k_wf_index");               // hm.put(kmer, 0) for every listing
            k_wf_index<<<wf_grid(nk), 256, 0, st>>>(index.p, cap - 1, c->hi.p, c->lo.p, nk, k, rep.p);
        }
        if (n_runs) {
            mf_ktimer tm(ctx, "k_wf_presence");
            k_wf_presence<<<wf_grid(n_runs), 256, 0, st>>>(bases, off, srun.p, n_reads, n_runs, k, mf_windex_view{index.p, cap - 1, c->hi.p, c->lo.p, nullptr, nk, k}, occ.p);
        }
        {
            mf_ktimer tm(ctx, "k_wf_occ");
            k_wf_occ<<<wf_grid(nk), 256, 0, st>>>(occ.p, rep.p, c->comp.p, nk, threshold, mask.p, dvec.p, dfound.p);
        }
        MF_HIP(hipGetLastError());
        MF_TRY(wf_finish(ctx, c, dvec.p, dfound.p, selected ? &selcnt : nullptr, threshold, vec, breadth));      // (synchronises: index, occ and rep go back to the arena)
        return MF_OK;
    }
    return wf_finish(ctx, c, dvec.p, dfound.p, selected ? &selcnt : nullptr, threshold, vec, breadth);
}
extern "C" int mf_features_reads_wide_device_selected(mf_ctx *ctx, mf_wcomps *c, const void *d_bases, const void *d_offsets, uint64_t n_reads, uint64_t n_bases,
                                                      mf_wtable *selected, int threshold, int64_t *vec, double *breadth) {
    mf_range rng_("mf:features_reads_wide");
    return wf_reads("mf_features_reads_wide_device_selected", ctx, c, d_bases, d_offsets, n_reads, n_bases, selected, threshold, vec, breadth);
}
extern "C" int mf_features_reads_wide_device(mf_ctx *ctx, mf_wcomps *c, const void *d_bases, const void *d_offsets, uint64_t n_reads, uint64_t n_bases, int threshold,
                                             int64_t *vec, double *breadth) {
    mf_range rng_("mf:features_reads_wide");
    return wf_reads("mf_features_reads_wide_device", ctx, c, d_bases, d_offsets, n_reads, n_bases, nullptr, threshold, vec, breadth);
}

// ---- the file forms: the shape of mf_features_selected / mf_features_reads_selected (mf_io.hip); nothing is written before mf_wcomps_load has
// accepted the components file, and nothing when a later step fails ----
static int wf_load_comps(const char *who, const char *narrow, mf_ctx *ctx, const char *components_bin, int k, mf_wcomps **c) {
    MF_TRY(wf_check_k(who, narrow, k));
    MF_TRY(mf_wcomps_load(ctx, components_bin, k, c));
    if ((*c)->n == 0) { mf_wcomps_destroy(*c); *c = nullptr; return mf_set_error("No components were found in input files! Can't continue the calculations."); }
    return MF_OK;
}
static int wf_kmers_files(const char *who, mf_ctx *ctx, const char *components_bin, const char *kmers_bin, int k, int threshold, mf_wtable *selected, const char *vec_path,
                          const char *breadth_path) {
    if (!ctx || !components_bin || !kmers_bin) return mf_set_error("%s: NULL argument", who);
    mf_wcomps *c = nullptr;
    MF_TRY(wf_load_comps(who, "mf_features", ctx, components_bin, k, &c));
    std::unique_ptr<mf_wcomps, void (*)(mf_wcomps *)> cg(c, mf_wcomps_destroy);
    mf_wtable *t = nullptr;
    const char *files[1] = {kmers_bin};
    MF_TRY(mf_wtable_load_kmers(ctx, files, 1, -1, k, &t));                   // (every record of the file, as mf_features)
    std::unique_ptr<mf_wtable, void (*)(mf_wtable *)> tg(t, mf_wtable_destroy);
    std::vector<int64_t> vec(c->n); std::vector<double> br(c->n);
    MF_TRY(wf_kmers(who, ctx, c, t, selected, threshold, vec.data(), br.data()));
    return mf_write_features_files(vec, br, vec_path, breadth_path);
}
extern "C" int mf_features_wide_selected(mf_ctx *ctx, const char *components_bin, const char *kmers_bin, int k, int threshold, mf_wtable *selected, const char *vec_path,
                                         const char *breadth_path) {
    mf_range rng_("mf:features_wide(files)");
    return wf_kmers_files("mf_features_wide_selected", ctx, components_bin, kmers_bin, k, threshold, selected, vec_path, breadth_path);
}
extern "C" int mf_features_wide(mf_ctx *ctx, const char *components_bin, const char *kmers_bin, int k, int threshold, const char *vec_path, const char *breadth_path) {
    mf_range rng_("mf:features_wide(files)");
    return wf_kmers_files("mf_features_wide", ctx, components_bin, kmers_bin, k, threshold, nullptr, vec_path, breadth_path);
}
// the files of ONE library
static int wf_reads_files(const char *who, mf_ctx *ctx, const char *components_bin, const char *const *files, int nfiles, int k, int threshold, mf_wtable *selected,
                          const char *vec_path, const char *breadth_path) {
    if (!ctx || !components_bin || nfiles < 0 || (nfiles > 0 && !files)) return mf_set_error("%s: NULL argument", who);
    mf_wcomps *c = nullptr;
    MF_TRY(wf_load_comps(who, "mf_features_reads", ctx, components_bin, k, &c));
    std::unique_ptr<mf_wcomps, void (*)(mf_wcomps *)> cg(c, mf_wcomps_destroy);
    mf_reads *r = nullptr;
    MF_TRY(mf_reads_load(ctx, files, nfiles, &r));
    std::unique_ptr<mf_reads, void (*)(mf_reads *)> rg(r, [](mf_reads *p) { mf_reads_destroy(p); });
    std::vector<int64_t> vec(c->n); std::vector<double> br(c->n);
    MF_TRY(wf_reads(who, ctx, c, r->d_bases, r->d_offsets, r->n, r->n_bases, selected, threshold, vec.data(), br.data()));
    return mf_write_features_files(vec, br, vec_path, breadth_path);
}
extern "C" int mf_features_reads_wide_selected(mf_ctx *ctx, const char *components_bin, const char *const *files, int nfiles, int k, int threshold, mf_wtable *selected,
                                               const char *vec_path, const char *breadth_path) {
    mf_range rng_("mf:features_reads_wide(files)");
    return wf_reads_files("mf_features_reads_wide_selected", ctx, components_bin, files, nfiles, k, threshold, selected, vec_path, breadth_path);
}
extern "C" int mf_features_reads_wide(mf_ctx *ctx, const char *components_bin, const char *const *files, int nfiles, int k, int threshold, const char *vec_path,
                                      const char *breadth_path) {
    mf_range rng_("mf:features_reads_wide(files)");
    return wf_reads_files("mf_features_reads_wide", ctx, components_bin, files, nfiles, k, threshold, nullptr, vec_path, breadth_path);
}
