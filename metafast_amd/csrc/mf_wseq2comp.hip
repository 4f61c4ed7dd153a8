// mf_wseq2comp.hip -- NO-REFERENCE EXTENSION (32 <= k <= 63): seq2comp on 2k-bit k-mers.  The semantics are those of mf_seq2comp.hip word for
// word: every sequence becomes one component, its members the DISTINCT canonical k-mers of the sequence, its weight the number of k-mer
// occurrences, thr = 0; a sequence shorter than k stays as an empty component.  ONE thing differs: mf_wcomps promises its members ascending in
// (hi, lo) inside every component ON THE DEVICE (mf_wcomps_export does not sort, mf_wcomps_load rejects a file that does not ascend strictly),
// so both classes below leave that order in place.
//
//   short (1 .. WS2C_T occurrences)  k_ws2c_lds: the sequence's canonical k-mers go into two LDS arrays of 64-bit words (high, low), padded to a
//                                    power of two with all ones (above every k-mer: a high word has at most 62 bits), and are sorted there
//                                    (bitonic, compare on (hi, lo)).  The heads key[i] != key[i - 1] are the distinct k-mers, already in
//                                    order: they are counted with wave ballots (pass 1: the sizes), the sizes are scanned, and pass 2 sorts
//                                    again and writes the heads at the scanned offsets.  No hash table, no compare-and-swap, no lane that
//                                    waits for another: a 2k-bit key has no LDS CAS, and a claim protocol with a BUSY marker would have had to
//                                    argue why a spinning lane never waits for a lane of its own wave.  Sequences of up to WS2C_WAVE_T
//                                    occurrences take one WAVE and a quarter of the arrays, four to a workgroup; longer ones the workgroup.
//                                    No scratch in HBM, no HBM atomics.
//   long  (more)                     k_ws2c_pairs: a flat kernel over runs of WS2C_RUN positions rolls two 128-bit registers and emits (hi, lo,
//                                    batch entry); three stable pair sorts that carry the pair's index (the low word, the 2k - 64 bits of the
//                                    high word, the entry: the pattern of wc2s_build_rows), heads on both words and the entry, mf_scan,
//                                    compaction, placement at the components' offsets.  Whole sequences are batched so that the pairs fit.
// Option s2c_lds = 0 sends every sequence through the long class (the A/B of profiles/wseq2comp_rate.txt, and the tests' cross-check).
#include "mf_wide.h"
#include "mf_roll.h"
#include <algorithm>
#include <memory>

#define WS2C_T 2048                   // short class: at most this many k-mer occurrences: 2 x 8 bytes each = 32 KiB of LDS per workgroup
#define WS2C_WAVE_T (WS2C_T / 4)      // one wave + a quarter of the arrays up to here
#define WS2C_RUN 32                   // long class: positions per thread

// (ws2c_roll: mf_roll.h)

// occ[i] = max(0, len_i - k + 1); a sequence of 2^32 - 1 or more occurrences (or offsets that go backwards) raises *bad
__global__ void k_ws2c_sizes(const uint64_t *__restrict__ off, uint64_t n, int k, uint32_t *__restrict__ occ, unsigned int *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = off[i], b = off[i + 1];
    uint64_t ni = 0;
    if (b < a) atomicOr(bad, 1u);
    else if (b - a >= (uint64_t)k) ni = b - a - (uint64_t)k + 1;
    if (ni >= 0xFFFFFFFFull) { atomicOr(bad, 1u); ni = 0; }
    occ[i] = (uint32_t)ni;
}

// TEAM = 64: a wave per sequence of lo .. hi occurrences (hi <= WS2C_WAVE_T), four sequences to a workgroup; TEAM = 256: the workgroup per
// sequence (hi <= WS2C_T).  WRITE = false: sizes[s] = distinct k-mers; WRITE = true: they go, ascending, to khi / klo / comp at moff[s].
// LDS: team t owns words [t * 2 CAP, (t + 1) * 2 CAP) -- CAP high words, then CAP low words --, and 4 words behind all of them hold the
// waves' head counts of a workgroup team.  A pair of a bitonic step is read and written by ONE lane, and the steps are apart by a barrier of
// the team (a wave's: the LDS operations of a wave complete in order, the fence keeps the compiler from moving them across).
template <int TEAM, bool WRITE>
__global__ __launch_bounds__(256) void k_ws2c_lds(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ off, const uint32_t *__restrict__ occ,
                                                  uint64_t n_seqs, int k, uint32_t lo, uint32_t hi, uint32_t *__restrict__ sizes,
                                                  const uint64_t *__restrict__ moff, uint64_t *__restrict__ khi, uint64_t *__restrict__ klo,
                                                  uint32_t *__restrict__ comp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ws2c_smem[];
    constexpr int TEAMS = 256 / TEAM, WAVES = TEAM / 64;
    constexpr uint32_t CAP = WS2C_T / TEAMS;
    const int team = threadIdx.x / TEAM, tl = threadIdx.x % TEAM;
    const uint32_t wave = (uint32_t)tl / 64u, lane = (uint32_t)tl % 64u;
    uint64_t *H = reinterpret_cast<uint64_t *>(ws2c_smem) + (size_t)team * 2 * CAP, *L = H + CAP;
    uint32_t *wtot = reinterpret_cast<uint32_t *>(ws2c_smem + (size_t)WS2C_T * 16);
    auto sync = [&]() {
        if (TEAM == 64) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }
        else __syncthreads();
    };
    const uint64_t nteams = (uint64_t)gridDim.x * TEAMS;
    for (uint64_t s = (uint64_t)blockIdx.x * TEAMS + team; s < n_seqs; s += nteams) {      // team-uniform
        const uint32_t ni = occ[s];
        if (ni < lo || ni > hi) continue;
        uint32_t N = 2;                                    // the arrays this sequence needs: a power of two >= ni, <= CAP as ni <= hi <= CAP
        while (N < ni) N <<= 1;
        // 1. the canonical k-mers at their positions, all ones behind them
        const uint32_t per = (ni + TEAM - 1) / TEAM, p0 = (uint32_t)tl * per;
        if (p0 < ni) {
            const uint32_t count = ni - p0 < per ? ni - p0 : per;
            ws2c_roll(bases + off[s] + p0, count, k, [&](uint32_t i, uint64_t h, uint64_t l) { H[p0 + i] = h; L[p0 + i] = l; });
        }
        for (uint32_t j = ni + (uint32_t)tl; j < N; j += TEAM) { H[j] = ~0ull; L[j] = ~0ull; }
        sync();
        // 2. bitonic sort, ascending in (hi, lo): N / 2 pairs a step
        for (uint32_t kk = 2; kk <= N; kk <<= 1)
            for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
                for (uint32_t t = (uint32_t)tl; t < N / 2; t += TEAM) {
                    const uint32_t a = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), b = a | j;
                    const uint64_t ha = H[a], la = L[a], hb = H[b], lb = L[b];
                    const bool gt = ha > hb || (ha == hb && la > lb), up = (a & kk) == 0u;
                    if (gt == up) { H[a] = hb; L[a] = lb; H[b] = ha; L[b] = la; }
                }
                sync();
            }
        // 3. the heads: wave w of the team takes [w * chunk, (w + 1) * chunk) of the ni sorted k-mers, 64 at a time
        const uint32_t chunk = (N + WAVES - 1) / WAVES, c0 = wave * chunk, c1 = c0 + chunk < ni ? c0 + chunk : ni;
        auto head = [&](uint32_t i) { return i < c1 && (i == 0u || H[i] != H[i - 1] || L[i] != L[i - 1]); };
        uint32_t cnt = 0;                                  // (wave-uniform)
        for (uint32_t b = c0; b < c1; b += 64u) cnt += (uint32_t)__popcll(__ballot(head(b + lane)));
        uint32_t before = 0, total = cnt;
        if (TEAM > 64) {
            if (lane == 0) wtot[wave] = cnt;
            __syncthreads();
            total = 0;
            for (uint32_t w = 0; w < (uint32_t)WAVES; w++) { const uint32_t c = wtot[w]; total += c; if (w < wave) before += c; }
        }
        if (!WRITE) { if (tl == 0) sizes[s] = total; }
        else {
            uint64_t at = moff[s] + before;
            for (uint32_t b = c0; b < c1; b += 64u) {
                const uint32_t i = b + lane;
                const bool hd = head(i);
                const unsigned long long m = __ballot(hd);
                if (hd) {
                    const uint64_t d = at + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
                    khi[d] = H[i]; klo[d] = L[i]; comp[d] = (uint32_t)s;
                }
                at += (uint64_t)__popcll(m);
            }
        }
        sync();
    }
}

// long class, one thread per run of WS2C_RUN positions of ONE sequence: batch entry j is sequence bseq[j], its runs are
// [brun[j], brun[j + 1]), its pairs [bocc[j], bocc[j + 1]); the id of a pair is j
__global__ __launch_bounds__(256) void k_ws2c_pairs(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ off, const uint32_t *__restrict__ bseq,
                                                    const uint64_t *__restrict__ brun, const uint64_t *__restrict__ bocc, uint32_t nb, uint64_t n_runs, int k,
                                                    uint64_t *__restrict__ khi, uint64_t *__restrict__ klo, uint32_t *__restrict__ ids, uint64_t *__restrict__ idx) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs) return;
    uint32_t a = 0, b = nb;                                // the last j with brun[j] <= r
    while (b - a > 1u) { const uint32_t m = a + (b - a) / 2u; if (brun[m] <= r) a = m; else b = m; }
    const uint64_t o0 = bocc[a], ni = bocc[a + 1] - o0, p0 = (r - brun[a]) * WS2C_RUN;
    if (p0 >= ni) return;
    const uint32_t count = (uint32_t)(ni - p0 < WS2C_RUN ? ni - p0 : WS2C_RUN);
    ws2c_roll(bases + off[bseq[a]] + p0, count, k, [&](uint32_t i, uint64_t h, uint64_t l) {
        const uint64_t p = o0 + p0 + i;
        khi[p] = h; klo[p] = l; ids[p] = a; idx[p] = p;
    });
}
__global__ void k_ws2c_gather64(const uint64_t *__restrict__ idx, const uint64_t *__restrict__ src, uint64_t n, uint64_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = src[idx[i]];
}
__global__ void k_ws2c_gather32(const uint64_t *__restrict__ idx, const uint32_t *__restrict__ src, uint64_t n, uint32_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = src[idx[i]];
}
// the sorted (entry, hi, lo) triples of a batch: flag[p] = 1 where a new k-mer starts, on BOTH words (and where a new entry starts)
__global__ void k_ws2c_heads(const uint32_t *__restrict__ ent, const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint64_t n,
                             uint32_t *__restrict__ flag) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) flag[p] = (p == 0 || ent[p] != ent[p - 1] || lo[p] != lo[p - 1] || hi[p] != hi[p - 1]) ? 1u : 0u;
}
// rank = exclusive scan of flag: dstart[j] = first distinct k-mer of batch entry j (dstart[nb] = all of them), sizes of the sequences
__global__ void k_ws2c_seg_sizes(const uint64_t *__restrict__ rank, const uint64_t *__restrict__ bocc, const uint32_t *__restrict__ bseq, uint32_t nb,
                                 uint64_t *__restrict__ dstart, uint32_t *__restrict__ sizes) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > nb) return;
    const uint64_t d = rank[bocc[j]];
    dstart[j] = d;
    if (j < nb) sizes[bseq[j]] = (uint32_t)(rank[bocc[j + 1]] - d);
}
__global__ void k_ws2c_compact(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, const uint32_t *__restrict__ flag,
                               const uint64_t *__restrict__ rank, uint64_t n, uint64_t *__restrict__ ohi, uint64_t *__restrict__ olo) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n && flag[p]) { const uint64_t d = rank[p]; ohi[d] = hi[p]; olo[d] = lo[p]; }
}
// the distinct k-mers of a batch to their components' places (ascending inside an entry, and so inside the component)
__global__ void k_ws2c_place(const uint64_t *__restrict__ dhi, const uint64_t *__restrict__ dlo, const uint64_t *__restrict__ dstart,
                             const uint32_t *__restrict__ bseq, uint32_t nb, uint64_t nd, const uint64_t *__restrict__ moff, uint64_t *__restrict__ khi,
                             uint64_t *__restrict__ klo, uint32_t *__restrict__ comp) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nd) return;
    uint32_t a = 0, b = nb;                                // the last j with dstart[j] <= e (every entry has a k-mer: dstart ascends strictly)
    while (b - a > 1u) { const uint32_t m = a + (b - a) / 2u; if (dstart[m] <= e) a = m; else b = m; }
    const uint32_t s = bseq[a];
    const uint64_t dst = moff[s] + (e - dstart[a]);
    khi[dst] = dhi[e]; klo[dst] = dlo[e];
    comp[dst] = s;
}
__global__ void k_ws2c_shift(const uint32_t *__restrict__ in, uint64_t n, uint32_t base, uint32_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] + base;
}

static inline unsigned ws2c_grid(uint64_t n, unsigned bs = 256) { return (unsigned)((n + bs - 1) / bs); }
static const size_t WS2C_LDS = (size_t)WS2C_T * 16 + 16;

static int ws2c_check_k(const char *who, const char *narrow, int k) {
    if (k < 32 || k > 63) return mf_set_error("%s: 32 <= k <= 63 (k <= 31: %s)", who, narrow);
    return MF_OK;
}

// what a finished batch of the long class leaves until the components' offsets are known
struct ws2c_batch {
    mf_buf<uint64_t> dhi, dlo, dstart; mf_buf<uint32_t> bseq;
    uint32_t nb = 0; uint64_t nd = 0;
};

template <bool WRITE>
static int ws2c_lds_pass(mf_ctx *ctx, const uint8_t *bases, const uint64_t *off, const uint32_t *occ, uint64_t n, int k, uint64_t n_wave, uint64_t n_wg,
                         uint32_t *sizes, const uint64_t *moff, uint64_t *khi, uint64_t *klo, uint32_t *comp) {
    hipStream_t st = ctx->stream;
    const unsigned cap = (unsigned)ctx->n_cu * 4u;             // four workgroups per CU fit (LDS: 32 KiB each)
    if (n_wave) {
        const unsigned grid = (unsigned)std::min<uint64_t>((n_wave + 3) / 4, cap);
        mf_ktimer tm(ctx, "k_ws2c_lds");
        k_ws2c_lds<64, WRITE><<<grid, 256, WS2C_LDS, st>>>(bases, off, occ, n, k, 1u, (uint32_t)WS2C_WAVE_T, sizes, moff, khi, klo, comp);
    }
    if (n_wg) {
        const unsigned grid = (unsigned)std::min<uint64_t>(n_wg, cap);
        mf_ktimer tm(ctx, "k_ws2c_lds");
        k_ws2c_lds<256, WRITE><<<grid, 256, WS2C_LDS, st>>>(bases, off, occ, n, k, (uint32_t)WS2C_WAVE_T + 1u, (uint32_t)WS2C_T, sizes, moff, khi, klo, comp);
    }
    MF_HIP(hipGetLastError());
    return MF_OK;
}

// one batch of whole sequences of the long class: nb sequences of `list`
static int ws2c_long_batch(mf_ctx *ctx, const uint8_t *bases, const uint64_t *off, const std::vector<uint32_t> &h_occ, const uint32_t *list, uint32_t nb, int k,
                           uint32_t *d_sizes, ws2c_batch &B) {
    hipStream_t st = ctx->stream;
    const int hb = 2 * k - 64;                             // bits of the high word, 0 .. 62
    std::vector<uint64_t> brun(nb + 1, 0), bocc(nb + 1, 0);
    for (uint32_t j = 0; j < nb; j++) {
        const uint64_t ni = h_occ[list[j]];
        bocc[j + 1] = bocc[j] + ni;
        brun[j + 1] = brun[j] + (ni + WS2C_RUN - 1) / WS2C_RUN;
    }
    const uint64_t np = bocc[nb], n_runs = brun[nb];
    if (np >= 0xFFFFFFFFull) return mf_set_error("seq2comp: a sequence of %llu k-mers (the sort takes fewer than 2^32 - 1 pairs)", (unsigned long long)np);
    B.nb = nb;
    MF_TRY(B.bseq.alloc(ctx, nb)); MF_TRY(B.dstart.alloc(ctx, (size_t)nb + 1));
    mf_buf<uint64_t> dbrun, dbocc, shi, slo, rank, tot; mf_buf<uint32_t> sent, flag;
    MF_TRY(dbrun.alloc(ctx, (size_t)nb + 1)); MF_TRY(dbocc.alloc(ctx, (size_t)nb + 1)); MF_TRY(tot.alloc(ctx, 1));
    MF_HIP(hipMemcpyAsync(B.bseq.p, list, (size_t)nb * 4, hipMemcpyHostToDevice, st));
    MF_HIP(hipMemcpyAsync(dbrun.p, brun.data(), ((size_t)nb + 1) * 8, hipMemcpyHostToDevice, st));
    MF_HIP(hipMemcpyAsync(dbocc.p, bocc.data(), ((size_t)nb + 1) * 8, hipMemcpyHostToDevice, st));
    MF_HIP(hipStreamSynchronize(st));                      // (the host arrays are done with)
    MF_TRY(shi.alloc(ctx, np)); MF_TRY(slo.alloc(ctx, np)); MF_TRY(sent.alloc(ctx, np));
    {
        mf_buf<uint64_t> khi, klo, k1, i0, i1; mf_buf<uint32_t> ids, c0;
        MF_TRY(khi.alloc(ctx, np)); MF_TRY(klo.alloc(ctx, np)); MF_TRY(k1.alloc(ctx, np)); MF_TRY(i0.alloc(ctx, np)); MF_TRY(i1.alloc(ctx, np));
        MF_TRY(ids.alloc(ctx, np)); MF_TRY(c0.alloc(ctx, np));
        {
            mf_ktimer tm(ctx, "k_ws2c_pairs");
            k_ws2c_pairs<<<ws2c_grid(n_runs), 256, 0, st>>>(bases, off, B.bseq.p, dbrun.p, dbocc.p, nb, n_runs, k, khi.p, klo.p, ids.p, i0.p);
        }
        MF_HIP(hipGetLastError());
        // three stable passes that carry the pair's index: the low word, the high word's 2k - 64 bits, the entry (wc2s_build_rows)
        int cb = 1; while (cb < 32 && (1ull << cb) < nb) cb++;
        mf_ktimer tm(ctx, "k_ws2c_sort");
        MF_TRY(mf_sort_u64_u64(ctx, klo.p, i0.p, np, 64, k1.p, i1.p));                         // (lo', idx') in (k1, i1)
        if (hb) {
            k_ws2c_gather64<<<ws2c_grid(np), 256, 0, st>>>(i1.p, khi.p, np, shi.p);            // hi' in shi
            MF_TRY(mf_sort_u64_u64(ctx, shi.p, i1.p, np, hb, k1.p, i0.p));                     // (hi'', idx'') in (k1, i0)
        } else i0.swap(i1);                                                                    // (k = 32: every high word is 0)
        k_ws2c_gather32<<<ws2c_grid(np), 256, 0, st>>>(i0.p, ids.p, np, c0.p);
        MF_TRY(mf_sort_u32_u64(ctx, c0.p, i0.p, np, cb, sent.p, i1.p));                        // (entry''', idx''') in (sent, i1)
        k_ws2c_gather64<<<ws2c_grid(np), 256, 0, st>>>(i1.p, khi.p, np, shi.p);                // the sorted triples: (sent, shi, slo)
        k_ws2c_gather64<<<ws2c_grid(np), 256, 0, st>>>(i1.p, klo.p, np, slo.p);
        MF_HIP(hipGetLastError());
        MF_HIP(hipStreamSynchronize(st));                  // (the sort's buffers go back to the arena)
    }
    MF_TRY(flag.alloc(ctx, np)); MF_TRY(rank.alloc(ctx, np + 1));
    k_ws2c_heads<<<ws2c_grid(np), 256, 0, st>>>(sent.p, shi.p, slo.p, np, flag.p);
    MF_TRY(mf_scan<1>(ctx, flag.p, rank.p, np, tot.p));
    k_ws2c_seg_sizes<<<ws2c_grid((uint64_t)nb + 1), 256, 0, st>>>(rank.p, dbocc.p, B.bseq.p, nb, B.dstart.p, d_sizes);
    MF_HIP(hipGetLastError());
    unsigned long long nd = 0;
    MF_HIP(hipMemcpyAsync(&nd, tot.p, 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    B.nd = nd;
    MF_TRY(B.dhi.alloc(ctx, nd)); MF_TRY(B.dlo.alloc(ctx, nd));
    k_ws2c_compact<<<ws2c_grid(np), 256, 0, st>>>(shi.p, slo.p, flag.p, rank.p, np, B.dhi.p, B.dlo.p);
    MF_HIP(hipGetLastError());
    MF_HIP(hipStreamSynchronize(st));                      // (the buffers of this batch go back to the arena)
    return MF_OK;
}

static int ws2c_new_comps(mf_ctx *ctx, int k, uint64_t n, uint64_t nk, mf_wcomps **out) {
    auto C = std::make_unique<mf_wcomps>();
    C->ctx = ctx; C->k = k; C->n = n; C->n_kmers = nk;
    C->sizes.assign(n, 0); C->weights.assign(n, 0); C->thr.assign(n, 0);
    MF_TRY(C->hi.alloc(ctx, nk)); MF_TRY(C->lo.alloc(ctx, nk)); MF_TRY(C->comp.alloc(ctx, nk));
    *out = C.release();
    return MF_OK;
}

extern "C" int mf_wcomps_from_sequences_device(mf_ctx *ctx, const void *d_bases, const void *d_offsets, uint64_t n_seqs, uint64_t n_bases, int k, mf_wcomps **out) {
    mf_range rng_("mf:seq2comp_wide");
    if (!ctx || !out) return mf_set_error("mf_wcomps_from_sequences_device: NULL argument");
    *out = nullptr;
    MF_TRY(ws2c_check_k("mf_wcomps_from_sequences_device", "mf_comps_from_sequences_device", k));
    if (n_seqs >= 0xFFFFFFFFull) return mf_set_error("seq2comp: %llu sequences (a component index has 32 bits: fewer than 2^32 - 1)", (unsigned long long)n_seqs);
    if (n_seqs && (!d_bases || !d_offsets)) return mf_set_error("mf_wcomps_from_sequences_device: NULL argument");
    MF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (!n_seqs) return ws2c_new_comps(ctx, k, 0, 0, out);
    const uint8_t *bases = (const uint8_t *)d_bases;
    const uint64_t *off = (const uint64_t *)d_offsets;
    const uint64_t n = n_seqs;

    // 1. the occurrences per sequence: the weights, and the classes
    mf_buf<uint32_t> occ, sizes; mf_buf<unsigned int> bad;
    MF_TRY(occ.alloc(ctx, n)); MF_TRY(sizes.alloc(ctx, n)); MF_TRY(bad.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(bad.p, 0, 4, st));
    MF_HIP(hipMemsetAsync(sizes.p, 0, n * 4, st));
    k_ws2c_sizes<<<ws2c_grid(n), 256, 0, st>>>(off, n, k, occ.p, bad.p);
    MF_HIP(hipGetLastError());
    std::vector<uint32_t> h_occ(n);
    unsigned int h_bad = 0; uint64_t h_end = 0;
    MF_HIP(hipMemcpyAsync(h_occ.data(), occ.p, n * 4, hipMemcpyDeviceToHost, st));
    MF_HIP(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, st));
    MF_HIP(hipMemcpyAsync(&h_end, off + n, 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    if (h_bad) return mf_set_error("seq2comp: offsets that go backwards, or a sequence of 2^32 - 1 or more k-mers");
    if (h_end != n_bases) return mf_set_error("seq2comp: the offsets end at %llu, n_bases = %llu", (unsigned long long)h_end, (unsigned long long)n_bases);
    const bool lds = ctx->opt_s2c_lds != 0;
    uint64_t n_wave = 0, n_wg = 0;
    std::vector<uint32_t> longs;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t ni = h_occ[i];
        if (!ni) continue;
        if (lds && ni <= WS2C_WAVE_T) n_wave++;
        else if (lds && ni <= WS2C_T) n_wg++;
        else longs.push_back((uint32_t)i);
    }

    // 2. the sizes: short sequences sort and count their heads in LDS, long ones are sorted batch by batch and stay aside
    MF_TRY((ws2c_lds_pass<false>(ctx, bases, off, occ.p, n, k, n_wave, n_wg, sizes.p, nullptr, nullptr, nullptr, nullptr)));
    std::vector<std::unique_ptr<ws2c_batch>> batches;
    const uint64_t cap = (uint64_t)std::max<int64_t>(1, ctx->opt_s2c_batch_pairs);
    for (size_t a = 0; a < longs.size();) {
        size_t b = a; uint64_t np = 0;
        while (b < longs.size() && (b == a || np + h_occ[longs[b]] <= cap)) np += h_occ[longs[b++]];
        batches.emplace_back(new ws2c_batch());
        MF_TRY(ws2c_long_batch(ctx, bases, off, h_occ, longs.data() + a, (uint32_t)(b - a), k, sizes.p, *batches.back()));
        a = b;
    }
    ctx->n_s2c_batches += batches.size();

    // 3. the components' places
    std::vector<uint32_t> h_sizes(n);
    MF_HIP(hipMemcpyAsync(h_sizes.data(), sizes.p, n * 4, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    uint64_t nk = 0;
    for (uint64_t i = 0; i < n; i++) nk += h_sizes[i];
    if (nk >= 0xFFFFFFFFull) return mf_set_error("components: too many k-mers (%llu members: fewer than 2^32 - 1)", (unsigned long long)nk);
    mf_wcomps *C = nullptr;
    MF_TRY(ws2c_new_comps(ctx, k, n, nk, &C));
    std::unique_ptr<mf_wcomps, void (*)(mf_wcomps *)> guard(C, mf_wcomps_destroy);
    for (uint64_t i = 0; i < n; i++) { C->sizes[i] = h_sizes[i]; C->weights[i] = (int64_t)h_occ[i]; }
    if (nk) {
        mf_buf<uint64_t> moff, tot;
        MF_TRY(moff.alloc(ctx, n + 1)); MF_TRY(tot.alloc(ctx, 1));
        MF_TRY(mf_scan<1>(ctx, sizes.p, moff.p, n, tot.p));
        // 4. the merge: short sequences sort again and write their heads, the batches' k-mers move to their places
        MF_TRY((ws2c_lds_pass<true>(ctx, bases, off, occ.p, n, k, n_wave, n_wg, nullptr, moff.p, C->hi.p, C->lo.p, C->comp.p)));
        for (auto &B : batches)
            if (B->nd) k_ws2c_place<<<ws2c_grid(B->nd), 256, 0, st>>>(B->dhi.p, B->dlo.p, B->dstart.p, B->bseq.p, B->nb, B->nd, moff.p, C->hi.p, C->lo.p, C->comp.p);
        MF_HIP(hipGetLastError());
        MF_HIP(hipStreamSynchronize(st));
    }
    *out = guard.release();
    return MF_OK;
}

// ---- the file form (the shape of mf_seq2comp) ----
extern "C" int mf_seq2comp_wide(mf_ctx *ctx, const char *const *files, int nfiles, int k, const char *components_bin, const char *stat_txt, uint64_t *n_components,
                                uint64_t *per_file) {
    mf_range rng_("mf:seq2comp_wide(files)");
    if (!ctx || !components_bin || nfiles < 0 || (nfiles > 0 && !files)) return mf_set_error("mf_seq2comp_wide: NULL argument");
    MF_TRY(ws2c_check_k("mf_seq2comp_wide", "mf_seq2comp", k));
    MF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<std::unique_ptr<mf_wcomps, void (*)(mf_wcomps *)>> parts;
    uint64_t n = 0, nk = 0;
    for (int f = 0; f < nfiles; f++) {                     // one file resident at a time, in the order given
        mf_reads *r = nullptr;
        MF_TRY(mf_reads_load(ctx, files + f, 1, &r));
        std::unique_ptr<mf_reads, void (*)(mf_reads *)> gr(r, [](mf_reads *p) { mf_reads_destroy(p); });
        mf_wcomps *c = nullptr;
        MF_TRY(mf_wcomps_from_sequences_device(ctx, r->d_bases, r->d_offsets, r->n, r->n_bases, k, &c));
        parts.emplace_back(c, mf_wcomps_destroy);
        if (per_file) per_file[f] = c->n;
        n += c->n; nk += c->n_kmers;
    }
    if (n >= 0xFFFFFFFFull) return mf_set_error("seq2comp: %llu sequences (a component index has 32 bits: fewer than 2^32 - 1)", (unsigned long long)n);
    if (nk >= 0xFFFFFFFFull) return mf_set_error("components: too many k-mers (%llu members: fewer than 2^32 - 1)", (unsigned long long)nk);
    mf_wcomps *all = nullptr;
    MF_TRY(ws2c_new_comps(ctx, k, n, nk, &all));
    std::unique_ptr<mf_wcomps, void (*)(mf_wcomps *)> guard(all, mf_wcomps_destroy);
    uint64_t cn = 0, ck = 0;
    for (auto &p : parts) {
        std::copy(p->sizes.begin(), p->sizes.end(), all->sizes.begin() + cn);
        std::copy(p->weights.begin(), p->weights.end(), all->weights.begin() + cn);
        if (p->n_kmers) {
            MF_HIP(hipMemcpyAsync(all->hi.p + ck, p->hi.p, p->n_kmers * 8, hipMemcpyDeviceToDevice, st));
            MF_HIP(hipMemcpyAsync(all->lo.p + ck, p->lo.p, p->n_kmers * 8, hipMemcpyDeviceToDevice, st));
            k_ws2c_shift<<<ws2c_grid(p->n_kmers), 256, 0, st>>>(p->comp.p, p->n_kmers, (uint32_t)cn, all->comp.p + ck);
        }
        cn += p->n; ck += p->n_kmers;
    }
    MF_HIP(hipGetLastError());
    MF_HIP(hipStreamSynchronize(st));
    parts.clear();
    MF_TRY(mf_wcomps_write(all, components_bin, nullptr));
    if (stat_txt) {                                        // three columns, as mf_seq2comp (mf_wcomps_write has the cutter's four)
        FILE *f = fopen(stat_txt, "w");
        if (!f) return mf_set_error("can't write '%s'", stat_txt);
        fprintf(f, "# component.no\tcomponent.size\tcomponent.weight\n");
        for (uint64_t i = 0; i < n; i++) fprintf(f, "%llu\t%llu\t%lld\n", (unsigned long long)(i + 1), (unsigned long long)all->sizes[i], (long long)all->weights[i]);
        if (fclose(f) != 0) return mf_set_error("can't write '%s'", stat_txt);
    }
    if (n_components) *n_components = n;
    return MF_OK;
}
