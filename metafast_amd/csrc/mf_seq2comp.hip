// mf_seq2comp.hip -- seq2comp (src/tools/SequencesToComponents.java:61-103, src/algo/ComponentFromSequence.java:24-30): every sequence
// becomes one component, its members the DISTINCT canonical k-mers of the sequence, its weight the number of k-mer occurrences.
//
// The reference adds the k-mers of a sequence to a LongArraySet one by one (a linear scan per add: O(L^2) per sequence).  Here it is a
// segmented set-build with two size classes, both parallel inside a sequence:
//   short (1 .. S2C_T occurrences)   k_s2c_lds: the sequence's k-mers go into an open-addressed set in LDS (64-bit keys, empty = all
//                                    ones, linear probing, LDS compare-and-swap); the winners of the swap are the distinct k-mers.
//                                    Sequences of up to S2C_WAVE_T occurrences take one WAVE and a quarter of the table, four to a
//                                    workgroup; longer ones the workgroup.  Pass 1 counts the winners (the sizes), the sizes are
//                                    scanned, pass 2 builds the set again and writes the winners at the scanned offsets: no scratch in
//                                    HBM, no HBM atomics, no sort.
//   long  (more)                     k_s2c_pairs: a flat kernel over runs of S2C_RUN positions emits (sequence, canonical k-mer) pairs,
//                                    mf_sort_kmers_by_comp orders them, the first of each run of equal k-mers inside a sequence is
//                                    kept (k_s2c_heads, mf_scan, k_s2c_compact).  Whole sequences are batched so that the pairs fit.
// Option s2c_lds = 0 sends every sequence through the long class (the A/B of profiles/seq2comp_rate.txt, and the tests' cross-check).
// Components come in sequence order; inside a component the resident order is unspecified (export and write sort it, as for the
// cutter's components).
#include "mf_common.h"
#include "mf_roll.h"
#include <algorithm>
#include <memory>

#define S2C_T 4096                    // short class: at most this many k-mer occurrences ...
#define S2C_SLOTS (2 * S2C_T)         // ... in a table of twice as many 8-byte slots: 64 KiB, two workgroups per CU
#define S2C_WAVE_T (S2C_T / 4)        // one wave + a quarter of the table up to here
#define S2C_RUN 32                    // long class: positions per thread

// (s2c_code, s2c_roll: mf_roll.h)

// occ[i] = max(0, len_i - k + 1); a sequence of 2^32 - 1 or more occurrences (or offsets that go backwards) raises *bad
__global__ void k_s2c_sizes(const uint64_t *__restrict__ off, uint64_t n, int k, uint32_t *__restrict__ occ, unsigned int *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = off[i], b = off[i + 1];
    uint64_t ni = 0;
    if (b < a) atomicOr(bad, 1u);
    else if (b - a >= (uint64_t)k) ni = b - a - (uint64_t)k + 1;
    if (ni >= 0xFFFFFFFFull) { atomicOr(bad, 1u); ni = 0; }
    occ[i] = (uint32_t)ni;
}

// TEAM = 64: a wave per sequence of lo .. hi occurrences (hi <= S2C_WAVE_T), four sequences to a workgroup; TEAM = 256: the workgroup
// per sequence (hi <= S2C_T).  WRITE = false: sizes[s] = distinct k-mers; WRITE = true: they go to kmers / comp at moff[s].
template <int TEAM, bool WRITE>
__global__ __launch_bounds__(256) void k_s2c_lds(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ off, const uint32_t *__restrict__ occ,
                                                 uint64_t n_seqs, int k, uint32_t lo, uint32_t hi, uint32_t *__restrict__ sizes,
                                                 const uint64_t *__restrict__ moff, uint64_t *__restrict__ kmers, uint32_t *__restrict__ comp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s2c_smem[];
    constexpr int TEAMS = 256 / TEAM;
    constexpr uint32_t SLOTS = S2C_SLOTS / TEAMS;
    const int team = threadIdx.x / TEAM, tl = threadIdx.x % TEAM;
    unsigned long long *tab = reinterpret_cast<unsigned long long *>(s2c_smem) + (size_t)team * SLOTS;
    unsigned int *cnt = reinterpret_cast<unsigned int *>(s2c_smem + (size_t)S2C_SLOTS * 8) + team;
    auto sync = [&]() {
        if (TEAM == 64) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }
        else __syncthreads();
    };
    const uint64_t nteams = (uint64_t)gridDim.x * TEAMS;
    for (uint64_t s = (uint64_t)blockIdx.x * TEAMS + team; s < n_seqs; s += nteams) {      // team-uniform
        const uint32_t ni = occ[s];
        if (ni < lo || ni > hi) continue;
        uint32_t S = 64;                                   // the table this sequence needs: a power of two >= 2 ni, <= SLOTS as ni <= SLOTS / 2
        while (S < 2u * ni) S <<= 1;
        for (uint32_t j = tl; j < S; j += TEAM) tab[j] = (unsigned long long)MF_EMPTY;
        if (tl == 0) *cnt = 0u;
        sync();
        const uint32_t per = (ni + TEAM - 1) / TEAM, p0 = (uint32_t)tl * per;
        if (p0 < ni) {
            const uint32_t count = ni - p0 < per ? ni - p0 : per;
            const uint64_t dst = WRITE ? moff[s] : 0ull;
            s2c_roll(bases + off[s] + p0, count, k, [&](uint32_t, uint64_t key) {
                uint32_t slot = mf_pslot(mf_phash(key)) & (S - 1u);
                bool won = false;
                for (;;) {
                    const unsigned long long old = atomicCAS(&tab[slot], (unsigned long long)MF_EMPTY, (unsigned long long)key);
                    if (old == (unsigned long long)MF_EMPTY) { won = true; break; }
                    if (old == (unsigned long long)key) break;
                    slot = (slot + 1u) & (S - 1u);
                }
                if (won) {
                    const uint32_t at = atomicAdd(cnt, 1u);      // (at < ni: a k-mer wins at most once)
                    if (WRITE) { kmers[dst + at] = key; comp[dst + at] = (uint32_t)s; }
                }
            });
        }
        sync();
        if (!WRITE && tl == 0) sizes[s] = *cnt;
        sync();
    }
}

// long class, one thread per run of S2C_RUN positions of ONE sequence: batch entry j is sequence bseq[j], its runs are
// [brun[j], brun[j + 1]), its pairs [bocc[j], bocc[j + 1]); the id of a pair is j
__global__ __launch_bounds__(256) void k_s2c_pairs(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ off, const uint32_t *__restrict__ bseq,
                                                   const uint64_t *__restrict__ brun, const uint64_t *__restrict__ bocc, uint32_t nb, uint64_t n_runs, int k,
                                                   uint64_t *__restrict__ keys, uint32_t *__restrict__ ids) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs) return;
    uint32_t a = 0, b = nb;                                // the last j with brun[j] <= r
    while (b - a > 1u) { const uint32_t m = a + (b - a) / 2u; if (brun[m] <= r) a = m; else b = m; }
    const uint64_t o0 = bocc[a], ni = bocc[a + 1] - o0, p0 = (r - brun[a]) * S2C_RUN;
    if (p0 >= ni) return;
    const uint32_t count = (uint32_t)(ni - p0 < S2C_RUN ? ni - p0 : S2C_RUN);
    s2c_roll(bases + off[bseq[a]] + p0, count, k, [&](uint32_t i, uint64_t key) { keys[o0 + p0 + i] = key; ids[o0 + p0 + i] = a; });
}
// the sorted pairs of a batch: flag[p] = 1 where a new k-mer starts (the first pair of every sequence: k_s2c_seg_heads)
__global__ void k_s2c_heads(const uint64_t *__restrict__ srt, uint64_t n, uint32_t *__restrict__ flag) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) flag[p] = (p == 0 || srt[p] != srt[p - 1]) ? 1u : 0u;
}
__global__ void k_s2c_seg_heads(const uint64_t *__restrict__ bocc, uint32_t nb, uint32_t *__restrict__ flag) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nb) flag[bocc[j]] = 1u;
}
// rank = exclusive scan of flag: dstart[j] = first distinct k-mer of batch entry j (dstart[nb] = all of them), sizes of the sequences
__global__ void k_s2c_seg_sizes(const uint64_t *__restrict__ rank, const uint64_t *__restrict__ bocc, const uint32_t *__restrict__ bseq, uint32_t nb,
                                uint64_t *__restrict__ dstart, uint32_t *__restrict__ sizes) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > nb) return;
    const uint64_t d = rank[bocc[j]];
    dstart[j] = d;
    if (j < nb) sizes[bseq[j]] = (uint32_t)(rank[bocc[j + 1]] - d);
}
__global__ void k_s2c_compact(const uint64_t *__restrict__ srt, const uint32_t *__restrict__ flag, const uint64_t *__restrict__ rank, uint64_t n,
                              uint64_t *__restrict__ out) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n && flag[p]) out[rank[p]] = srt[p];
}
// the distinct k-mers of a batch to their components' places
__global__ void k_s2c_place(const uint64_t *__restrict__ dk, const uint64_t *__restrict__ dstart, const uint32_t *__restrict__ bseq, uint32_t nb, uint64_t nd,
                            const uint64_t *__restrict__ moff, uint64_t *__restrict__ kmers, uint32_t *__restrict__ comp) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nd) return;
    uint32_t a = 0, b = nb;                                // the last j with dstart[j] <= e (every entry has a k-mer: dstart ascends strictly)
    while (b - a > 1u) { const uint32_t m = a + (b - a) / 2u; if (dstart[m] <= e) a = m; else b = m; }
    const uint32_t s = bseq[a];
    const uint64_t dst = moff[s] + (e - dstart[a]);
    kmers[dst] = dk[e];
    comp[dst] = s;
}
__global__ void k_s2c_shift(const uint32_t *__restrict__ in, uint64_t n, uint32_t base, uint32_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] + base;
}

static inline unsigned s2c_grid(uint64_t n, unsigned bs = 256) { return (unsigned)((n + bs - 1) / bs); }
template <typename KF> static int s2c_set_lds(KF kern, size_t bytes) {
    MF_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return MF_OK;
}
static const size_t S2C_LDS = (size_t)S2C_SLOTS * 8 + 16;

// what a finished batch of the long class leaves until the components' offsets are known
struct s2c_batch {
    mf_buf<uint64_t> dk, dstart; mf_buf<uint32_t> bseq;
    uint32_t nb = 0; uint64_t nd = 0;
};

template <bool WRITE>
static int s2c_lds_pass(mf_ctx *ctx, const uint8_t *bases, const uint64_t *off, const uint32_t *occ, uint64_t n, int k, uint64_t n_wave, uint64_t n_wg,
                        uint32_t *sizes, const uint64_t *moff, uint64_t *kmers, uint32_t *comp) {
    hipStream_t st = ctx->stream;
    const unsigned cap = (unsigned)ctx->n_cu * 2u;             // two workgroups per CU fit (LDS)
    if (n_wave) {
        MF_TRY(s2c_set_lds(k_s2c_lds<64, WRITE>, S2C_LDS));
        const unsigned grid = (unsigned)std::min<uint64_t>((n_wave + 3) / 4, cap);
        mf_ktimer tm(ctx, "k_s2c_lds");
        k_s2c_lds<64, WRITE><<<grid, 256, S2C_LDS, st>>>(bases, off, occ, n, k, 1u, (uint32_t)S2C_WAVE_T, sizes, moff, kmers, comp);
    }
    if (n_wg) {
        MF_TRY(s2c_set_lds(k_s2c_lds<256, WRITE>, S2C_LDS));
        const unsigned grid = (unsigned)std::min<uint64_t>(n_wg, cap);
        mf_ktimer tm(ctx, "k_s2c_lds");
        k_s2c_lds<256, WRITE><<<grid, 256, S2C_LDS, st>>>(bases, off, occ, n, k, (uint32_t)S2C_WAVE_T + 1u, (uint32_t)S2C_T, sizes, moff, kmers, comp);
    }
    MF_HIP(hipGetLastError());
    return MF_OK;
}

// one batch of whole sequences of the long class: seqs[first .. last) of `list`
static int s2c_long_batch(mf_ctx *ctx, const uint8_t *bases, const uint64_t *off, const std::vector<uint32_t> &h_occ, const uint32_t *list, uint32_t nb, int k,
                          uint32_t *d_sizes, s2c_batch &B) {
    hipStream_t st = ctx->stream;
    std::vector<uint64_t> brun(nb + 1, 0), bocc(nb + 1, 0);
    for (uint32_t j = 0; j < nb; j++) {
        const uint64_t ni = h_occ[list[j]];
        bocc[j + 1] = bocc[j] + ni;
        brun[j + 1] = brun[j] + (ni + S2C_RUN - 1) / S2C_RUN;
    }
    const uint64_t np = bocc[nb], n_runs = brun[nb];
    if (np >= 0xFFFFFFFFull) return mf_set_error("seq2comp: a sequence of %llu k-mers (the sort takes fewer than 2^32 - 1 pairs)", (unsigned long long)np);
    B.nb = nb;
    MF_TRY(B.bseq.alloc(ctx, nb)); MF_TRY(B.dstart.alloc(ctx, (size_t)nb + 1));
    mf_buf<uint64_t> dbrun, dbocc, srt, rank, tot; mf_buf<uint32_t> flag;
    MF_TRY(dbrun.alloc(ctx, (size_t)nb + 1)); MF_TRY(dbocc.alloc(ctx, (size_t)nb + 1)); MF_TRY(tot.alloc(ctx, 1));
    MF_HIP(hipMemcpyAsync(B.bseq.p, list, (size_t)nb * 4, hipMemcpyHostToDevice, st));
    MF_HIP(hipMemcpyAsync(dbrun.p, brun.data(), ((size_t)nb + 1) * 8, hipMemcpyHostToDevice, st));
    MF_HIP(hipMemcpyAsync(dbocc.p, bocc.data(), ((size_t)nb + 1) * 8, hipMemcpyHostToDevice, st));
    MF_HIP(hipStreamSynchronize(st));                      // (the host arrays are done with)
    MF_TRY(srt.alloc(ctx, np));
    {
        mf_buf<uint64_t> keys; mf_buf<uint32_t> ids;
        MF_TRY(keys.alloc(ctx, np)); MF_TRY(ids.alloc(ctx, np));
        {
            mf_ktimer tm(ctx, "k_s2c_pairs");
            k_s2c_pairs<<<s2c_grid(n_runs), 256, 0, st>>>(bases, off, B.bseq.p, dbrun.p, dbocc.p, nb, n_runs, k, keys.p, ids.p);
        }
        MF_HIP(hipGetLastError());
        MF_TRY(mf_sort_kmers_by_comp(ctx, ids.p, keys.p, np, 2 * k, nb, srt.p));
    }
    MF_TRY(flag.alloc(ctx, np)); MF_TRY(rank.alloc(ctx, np + 1));
    k_s2c_heads<<<s2c_grid(np), 256, 0, st>>>(srt.p, np, flag.p);
    k_s2c_seg_heads<<<s2c_grid(nb), 256, 0, st>>>(dbocc.p, nb, flag.p);
    MF_TRY(mf_scan<1>(ctx, flag.p, rank.p, np, tot.p));
    k_s2c_seg_sizes<<<s2c_grid((uint64_t)nb + 1), 256, 0, st>>>(rank.p, dbocc.p, B.bseq.p, nb, B.dstart.p, d_sizes);
    MF_HIP(hipGetLastError());
    unsigned long long nd = 0;
    MF_HIP(hipMemcpyAsync(&nd, tot.p, 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    B.nd = nd;
    MF_TRY(B.dk.alloc(ctx, nd));
    k_s2c_compact<<<s2c_grid(np), 256, 0, st>>>(srt.p, flag.p, rank.p, np, B.dk.p);
    MF_HIP(hipGetLastError());
    MF_HIP(hipStreamSynchronize(st));                      // (the buffers of this batch go back to the arena)
    return MF_OK;
}

static int s2c_new_comps(mf_ctx *ctx, int k, uint64_t n, uint64_t nk, mf_comps **out) {
    std::unique_ptr<mf_comps, void (*)(mf_comps *)> C(new mf_comps(), [](mf_comps *c) { mf_comps_destroy(c); });
    C->ctx = ctx; C->k = k; C->n = n; C->n_kmers = nk;
    C->sizes.assign(n, 0); C->weights.assign(n, 0); C->thr.assign(n, 0);
    void *p = nullptr;
    MF_TRY(mf_alloc(ctx, (nk ? nk : 1) * 8, &p)); C->d_kmers = (uint64_t *)p; C->kmers_bytes = (nk ? nk : 1) * 8;
    MF_TRY(mf_alloc(ctx, (nk ? nk : 1) * 4, &p)); C->d_comp = (uint32_t *)p; C->comp_bytes = (nk ? nk : 1) * 4;
    C->host_ready = false;
    *out = C.release();
    return MF_OK;
}

extern "C" int mf_comps_from_sequences_device(mf_ctx *ctx, const void *d_bases, const void *d_offsets, uint64_t n_seqs, uint64_t n_bases, int k, mf_comps **out) {
    mf_range rng_("mf:seq2comp");
    if (!ctx || !out) return mf_set_error("mf_comps_from_sequences_device: NULL argument");
    *out = nullptr;
    if (k < 1 || k > 31) return mf_set_error("k must be in [1,31]");
    if (n_seqs >= 0xFFFFFFFFull) return mf_set_error("seq2comp: %llu sequences (a component index has 32 bits: fewer than 2^32 - 1)", (unsigned long long)n_seqs);
    if (n_seqs && (!d_bases || !d_offsets)) return mf_set_error("mf_comps_from_sequences_device: NULL argument");
    MF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (!n_seqs) return s2c_new_comps(ctx, k, 0, 0, out);
    const uint8_t *bases = (const uint8_t *)d_bases;
    const uint64_t *off = (const uint64_t *)d_offsets;
    const uint64_t n = n_seqs;

    // 1. the occurrences per sequence: the weights, and the classes
    mf_buf<uint32_t> occ, sizes; mf_buf<unsigned int> bad;
    MF_TRY(occ.alloc(ctx, n)); MF_TRY(sizes.alloc(ctx, n)); MF_TRY(bad.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(bad.p, 0, 4, st));
    MF_HIP(hipMemsetAsync(sizes.p, 0, n * 4, st));
    k_s2c_sizes<<<s2c_grid(n), 256, 0, st>>>(off, n, k, occ.p, bad.p);
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
        if (lds && ni <= S2C_WAVE_T) n_wave++;
        else if (lds && ni <= S2C_T) n_wg++;
        else longs.push_back((uint32_t)i);
    }

    // 2. the sizes: short sequences count their sets in LDS, long ones are sorted batch by batch and stay aside
    MF_TRY((s2c_lds_pass<false>(ctx, bases, off, occ.p, n, k, n_wave, n_wg, sizes.p, nullptr, nullptr, nullptr)));
    std::vector<std::unique_ptr<s2c_batch>> batches;
    const uint64_t cap = (uint64_t)std::max<int64_t>(1, ctx->opt_s2c_batch_pairs);
    for (size_t a = 0; a < longs.size();) {
        size_t b = a; uint64_t np = 0;
        while (b < longs.size() && (b == a || np + h_occ[longs[b]] <= cap)) np += h_occ[longs[b++]];
        batches.emplace_back(new s2c_batch());
        MF_TRY(s2c_long_batch(ctx, bases, off, h_occ, longs.data() + a, (uint32_t)(b - a), k, sizes.p, *batches.back()));
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
    mf_comps *C = nullptr;
    MF_TRY(s2c_new_comps(ctx, k, n, nk, &C));
    std::unique_ptr<mf_comps, void (*)(mf_comps *)> guard(C, [](mf_comps *c) { mf_comps_destroy(c); });
    for (uint64_t i = 0; i < n; i++) { C->sizes[i] = h_sizes[i]; C->weights[i] = (int64_t)h_occ[i]; }
    if (nk) {
        mf_buf<uint64_t> moff, tot;
        MF_TRY(moff.alloc(ctx, n + 1)); MF_TRY(tot.alloc(ctx, 1));
        MF_TRY(mf_scan<1>(ctx, sizes.p, moff.p, n, tot.p));
        // 4. the merge: short sequences build their sets again and write them, the batches' k-mers move to their places
        MF_TRY((s2c_lds_pass<true>(ctx, bases, off, occ.p, n, k, n_wave, n_wg, nullptr, moff.p, C->d_kmers, C->d_comp)));
        for (auto &B : batches)
            if (B->nd) k_s2c_place<<<s2c_grid(B->nd), 256, 0, st>>>(B->dk.p, B->dstart.p, B->bseq.p, B->nb, B->nd, moff.p, C->d_kmers, C->d_comp);
        MF_HIP(hipGetLastError());
        MF_HIP(hipStreamSynchronize(st));
    }
    *out = guard.release();
    return MF_OK;
}

// ---- the file form (SequencesToComponents.runImpl :61-103) ----
extern "C" int mf_seq2comp(mf_ctx *ctx, const char *const *files, int nfiles, int k, const char *components_bin, const char *stat_txt, uint64_t *n_components,
                           uint64_t *per_file) {
    mf_range rng_("mf:seq2comp(files)");
    if (!ctx || !components_bin || nfiles < 0 || (nfiles > 0 && !files)) return mf_set_error("mf_seq2comp: NULL argument");
    if (k < 1 || k > 31) return mf_set_error("k must be in [1,31]");
    MF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<std::unique_ptr<mf_comps, void (*)(mf_comps *)>> parts;
    uint64_t n = 0, nk = 0;
    for (int f = 0; f < nfiles; f++) {                     // one file resident at a time, in the order given (:65-80)
        mf_reads *r = nullptr;
        MF_TRY(mf_reads_load(ctx, files + f, 1, &r));
        std::unique_ptr<mf_reads, void (*)(mf_reads *)> gr(r, [](mf_reads *p) { mf_reads_destroy(p); });
        mf_comps *c = nullptr;
        MF_TRY(mf_comps_from_sequences_device(ctx, r->d_bases, r->d_offsets, r->n, r->n_bases, k, &c));
        parts.emplace_back(c, [](mf_comps *p) { mf_comps_destroy(p); });
        if (per_file) per_file[f] = c->n;
        n += c->n; nk += c->n_kmers;
    }
    if (n >= 0xFFFFFFFFull) return mf_set_error("seq2comp: %llu sequences (a component index has 32 bits: fewer than 2^32 - 1)", (unsigned long long)n);
    if (nk >= 0xFFFFFFFFull) return mf_set_error("components: too many k-mers (%llu members: fewer than 2^32 - 1)", (unsigned long long)nk);
    mf_comps *all = nullptr;
    MF_TRY(s2c_new_comps(ctx, k, n, nk, &all));
    std::unique_ptr<mf_comps, void (*)(mf_comps *)> guard(all, [](mf_comps *c) { mf_comps_destroy(c); });
    uint64_t cn = 0, ck = 0;
    for (auto &p : parts) {
        std::copy(p->sizes.begin(), p->sizes.end(), all->sizes.begin() + cn);
        std::copy(p->weights.begin(), p->weights.end(), all->weights.begin() + cn);
        if (p->n_kmers) {
            MF_HIP(hipMemcpyAsync(all->d_kmers + ck, p->d_kmers, p->n_kmers * 8, hipMemcpyDeviceToDevice, st));
            k_s2c_shift<<<s2c_grid(p->n_kmers), 256, 0, st>>>(p->d_comp, p->n_kmers, (uint32_t)cn, all->d_comp + ck);
        }
        cn += p->n; ck += p->n_kmers;
    }
    MF_HIP(hipGetLastError());
    MF_HIP(hipStreamSynchronize(st));
    parts.clear();
    MF_TRY(mf_comps_write(all, components_bin, nullptr));
    if (stat_txt) {                                        // three columns (:84-91), not the cutter's four
        FILE *f = fopen(stat_txt, "w");
        if (!f) return mf_set_error("can't write '%s'", stat_txt);
        fprintf(f, "# component.no\tcomponent.size\tcomponent.weight\n");
        for (uint64_t i = 0; i < n; i++) fprintf(f, "%llu\t%llu\t%lld\n", (unsigned long long)(i + 1), (unsigned long long)all->sizes[i], (long long)all->weights[i]);
        if (fclose(f) != 0) return mf_set_error("can't write '%s'", stat_txt);
    }
    if (n_components) *n_components = n;
    return MF_OK;
}
