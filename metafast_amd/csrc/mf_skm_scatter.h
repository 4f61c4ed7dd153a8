// mf_skm_scatter.h -- super-k-mer counting (mf_skm.hip), level 1: S1 k_skm_hist (the records' level-1 digits counted per block) and S2 k_skm_scatter
// (the records built and radix-partitioned through 64-byte LDS staging lines, with exact ranges or in the one-pass form), the region sizes and the
// directory kernels that follow them.  The staging lines serve S3 (mf_skm_split.h) too.
#pragma once
#include "mf_skm_scan.h"

// =============================================================================================
// S1: per-block histogram of the records' level-1 digit (and of their k-mers, for plans without a split level)
// =============================================================================================
template <int K>
__global__ __launch_bounds__(1024) void k_skm_hist(const uint8_t *__restrict__ bases, uint64_t n_bases, const uint32_t *__restrict__ vmask,
                                                   uint64_t n_words, uint64_t words_per_block, int bits1,
                                                   uint32_t *__restrict__ blockhist, uint32_t *__restrict__ blockocc, int G, int stride,
                                                   uint32_t dlo, uint32_t dhi) {
    // [dlo, dhi): the level-1 digits of this SLICE of the run (skm_run); records of other digits belong to other slices
    // stride > 1: a SAMPLE (every stride-th tile of 1024 words), used to size the digit regions of the one-pass scatter
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nd = 1 << bits1;
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem), *occ = hist + nd;
    for (int i = threadIdx.x; i < 2 * nd; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    const uint64_t wlo = (uint64_t)blockIdx.x * words_per_block;
    const uint64_t whi = wlo + words_per_block < n_words ? wlo + words_per_block : n_words;
    for (uint64_t wb = wlo; wb < whi; wb += (uint64_t)blockDim.x * (uint64_t)stride) {
        const uint64_t w = wb + threadIdx.x;
        const uint32_t m = w < whi ? vmask[w] : 0u;
        if (__ballot(m != 0u) == 0ull) continue;
        skm_word<K> S;
        skm_scan_word<K>(S, bases, n_bases, w < n_words ? w : 0, m);
        uint32_t cut = S.cut;
        while (__ballot(cut != 0u) != 0ull) {
            if (cut) {
                uint32_t s, len, d1, digits;
                skm_next_run<K>(S, cut, s, len);
                skm_route(skm_mh_at<K>(S, s), bits1, d1, digits);
                if (d1 >= dlo && d1 < dhi) {
                    atomicAdd(&hist[d1], 1u);
                    if (blockocc) atomicAdd(&occ[d1], len);
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nd; i += blockDim.x) {
        blockhist[(size_t)i * G + blockIdx.x] = hist[i];
        if (blockocc) blockocc[(size_t)i * G + blockIdx.x] = occ[i];
    }
}

// =============================================================================================
// LDS staging of 16-byte records: one 64-byte line (4 records) per digit; same protocol as mf_stage (mf_count.hip):
// reserve a slot, write it, commit; the 4th committer's line is written to HBM by four lanes with one store instruction
// =============================================================================================
struct skm_stage {
    skm_rec *line;     // [nd][4]
    uint64_t *cur;     // [nd] next record index of this workgroup's range of digit d
    uint64_t *q_pos;   // [16 waves][SKM_QCAP]
    uint32_t *ctr;     // [nd] low 16 = reserved, high 16 = committed
    uint32_t *q_d;     // [16 waves][SKM_QCAP]
    int nd;
};
__device__ __forceinline__ skm_stage skm_stage_carve(unsigned char *smem, int nd) {
    skm_stage L;
    L.nd = nd;
    L.line = reinterpret_cast<skm_rec *>(smem);
    L.cur = reinterpret_cast<uint64_t *>(L.line + (size_t)nd * SKM_LINE);
    L.q_pos = L.cur + nd;
    L.ctr = reinterpret_cast<uint32_t *>(L.q_pos + 16 * SKM_QCAP);
    L.q_d = L.ctr + nd;
    return L;
}
__host__ __device__ static inline size_t skm_stage_bytes(int nd) {
    return (size_t)nd * SKM_LINE * 16 + (size_t)nd * 8 + 16 * SKM_QCAP * 8 + (size_t)nd * 4 + 16 * SKM_QCAP * 4;
}
// The four-wide LDS steps of the staging protocol, each operation under a lane mask of its own: exec is set from the mask (a ballot, so
// a subset of the lanes that are active here) in front of the operation and put back behind the last one, and lanes outside the mask
// touch no LDS -- they used to run the whole protocol against a counter and a slot of their own.  An operation whose mask is empty is
// issued with exec = 0 and does nothing.  A result register keeps its old contents in the lanes outside its mask: the caller reads it
// under the same condition only.  (Inline asm for the reason given in mf_count_dev.h: written as `if`s these become a branch and a
// wait per operation.)
__device__ __forceinline__ void skm_lds_read4_if(const unsigned long long (&m)[4], const uint32_t (&a)[4], uint32_t (&v)[4]) {
    unsigned long long sv;
    asm volatile("s_mov_b64 %4, exec\n\t"
                 "s_mov_b64 exec, %5\n\tds_read_b32 %0, %9\n\t"
                 "s_mov_b64 exec, %6\n\tds_read_b32 %1, %10\n\t"
                 "s_mov_b64 exec, %7\n\tds_read_b32 %2, %11\n\t"
                 "s_mov_b64 exec, %8\n\tds_read_b32 %3, %12\n\t"
                 "s_mov_b64 exec, %4\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&s"(sv)
                 : "s"(m[0]), "s"(m[1]), "s"(m[2]), "s"(m[3]), "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3])
                 : "memory");
}
__device__ __forceinline__ void skm_lds_add_rtn4_if(const unsigned long long (&m)[4], const uint32_t (&a)[4], uint32_t inc, uint32_t (&old)[4]) {
    unsigned long long sv;
    asm volatile("s_mov_b64 %4, exec\n\t"
                 "s_mov_b64 exec, %5\n\tds_add_rtn_u32 %0, %9, %13\n\t"
                 "s_mov_b64 exec, %6\n\tds_add_rtn_u32 %1, %10, %13\n\t"
                 "s_mov_b64 exec, %7\n\tds_add_rtn_u32 %2, %11, %13\n\t"
                 "s_mov_b64 exec, %8\n\tds_add_rtn_u32 %3, %12, %13\n\t"
                 "s_mov_b64 exec, %4\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(old[0]), "=&v"(old[1]), "=&v"(old[2]), "=&v"(old[3]), "=&s"(sv)
                 : "s"(m[0]), "s"(m[1]), "s"(m[2]), "s"(m[3]), "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(inc)
                 : "memory");
}
// a 16-byte store and the returning add that commits it, pair by pair.  LDS operations of one wave execute in order and both halves of
// a pair run under the same mask, so every lane's store is in front of its own commit -- all a commit vouches for is its own slot
__device__ __forceinline__ void skm_lds_write4_add_rtn4_if(const unsigned long long (&m)[4], const uint32_t (&wa)[4], const skm_v4 (&wv)[4],
                                                           const uint32_t (&a)[4], uint32_t inc, uint32_t (&old)[4]) {
    unsigned long long sv;
    asm volatile("s_mov_b64 %4, exec\n\t"
                 "s_mov_b64 exec, %5\n\tds_write_b128 %9, %13\n\tds_add_rtn_u32 %0, %17, %21\n\t"
                 "s_mov_b64 exec, %6\n\tds_write_b128 %10, %14\n\tds_add_rtn_u32 %1, %18, %21\n\t"
                 "s_mov_b64 exec, %7\n\tds_write_b128 %11, %15\n\tds_add_rtn_u32 %2, %19, %21\n\t"
                 "s_mov_b64 exec, %8\n\tds_write_b128 %12, %16\n\tds_add_rtn_u32 %3, %20, %21\n\t"
                 "s_mov_b64 exec, %4\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(old[0]), "=&v"(old[1]), "=&v"(old[2]), "=&v"(old[3]), "=&s"(sv)
                 : "s"(m[0]), "s"(m[1]), "s"(m[2]), "s"(m[3]), "v"(wa[0]), "v"(wa[1]), "v"(wa[2]), "v"(wa[3]),
                   "v"(wv[0]), "v"(wv[1]), "v"(wv[2]), "v"(wv[3]), "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(inc)
                 : "memory");
}
// DYN (one-pass level-1 scatter): a workgroup does not know its share of a digit in advance; it reserves the digit's region
// chunk by chunk (SKM_CH records) with a global atomic when its current chunk is used up.  Chunk starts are multiples of
// SKM_CH and a position is advanced right after it is taken, so "position % SKM_CH == 0" means "no room left".
#define SKM_CH 256
#define SKM_NONE (~0ull)
struct skm_dyn {
    unsigned long long *gcur;     // [nd] next free record of every digit's region
    const uint64_t *rend;         // [nd] end of the region
    unsigned int *overflow;       // set when a region was too small (the caller repeats the level with exact ranges)
    uint64_t dump;                // a scratch chunk of this workgroup: where lines go after an overflow
    unsigned long long *save;     // [G][nd] or null.  STREAMED level 1 (mf_stream.hip: the reads arrive piece by piece, a launch per piece): a workgroup's
                                  // position inside its current chunk of every digit outlives the launch, so that a piece leaves a partly filled LINE per
                                  // workgroup and digit behind, not a partly filled chunk (30 pieces x 256 workgroups x 1024 digits x 256 records = 30 GB of padding)
};
template <bool DYN>
__device__ __forceinline__ uint64_t skm_take_line(const skm_stage &L, uint32_t dg, const skm_dyn &Dy) {
    uint64_t pos = L.cur[dg];
    if (DYN && (pos == SKM_NONE || (pos & (uint64_t)(SKM_CH - 1)) == 0ull)) {
        pos = atomicAdd(&Dy.gcur[dg], (unsigned long long)SKM_CH);
        if (pos + SKM_CH > Dy.rend[dg]) { atomicExch(Dy.overflow, 1u); pos = Dy.dump; }
    }
    L.cur[dg] = pos + SKM_LINE;
    return pos;
}
// ALL 64 lanes of the wave must call this together (wave-uniform loop, wave-cooperative flush)
template <bool DYN = false>
__device__ __forceinline__ void skm_stage_insert(const skm_stage &L, skm_rec *__restrict__ out, const uint32_t (&d)[4],
                                                 const skm_rec (&rec)[4], bool (&pending)[4], const skm_dyn &Dy = skm_dyn()) {
    // (d and rec of a lane that is not pending are never looked at: every LDS step below runs under the mask of the lanes it is for)
    const uint32_t ctr0 = mf_lds_addr(L.ctr), line0 = mf_lds_addr(L.line);
    skm_v4 wv[4];
    uint32_t ca[4], la[4];
#pragma unroll
    for (int b = 0; b < 4; b++) {
        wv[b].x = (uint32_t)rec[b].x; wv[b].y = (uint32_t)(rec[b].x >> 32); wv[b].z = (uint32_t)rec[b].y; wv[b].w = (uint32_t)(rec[b].y >> 32);
        ca[b] = ctr0 + 4u * d[b];
        la[b] = line0 + 16u * SKM_LINE * d[b];
    }
    for (;;) {
        unsigned long long P[4], R[4], G[4];
#pragma unroll
        for (int b = 0; b < 4; b++) P[b] = __ballot(pending[b]);
        if ((P[0] | P[1] | P[2] | P[3]) == 0ull) break;
        uint32_t w[4], old[4], old2[4], wa[4];
        bool got[4];
        // peek: is the line open?  The peek is what bounds the reserved half-word.  A reservation on a full line leaves a surplus there
        // that only the re-opening store wipes; with the peek a record adds to a full line at most once per re-opening (it saw the line
        // open), so the surplus stays below 4 x 1024.  Reserving blindly, a waiting lane would add once per turn of this loop for as long
        // as the line is closed -- up to 256 per wave and turn when one digit takes everything (copies of one read), while the closing
        // wave may be waiting for its chunk (a global atomic, thousands of cycles): 16 waves reach 65536, the carry enters the committed
        // half-word, and a line is written early or never.  So the peek stays.
        // Only pending lanes peek, only lanes that saw their line open reserve, and only lanes that got a slot write and commit.
        skm_lds_read4_if(P, ca, w);
#pragma unroll
        for (int b = 0; b < 4; b++) { got[b] = pending[b] && (w[b] & 0xFFFFu) < (uint32_t)SKM_LINE; R[b] = __ballot(got[b]); }
        skm_lds_add_rtn4_if(R, ca, 1u, old);                                     // reserve a slot
#pragma unroll
        for (int b = 0; b < 4; b++) {
            got[b] = got[b] && (old[b] & 0xFFFFu) < (uint32_t)SKM_LINE;
            wa[b] = la[b] + 16u * (old[b] & (uint32_t)(SKM_LINE - 1));           // (got: the reserved half-word was below SKM_LINE)
            G[b] = __ballot(got[b]);
        }
        skm_lds_write4_add_rtn4_if(G, wa, wv, ca, 0x10000u, old2);               // write the slot, commit
        uint64_t *qpos = L.q_pos + (threadIdx.x >> 6) * SKM_QCAP;
        uint32_t *qd = L.q_d + (threadIdx.x >> 6) * SKM_QCAP;
        const uint64_t lt_mask = (1ull << mf_lane()) - 1ull;
        bool fl4[4], anyfl = false;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            fl4[b] = got[b] && (old2[b] >> 16) == (uint32_t)(SKM_LINE - 1);      // last committer of its line
            anyfl |= fl4[b];
            if (got[b]) pending[b] = false;
        }
        // one ballot for the four flush blocks: a turn in which no line closed (the tail of a batch, a narrow slice) tests nothing else
        if (__ballot(anyfl) == 0ull) continue;                  // (nothing above leaves an LDS operation in flight)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const bool fl = fl4[b];
            const unsigned long long F = __ballot(fl);
            if (F == 0ull) continue;
            const uint32_t n = (uint32_t)__popcll(F), qi = (uint32_t)__popcll(F & lt_mask);
            uint64_t mypos = 0;
            if (fl) mypos = skm_take_line<DYN>(L, d[b], Dy);
            for (uint32_t e0 = 0; e0 < n; e0 += SKM_QCAP) {
                if (fl && qi >= e0 && qi < e0 + SKM_QCAP) { qpos[qi - e0] = mypos; qd[qi - e0] = d[b]; }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // queue visible to the wave (in-order LDS)
                const uint32_t e = e0 + ((uint32_t)mf_lane() >> 2), c = (uint32_t)mf_lane() & 3u;
                if (e < n) {
                    const uint32_t dd = qd[e - e0];
                    const uint64_t pp = qpos[e - e0];
                    const skm_rec v = L.line[dd * SKM_LINE + c];
                    out[pp + c] = v;
                    asm volatile("" ::: "memory");
                    if (c == 0) __hip_atomic_store(&L.ctr[dd], 0u, __ATOMIC_RELEASE, MF_WG);   // reopen (after the reads above)
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // before the queue is reused
            }
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    }
}
// after a barrier: write every partly filled line, padded with sentinel records (DYN: and the unused rest of the
// workgroup's last chunk of every digit, the reader of the region skips sentinels)
template <bool DYN = false>
__device__ __forceinline__ void skm_stage_flush_all(const skm_stage &L, skm_rec *__restrict__ out, int nd, const skm_dyn &Dy = skm_dyn()) {
    const skm_rec SENT = make_ulonglong2(~0ull, ~0ull);
    for (int d = threadIdx.x; d < nd; d += blockDim.x) {
        const uint32_t c = L.ctr[d] >> 16;
        if (c) {
            const uint64_t pos = skm_take_line<DYN>(L, (uint32_t)d, Dy);
            // (the slot is read, then replaced: `s < c ? line : SENT` selects between two ADDRESSES and puts SENT on the stack -- 16 of
            // the kernels' bytes of scratch)
            for (uint32_t s = 0; s < (uint32_t)SKM_LINE; s++) {
                skm_rec v = L.line[d * SKM_LINE + s];
                if (s >= c) v = SENT;
                out[pos + s] = v;
            }
            L.ctr[d] = 0;
        }
        if (DYN) {
            uint64_t pos = L.cur[d];
            if (Dy.save) Dy.save[(size_t)blockIdx.x * nd + d] = pos;         // (k_skm_close_chunks pads them after the last piece)
            else if (pos != SKM_NONE) for (; (pos & (uint64_t)(SKM_CH - 1)) != 0ull; pos++) out[pos] = SENT;
        }
    }
}
// after the last piece of a streamed level 1: the unused rest of every workgroup's current chunk becomes sentinels (positions in the dump
// area -- after an overflow: the level is thrown away -- are left alone)
__global__ void k_skm_close_chunks(const unsigned long long *__restrict__ save, uint64_t n, uint64_t cap, skm_rec *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t pos = save[i];
    if (pos == SKM_NONE || pos >= cap) return;
    const skm_rec SENT = make_ulonglong2(~0ull, ~0ull);
    for (; (pos & (uint64_t)(SKM_CH - 1)) != 0ull; pos++) out[pos] = SENT;
}

// =============================================================================================
// S2: records of every run, radix-partitioned by the level-1 digit
// =============================================================================================
// FAST (level 1 of <= 10 bits: the staging lines leave LDS for it): the runs of a wave's 64 words are dealt EVENLY over its
// lanes through LDS.  A word has 3.7 runs on average but the fullest of 64 has 8 or 9, so four runs per lane and iteration
// meant a second, nearly empty iteration for the whole wave (r02: ~580 of the kernel's 2120 instructions per word), and every
// run slot paid a 41-instruction select tree for the run's minimizer hash (a register array cannot be indexed per lane).  Now:
// every lane parks its word (bases, run starts, valid starts: 24 bytes) and writes one 8-byte descriptor per run -- the loop
// is over the 32 POSITIONS, so the hash is a fixed register, and only the lanes with a run at that position write
// (skm_runlist8) --; then lane l takes the runs l, l + 64, l + 128, l + 192 of the list: one four-wide iteration per 256 runs (237 on
// average per batch).  Rare batches (a run longer than RMAX that must be cut, more runs than the list holds) take the per-lane loop.
// RUNS GO ON ACROSS WORD BOUNDARIES here: a word used to start a new run whatever its first k-mer's minimizer -- a quarter of
// all records began at a word boundary.  Now a lane whose first k-mer continues the previous lane's last run (same minimizer
// hash, both valid: the same read) hands the head of its word over to that run, as far as the run's RMAX allows (`ext`
// k-mers; the rest of the head becomes a run of its own), and the lane that owns the run builds the record from its own 64
// bases + the next lane's (parked) -- 1.75e9 -> ~1.35e9 records at 100 M reads: less to write, to split and to unpack.
#define SKM_LCAP 384               // run descriptors per wave and batch
#define SKM_FAST_WAVE_BYTES (64 * 16 + 64 * 8 + SKM_LCAP * 8)
// Eight positions J0 .. J0 + 7 of the run list.  `c` holds the run starts not yet dealt with, bit-reversed (the next position in the top
// bit); `at` is the lane's next free descriptor.  A position costs three VALU, one SALU and the LDS write: c + c shifts the position's
// bit out as the carry of all 64 lanes (an SGPR pair, eight of them up front), exec is set from that pair, and the tag (lane << 5 | position), the
// (hash, tag) write and the step of `at` run under it -- 12 % of the lanes on average, none of them at a position where no lane of the
// wave starts a run (exec = 0: the three instructions do nothing).  It used to be six VALU and a write per position with a dummy
// slot for the other 88 %.
template <int J0>
__device__ __forceinline__ void skm_runlist8(uint32_t &c, uint32_t &at, uint32_t lane, uint32_t h0, uint32_t h1, uint32_t h2, uint32_t h3,
                                             uint32_t h4, uint32_t h5, uint32_t h6, uint32_t h7) {
    uint32_t t;
    unsigned long long sv, m0, m1, m2, m3, m4, m5, m6, m7;
#define SKM_RL_STEP(M, H, J) "s_mov_b64 exec, %[" M "]\n\tv_lshl_or_b32 %[t], %[lane], 5, %[" J "]\n\tds_write2_b32 %[at], %[" H "], %[t] offset1:1\n\tv_add_u32 %[at], 8, %[at]\n\t"
    asm volatile("v_add_co_u32 %[c], %[m0], %[c], %[c]\n\tv_add_co_u32 %[c], %[m1], %[c], %[c]\n\t"
                 "v_add_co_u32 %[c], %[m2], %[c], %[c]\n\tv_add_co_u32 %[c], %[m3], %[c], %[c]\n\t"
                 "v_add_co_u32 %[c], %[m4], %[c], %[c]\n\tv_add_co_u32 %[c], %[m5], %[c], %[c]\n\t"
                 "v_add_co_u32 %[c], %[m6], %[c], %[c]\n\tv_add_co_u32 %[c], %[m7], %[c], %[c]\n\t"
                 "s_mov_b64 %[sv], exec\n\t"
                 SKM_RL_STEP("m0", "h0", "j0") SKM_RL_STEP("m1", "h1", "j1") SKM_RL_STEP("m2", "h2", "j2") SKM_RL_STEP("m3", "h3", "j3")
                 SKM_RL_STEP("m4", "h4", "j4") SKM_RL_STEP("m5", "h5", "j5") SKM_RL_STEP("m6", "h6", "j6") SKM_RL_STEP("m7", "h7", "j7")
                 "s_mov_b64 exec, %[sv]"
                 : [c] "+v"(c), [at] "+v"(at), [t] "=&v"(t), [sv] "=&s"(sv), [m0] "=&s"(m0), [m1] "=&s"(m1), [m2] "=&s"(m2), [m3] "=&s"(m3),
                   [m4] "=&s"(m4), [m5] "=&s"(m5), [m6] "=&s"(m6), [m7] "=&s"(m7)
                 : [lane] "v"(lane), [h0] "v"(h0), [h1] "v"(h1), [h2] "v"(h2), [h3] "v"(h3), [h4] "v"(h4), [h5] "v"(h5), [h6] "v"(h6), [h7] "v"(h7),
                   [j0] "i"(J0), [j1] "i"(J0 + 1), [j2] "i"(J0 + 2), [j3] "i"(J0 + 3), [j4] "i"(J0 + 4), [j5] "i"(J0 + 5), [j6] "i"(J0 + 6), [j7] "i"(J0 + 7)
                 : "memory");
#undef SKM_RL_STEP
}
template <int K, bool DYN, bool FAST>
__global__ __launch_bounds__(1024) void k_skm_scatter(const uint8_t *__restrict__ bases, uint64_t n_bases, const uint32_t *__restrict__ vmask,
                                                      uint64_t n_words, uint64_t words_per_block, int bits1,
                                                      const uint64_t *__restrict__ blockstart, int G, skm_rec *__restrict__ out, skm_dyn Dy,
                                                      uint32_t dlo, uint32_t dhi) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nd = 1 << bits1;
    skm_stage L = skm_stage_carve(smem, nd);
    if (DYN) Dy.dump += (uint64_t)blockIdx.x * SKM_CH;
    for (int i = threadIdx.x; i < nd; i += blockDim.x) {
        L.cur[i] = DYN ? (Dy.save ? (uint64_t)Dy.save[(size_t)blockIdx.x * nd + i] : SKM_NONE) : blockstart[(size_t)i * G + blockIdx.x];
        L.ctr[i] = 0;
    }
    __syncthreads();
    // FAST: this wave's parking area and run list, behind the staging area
    const uint32_t lane = (uint32_t)mf_lane();
    unsigned char *wbase = smem + ((skm_stage_bytes(nd) + 15) & ~(size_t)15) + (size_t)(threadIdx.x >> 6) * SKM_FAST_WAVE_BYTES;
    uint4 *pd = reinterpret_cast<uint4 *>(wbase);                               // [64] the words' bases
    uint2 *pc = reinterpret_cast<uint2 *>(wbase + 64 * 16);                     // [64] (positions where a run stops, k-mers of the word's head that belong to the previous lane's run)
    uint2 *rl = reinterpret_cast<uint2 *>(wbase + 64 * 16 + 64 * 8);            // [SKM_LCAP] (minimizer hash, lane << 5 | position)
    const uint64_t wlo = (uint64_t)blockIdx.x * words_per_block;
    const uint64_t whi = wlo + words_per_block < n_words ? wlo + words_per_block : n_words;
    // a wave takes 63 words per batch: lane 63 only provides lane 62's halo (skm_scan_word_halo), the word it scans is lane 0's
    // of the wave's next batch
    // (the step and the wave's share as provably wave-uniform values: the loop is then counted in scalar registers.  As 64-bit
    // per-lane values both were spilled to scratch and reloaded every batch)
    const uint64_t wstep = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(blockDim.x >> 6)) * 63u;
    const uint64_t wave0 = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * 63u;
    for (uint64_t wb = wlo; wb < whi; wb += wstep) {          // wave-uniform: all lanes reach skm_stage_insert together
        // the wave's first word of this batch, kept scalar: as (wave0 + lane) + wb the per-lane half lives across the loop -- in scratch
        uint32_t wlo32 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(wb + wave0));
        uint32_t whi32 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((wb + wave0) >> 32));
        asm("" : "+s"(wlo32), "+s"(whi32));
        const uint64_t w = (((uint64_t)whi32 << 32) | wlo32) + lane;
        const uint32_t m = (lane < 63u && w < whi) ? vmask[w] : 0u;
        if (__ballot(m != 0u) == 0ull) continue;
        skm_word<K> S;
        skm_scan_word_halo<K>(S, bases, n_bases, w < n_words ? w : 0, m);
        uint32_t cut = S.cut;
        bool fast = FAST;
        uint32_t NR = 0, roff = 0, cutf = cut, ext = 0;
        if (FAST) {
            // a run of more than RMAX k-mers (RMAX continuation positions in a row) has to be cut: the per-lane loop does that
            constexpr int R = skm_word<K>::RMAX;
            static_assert(R >= 16 && R <= 20, "run-length check");
            const uint32_t z = ~(cut | ~S.valid);
            const uint32_t z2 = z & (z >> 1), z4 = z2 & (z2 >> 2), z8 = z4 & (z4 >> 4), z16 = z8 & (z8 >> 8);
            const uint32_t zr = R == 16 ? z16 : (R == 17 ? (z16 & (z >> 16)) : (R == 18 ? (z16 & (z2 >> 16)) : (R == 19 ? (z16 & (z2 >> 16) & (z >> 18)) : (z16 & (z4 >> 16)))));
            // the head of this word joins the previous lane's last run?  (zr == 0 everywhere, or the batch takes the other path: then
            // the previous lane's last run starts at its highest cut and is at most R k-mers long inside its word)
            const uint32_t pcut = skm_from_prev_lane(cut), pvalid = skm_from_prev_lane(S.valid), pm31 = skm_from_prev_lane(S.mh[31]);
            const bool cont = (S.valid & 1u) && (pvalid >> 31) && S.mh[0] == pm31;
            const uint32_t hstop = (cut & ~1u) | ~S.valid;
            const uint32_t h = hstop ? (uint32_t)__builtin_ctz(hstop) : 32u;
            const uint32_t tail = pcut ? (uint32_t)__builtin_clz(pcut) + 1u : 32u;           // k-mers of that run in the previous word
            // (the owner builds the record from bases 0 .. 79 of its word: the last base of the run, 32 + ext + K - 2, must be one of them)
            constexpr uint32_t XMAX = 49 - K < R ? (uint32_t)(49 - K) : (uint32_t)R;
            uint32_t allowed = tail < (uint32_t)R ? (uint32_t)R - tail : 0u;
            if (allowed > XMAX) allowed = XMAX;
            // (only in the one-pass form: with exact output ranges -- small inputs, the retry after an overflow -- the histogram
            // pass has counted a run per word start, and the ranges must be filled exactly)
            ext = (DYN && cont) ? (h < allowed ? h : allowed) : 0u;
            cutf = ext ? ((cut & ~1u) | (ext < h ? (1u << ext) : 0u)) : cut;
            roff = mf_wave_excl_scan((uint32_t)__popc(cutf), &NR);
            fast = __ballot(zr != 0u) == 0ull && NR <= (uint32_t)SKM_LCAP;
        }
        if (FAST && fast) {
            pd[lane] = make_uint4(S.D[0], S.D[1], S.D[2], S.D[3]);
            pc[lane] = make_uint2(cutf | ~S.valid, ext);                 // (positions where a run stops, k-mers handed to the previous lane's run)
            {
                // (a lane's descriptors are rl[roff .. roff + popc(cutf)): inside the list, NR <= SKM_LCAP here)
                uint32_t at = mf_lds_addr(rl) + 8u * roff, c = __brev(cutf);
                skm_runlist8<0>(c, at, lane, S.mh[0], S.mh[1], S.mh[2], S.mh[3], S.mh[4], S.mh[5], S.mh[6], S.mh[7]);
                skm_runlist8<8>(c, at, lane, S.mh[8], S.mh[9], S.mh[10], S.mh[11], S.mh[12], S.mh[13], S.mh[14], S.mh[15]);
                skm_runlist8<16>(c, at, lane, S.mh[16], S.mh[17], S.mh[18], S.mh[19], S.mh[20], S.mh[21], S.mh[22], S.mh[23]);
                skm_runlist8<24>(c, at, lane, S.mh[24], S.mh[25], S.mh[26], S.mh[27], S.mh[28], S.mh[29], S.mh[30], S.mh[31]);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            for (uint32_t g0 = 0; g0 < NR; g0 += 256) {                     // wave-uniform
                uint32_t d[4]; skm_rec rec[4]; bool pend[4];
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const uint32_t g = g0 + 64u * (uint32_t)b + lane;
                    pend[b] = g < NR;
                    const uint2 de = rl[pend[b] ? g : 0u];
                    const uint32_t src = (de.y >> 5) & 63u, s0 = de.y & 31u;
                    const uint4 Dw = pd[src]; const uint2 cv = pc[src];
                    const uint4 Dn = pd[(src + 1u) & 63u]; const uint2 cn = pc[(src + 1u) & 63u];        // (a run's lane is <= 62)
                    const uint32_t stop = cv.x & ~((2u << s0) - 1u);
                    const uint32_t e = stop ? (uint32_t)__builtin_ctz(stop) : 32u;
                    const uint32_t len = e - s0 + (e == 32u ? cn.y : 0u);                                // + the head of the next word
                    const uint32_t DD[4] = {Dw.x, Dw.y, Dw.z, Dw.w};
                    uint32_t digits;
                    skm_route(de.x, bits1, d[b], digits);
                    rec[b] = skm_make_rec<K>(DD, s0, len, digits, Dn.z);
                    if (d[b] < dlo || d[b] >= dhi) pend[b] = false;                                       // (another slice's record)
                }
                skm_stage_insert<DYN>(L, out, d, rec, pend, Dy);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // (the parked words are rewritten by the next batch)
            __builtin_amdgcn_wave_barrier();
            continue;
        }
        while (__ballot(cut != 0u) != 0ull) {
            uint32_t d[4]; skm_rec rec[4]; bool pend[4];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                pend[b] = cut != 0u;
                d[b] = 0; rec[b] = make_ulonglong2(~0ull, ~0ull);
                if (pend[b]) {
                    uint32_t s, len, digits;
                    skm_next_run<K>(S, cut, s, len);
                    skm_route(skm_mh_at<K>(S, s), bits1, d[b], digits);
                    rec[b] = skm_make_rec<K>(S.D, s, len, digits);
                    if (d[b] < dlo || d[b] >= dhi) { pend[b] = false; d[b] = 0; }      // (another slice's record)
                }
            }
            skm_stage_insert<DYN>(L, out, d, rec, pend, Dy);
        }
    }
    __syncthreads();
    skm_stage_flush_all<DYN>(L, out, nd, Dy);
}

// one-pass level 1: region size of every digit from a sampled histogram, and the directory afterwards
__global__ void k_skm_region_sizes(const uint32_t *__restrict__ blockhist, int G, int nd, uint32_t scale, uint32_t *__restrict__ rsize,
                                   uint32_t dlo, uint32_t dhi) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= nd) return;
    if ((uint32_t)d < dlo || (uint32_t)d >= dhi) { rsize[d] = 0; return; }
    uint64_t t = 0;
    for (int b = 0; b < G; b++) t += blockhist[(size_t)d * G + b];
    t *= scale;
    t += t / 16 + (uint64_t)G * SKM_CH + 8192;          // sampling error + a partly used chunk per workgroup
    t = (t + SKM_CH - 1) & ~(uint64_t)(SKM_CH - 1);
    rsize[d] = t > 0xFFFFFF00ull ? 0xFFFFFF00u : (uint32_t)t;
}
__global__ void k_skm_dir_dyn(const uint64_t *__restrict__ rstart, const unsigned long long *__restrict__ gcur, int nd,
                              uint64_t *__restrict__ pstart, uint32_t *__restrict__ plen) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= nd) return;
    pstart[d] = rstart[d];
    plen[d] = (uint32_t)(gcur[d] - rstart[d]);          // whole chunks; unused records are sentinels
}

// partition directory after level 1: start / padded length per digit; k-mers per digit (plans without a split level)
__global__ void k_skm_dir(const uint64_t *__restrict__ blockstart, const uint32_t *__restrict__ blockocc, int G, int nd,
                          uint64_t *__restrict__ pstart, uint32_t *__restrict__ plen, uint32_t *__restrict__ pocc) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= nd) return;
    const uint64_t s = blockstart[(size_t)d * G], e = blockstart[(size_t)(d + 1) * G];
    pstart[d] = s;
    plen[d] = (uint32_t)(e - s);
    if (blockocc) {
        uint64_t t = 0;
        for (int b = 0; b < G; b++) t += blockocc[(size_t)d * G + b];
        pocc[d] = t > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)t;
    }
}
