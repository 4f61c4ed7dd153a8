// mf_skm_count.h -- super-k-mer counting (mf_skm.hip), S4: k_skm_count (one counting unit per workgroup at a time -> compacted (key,count) slices) and
// the gathers that make the dense table of a batch of units.
#pragma once
#include "mf_skm_split.h"

// =============================================================================================
// S4: count one partition per workgroup.  Second generation: the first one (round 1, profiles/r01j_pmc_100M: 160 VALU lane-
// operations per k-mer occurrence, 76 ms at 100 M reads) probed four-wide with a separate read, CAS and claim-list scan per
// step and expanded records with 64-bit shifts.  What this one is built on (ablations: profiles/r02_count_ablation_*.txt):
//   * all arithmetic on 32-bit halves (v_alignbit funnel shifts, v_bfrev): the 64-bit variable shifts of the record
//     expansion and of mf_revcomp are multi-instruction sequences on CDNA;
//   * the probe IS the claim: one ds_cmpst_rtn_b64(slot, EMPTY, key) per key, four keys per lane.  It returns EMPTY (the
//     slot is ours now), the key (a hit) or another key (a collision, 5 %: those go to the wave's queue and are finished 64
//     at a time, one key per lane).  A separate read first (hits only, first sightings queued) looked cheaper on paper
//     -- a CAS costs its LDS cycles whether 8 lanes or 64 need it -- but all eight waves meet a partition's k-mers at the
//     same time: with the claims deferred, every copy of a new k-mer missed and went through the slow path (27 of 59 ms);
//   * lanes without work are switched off with EXEC inside the asm blocks, not parked on dummy slots (no address selects);
//   * the records are parked in LDS shifted right by ONE bit: the k-mer at base offset t then starts at the odd bit
//     2t+1, so the funnel-shift amount 32 - ((2t+1) & 31) is never 32 and the extraction needs no special case;
//   * the step is software-pipelined over LDS: the next step's item is fetched beside the probes and its record beside the
//     count updates, so one LDS round trip per step is exposed instead of three.
// Items carry everything the consumer lane needs (record slot, funnel-shift amount, word select, k-mers in the item) in
// 16 bits.  Two workgroup barriers per partition (flags are double-buffered by partition parity).
// The all-counts histogram of IOUtils.printKmers (src/io/IOUtils.java:45-71, the .stat.txt file) needs the entries the
// cut drops: their counts (<= thr) are tallied here (count 1 by ballot, the others in a small LDS histogram).
// =============================================================================================
#define C2_WG_PER_CU 2
#define C2_SLOTS 4096            // table slots: at the planned ~800 distinct k-mers per partition the table is 1/5 full.  (2048 slots
                                 // = three workgroups per CU instead of two, but an 80-VGPR budget: 54 ms against 45.)
#define C2_FILL 3400             // claims beyond which a partition is counted again in several passes
#define C2_PASS_GROWTH 4u        // ... their number x 4 after every overflow (x 2: no difference, profiles/r05x_pass_mult.txt)
#define C2_QN 128                // queue entries per wave (keys): drained at 64, one push (<= 64 keys) between checks
#define C2_LH 64                 // bins of the workgroup's dropped-count histogram (a cut with thr >= C2_LH is made after the kernel)
#define C2_ITEMS 848             // item entries per wave: 64 records x 10 items + two steps of padding (the read-ahead of the last step runs past them, unused) + the dummy area of the item stores
#define C2_W 2                   // k-mers per item
#define DD_BITS 11               // bits of a record's index in its unit (the search for identical records: C2_DD * SKM_CT records)
#define C2_DD 4                  // records per thread of a unit whose identical records are counted once (k_skm_count): units of up to C2_DD * SKM_CT records
static constexpr size_t C2_LDS = (size_t)C2_SLOTS * 12 + (size_t)SKM_CT * 16 + (size_t)(SKM_CT / 64) * (C2_ITEMS * 2 + C2_QN * 8 + C2_QN * 2) + 2 * C2_LH * 4 + 48;
static_assert(C2_LDS <= 160 * 1024 / C2_WG_PER_CU, "workgroups per CU");

__device__ __forceinline__ uint32_t c2_swap_pairs(uint32_t x) {                 // exchanges the two bits of every base
    return ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
}
// slot of a key: full-rate instructions only (v_mul_lo_u32 is a quarter-rate instruction, and this is evaluated per k-mer
// occurrence): fold the halves, fold the top bits down, one 24-bit multiply, bits 11..22 of the product
__device__ __forceinline__ uint32_t c2_slot(uint32_t hi, uint32_t lo) {
    uint32_t x = lo ^ __builtin_amdgcn_alignbit(hi, hi, 19);
    x ^= x >> 15;
    uint32_t t;
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(t) : "v"(x), "s"(0x9E3779u));      // (low 24 bits of x) * constant, low 32 bits of the product
    return (t >> 11) & (uint32_t)(C2_SLOTS - 1);
}
struct c2_wave {                 // LDS byte addresses of this wave's private areas + the table
    uint32_t tk0, tc0, rb0, items0, qk0, qw0;
};
// ---- lane masks straight from the compare (a C++ bool that meets __ballot costs a v_cndmask + v_cmp round trip per use)
__device__ __forceinline__ unsigned long long c2_eq_u64(uint64_t a, uint64_t b) {
    unsigned long long m;
    asm("v_cmp_eq_u64_e64 %0, %1, %2" : "=s"(m) : "v"(a), "v"(b));
    return m;
}
__device__ __forceinline__ unsigned long long c2_lt_u32(uint32_t a, uint32_t b) {      // lanes with a < b
    unsigned long long m;
    asm("v_cmp_lt_u32_e64 %0, %1, %2" : "=s"(m) : "v"(a), "v"(b));
    return m;
}
template <int U> __device__ __forceinline__ unsigned long long c2_gt(uint32_t a) {       // lanes with a > U (U: inline constant)
    unsigned long long m;
    asm("v_cmp_lt_u32_e64 %0, %2, %1" : "=s"(m) : "v"(a), "n"(U));
    return m;
}
// Workgroup barrier for LDS traffic only.  __syncthreads() is a workgroup-scope fence + s_barrier, and the fence makes hipcc
// wait for vmcnt(0) first: every wave would sit out the HBM latency of the NEXT partition's record prefetch at each barrier
// (the prefetch is issued a whole partition ahead precisely so that nobody waits for it).  The data the barriers order
// lives in LDS; the global stores of the compaction are read by later kernels only.
__device__ __forceinline__ void c2_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// a wave-uniform 64-bit value that lives in VGPRs -> SGPRs (readfirstlane returns int: no sign extension on the way back)
__device__ __forceinline__ uint64_t c2_uniform64(uint64_t v) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) | ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32);
}
// ---- LDS operations of the lanes of a mask (EXEC is switched inside the block and restored)
__device__ __forceinline__ void c2_push64(unsigned long long m, uint32_t addr, uint64_t v) {
    unsigned long long save;
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %1\n\tds_write_b64 %2, %3\n\ts_mov_b64 exec, %0"
                 : "=&s"(save) : "s"(m), "v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ void c2_push16(unsigned long long m, uint32_t addr, uint32_t v) {
    unsigned long long save;
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %1\n\tds_write_b16 %2, %3\n\ts_mov_b64 exec, %0"
                 : "=&s"(save) : "s"(m), "v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ uint64_t c2_cas_m(unsigned long long m, uint32_t addr, uint64_t key) {      // waited for
    unsigned long long save; uint64_t ret;
    asm volatile("s_mov_b64 %1, exec\n\ts_mov_b64 exec, %2\n\tds_cmpst_rtn_b64 %0, %3, %4, %5\n\ts_mov_b64 exec, %1\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(ret), "=&s"(save) : "s"(m), "v"(addr), "v"(MF_EMPTY), "v"(key) : "memory");
    return ret;
}
__device__ __forceinline__ void c2_add_m(unsigned long long m, uint32_t addr, uint32_t one) {
    unsigned long long save;
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %1\n\tds_add_u32 %2, %3\n\ts_mov_b64 exec, %0"
                 : "=&s"(save) : "s"(m), "v"(addr), "v"(one) : "memory");
}
__device__ __forceinline__ uint32_t c2_lds_u32(const uint32_t *p) {                    // a volatile C++ read of LDS becomes a flat load
    uint32_t v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(mf_lds_addr(p)) : "memory");
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
// finish up to 64 queued keys (collisions), one per lane, by linear probing from the slot AFTER the home slot.  Four slots
// are read ahead per round (reads are cheap and go out together): the key is found (-> count), or an empty slot comes first
// (-> CAS there; if another key got in first, on from the next slot), or neither (-> four slots further).  Most keys need
// one round; one slot per round cost four to six dependent LDS round trips per drain.
__device__ __forceinline__ void c2_drain(const c2_wave &L, uint32_t &qn, uint32_t &won_acc, uint32_t *part_over) {
    const uint32_t lane = (uint32_t)mf_lane();
    constexpr uint32_t mask = (uint32_t)(C2_SLOTS - 1);
    const uint32_t c = qn < 64u ? qn : 64u;
    qn -= c;
    unsigned long long pend = c2_lt_u32(lane, c);
    uint64_t key; uint32_t one;                                                  // (one: the weight of the key's record)
    asm volatile("ds_read_b64 %0, %2\n\tds_read_u16 %1, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(key), "=&v"(one) : "v"(L.qk0 + 8u * (qn + lane)), "v"(L.qw0 + 2u * (qn + lane)) : "memory");   // (idle lanes: an in-range entry)
    uint32_t s = (c2_slot((uint32_t)(key >> 32), (uint32_t)key) + 1u) & mask;
    for (uint32_t probes = 0; pend != 0ull; probes += 4) {
        if (probes >= 256u && ((probes & 255u) == 0u)) {
            if (probes > (uint32_t)C2_SLOTS) { if (lane == 0) *part_over = 1u; break; }
            if (c2_lds_u32(part_over)) break;
        }
        uint32_t a[4]; uint64_t v[4]; unsigned long long save;
#pragma unroll
        for (int j = 0; j < 4; j++) a[j] = L.tk0 + 8u * ((s + (uint32_t)j) & mask);
        asm volatile("s_mov_b64 %4, exec\n\ts_mov_b64 exec, %5\n\tds_read_b64 %0, %6\n\tds_read_b64 %1, %7\n\tds_read_b64 %2, %8\n\tds_read_b64 %3, %9\n\t"
                     "s_mov_b64 exec, %4\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&s"(save)
                     : "s"(pend), "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]) : "memory");
        // first slot among the four that holds the key or is empty
        unsigned long long eK[4], ev[4];
#pragma unroll
        for (int j = 0; j < 4; j++) { eK[j] = c2_eq_u64(v[j], key); ev[j] = eK[j] | c2_eq_u64(v[j], MF_EMPTY); }
        const unsigned long long any = pend & (ev[0] | ev[1] | ev[2] | ev[3]);
        uint32_t j = skm_sel(3u, 2u, ev[2]); j = skm_sel(j, 1u, ev[1]); j = skm_sel(j, 0u, ev[0]);
        const unsigned long long f0 = ev[0], f1 = ev[1] & ~ev[0], f2 = ev[2] & ~(ev[0] | ev[1]), f3 = ev[3] & ~(ev[0] | ev[1] | ev[2]);
        unsigned long long ok = pend & ((f0 & eK[0]) | (f1 & eK[1]) | (f2 & eK[2]) | (f3 & eK[3]));      // found: count
        const unsigned long long need = any & ~ok;                                                          // an empty slot first: claim it
        const uint32_t sj = (s + j) & mask;
        unsigned long long lost = 0ull;
        if (need != 0ull) {
            const uint64_t ret = c2_cas_m(need, L.tk0 + 8u * sj, key);
            const unsigned long long won = need & c2_eq_u64(ret, MF_EMPTY);
            ok |= won | (need & c2_eq_u64(ret, key));
            lost = need & ~ok;                                              // another key got the slot: on from the next one
            won_acc += (uint32_t)__popcll(won);
        }
        c2_add_m(ok, L.tc0 + 4u * sj, one);
        pend &= ~ok;
        s = skm_sel((s + 4u) & mask, (sj + 1u) & mask, lost);
    }
}

// ---- the pipelined step.  State carried from step to step: the item and the parked record of THIS step (fetched during
// the previous one).  An item is up to TWO consecutive k-mers of one record: with four, the last item of a record is half
// empty on average and a step's instructions (VALU and LDS alike cost the same for 8 live lanes as for 64) ran at 71 %
// occupancy; with two at 93 %.  Item entry (16 bits): [0,2) k-mers in the item (0 = the padding after the list), [4,10)
// record slot, [10,16) = 63 - 4c for the record's item c: its low five bits are the funnel-shift amount, bit 15 says that the
// item starts in the record's FIRST word (c < 8) -- one field that falls by 4 from item to item, so the entries of a record
// are e0, e0 - 0x1000, e0 - 0x2000 ... and the list is written without a branch per item (k_skm_count).
template <int K>
__device__ __forceinline__ void c2_step(const c2_wave &L, uint32_t i0, uint32_t &it, skm_v4 &W, uint32_t &it1, uint32_t &qn,
                                        uint32_t &won_acc, uint32_t *part_over, uint32_t P, uint32_t pass) {
    constexpr int sh = 64 - 2 * K;              // 2 .. 24
    constexpr int nb = 2 * K - 34;              // bit of the high word where a new base enters the reverse complement
    const uint32_t lane = (uint32_t)mf_lane();
    const uint32_t nk = it & 3u;
    const uint32_t sa = it >> 10;                                          // funnel-shift amount in the low five bits
    unsigned long long q;                                                  // (VOP3 takes no 32-bit literal on gfx950: the bound sits in an SGPR)
    asm("v_cmp_lt_u32_e64 %0, %2, %1" : "=s"(q) : "v"(it), "s"(0x7FFFu));
    // two k-mers span 2K + 2 <= 64 bits from the item's first base: two funnel shifts over three words
    const uint32_t A = skm_sel(W.y, W.x, q), B = skm_sel(W.z, W.y, q), C = skm_sel(W.w, W.z, q);      // (q: first word)
    const uint32_t hr = __builtin_amdgcn_alignbit(A, B, sa), lr = __builtin_amdgcn_alignbit(B, C, sa);
    uint32_t fh[2], fl[2], ch[2], cl[2];
    fh[0] = hr >> sh; fl[0] = __builtin_amdgcn_alignbit(hr, lr, sh);
    { const uint32_t Vh = __builtin_amdgcn_alignbit(hr, lr, 30), Vl = lr << 2; fh[1] = Vh >> sh; fl[1] = __builtin_amdgcn_alignbit(Vh, Vl, sh); }
    uint32_t rh, rl;
    {
        const uint32_t H = c2_swap_pairs(__builtin_bitreverse32(~fl[0])), Lo = c2_swap_pairs(__builtin_bitreverse32(~fh[0]));
        rh = H >> sh;
        rl = __builtin_amdgcn_alignbit(H, Lo, sh);
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
        if (u) {
            rl = __builtin_amdgcn_alignbit(rh, rl, 2);
            rh = (rh >> 2) | (((~fl[u]) & 3u) << nb);
        }
        const bool lt = (((uint64_t)fh[u] << 32) | fl[u]) < (((uint64_t)rh << 32) | rl);      // one v_cmp_lt_u64
        ch[u] = lt ? fh[u] : rh;
        cl[u] = lt ? fl[u] : rl;
    }
    uint32_t s[2], ka[2]; uint64_t key[2], ret[2]; unsigned long long live[2];
    live[0] = c2_gt<0>(nk); live[1] = c2_gt<1>(nk);
#pragma unroll
    for (int u = 0; u < 2; u++) {
        key[u] = ((uint64_t)ch[u] << 32) | cl[u];
        s[u] = c2_slot(ch[u], cl[u]);
        ka[u] = L.tk0 + 8u * s[u];
    }
    if (P > 1u) {                                   // a partition counted in P passes: this pass takes the keys of its residue class
#pragma unroll
        for (int u = 0; u < 2; u++) live[u] &= c2_lt_u32((skm_pass_of(key[u]) & (P - 1u)) ^ pass, 1u);
    }
    // ---- probes (= claims) of this step, the NEXT step's record and the item of the step after that: one block, one wait.
    // (Everything an asm block reads ahead is waited for inside the same block: a register that is still in flight when the
    // block ends may be copied or spilled by the compiler before the data has landed.)
    uint32_t it2; skm_v4 W_n; unsigned long long save;
    const uint32_t ia2 = L.items0 + 2u * (i0 + 128u + lane);
    const uint32_t ra1 = L.rb0 | (it1 & 0x3F0u);                           // (rb0 is 1024-byte aligned)
    asm volatile("s_mov_b64 %4, exec\n\tds_read_u16 %2, %5\n\tds_read_b128 %3, %6\n\t"
                 "s_mov_b64 exec, %7\n\tds_cmpst_rtn_b64 %0, %9, %11, %12\n\t"
                 "s_mov_b64 exec, %8\n\tds_cmpst_rtn_b64 %1, %10, %11, %13\n\t"
                 "s_mov_b64 exec, %4\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(ret[0]), "=&v"(ret[1]), "=&v"(it2), "=&v"(W_n), "=&s"(save)
                 : "v"(ia2), "v"(ra1), "s"(live[0]), "s"(live[1]), "v"(ka[0]), "v"(ka[1]), "v"(MF_EMPTY), "v"(key[0]), "v"(key[1])
                 : "memory");
    unsigned long long won[2], ok[2], coll[2]; uint32_t aa[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
        won[u] = live[u] & c2_eq_u64(ret[u], MF_EMPTY);
        ok[u] = won[u] | (live[u] & c2_eq_u64(ret[u], key[u]));
        coll[u] = live[u] & ~ok[u];
        aa[u] = L.tc0 + 4u * s[u];
    }
    // ---- count updates of this step (nothing to wait for): + the weight of the item's record (the low half of the parked
    // record's last word: the number of identical records it stands for)
    const uint32_t one = W.w & 0xFFFFu;
    asm volatile("s_mov_b64 %0, exec\n\t"
                 "s_mov_b64 exec, %1\n\tds_add_u32 %3, %5\n\t"
                 "s_mov_b64 exec, %2\n\tds_add_u32 %4, %5\n\t"
                 "s_mov_b64 exec, %0"
                 : "=&s"(save)
                 : "s"(ok[0]), "s"(ok[1]), "v"(aa[0]), "v"(aa[1]), "v"(one)
                 : "memory");
    won_acc += (uint32_t)__popcll(won[0]) + (uint32_t)__popcll(won[1]);
#pragma unroll
    for (int u = 0; u < 2; u++) {
        if (coll[u] != 0ull) {
            const uint32_t at = __builtin_amdgcn_mbcnt_hi((uint32_t)(coll[u] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)coll[u], qn));
            c2_push64(coll[u], L.qk0 + 8u * at, key[u]);
            c2_push16(coll[u], L.qw0 + 2u * at, one);
            qn += (uint32_t)__popcll(coll[u]);
            while (qn >= 64u) c2_drain(L, qn, won_acc, part_over);       // (then qn < 64: + one push <= C2_QN)
        }
    }
    it = it1; W = W_n; it1 = it2;
}

template <int K>
__global__ __launch_bounds__(SKM_CT, 4) void k_skm_count(const skm_rec *__restrict__ recs, const uint64_t *__restrict__ pstart,
                                                           const uint32_t *__restrict__ plen, uint32_t np,
                                                           const uint64_t *__restrict__ toff, uint64_t *__restrict__ tkeys,
                                                           uint16_t *__restrict__ tcnt, uint32_t *__restrict__ dcount,
                                                           unsigned int *__restrict__ overflow, uint32_t p0, uint64_t tbase, int thr,
                                                           unsigned long long *__restrict__ n_all,
                                                           unsigned int *__restrict__ n_redo, unsigned long long *__restrict__ drop_hist,
                                                           unsigned long long *__restrict__ prof_out, uint64_t tcap, uint32_t dedupe,
                                                           unsigned int *__restrict__ unit_ctr) {
    // unit_ctr != nullptr (zero at launch): units are handed out as the workgroups get to them (round 4).  A workgroup's first three
    // units are blockIdx.x + {0, 1, 2} x gridDim.x; every further one is claimed from the counter THREE units ahead -- the directory entry
    // of a unit is asked for two units ahead, and the claim passes through LDS behind a barrier of the unit before that.  With the
    // fixed stride a workgroup's 1024 units add up to a total that differs by a few per cent from workgroup to workgroup (heavy
    // minimizers counted in several passes among them), and a launch ends when the slowest is done.
    // partitions [p0, np); slice of p in tkeys / tcnt starts at toff[p] - tbase; thr >= 0: entries with count <= thr are
    // dropped and tallied in drop_hist[count] (thr < C2_LH); *n_all += distinct k-mers before the cut.
    // (Two neighbouring partitions per table pass, told apart by a tag bit in the key, were tried in round 3: 48.3 ms against
    // 46.6 at 100 M reads -- a table twice as full costs more in collisions and extra passes than the halved per-partition
    // work saves.)
    // NO static __shared__ in this kernel: the dynamic array must start at LDS address 0 (the parked records are
    // addressed with `rb0 | offset`; an alignment attribute on the extern array is not honoured behind static variables)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t wave = threadIdx.x >> 6, lane = (uint32_t)mf_lane();
    skm_v4 *rbuf_all = reinterpret_cast<skm_v4 *>(smem);                        // [SKM_CT] parked records (1 KiB per wave, aligned)
    uint64_t *tk = reinterpret_cast<uint64_t *>(rbuf_all + SKM_CT);             // [C2_SLOTS]
    uint32_t *tc = reinterpret_cast<uint32_t *>(tk + C2_SLOTS);           // [C2_SLOTS]
    uint16_t *items_all = reinterpret_cast<uint16_t *>(tc + C2_SLOTS);    // [waves][C2_ITEMS]
    uint64_t *qk_all = reinterpret_cast<uint64_t *>(items_all + (SKM_CT / 64) * C2_ITEMS);   // [waves][C2_QN]
    uint16_t *qw_all = reinterpret_cast<uint16_t *>(qk_all + (SKM_CT / 64) * C2_QN);         // [waves][C2_QN] the queued keys' weights
    uint32_t *lhist = reinterpret_cast<uint32_t *>(qw_all + (SKM_CT / 64) * C2_QN);          // [C2_LH] dropped counts, committed
    uint32_t *lhist_try = lhist + C2_LH;                                                     // [C2_LH] ... of the running attempt at a partition
    uint32_t (*pflags)[2] = reinterpret_cast<uint32_t (*)[2]>(lhist_try + C2_LH);            // [parity][1] part_over
    uint32_t &out_cursor = lhist_try[C2_LH + 4], &blk_claims = lhist_try[C2_LH + 6];
    uint32_t &dd_gone = lhist_try[C2_LH + 5], &dd_all = lhist_try[C2_LH + 7];                // records that dropped out / that were looked at, of the last such unit
    uint32_t &claim = lhist_try[C2_LH + 8];                                                  // the unit claimed for three units ahead (unit_ctr)
    c2_wave L;
    L.tk0 = mf_lds_addr(tk); L.tc0 = mf_lds_addr(tc);
    L.rb0 = mf_lds_addr(rbuf_all + wave * 64);
    L.items0 = mf_lds_addr(items_all + wave * C2_ITEMS);
    L.qk0 = mf_lds_addr(qk_all + wave * C2_QN);
    L.qw0 = mf_lds_addr(qw_all + wave * C2_QN);
    uint32_t qn = 0, won_acc = 0;                                               // wave-uniform
    unsigned long long all_acc = 0;                                             // per wave: distinct k-mers of its share of the tables
    uint32_t ones_acc = 0;                                                      // per wave: dropped entries with count 1
    // the table is cleared ONCE; after that every partition leaves it clean (its compaction clears the slots it claimed)
    for (uint32_t i = threadIdx.x; i < (uint32_t)C2_SLOTS; i += (uint32_t)SKM_CT) { tk[i] = MF_EMPTY; tc[i] = 0; }
    for (uint32_t i = threadIdx.x; i < 2u * (uint32_t)C2_LH; i += (uint32_t)SKM_CT) lhist[i] = 0;
    if (threadIdx.x == 0) { out_cursor = 0; blk_claims = 0; dd_gone = 0; dd_all = 0; pflags[0][0] = pflags[0][1] = pflags[1][0] = pflags[1][1] = 0; }
    const skm_rec SENT = make_ulonglong2(~0ull, ~0ull);
    const uint32_t mine = (lane >> 3) * (uint32_t)(SKM_NW * 8) + wave * 8u + (lane & 7u);          // this lane's record within a round of SKM_CT
    const uint32_t nu = np - p0;                                                // unit u = partition p0 + u
    uint32_t ui = blockIdx.x;
    if (ui >= nu) return;
    // (an address select between the record and a sentinel object would turn the load into a flat load from scratch)
    // (a uniform base and a 32-bit lane offset: the load takes its address from an SGPR pair + one VGPR, and no 64-bit lane
    // addresses live across the unit loop)
    auto load_rec = [&](uint64_t first, uint32_t j, uint32_t n) -> skm_rec {
        const bool ok = j < n;
        const uint4 *const base = reinterpret_cast<const uint4 *>(recs) + (n ? first : 0ull);
        uint32_t jj = ok ? j : 0u;
        asm volatile("" : "+v"(jj));                       // (the address is made here, not ahead of time and kept -- or spilt -- until here)
        const uint4 w = base[jj];
        skm_rec v = make_ulonglong2(((uint64_t)w.y << 32) | w.x, ((uint64_t)w.w << 32) | w.z);
        if (!ok) v = SENT;
        return v;
    };
    // Directory entries are fetched TWO units ahead, with VECTOR loads: a scalar load (what hipcc makes of a uniform
    // address) is counted in lgkmcnt, and the next LDS wait would sit out its whole memory latency (and hipcc spilt the
    // scalars to VGPR lanes at once, with a wait after every load).  `vz` is a zero the compiler cannot see through.
    // (made anew for every entry: a register that lives across the unit loop is one the allocator may spill, and a reload from
    // scratch waits with vmcnt(0), i.e. for the compaction's stores to be acknowledged -- 13 % of the wave cycles at the loop's top)
    struct dirent { uint64_t start, toff0, toff1; uint32_t len; };
    auto load_dir = [&](uint32_t u) -> dirent {
        uint32_t vz; asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
        dirent d; const uint32_t i = p0 + u + vz;
        d.start = pstart[i]; d.len = plen[i]; d.toff0 = toff[i]; d.toff1 = toff[i + 1];
        return d;
    };
    dirent dc = load_dir(ui);
    uint64_t start = c2_uniform64(dc.start);
    uint32_t len = (uint32_t)__builtin_amdgcn_readfirstlane((int)dc.len);
    uint64_t o = c2_uniform64(dc.toff0) - tbase; uint32_t room = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(dc.toff1 - dc.toff0));
    // ---- identical records are counted once (round 3).  A minimizer partition of deeply sequenced reads holds the same
    // super-k-mer many times over (the same stretch of a genome read again and again: 100 M reads of the benchmark's community
    // have 27 % distinct records, holding 27 % of the k-mers).  A unit of up to C2_DD * SKM_CT records therefore goes through
    // the (empty) k-mer table once as RECORDS: a 64-bit compare-and-swap of (fingerprint, index in the unit) claims a slot;
    // a record that finds its fingerprint there fetches the claimant (L2: the unit has just been read) and, if the two are
    // the same bases, adds itself to the slot's weight and drops out.  The claimants take their weights, hand the slots
    // back, and only they (and the records whose slot was taken by somebody else) are dealt out as items, their weight in the
    // parked record's last word (c2_step adds it instead of 1).  Two more workgroup barriers per unit; exact, because a
    // record only drops out after a full comparison with the record that counts for it.
    // the same load in two halves: the raw words now, the record (or the sentinel) when they are wanted -- nothing looks at the
    // loaded registers in between
    auto load_raw = [&](uint64_t first, uint32_t j, uint32_t n) -> uint4 {
        const uint4 *const base = reinterpret_cast<const uint4 *>(recs) + (n ? first : 0ull);
        uint32_t jj = j < n ? j : 0u;
        asm volatile("" : "+v"(jj));
        return base[jj];
    };
    auto from_raw = [&](const uint4 &w, uint32_t j, uint32_t n) -> skm_rec {
        skm_rec v = make_ulonglong2(((uint64_t)w.y << 32) | w.x, ((uint64_t)w.w << 32) | w.z);
        if (!(j < n)) v = SENT;
        return v;
    };
    auto load4 = [&](uint64_t first, uint32_t n, skm_rec (&R)[C2_DD]) {
#pragma unroll
        for (int i = 0; i < C2_DD; i++) R[i] = load_rec(first, (uint32_t)i * (uint32_t)SKM_CT + mine, n);
    };
    // the record as the steps want it: shifted right by one bit, bases only; `low` = k-mers << 16 | weight
    auto park = [&](const skm_rec &c, uint32_t low, uint32_t slot) {
        const uint32_t x1 = (uint32_t)(c.x >> 32), x0 = (uint32_t)c.x, y1 = (uint32_t)(c.y >> 32), y0 = (uint32_t)c.y & 0xF0000000u;
        skm_v4 Pk;
        Pk.x = x1 >> 1; Pk.y = __builtin_amdgcn_alignbit(x1, x0, 1); Pk.z = __builtin_amdgcn_alignbit(x0, y1, 1); Pk.w = __builtin_amdgcn_alignbit(y1, y0, 1) | low;
        *reinterpret_cast<__attribute__((address_space(3))) skm_v4 *>((uintptr_t)(L.rb0 + 16u * slot)) = Pk;
    };
    // one round of a wave: the records parked in its slots (lane = slot, r = the slot's k-mers) are dealt out as items of two
    // k-mers and inserted; false: nothing to do
    auto run_round = [&](uint32_t r, uint32_t *part_over, uint32_t P, uint32_t pass) {
        const uint32_t nch = (r + (uint32_t)(C2_W - 1)) / (uint32_t)C2_W;
        uint32_t NI;
        const uint32_t ioff = mf_wave_excl_scan(nch, &NI);
        if (NI == 0) return;                                                // wave-uniform
        {   // the record's items: entry c = e0 - c * 0x1000 (two k-mers; see c2_step), lanes without an item c write to
            // their dummy slot -- no branch per item; a last item of ONE k-mer is written again afterwards
            static_assert(C2_W == 2 && C2_ITEMS >= 640 + 128 + 64 + 10, "item list layout");
            const uint32_t e0 = 2u | (lane << 4) | (63u << 10);
            const uint32_t ia = L.items0 + 2u * ioff, dummy = L.items0 + 2u * (uint32_t)(C2_ITEMS - 74) + 2u * lane;
#pragma unroll
            for (int c = 0; c < 10; c++) {
                const uint32_t addr = (uint32_t)c < nch ? ia : dummy;
                const uint32_t e = e0 - (uint32_t)c * 0x1000u;
                asm volatile("ds_write_b16 %0, %1 offset:%2" :: "v"(addr), "v"(e), "n"(2 * c) : "memory");
            }
            if (r & 1u) {
                const uint32_t e = e0 - (nch - 1u) * 0x1000u - 1u;
                *reinterpret_cast<__attribute__((address_space(3))) uint16_t *>((uintptr_t)(ia + 2u * (nch - 1u))) = (uint16_t)e;
            }
        }
        // padding after the list: items without k-mers for the idle lanes of the last step (the step after
        // that is only read ahead, never used)
        {
            const uint32_t z = 0u;
#pragma unroll
            for (int t = 0; t < 2; t++)
                *reinterpret_cast<__attribute__((address_space(3))) uint16_t *>((uintptr_t)(L.items0 + 2u * (NI + 64u * (uint32_t)t + lane))) = (uint16_t)z;
        }
        __builtin_amdgcn_wave_barrier();
        uint32_t it, it1; skm_v4 W;
        // (LDS operations of one wave execute in order: the reads see the stores above without a wait in between)
        asm volatile("ds_read_u16 %0, %2\n\tds_read_u16 %1, %2 offset:128\n\ts_waitcnt lgkmcnt(0)" : "=&v"(it), "=&v"(it1) : "v"(L.items0 + 2u * lane) : "memory");
        asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(W) : "v"(L.rb0 | (it & 0x3F0u)) : "memory");
        for (uint32_t i0 = 0; i0 < NI; i0 += 64) c2_step<K>(L, i0, it, W, it1, qn, won_acc, part_over, P, pass);      // wave-uniform
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                 // items / rbuf are rewritten in the next round
        __builtin_amdgcn_wave_barrier();
    };
    // the records of a unit's first C2_DD rounds are in registers before the unit starts (fetched while the unit before it
    // is worked on); a longer unit fetches every further round while the round before it is worked on
    skm_rec R[C2_DD];
    uint32_t dd_skip = 0, dd_seen = 0;                                          // wave-uniform: units still to go without looking for identical records; units that looked
    load4(start, len, R);
    // (a directory entry lives in VGPRs only while its loads are in flight: once landed it moves to SGPRs)
    struct sdirent { uint64_t start, o; uint32_t len, room; };
    auto to_scalar = [&](const dirent &d) -> sdirent {
        sdirent q; q.start = c2_uniform64(d.start); q.o = c2_uniform64(d.toff0) - tbase;
        q.len = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.len); q.room = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(d.toff1 - d.toff0));
        return q;
    };
    dirent dn = {0, 0, 0, 0};
    uint32_t un = ui + gridDim.x, unn = ui + 2u * gridDim.x;                   // the next unit, and the one after it
    if (un < nu) dn = load_dir(un);
    // (settled before the loop: a load still pending on entry would make the compiler wait at the loop's top -- behind the
    // directory loads it has just issued there -- on every iteration)
    asm volatile("" :: "v"(R[0].x), "v"(R[0].y), "v"(R[1].x), "v"(R[1].y), "v"(R[2].x), "v"(R[2].y), "v"(R[3].x), "v"(R[3].y),
                       "v"(dn.start), "v"(dn.toff0), "v"(dn.toff1), "v"(dn.len));
    static_assert(C2_DD == 4, "the settle lists name R[0..3]");
    sdirent sn = to_scalar(dn);                                                 // the next unit
    __syncthreads();
    uint32_t parity = 0;
    for (;;) {
        bool abandon = false;
        uint32_t claimed = 0; bool claim_pending = false;
        uint32_t next_claim = 0; bool claim_latched = false;                      // the claim as every wave read it behind B1 of the first pass
        if (unit_ctr && threadIdx.x == 0) { claimed = atomicAdd(unit_ctr, 1u); claim_pending = true; }      // (in flight until the unit's first barrier B1)
        dirent dnn = {0, 0, 0, 0};
        bool dnn_asked = false;
        const uint64_t start_n = sn.start;
        const uint32_t len_n = sn.len;
        sdirent snn = {0, 0, 0, 0};                                             // the unit after the next (from dnn, once it has landed)
        // ---- identical records of the unit: weights wl[i] (0: no record, or counted by another one)
        // (reads without depth have nothing to tell apart: where fewer than a quarter of a unit's records dropped out, the next
        // 15 units of this workgroup go without the search; dedupe & 4: never skip -- tests)
        // A unit of more than C2_DD * SKM_CT records: the search covers its first records, the others follow round by round.
        const bool fast = dedupe != 0u && dd_skip == 0u;
        if (dd_skip) dd_skip--;
        uint32_t wl[C2_DD] = {0u, 0u, 0u, 0u};
        if (fast) {
            constexpr uint64_t YM = ~(((1ull << SKM_DIGIT_BITS) - 1ull) << 6);  // (the digit bits say where a record went, not what it holds)
            uint32_t sa[C2_DD], st[C2_DD];                                      // slot address; 1: claimed the slot, 2: found its fingerprint there
            uint64_t ret[C2_DD];
#pragma unroll
            for (int i = 0; i < C2_DD; i++) {
                const bool have = skm_rec_valid(R[i]) && skm_rec_n(R[i]) != 0u;
                wl[i] = have ? 1u : 0u; st[i] = 0; sa[i] = L.tk0; ret[i] = 0;
                if (have) {
                    const uint64_t ym = R[i].y & YM;
                    // (full-rate instructions and one multiply: what two different records share here only costs them their chance)
                    uint32_t h = (uint32_t)(R[i].x >> 32) ^ __builtin_amdgcn_alignbit((uint32_t)R[i].x, (uint32_t)R[i].x, 11)
                                 ^ __builtin_amdgcn_alignbit((uint32_t)(ym >> 32), (uint32_t)(ym >> 32), 21) ^ __builtin_amdgcn_alignbit((uint32_t)ym, (uint32_t)ym, 5);
                    h ^= h >> 16; h *= 0x9E3779B1u; h ^= h >> 15;
                    sa[i] = L.tk0 + 8u * (h & (uint32_t)(C2_SLOTS - 1));
                    const uint64_t word = (1ull << 32) | (uint64_t)(((h >> DD_BITS) << DD_BITS) | ((uint32_t)i * (uint32_t)SKM_CT + mine));
                    asm volatile("ds_cmpst_rtn_b64 %0, %1, %2, %3" : "=&v"(ret[i]) : "v"(sa[i]), "v"(MF_EMPTY), "v"(word) : "memory");
                    st[i] = h >> DD_BITS;                                       // (the fingerprint, until the answer is in)
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            static_assert(C2_DD * SKM_CT <= (1 << DD_BITS), "index in the unit");
            skm_rec G[C2_DD];
#pragma unroll
            for (int i = 0; i < C2_DD; i++) {
                const uint32_t fp = st[i];
                st[i] = 0;
                if (wl[i]) {
                    if (ret[i] == MF_EMPTY) st[i] = 1;
                    else if (((uint32_t)ret[i] >> DD_BITS) == fp) st[i] = 2;
                }
                G[i] = SENT;
                if (st[i] == 2) G[i] = load_rec(start, (uint32_t)ret[i] & ((1u << DD_BITS) - 1u), len);          // the claimant
            }
#pragma unroll
            for (int i = 0; i < C2_DD; i++) {
                if (st[i] == 2 && G[i].x == R[i].x && ((G[i].y ^ R[i].y) & YM) == 0ull) {
                    const uint32_t one = 1u;
                    asm volatile("ds_add_u32 %0, %1 offset:4" :: "v"(sa[i]), "v"(one) : "memory");
                    wl[i] = 0;
                }
            }
            const bool dd_look = (dd_seen++ & 3u) == 0u;                        // (every fourth such unit is looked at)
            if (dd_look) {   // how many dropped out (the next units' decision)
                uint32_t gone = 0, all = 0;
#pragma unroll
                for (int i = 0; i < C2_DD; i++) { gone += (uint32_t)__popcll(__ballot(st[i] == 2 && wl[i] == 0u)); all += (uint32_t)__popcll(__ballot(st[i] != 0u || wl[i] != 0u)); }
                if (lane == 0) { atomicAdd(&dd_gone, gone); atomicAdd(&dd_all, all); }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            c2_barrier();                                                       // ---- every record has claimed, added itself or stays as it is
            if (dd_look) {
                const uint32_t gone = c2_lds_u32(&dd_gone), all = c2_lds_u32(&dd_all);
                if (gone * 4u < all && !(dedupe & 4u)) dd_skip = 15;
            }
            {   // the claimants take their weights and hand the slots back: four exchanges under their lane masks, ONE wait
                static_assert(C2_DD == 4, "four exchanges");
                const unsigned long long m0 = __ballot(st[0] == 1), m1 = __ballot(st[1] == 1), m2 = __ballot(st[2] == 1), m3 = __ballot(st[3] == 1);
                uint64_t v0 = 0, v1 = 0, v2 = 0, v3 = 0; unsigned long long save;
                asm volatile("s_mov_b64 %4, exec\n\t"
                             "s_mov_b64 exec, %5\n\tds_wrxchg_rtn_b64 %0, %9, %13\n\t"
                             "s_mov_b64 exec, %6\n\tds_wrxchg_rtn_b64 %1, %10, %13\n\t"
                             "s_mov_b64 exec, %7\n\tds_wrxchg_rtn_b64 %2, %11, %13\n\t"
                             "s_mov_b64 exec, %8\n\tds_wrxchg_rtn_b64 %3, %12, %13\n\t"
                             "s_mov_b64 exec, %4\n\ts_waitcnt lgkmcnt(0)"
                             : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "=&s"(save)
                             : "s"(m0), "s"(m1), "s"(m2), "s"(m3), "v"(sa[0]), "v"(sa[1]), "v"(sa[2]), "v"(sa[3]), "v"(MF_EMPTY) : "memory");
                if (st[0] == 1) wl[0] = (uint32_t)(v0 >> 32);
                if (st[1] == 1) wl[1] = (uint32_t)(v1 >> 32);
                if (st[2] == 1) wl[2] = (uint32_t)(v2 >> 32);
                if (st[3] == 1) wl[3] = (uint32_t)(v3 >> 32);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            c2_barrier();                                                       // ---- the table is empty again
            if (dd_look && threadIdx.x == 0) { dd_gone = 0; dd_all = 0; }       // (read by everybody before this barrier; added to again a unit later)
        }
        // A unit with more distinct k-mers than the table takes (a heavy minimizer: low-complexity sequence between many
        // different flanks) is counted again in P = 4, 16, 64 passes over its records, pass i inserting the k-mers with
        // skm_pass_of(key) mod P = i; the passes append to the same slices.  More than 64 passes: the global overflow flag,
        // and the caller falls back to the k-mer path.  What a failed attempt tallied is not committed.
        uint32_t P = 1, pass = 0, ones_try = 0, all_try = 0;
        bool have_cur = true;                                                   // R holds THIS unit's records (not yet the next unit's)
        for (;;) {
        P = (uint32_t)__builtin_amdgcn_readfirstlane((int)P); pass = (uint32_t)__builtin_amdgcn_readfirstlane((int)pass);      // (uniform: say so)
        uint32_t *part_over = &pflags[parity][1];
        const bool fetch_next = pass + 1u == P && un < nu;                      // (the pass that is meant to be the unit's last)
        // (Tried: the survivors DEALT evenly over the eight waves through the parked-record area before the barrier that ends the
        // search, so that every unit is one round of equal shares -- 34.2 ms per step round-robin, 34.5 in blocks, against 31.7
        // with every wave parking its own survivors: waves in lock step want the same unit of the CU at the same time.)
        // One loop of rounds for both kinds of unit.  A unit whose identical records have been told apart parks its surviving
        // records 64 to a round (wave by wave: `total` of them in this wave, numbered in the order i, lane); any other unit
        // parks round after round of its records as they come, each lane its own.
        uint32_t total = 0;
        constexpr uint32_t DDN = (uint32_t)(C2_DD * SKM_CT);
        if (fast) {
            if (!have_cur) { load4(start, len, R); have_cur = true; }          // (the pass before fetched the next unit and then overflowed)
#pragma unroll
            for (int i = 0; i < C2_DD; i++) total += (uint32_t)__popcll(__ballot(wl[i] != 0u));
        } else if (!have_cur) { R[0] = load_rec(start, mine, len); have_cur = true; }      // (any other unit: R[0] is the round's record)
        // rounds of surviving records, then rounds of the records as they come (from record `plain0` on)
        const uint32_t n_dense = fast ? (total + 63u) >> 6 : 0u;
        const uint32_t plain0 = fast ? DDN : 0u;
        const uint32_t n_plain = len > plain0 ? (len - plain0 + (uint32_t)SKM_CT - 1u) / (uint32_t)SKM_CT : 0u;
        bool gave_up = false;
        for (uint32_t rr = 0; rr < n_dense; rr++) {
            if (rr && c2_lds_u32(part_over)) { gave_up = true; break; }        // (abandoned)
            uint32_t before = 0;
#pragma unroll
            for (int i = 0; i < C2_DD; i++) {
                const unsigned long long m = __ballot(wl[i] != 0u);
                const uint32_t pos = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, before));
                before += (uint32_t)__popcll(m);
                if (wl[i] != 0u && (pos >> 6) == rr) park(R[i], (skm_rec_n(R[i]) << 16) | wl[i], pos & 63u);
            }
            __builtin_amdgcn_wave_barrier();
            uint32_t w3;
            asm volatile("ds_read_b32 %0, %1 offset:12\n\ts_waitcnt lgkmcnt(0)" : "=v"(w3) : "v"(L.rb0 + 16u * lane) : "memory");
            run_round(lane < total - rr * 64u ? (w3 >> 16) & 63u : 0u, part_over, P, pass);
        }
        if (fast && n_plain != 0u && !gave_up) R[0] = load_rec(start, plain0 + mine, len);      // (a long unit's other records; waited for on the spot)
        for (uint32_t rr = 0; rr < n_plain && !gave_up; rr++) {
            if ((rr || n_dense) && c2_lds_u32(part_over)) break;                // (abandoned)
            // hipcc waits with vmcnt(0) at the first use of a loaded register, i.e. for EVERY load in flight.  This round's
            // records (loaded a round ago) are "used" here, BEFORE the next round's load goes out: the wait the compiler puts
            // in front of this statement finds them landed, and nothing further down waits for the prefetch (with the use
            // after the prefetch every round sat out a full HBM round trip: profiles/r03_count_vmcnt.txt).
            asm volatile("" :: "v"(R[0].x), "v"(R[0].y));
            const uint32_t r = skm_rec_valid(R[0]) ? skm_rec_n(R[0]) : 0u;
            park(R[0], (r << 16) | 1u, lane);
            if (rr + 1u < n_plain) R[0] = load_rec(start, plain0 + (rr + 1u) * (uint32_t)SKM_CT + mine, len);      // the round after this one
            run_round(r, part_over, P, pass);
        }
        if (n_plain) have_cur = false;                                          // (R[0] has moved on, or the pass was abandoned on the way)
        // ---- the next unit's records and the directory entry after it, in ONE place and in straight-line code: they are in
        // flight during the drains, the wait for the other waves and the compaction, and are settled after it.  (Asked for
        // inside the round loops, the compiler joined the loaded registers with the loop's own copies of R right behind the
        // loads -- a copy is a use, and a use waits for the load: every unit sat out an HBM round trip before its first step.)
        // The raw words go into registers of their own (T) and become R only where they are settled: R is carried around the
        // pass loop and the unit loop, and where the loaded registers were R themselves the compiler copied them into R's loop
        // registers right behind the loads.
        uint4 T[C2_DD];
#pragma unroll
        for (int i = 0; i < C2_DD; i++) T[i] = make_uint4(0u, 0u, 0u, 0u);
        if (fetch_next) {
            // (a unit that will not search for identical records takes its rounds one by one: only the first is read ahead)
            const bool next_fast = dedupe != 0u && dd_skip == 0u;
            T[0] = load_raw(start_n, mine, len_n);
            if (next_fast) {
#pragma unroll
                for (int i = 1; i < C2_DD; i++) T[i] = load_raw(start_n, (uint32_t)i * (uint32_t)SKM_CT + mine, len_n);
            }
        }
        if (!dnn_asked) { if (unn < nu) dnn = load_dir(unn); dnn_asked = true; }
        while (qn) c2_drain(L, qn, won_acc, part_over);                        // wave-uniform
        // a crowded table probes slowly: past C2_FILL claims the unit is counted in (more) passes
        if (won_acc) { if (lane == 0) atomicAdd(&blk_claims, won_acc); won_acc = 0; }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the LDS operations of the asm blocks are invisible to hipcc's waitcnt pass
        if (claim_pending) { claim = 3u * gridDim.x + claimed; claim_pending = false; }
        c2_barrier();                                                           // ---- B1: every insert of the pass is done
        const bool over = c2_lds_u32(part_over) != 0u || c2_lds_u32(&blk_claims) > (uint32_t)C2_FILL;
        // (the claim is read HERE, one barrier behind thread 0's write and at least one -- B2 of this unit, or the barriers of
        // its further passes -- before thread 0 writes the next unit's; read at the bottom of the unit loop, a wave that lagged behind B2
        // could have met the newer value when the search for identical records is off and nothing else separates the two)
        if (unit_ctr && !claim_latched) { next_claim = c2_lds_u32(&claim); claim_latched = true; }
        if (threadIdx.x == 0) pflags[parity ^ 1u][1] = 0;                      // for the next pass / unit
        // the records and the directory entries read ahead are settled HERE, before the compaction's stores go out (they had the drains
        // and the wait for the other waves to land): behind the stores the wait would be for the stores' acknowledgements too
        asm volatile("" :: "v"(T[0].x), "v"(T[0].w), "v"(T[1].x), "v"(T[1].w), "v"(T[2].x), "v"(T[2].w), "v"(T[3].x), "v"(T[3].w),
                           "v"(dnn.start), "v"(dnn.toff0), "v"(dnn.toff1), "v"(dnn.len));
        snn = to_scalar(dnn);
        if (fetch_next) {
#pragma unroll
            for (int i = 0; i < C2_DD; i++) R[i] = from_raw(T[i], (uint32_t)i * (uint32_t)SKM_CT + mine, len_n);
            have_cur = false;
        }
        // ---- compaction: every wave sweeps ITS eighth of the table (consecutive slots, lane = slot: conflict-free),
        // 8 chunks of 64 in flight: keys are read and reset with one exchange, the counts of the occupied slots likewise.
        // (Claim lists -- visit only the slots that were won -- cost a list append per key slot in the hot loop and four
        // dependent LDS round trips per 64 entries here; with the table 2/5 full the sweep is cheaper on both counts.)
        {
            constexpr int NCH = 8;                                      // chunks in flight
            static_assert(C2_SLOTS % (SKM_NW * 64 * NCH) == 0, "sweep: whole groups of eight chunks per wave");
#pragma unroll 1
            for (uint32_t g = 0; g < (uint32_t)(C2_SLOTS / (SKM_NW * 64 * NCH)); g++) {
            uint64_t ck[NCH]; uint32_t cc[NCH]; unsigned long long have[NCH], keep[NCH];
            const uint32_t sl0 = wave * (uint32_t)(C2_SLOTS / SKM_NW) + g * (uint32_t)(64 * NCH) + lane;
            const uint32_t ka0 = L.tk0 + 8u * sl0, ca0 = L.tc0 + 4u * sl0;
            const uint64_t E = MF_EMPTY; const uint32_t zero = 0u;
            // (the counters of ALL lanes: an exchange costs the same for 8 lanes as for 64)
            asm volatile("ds_wrxchg_rtn_b64 %0, %16, %17\n\tds_wrxchg_rtn_b64 %1, %16, %17 offset:512\n\tds_wrxchg_rtn_b64 %2, %16, %17 offset:1024\n\t"
                         "ds_wrxchg_rtn_b64 %3, %16, %17 offset:1536\n\tds_wrxchg_rtn_b64 %4, %16, %17 offset:2048\n\tds_wrxchg_rtn_b64 %5, %16, %17 offset:2560\n\t"
                         "ds_wrxchg_rtn_b64 %6, %16, %17 offset:3072\n\tds_wrxchg_rtn_b64 %7, %16, %17 offset:3584\n\t"
                         "ds_wrxchg_rtn_b32 %8, %18, %19\n\tds_wrxchg_rtn_b32 %9, %18, %19 offset:256\n\tds_wrxchg_rtn_b32 %10, %18, %19 offset:512\n\t"
                         "ds_wrxchg_rtn_b32 %11, %18, %19 offset:768\n\tds_wrxchg_rtn_b32 %12, %18, %19 offset:1024\n\tds_wrxchg_rtn_b32 %13, %18, %19 offset:1280\n\t"
                         "ds_wrxchg_rtn_b32 %14, %18, %19 offset:1536\n\tds_wrxchg_rtn_b32 %15, %18, %19 offset:1792\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(ck[0]), "=&v"(ck[1]), "=&v"(ck[2]), "=&v"(ck[3]), "=&v"(ck[4]), "=&v"(ck[5]), "=&v"(ck[6]), "=&v"(ck[7]),
                           "=&v"(cc[0]), "=&v"(cc[1]), "=&v"(cc[2]), "=&v"(cc[3]), "=&v"(cc[4]), "=&v"(cc[5]), "=&v"(cc[6]), "=&v"(cc[7])
                         : "v"(ka0), "v"(E), "v"(ca0), "v"(zero) : "memory");
#pragma unroll
            for (int i = 0; i < NCH; i++) have[i] = ~c2_eq_u64(ck[i], MF_EMPTY) & __builtin_amdgcn_ballot_w64(true);
            if (!over) {
                // (straight-line code: eight chunks of branches -- is there a cut, did anything drop, is anything kept -- cost more
                // than the work they skipped; the cut is one signed compare, count > thr, which holds for every entry when thr = -1)
                uint32_t nkeep = 0, nhave = 0;
                unsigned long long odd = 0ull;                                  // chunks with dropped entries of a count other than 1
#pragma unroll
                for (int i = 0; i < NCH; i++) {
                    asm("v_min_u32 %0, %0, %1" : "+v"(cc[i]) : "s"((uint32_t)MF_MAX_COUNT));
                    unsigned long long gt;
                    asm("v_cmp_gt_i32_e64 %0, %1, %2" : "=s"(gt) : "v"(cc[i]), "s"(thr));
                    keep[i] = have[i] & gt;
                    const unsigned long long drop = have[i] & ~gt;
                    const unsigned long long d1 = drop & c2_lt_u32(cc[i], 2u);       // (count 1: nearly all of them)
                    ones_try += (uint32_t)__popcll(d1);
                    odd |= drop & ~d1;
                    nkeep += (uint32_t)__popcll(keep[i]); nhave += (uint32_t)__popcll(have[i]);
                }
                if (odd != 0ull) {                                              // (rare with the usual cut at 1: never)
#pragma unroll
                    for (int i = 0; i < NCH; i++) {
                        const unsigned long long dx = have[i] & ~keep[i] & ~c2_lt_u32(cc[i], 2u);
                        if ((dx >> lane) & 1ull) atomicAdd(&lhist_try[cc[i]], 1u);
                    }
                }
                all_try += nhave;
                uint32_t wb = 0;
                if (lane == 0 && nkeep) wb = atomicAdd(&out_cursor, nkeep);
                wb = (uint32_t)__builtin_amdgcn_readfirstlane((int)wb);
                if (nkeep && (wb + nkeep > room || o + wb + nkeep > tcap)) {                   // (only if a partition's k-mer count wrapped)
                    if (lane == 0) {
                        if (atomicExch(overflow, 2u) == 0u && prof_out) {
                            prof_out[8] = p0 + ui; prof_out[9] = o; prof_out[10] = room; prof_out[11] = wb; prof_out[12] = nkeep; prof_out[13] = tcap;
                            prof_out[14] = p0; prof_out[15] = np;
                        }
                    }
                }
                else {
                    // the kept entries of a chunk go out under the chunk's lane mask (EXEC is switched around the two stores: a
                    // C++ `if` on the lane's bit is a compare, a saved EXEC and a branch per chunk)
                    uint64_t *const kb = tkeys + o; uint16_t *const cb = tcnt + o;
#pragma unroll
                    for (int i = 0; i < NCH; i++) {
                        const uint32_t at = __builtin_amdgcn_mbcnt_hi((uint32_t)(keep[i] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)keep[i], wb));
                        const uint64_t ka = (uint64_t)(uintptr_t)(kb + at), ca = (uint64_t)(uintptr_t)(cb + at);
                        unsigned long long save;
                        asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %1\n\tglobal_store_dwordx2 %2, %3, off\n\tglobal_store_short %4, %5, off\n\ts_mov_b64 exec, %0"
                                     : "=&s"(save) : "s"(keep[i]), "v"(ka), "v"(ck[i]), "v"(ca), "v"(cc[i]) : "memory");
                        wb += (uint32_t)__popcll(keep[i]);
                    }
                }
            }
        }
        }
        qn = 0;
        c2_barrier();                                                           // ---- B2: the table is clean, the cursors final
        parity ^= 1u;
        if (threadIdx.x == 0) blk_claims = 0;
        bool done = false;
        if (over) {
            // start again with four times the passes; nothing of this attempt counts
            ones_try = 0; all_try = 0; pass = 0;
            if (threadIdx.x == 0) out_cursor = 0;
            if (thr >= 0) for (uint32_t i = threadIdx.x; i < (uint32_t)C2_LH; i += (uint32_t)SKM_CT) lhist_try[i] = 0;
            if (P >= (uint32_t)SKM_MAX_PASSES) { if (threadIdx.x == 0) atomicExch(overflow, 1u); done = true; abandon = true; }
            P *= C2_PASS_GROWTH;
            if (threadIdx.x == 0 && n_redo && P == C2_PASS_GROWTH) atomicAdd(n_redo, 1u);    // (statistics: units counted in several passes)
        } else if (++pass == P) {
            done = true;
            // (wave-uniform sums, and told so: in SGPRs they cost nothing across the unit loop, as VGPRs the allocator spilt them to
            // scratch at the loop's top -- a reload waits with vmcnt(0) for the compaction's stores)
            ones_acc = (uint32_t)__builtin_amdgcn_readfirstlane((int)(ones_acc + ones_try)); all_acc = c2_uniform64(all_acc + all_try);
            if (thr >= 2) for (uint32_t i = threadIdx.x; i < (uint32_t)C2_LH; i += (uint32_t)SKM_CT) { const uint32_t v = lhist_try[i]; if (v) { atomicAdd(&lhist[i], v); lhist_try[i] = 0; } }
        }
        // (said to be uniform: behind an exit the compiler takes for divergent, everything the loop hands on -- the directory
        // entries read ahead among it -- is kept in VGPRs, six more across the unit loop)
        if (__builtin_amdgcn_readfirstlane((int)done)) break;
        c2_barrier();                                                           // (the cursors / the tallies are reset before the next pass appends)
        }
        if (threadIdx.x == 0) { dcount[p0 + ui] = out_cursor; out_cursor = 0; }
        // (a unit beyond SKM_MAX_PASSES: the run is void -- the host sees the flag and takes the k-mer path -- and this workgroup stops
        // here: the registers that were to hold the next unit's records still hold this one's)
        if (__builtin_amdgcn_readfirstlane((int)abandon)) break;
        if (un >= nu) break;
        ui = un; un = unn; unn = unit_ctr ? next_claim : unn + gridDim.x;
        start = start_n; len = len_n;
        o = sn.o; room = sn.room;
        sn = snn;
    }
    {   // distinct k-mers before the cut: one atomic per wave
        if (lane == 0 && n_all && all_acc) atomicAdd(n_all, all_acc);
    }
    if (thr >= 0 && drop_hist) {
        if (lane == 0 && ones_acc) atomicAdd(&lhist[1], ones_acc);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < (uint32_t)C2_LH; i += (uint32_t)SKM_CT) { const uint32_t v = lhist[i]; if (v) atomicAdd(&drop_hist[i], (unsigned long long)v); }
    }
}

// Slices of a batch -> dense table, every COUNTING partition cut in two TABLE partitions on the way: the counting kernel likes
// its partitions twice as large as the graph kernels like theirs (100 M reads: 38.8 ms at 12288 occurrences per partition against
// 44.9 at 6144 -- fixed costs per partition --, while the neighbour lookup's LDS table (mf_nbr.h) wants the ~170 good k-mers of a
// 6144-occurrence partition).  The next bit of the partition hash comes from the k-mer itself (its minimizer: 17 M-mer hashes per
// kept k-mer, ~2 ms at 3.6e8 of them).  One wave per counting partition; the keys with bit 0 grow from the front of the
// partition's range in the dense table, the others from its back (no order inside a partition).
template <int K>
__global__ __launch_bounds__(256) void k_gather_split(const uint64_t *__restrict__ keys, const uint16_t *__restrict__ cnt,
                                                      const uint64_t *__restrict__ pstart, const uint32_t *__restrict__ dcount,
                                                      const uint64_t *__restrict__ coff, uint32_t np, uint64_t *__restrict__ dk,
                                                      uint16_t *__restrict__ dc, uint32_t p0, uint64_t sbase, uint64_t *__restrict__ dfine,
                                                      uint64_t dbase, int bit) {
    // partitions [p0, np) of the counting pass; coff[p]: offset of p's entries in dk / dc (this batch's part of the table, which
    // starts at entry dbase of the whole); dfine[2p], dfine[2p+1] (and dfine[2 np] by the last one): offsets of the table's partitions
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint32_t p = p0 + blockIdx.x * 4u + wave; p < np; p += gridDim.x * 4u) {
        const uint64_t s = pstart[p] - sbase, o = coff[p];
        const uint32_t d = dcount[p];
        uint32_t front = 0, back = d;                                       // wave-uniform
        for (uint32_t j0 = 0; j0 < d; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool have = j < d;
            const uint64_t key = have ? keys[s + j] : 0ull;
            const uint16_t c = have ? cnt[s + j] : (uint16_t)0;
            const bool hi = ((mf_skm_ph(key, K) >> bit) & 1u) != 0u;
            const unsigned long long m1 = __ballot(have && hi), m0 = __ballot(have && !hi);
            const uint32_t n1 = (uint32_t)__popcll(m1), n0 = (uint32_t)__popcll(m0);
            const uint32_t pos = hi ? back - n1 + __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u))
                                    : front + __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, 0u));
            if (have) { dk[o + pos] = key; dc[o + pos] = c; }
            front += n0; back -= n1;
        }
        if (lane == 0) {
            dfine[2 * (size_t)p] = dbase + o;
            dfine[2 * (size_t)p + 1] = dbase + o + front;
            if (p + 1 == np) dfine[2 * (size_t)np] = dbase + coff[np];
        }
    }
}
// The same with every counting partition cut in 2^S table partitions, S = 0 ... 4 (round 4): what the counting kernel likes --
// units of ~2000 distinct k-mers, it pays four workgroup barriers and a sweep of its table per unit -- and what the graph kernels
// like -- ~170 k-mers per table partition, their LDS lookup table takes 352 -- are further apart than a factor of two for
// assembled sequences (the cutter's input: nearly every k-mer distinct, 256 occurrences per table partition) and for shallow
// reads (most distinct k-mers survive the cut).  Two passes over a partition's entries: the bins (the next S bits of each
// k-mer's partition hash) are counted and parked in LDS, then every entry goes to its bin's range; partitions of more than
// GS_CAP entries (counted in several passes: rare) hash twice instead.
#define GS_CAP 4096
template <int K>
__global__ __launch_bounds__(256) void k_gather_split_n(const uint64_t *__restrict__ keys, const uint16_t *__restrict__ cnt,
                                                        const uint64_t *__restrict__ pstart, const uint32_t *__restrict__ dcount,
                                                        const uint64_t *__restrict__ coff, uint32_t np, uint64_t *__restrict__ dk,
                                                        uint16_t *__restrict__ dc, uint32_t p0, uint64_t sbase, uint64_t *__restrict__ dfine,
                                                        uint64_t dbase, int bit, int S) {
    // bit: position of the lowest of the S bits in the partition hash; dfine[(p << S) + b]: first entry of table partition b of p
    __shared__ uint8_t bins_all[4][GS_CAP];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint8_t *const bins = bins_all[wave];
    const uint32_t nb = 1u << S, bmask = nb - 1u;
    for (uint32_t p = p0 + blockIdx.x * 4u + wave; p < np; p += gridDim.x * 4u) {
        const uint64_t s = pstart[p] - sbase, o = coff[p];
        const uint32_t d = dcount[p];
        const bool park = d <= (uint32_t)GS_CAP;
        uint32_t start[16];                                                 // wave-uniform
#pragma unroll
        for (int b = 0; b < 16; b++) start[b] = 0;
        for (uint32_t j0 = 0; j0 < d; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool have = j < d;
            const uint64_t key = have ? keys[s + j] : 0ull;
            const uint32_t bin = (mf_skm_ph(key, K) >> bit) & bmask;
            if (park && have) bins[j] = (uint8_t)bin;
#pragma unroll
            for (int b = 0; b < 16; b++)
                if ((uint32_t)b < nb) start[b] += (uint32_t)__popcll(__ballot(have && bin == (uint32_t)b));
        }
        {   // counts -> first entries
            uint32_t acc = 0;
#pragma unroll
            for (int b = 0; b < 16; b++) { const uint32_t c = start[b]; start[b] = acc; acc += c; }
        }
        if (lane < nb) {
            uint32_t mine = 0;
#pragma unroll
            for (int b = 0; b < 16; b++) if (lane == (uint32_t)b) mine = start[b];
            dfine[((size_t)p << S) + lane] = dbase + o + mine;
        }
        if (lane == 0 && p + 1 == np) dfine[(size_t)np << S] = dbase + coff[np];
        __builtin_amdgcn_wave_barrier();
        for (uint32_t j0 = 0; j0 < d; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool have = j < d;
            const uint64_t key = have ? keys[s + j] : 0ull;
            const uint16_t c = have ? cnt[s + j] : (uint16_t)0;
            const uint32_t bin = park ? (have ? (uint32_t)bins[j] : 0u) : ((mf_skm_ph(key, K) >> bit) & bmask);
            uint32_t pos = 0;
#pragma unroll
            for (int b = 0; b < 16; b++) {
                if ((uint32_t)b < nb) {
                    const unsigned long long m = __ballot(have && bin == (uint32_t)b);
                    if (bin == (uint32_t)b) pos = start[b] + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    start[b] += (uint32_t)__popcll(m);
                }
            }
            if (have) { dk[o + pos] = key; dc[o + pos] = c; }
        }
        __builtin_amdgcn_wave_barrier();
    }
}
__global__ void k_skm_add_base(uint64_t *__restrict__ v, uint64_t n, uint64_t base) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] += base;
}
// capacity of a partition's slice of the temporary (key,count) lists: it cannot hold more distinct k-mers than it has
// k-mers (a partition counted in several passes may hold more than the LDS table)
// ... and with the cut made inside the counting kernel (count > thr) every k-mer that is written stands for at least thr + 1
// occurrences: a partition of o occurrences writes at most o / (thr + 1) entries -- half the temporary lists at the usual thr = 1
// (12 instead of 24 GB for a 20 M-read sample; 26 GB less per slice where 8 x 200 M reads fight for the device)
__global__ void k_skm_cap(const uint32_t *__restrict__ pocc, uint32_t np, uint32_t *__restrict__ cap, uint32_t div) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < np) cap[p] = pocc[p] / div;
}
