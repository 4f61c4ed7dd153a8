// mf_skm_scan.h -- super-k-mer counting (mf_skm.hip), what S1 and S2 share: the 16-byte record, and the minimizer scan of one 32-position word of
// the base stream per lane (minimizer hashes, run starts, the next run, its record, its level-1 digit and the digit bits that travel with it).
#pragma once
#include "mf_common.h"
#include "mf_count_dev.h"

typedef ulonglong2 skm_rec;
typedef uint32_t skm_v4 __attribute__((ext_vector_type(4)));
#define SKM_LINE 4                 // records per 64-byte staging line
#define SKM_QCAP 16
#define SKM_DIGIT_BITS 22          // digit bits stored in a record (levels after the first)
#define SKM_CT 512                 // threads of k_skm_count (1024 with a table twice as large: 25.9 -> 27.9 ms, profiles/r05y_big_units.txt; 256 with half: 35.7 ms, profiles/r06c_small_units.json)
#define SKM_NW (SKM_CT / 64)       // its waves

__device__ __forceinline__ bool skm_rec_valid(const skm_rec &r) { return ((uint32_t)r.y & 63u) != 63u; }
__device__ __forceinline__ uint32_t skm_rec_n(const skm_rec &r) { return (uint32_t)r.y & 63u; }
__device__ __forceinline__ uint32_t skm_rec_digits(const skm_rec &r) { return (uint32_t)(r.y >> 6) & ((1u << SKM_DIGIT_BITS) - 1u); }

// =============================================================================================
// one lane = one 32-position word of the base stream: minimizer hash of each of its 32 k-mers, run starts
// =============================================================================================
template <int K> struct skm_word {
    static constexpr int W = K - mf_skm_m(K) + 1;       // M-mers per k-mer
    static constexpr int NM = 31 + W;                   // M-mers of the word's 32 k-mers
    static constexpr int RMAX = (MF_SKM_BASES - (K - 1)) < 20 ? (MF_SKM_BASES - (K - 1)) : 20;   // k-mers per record (<= 10 items of 2 in k_skm_count)
    uint32_t D[4];        // 64 bases from the word's first position, 2 bits each, first base in the top bits of D[0]
    uint32_t mh[32];      // minimizer hash of the k-mer at each position
    uint32_t valid;       // positions that start a k-mer (from the bitmap)
    uint32_t cut;         // positions where a run starts
};

// run starts from the 32 minimizer hashes.  bit j of `same`: the k-mer at j has the minimizer of the one before it.  Built from the top
// with compare + add-with-carry (two instructions per position instead of compare, select, or)
template <int K>
__device__ __forceinline__ void skm_cut_mask(skm_word<K> &S, uint32_t m) {
    uint32_t acc = 0;
#pragma unroll
    for (int j = 31; j >= 1; j--)
        asm("v_cmp_eq_u32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(acc) : "v"(S.mh[j]), "v"(S.mh[j - 1]) : "vcc");
    const uint32_t same = acc << 1;
    S.cut = m & ~(same & (m << 1));
}

// The reverse complement of 16 bases (first base in the top bits): the last base's complement comes first.  An M-mer's reverse
// complement is then cut out of the reversed words exactly as the M-mer is cut out of the forward ones (funnel shift + shift: two
// instructions) instead of being rolled base by base (shift, and, subtract, shift-or: four) -- with R[3 - q] = skm_rc16(D[q]) the M-mer
// that starts at base i of the 64 has its reverse complement at base 64 - M - i of R[0..3].
__device__ __forceinline__ uint32_t skm_rc16(uint32_t d) {
    const uint32_t r = __brev(~d);
    return ((r & 0xAAAAAAAAu) >> 1) | ((r & 0x55555555u) << 1);
}
// M bases from base p (0 <= p <= 64 - M) of the 64 in X[0..3], right-aligned
template <int M>
__device__ __forceinline__ uint32_t skm_mmer_at(const uint32_t (&X)[4], int p) {
    const int q = p >> 4, o = p & 15;
    const uint32_t top = o ? __builtin_amdgcn_alignbit(X[q], q + 1 < 4 ? X[q + 1] : 0u, 32 - 2 * o) : X[q];
    return top >> (32 - 2 * M);
}

// the second half of the scan: minimizer hash of each of the word's 32 k-mers from its M-mers' hashes, run starts
template <int K>
__device__ __forceinline__ void skm_scan_tail(skm_word<K> &S, uint32_t (&hs)[skm_word<K>::NM], uint32_t m) {
    constexpr int W = skm_word<K>::W, NM = skm_word<K>::NM;
    // sliding-window minimum over W M-mers with three-input minima (v_min3_u32): spans of 3, then of 9, then two (or
    // three) overlapping spans: 118 instructions for W = 17 instead of 214 with doubling
    static_assert(W >= 3 && W <= 18, "window");
    auto min3 = [](uint32_t a, uint32_t b, uint32_t c) { const uint32_t m = a < b ? a : b; return m < c ? m : c; };
#pragma unroll
    for (int i = 0; i + 2 < NM; i++) hs[i] = min3(hs[i], hs[i + 1], hs[i + 2]);                 // hs[i] = min of M-mers i .. i+2
    if (W >= 9) {
#pragma unroll
        for (int i = 0; i + 8 < NM; i++) hs[i] = min3(hs[i], hs[i + 3], hs[i + 6]);             // i .. i+8
#pragma unroll
        for (int j = 0; j < 32; j++) S.mh[j] = hs[j] < hs[j + W - 9] ? hs[j] : hs[j + W - 9];
    } else {
        constexpr int D = W - 3 < 3 ? W - 3 : 3;
#pragma unroll
        for (int j = 0; j < 32; j++) S.mh[j] = min3(hs[j], hs[j + D], hs[j + W - 3]);
    }
    skm_cut_mask<K>(S, m);
}

template <int K>
__device__ __forceinline__ void skm_scan_word(skm_word<K> &S, const uint8_t *__restrict__ bases, uint64_t n_bases, uint64_t w, uint32_t m) {
    constexpr int NM = skm_word<K>::NM, M = mf_skm_m(K);
    // four unconditional 16-byte loads (a guarded `cond ? p[i] : zero` compiles to sixteen predicated dword loads); chunks
    // that start beyond the buffer are re-pointed at the first one and zeroed afterwards
    const uint64_t b0 = w * 32;
    const uint4 *p = reinterpret_cast<const uint4 *>(bases + (b0 < n_bases ? b0 : 0));
    const bool in1 = b0 + 16 < n_bases, in2 = b0 + 32 < n_bases, in3 = b0 + 48 < n_bases;
    const uint4 c0 = p[0], c1 = p[in1 ? 1 : 0], c2 = p[in2 ? 2 : 0], c3 = p[in3 ? 3 : 0];
    S.D[0] = b0 < n_bases ? mf_dec16(c0) : 0u; S.D[1] = in1 ? mf_dec16(c1) : 0u; S.D[2] = in2 ? mf_dec16(c2) : 0u; S.D[3] = in3 ? mf_dec16(c3) : 0u;
    S.valid = m;
    uint32_t hs[NM];
    const uint32_t R[4] = {skm_rc16(S.D[3]), skm_rc16(S.D[2]), skm_rc16(S.D[1]), skm_rc16(S.D[0])};
#pragma unroll
    for (int i = 0; i < NM; i++) {             // (the last M-mer ends at base NM + M - 2 = K + 29 < 64)
        const uint32_t f = skm_mmer_at<M>(S.D, i), r = skm_mmer_at<M>(R, 64 - M - i);
        hs[i] = mf_mmer_hash(f < r ? f : r, M);
    }
    skm_scan_tail<K>(S, hs, m);
}
// The same scan with the HALO taken from the next lane: a word's 32 k-mers need the M-mers of 48 positions and 64 bases, the
// last 16 / 32 of which are the next word's first ones -- which the next lane computes anyway.  v_mov_b32_dpp wave_shl:1 hands
// them over (18 moves instead of two 16-byte loads, their decoding and 16 M-mer hashes: ~170 of the scan's ~900 instructions).
// Lane 63 has no next lane: the caller gives it no k-mers of its own (it scans the word that lane 0 of the wave's NEXT batch
// owns), a wave covers 63 words.
__device__ __forceinline__ uint32_t skm_from_next_lane(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /* wave_shl:1 */, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t skm_from_prev_lane(uint32_t v) {          // (lane 0: 0)
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}
template <int K>
__device__ __forceinline__ void skm_scan_word_halo(skm_word<K> &S, const uint8_t *__restrict__ bases, uint64_t n_bases, uint64_t w, uint32_t m) {
    constexpr int NM = skm_word<K>::NM, M = mf_skm_m(K);
    const uint64_t b0 = w * 32;
    const uint4 *p = reinterpret_cast<const uint4 *>(bases + (b0 < n_bases ? b0 : 0));
    const bool in1 = b0 + 16 < n_bases;
    const uint4 c0 = p[0], c1 = p[in1 ? 1 : 0];
    S.D[0] = b0 < n_bases ? mf_dec16(c0) : 0u; S.D[1] = in1 ? mf_dec16(c1) : 0u;
    S.D[2] = skm_from_next_lane(S.D[0]); S.D[3] = skm_from_next_lane(S.D[1]);
    S.valid = m;
    // the lane's own 32 M-mers end by base 31 + M - 1 < 48: their reverse complements lie in R[1..3], and R[1] = rc(D[2]) is the next
    // lane's rc(D[0]); R[0] is not read
    static_assert(64 - M - 31 >= 16, "reversed words");
    const uint32_t R3 = skm_rc16(S.D[0]);
    const uint32_t R[4] = {0u, skm_from_next_lane(R3), skm_rc16(S.D[1]), R3};
    uint32_t hs[34];
#pragma unroll
    for (int i = 0; i < 32; i++) {
        const uint32_t f = skm_mmer_at<M>(S.D, i), r = skm_mmer_at<M>(R, 64 - M - i);
        hs[i] = mf_mmer_hash(f < r ? f : r, M);
    }
    // The sliding minimum of skm_scan_tail with the halo taken as late as possible: a minimum over M-mers 32 .. of this word is the
    // next lane's minimum over its M-mers 0 .., so the next lane's partial minima are moved instead of its hashes (W = 17: 2 + 6 + 8
    // moves and 3 x 32 minima instead of 16 moves and 118 minima).  Every value moved depends on the next lane's OWN hashes only.
    constexpr int W = skm_word<K>::W;
    static_assert(W >= 3 && W <= 18, "window");
    static_assert(NM <= 64, "halo");
    auto min3 = [](uint32_t a, uint32_t b, uint32_t c) { const uint32_t m = a < b ? a : b; return m < c ? m : c; };
    hs[32] = skm_from_next_lane(hs[0]); hs[33] = skm_from_next_lane(hs[1]);
    uint32_t a[38];
#pragma unroll
    for (int i = 0; i < 32; i++) a[i] = min3(hs[i], hs[i + 1], hs[i + 2]);                     // M-mers i .. i+2
    if (W >= 9) {
        uint32_t b[32 + 9];
#pragma unroll
        for (int i = 32; i < 38; i++) a[i] = skm_from_next_lane(a[i - 32]);
#pragma unroll
        for (int i = 0; i < 32; i++) b[i] = min3(a[i], a[i + 3], a[i + 6]);                    // i .. i+8
#pragma unroll
        for (int i = 32; i < 32 + W - 9; i++) b[i] = skm_from_next_lane(b[i - 32]);
#pragma unroll
        for (int j = 0; j < 32; j++) S.mh[j] = b[j] < b[j + W - 9] ? b[j] : b[j + W - 9];
    } else {
        constexpr int D = W - 3 < 3 ? W - 3 : 3;
#pragma unroll
        for (int i = 32; i < 32 + W - 3; i++) a[i] = skm_from_next_lane(a[i - 32]);
#pragma unroll
        for (int j = 0; j < 32; j++) S.mh[j] = min3(a[j], a[j + D], a[j + W - 3]);
    }
    skm_cut_mask<K>(S, m);
}

// lane-wise m ? b : a as ONE v_cndmask.  Written in C++ (`c ? x[2i+1] : x[2i]`) hipcc turns the select between two
// neighbouring array elements into a load with a run-time index, i.e. the whole register array goes to scratch memory and
// every select becomes a scratch round trip (k_skm_hist spent 40 % of its wave time in s_waitcnt on those).
__device__ __forceinline__ uint32_t skm_sel(uint32_t a, uint32_t b, unsigned long long m) {
    uint32_t r;
    asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(m));
    return r;
}
// S.mh[s] for a per-lane s: binary select tree over the register array
template <int K>
__device__ __forceinline__ uint32_t skm_mh_at(const skm_word<K> &S, uint32_t s) {
    uint32_t a[16], b[8], c[4], d[2];
    const unsigned long long s0 = __ballot((s & 1u) != 0), s1 = __ballot((s & 2u) != 0), s2 = __ballot((s & 4u) != 0),
                             s3 = __ballot((s & 8u) != 0), s4 = __ballot((s & 16u) != 0);
#pragma unroll
    for (int i = 0; i < 16; i++) a[i] = skm_sel(S.mh[2 * i], S.mh[2 * i + 1], s0);
#pragma unroll
    for (int i = 0; i < 8; i++) b[i] = skm_sel(a[2 * i], a[2 * i + 1], s1);
#pragma unroll
    for (int i = 0; i < 4; i++) c[i] = skm_sel(b[2 * i], b[2 * i + 1], s2);
#pragma unroll
    for (int i = 0; i < 2; i++) d[i] = skm_sel(c[2 * i], c[2 * i + 1], s3);
    return skm_sel(d[0], d[1], s4);
}

// takes the next run off `cut`: start s, number of k-mers len (<= RMAX; a longer run leaves its rest in `cut`)
template <int K>
__device__ __forceinline__ void skm_next_run(const skm_word<K> &S, uint32_t &cut, uint32_t &s, uint32_t &len) {
    s = (uint32_t)__builtin_ctz(cut);
    cut &= cut - 1u;
    const uint32_t stop = (cut | ~S.valid) & ~((2u << s) - 1u);
    const uint32_t e = stop ? (uint32_t)__builtin_ctz(stop) : 32u;
    len = e - s;
    if (len > (uint32_t)skm_word<K>::RMAX) { len = (uint32_t)skm_word<K>::RMAX; cut |= 1u << (s + len); }
}

// the record of the run [s, s+len): its len+K-1 bases left-aligned, the remaining bits zero, digit bits, k-mer count
template <int K>
__device__ __forceinline__ skm_rec skm_make_rec(const uint32_t (&D)[4], uint32_t s, uint32_t len, uint32_t digits, uint32_t D4 = 0u) {
    // D4: bases 64 .. 79 from the word's start (a run that goes on into the next word, k_skm_scatter)
    const uint32_t o = (2u * s) & 31u;
    const unsigned long long q = __ballot(s >= 16u);
    // (a run from s < 16 may need base 64, the first of D4; one from s >= 16 ends by base 79: the caller bounds its length)
    const uint32_t E0 = skm_sel(D[0], D[1], q), E1 = skm_sel(D[1], D[2], q), E2 = skm_sel(D[2], D[3], q), E3 = skm_sel(D[3], D4, q), E4 = skm_sel(D4, 0u, q);
    uint32_t T0 = E0, T1 = E1, T2 = E2, T3 = E3;
    if (o) {
        T0 = __builtin_amdgcn_alignbit(E0, E1, 32u - o);
        T1 = __builtin_amdgcn_alignbit(E1, E2, 32u - o);
        T2 = __builtin_amdgcn_alignbit(E2, E3, 32u - o);
        T3 = __builtin_amdgcn_alignbit(E3, E4, 32u - o);
    }
    // bits to keep: 2 K <= kb <= 100, so T0 stays whole; T0:T1 keep their top min(kb, 64) bits and T2:T3 their top max(kb - 64, 0): two
    // 64-bit shifts and three ands instead of a compare-and-select pair per dword
    static_assert(K >= 17 && K <= 32, "the first dword is kept whole");
    const int kb = 2 * (int)(len + K - 1);
    const uint64_t m01 = (uint64_t)((int64_t)0x8000000000000000ull >> ((kb < 64 ? kb : 64) - 1));
    const uint64_t m23 = ~(~0ull >> (kb > 64 ? kb - 64 : 0));
    T1 &= (uint32_t)m01; T2 &= (uint32_t)(m23 >> 32); T3 &= (uint32_t)m23;
    skm_rec r;
    r.x = ((uint64_t)T0 << 32) | T1;
    r.y = ((uint64_t)T2 << 32) | (uint64_t)(T3 & 0xF0000000u) | ((uint64_t)digits << 6) | (uint64_t)len;
    return r;
}
// level-1 digit and the digit bits that travel in the record, from the run's minimizer hash
__device__ __forceinline__ void skm_route(uint32_t mh, int bits1, uint32_t &d1, uint32_t &digits) {
    const uint32_t ph = mf_remix32(mh);
    d1 = bits1 ? ph >> (32 - bits1) : 0u;
    digits = (bits1 ? (ph << bits1) : ph) >> (32 - SKM_DIGIT_BITS);
}
