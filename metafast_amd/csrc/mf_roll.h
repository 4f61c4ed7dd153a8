// mf_roll.h -- the rolling canonical k-mer over ASCII bases, one thread per stretch of positions (mf_seq2comp.hip, mf_comppaths.hip)
#pragma once
#include "mf_common.h"

#ifdef __HIPCC__
// A0 G1 C2 T3 from the ASCII letter, either case (the decoding of mf_dec4, one byte)
__device__ __forceinline__ uint32_t s2c_code(uint8_t b) {
    const uint32_t t = ((uint32_t)b >> 1) & 3u;
    return (((t ^ (t >> 1)) & 1u) << 1) | (t >> 1);
}
// the canonical k-mers at positions [0, count) of p (count + k - 1 bases are read: k - 1 of lead-in, then one per k-mer)
template <typename F>
__device__ __forceinline__ void s2c_roll(const uint8_t *__restrict__ p, uint32_t count, int k, F &&f) {
    const int top = 2 * k - 2;
    const uint64_t mask = (k == 32) ? ~0ull : ((1ull << (2 * k)) - 1ull);
    uint64_t fw = 0, rc = 0;
    for (int j = 0; j < k - 1; j++) {
        const uint64_t c = s2c_code(p[j]);
        fw = (fw << 2) | c;
        rc = (rc >> 2) | ((3ull - c) << top);
    }
    for (uint32_t i = 0; i < count; i++) {
        const uint64_t c = s2c_code(p[(uint32_t)(k - 1) + i]);
        fw = ((fw << 2) | c) & mask;
        rc = (rc >> 2) | ((3ull - c) << top);
        f(i, fw < rc ? fw : rc);
    }
}
// the same on 2k-bit k-mers, 32 <= k <= 63 (mf_wseq2comp.hip): f(i, high word, low word) of the canonical k-mer at position i
template <typename F>
__device__ __forceinline__ void ws2c_roll(const uint8_t *__restrict__ p, uint32_t count, int k, F &&f) {
    typedef unsigned __int128 u128;
    const int top = 2 * k - 2;                             // 62 .. 124
    const u128 mask = (((u128)1) << (2 * k)) - 1;
    u128 fw = 0, rc = 0;
    for (int j = 0; j < k - 1; j++) {
        const u128 c = s2c_code(p[j]);
        fw = (fw << 2) | c;
        rc = (rc >> 2) | (((u128)3 - c) << top);
    }
    for (uint32_t i = 0; i < count; i++) {
        const u128 c = s2c_code(p[(uint32_t)(k - 1) + i]);
        fw = ((fw << 2) | c) & mask;
        rc = (rc >> 2) | (((u128)3 - c) << top);
        const u128 m = fw < rc ? fw : rc;
        f(i, (uint64_t)(m >> 64), (uint64_t)m);
    }
}
#endif
