// mf_wc2s.h -- what comp2seq on wide components (mf_wcomp2seq.hip) shares with comp2graph on them (mf_wcomp2graph.hip), as mf_c2s.h does
// for the k <= 31 pair: the rows (component, canonical hi, canonical lo, multiplicity) of all components, the pair index over them and the
// per-row flags of k_wc2s_flags.  The kernels stay in mf_wcomp2seq.hip; here are the probe every user of the pair index needs and the host
// entry points.
#pragma once
#include <algorithm>
#include "mf_common.h"
#include "mf_wide.h"
#include "mf_c2s.h"

#define WC2S_EMPTY 0xFFFFFFFFFFFFFFFFull

static inline unsigned wc2s_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 0x7FFFFFFFull); }

// rows sorted by (component, hi, lo)
struct wc2s_rows { mf_buf<uint64_t> hi, lo; mf_buf<uint32_t> comp; mf_buf<uint16_t> cnt; uint64_t n = 0; };
// the pair index: open-addressed over (k-mer, component), 8-byte slots = row (low 32 bits) | tag (the hash's high 32 bits), ~0 = empty,
// load <= 0.5; the key words and the component are read from the row arrays behind a matching tag
struct wc2s_index { const unsigned long long *slots; uint64_t mask; const uint64_t *hi, *lo; const uint32_t *comp; };

#ifdef __HIPCC__
// home slot = low bits of the hash, tag = its high 32 bits
__device__ __forceinline__ uint64_t wc2s_hash(uint64_t hi, uint64_t lo, uint32_t comp) {
    return mf_hash64((lo * 0x9E3779B97F4A7C15ull ^ hi) + (uint64_t)comp * 0xC2B2AE3D27D4EB4Full);
}
// the row of (k-mer, component) or C2S_NONE
__device__ __forceinline__ uint32_t wc2s_find(const wc2s_index &ix, mf_u128 key, uint32_t comp) {
    const uint64_t hi = (uint64_t)(key >> 64), lo = (uint64_t)key;
    const uint64_t h = wc2s_hash(hi, lo, comp);
    const uint32_t tag = (uint32_t)(h >> 32);
    uint64_t s = h & ix.mask;
    for (;;) {                                               // (load <= 0.5: an empty slot is always there)
        const unsigned long long v = ix.slots[s];
        if (v == WC2S_EMPTY) return C2S_NONE;
        if ((uint32_t)(v >> 32) == tag) {
            const uint32_t p = (uint32_t)v;
            if (ix.lo[p] == lo && ix.hi[p] == hi && ix.comp[p] == comp) return p;
        }
        s = (s + 1) & ix.mask;
    }
}
#endif

// who: the entry point or the tool the message names
int wc2s_check_k(const char *who, int k);
int wc2s_member_count(const char *who, const mf_wcomps *c);
// the rows of all components, built from the member lists
int wc2s_build_rows(mf_ctx *ctx, const mf_wcomps *c, wc2s_rows &R);
// the pair index of the rows (ix stays empty without rows); k_wc2s_flags over A.n rows (A.gk = low words, A.ghi = high words) into
// A.info / A.ridx / A.lidx / A.pal
int wc2s_pair_index(mf_ctx *ctx, const wc2s_rows &R, mf_buf<unsigned long long> &slots, wc2s_index *ix);
int wc2s_flags_launch(mf_ctx *ctx, const wc2s_index &ix, const ut_arrays &A);
