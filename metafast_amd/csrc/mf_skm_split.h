// mf_skm_split.h -- super-k-mer counting (mf_skm.hip), the levels after the first: S3 k_skm_split.
#pragma once
#include "mf_skm_scatter.h"

// =============================================================================================
// S3: split every partition into 2^bits sub-partitions by the next digit bits stored in the records
// =============================================================================================
__global__ __launch_bounds__(1024) void k_skm_split(const skm_rec *__restrict__ in, const uint64_t *__restrict__ pstart,
                                                    const uint32_t *__restrict__ plen, uint32_t np, int shift, int bits,
                                                    skm_rec *__restrict__ out, uint64_t *__restrict__ ostart, uint32_t *__restrict__ olen,
                                                    uint32_t *__restrict__ oocc, unsigned long long *__restrict__ n_valid, uint64_t rebase) {
    // rebase: `in` is a buffer shared by several slices (skm_shared) and `out` belongs to this slice: its regions start at 0
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t scratch[17];
    const int nd = 1 << bits;
    const uint32_t dmask = (uint32_t)nd - 1u;
    skm_stage L = skm_stage_carve(smem, nd);
    uint32_t *occ = reinterpret_cast<uint32_t *>(L.line);       // k-mers per digit: lives in the (idle) staging lines during the histogram
    const int ipt = (nd + (int)blockDim.x - 1) / (int)blockDim.x;
    for (uint32_t p = blockIdx.x; p < np; p += gridDim.x) {
        const uint64_t start = pstart[p];
        const uint32_t len = plen[p];
        const uint64_t obase = start - rebase + (uint64_t)p * (uint64_t)(SKM_LINE * nd);   // room for per-digit padding
        for (int i = threadIdx.x; i < nd; i += blockDim.x) { L.ctr[i] = 0; occ[i] = 0; }
        __syncthreads();
        const skm_rec *src = in + start;
        for (uint32_t jb = 0; jb < len; jb += 4 * blockDim.x) {
            skm_rec v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { const uint32_t j = jb + u * blockDim.x + threadIdx.x; v[u] = j < len ? src[j] : make_ulonglong2(~0ull, ~0ull); }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (skm_rec_valid(v[u])) {
                    const uint32_t dg = (skm_rec_digits(v[u]) >> shift) & dmask;
                    atomicAdd(&L.ctr[dg], 1u);
                    if (oocc) atomicAdd(&occ[dg], skm_rec_n(v[u]));
                }
        }
        __syncthreads();
        uint32_t mine = 0, raw = 0;
        const int b0 = threadIdx.x * ipt;
        for (int j = 0; j < ipt; j++) { const int b = b0 + j; if (b < nd) { mine += (L.ctr[b] + 3u) & ~3u; raw += L.ctr[b]; } }
        if (n_valid) {                                            // records without the padding (measurement: mf_table_records)
            for (int dd = 32; dd >= 1; dd >>= 1) raw += __shfl_down(raw, dd, 64);
            if (mf_lane() == 0 && raw) atomicAdd(n_valid, (unsigned long long)raw);
        }
        uint32_t tot;
        uint32_t ex = mf_block_excl_scan(mine, scratch, &tot);
        for (int j = 0; j < ipt; j++) {
            const int b = b0 + j;
            if (b < nd) {
                const uint32_t c = (L.ctr[b] + 3u) & ~3u;
                L.cur[b] = obase + ex;
                ostart[(size_t)p * nd + b] = obase + ex;
                olen[(size_t)p * nd + b] = c;
                if (oocc) oocc[(size_t)p * nd + b] = occ[b];
                ex += c;
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < nd; i += blockDim.x) L.ctr[i] = 0;
        __syncthreads();
        // wave-uniform loop bounds: every lane reaches skm_stage_insert
        for (uint32_t jb = 0; jb < len; jb += 4 * blockDim.x) {
            skm_rec v[4]; uint32_t d[4]; bool pend[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t j = jb + u * blockDim.x + threadIdx.x;
                v[u] = j < len ? src[j] : make_ulonglong2(~0ull, ~0ull);
                pend[u] = skm_rec_valid(v[u]);
                d[u] = pend[u] ? ((skm_rec_digits(v[u]) >> shift) & dmask) : 0u;
            }
            skm_stage_insert(L, out, d, v, pend);
        }
        __syncthreads();
        skm_stage_flush_all(L, out, nd);
        __syncthreads();
    }
}

#define SKM_MAX_PASSES 64
// pass of a key when its partition is counted in several passes (bits independent of the slot hash's)
__device__ __forceinline__ uint32_t skm_pass_of(uint64_t key) {
    uint32_t g = ((uint32_t)(key >> 32) * 0xC2B2AE35u) ^ ((uint32_t)key * 0x27D4EB2Fu);
    g ^= g >> 15; g *= 0x165667B1u;
    return g >> 24;
}
