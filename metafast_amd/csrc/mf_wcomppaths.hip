// mf_wcomppaths.hip -- NO-REFERENCE EXTENSION (32 <= k <= 63): component-paths on wide components.  The semantics are those of
// mf_comppaths.hip word for word, because everything behind the marking kernel IS that file's code: the handle is the same mf_paths, and
// mf_paths_add / finish / stats / slots / text / write run unchanged on (slot, position) records and bytes.  Two things see a k-mer, and
// they are here on two words:
//   create   the listings of the selected components as (hi, lo, slot), ordered by (hi, lo, slot) with three stable pair sorts that carry
//            the listing's index (the slot's bits, the low word, the 2k - 64 bits of the high word: the pattern of mf_wseq2comp.hip's long
//            class) and three gathers; the head flag compares BOTH words; the distinct k-mers stay resident as two arrays under an index
//            of 8-byte slots (position | tag, load <= 0.5, hashed by mf_whash_key: mf_windex_build, the one a wide table has); lo[] and
//            slots[] exactly as for k <= 31.
//   add      k_cp_mark (mf_cp.h) instantiated over cp_keys128: ws2c_roll for the canonical k-mers, mf_windex_find for a k-mer's place
//            among the distinct ones.  The launch shape, the decide step and what it writes are the k <= 31 kernel's.
// Every device loop ends by construction: the index has load <= 0.5, so a probe meets an empty slot.
#include "mf_cp.h"
#include "mf_wide.h"
#include "mf_roll.h"
#include <algorithm>
#include <memory>

struct cp_keys128 {
    mf_windex_view ix;
    template <typename F> __device__ __forceinline__ void each(const uint8_t *__restrict__ p, uint32_t count, int k, F &&f) const {
        ws2c_roll(p, count, k, [&](uint32_t i, uint64_t h, uint64_t l) {
            const uint32_t idx = mf_windex_find(ix, h, l);
            f(i, idx != 0xFFFFFFFFu, idx);
        });
    }
};

// the listings of the selected components in member order: (hi, lo, slot) and the listing's own index
__global__ void k_cp_wmembers(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, const uint32_t *__restrict__ comp, const uint32_t *__restrict__ slot_of,
                              const uint32_t *__restrict__ flag, const uint64_t *__restrict__ rank, uint64_t nk, uint64_t *__restrict__ mhi, uint64_t *__restrict__ mlo,
                              uint32_t *__restrict__ ms, uint64_t *__restrict__ idx) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nk && flag[j]) { const uint64_t d = rank[j]; mhi[d] = hi[j]; mlo[d] = lo[j]; ms[d] = slot_of[comp[j]]; idx[d] = d; }
}
__global__ void k_cp_gather64(const uint64_t *__restrict__ idx, const uint64_t *__restrict__ src, uint64_t n, uint64_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = src[idx[i]];
}
__global__ void k_cp_gather32(const uint64_t *__restrict__ idx, const uint32_t *__restrict__ src, uint64_t n, uint32_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = src[idx[i]];
}
// the listings ordered by (hi, lo, slot): flag[i] = 1 where a new k-mer starts, on EITHER word; a k-mer that does not fit k bases raises *bad
__global__ void k_cp_wheads(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint64_t nm, int k, uint32_t *__restrict__ flag, unsigned int *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nm) return;
    flag[i] = (i == 0 || lo[i] != lo[i - 1] || hi[i] != hi[i - 1]) ? 1u : 0u;
    if (hi[i] >> (2 * k - 64)) atomicOr(bad, 1u);          // (32 <= k <= 63: a shift of 0 .. 62)
}
// the distinct k-mers and the first listing of each (lo[nd] = nm)
__global__ void k_cp_wdistinct(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, const uint32_t *__restrict__ flag, const uint64_t *__restrict__ rank,
                               uint64_t nm, uint64_t *__restrict__ dhi, uint64_t *__restrict__ dlo, uint32_t *__restrict__ first) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nm) return;
    if (i == nm) { first[rank[nm]] = (uint32_t)nm; return; }
    if (flag[i]) { const uint64_t d = rank[i]; dhi[d] = hi[i]; dlo[d] = lo[i]; first[d] = (uint32_t)i; }
}

static int wcp_check_k(const char *who, const char *narrow, int k) {
    if (k < 32 || k > 63) return mf_set_error("%s: 32 <= k <= 63 (k <= 31: %s)", who, narrow);
    return MF_OK;
}

int cp_mark_wide(const mf_paths *P, bool write, const cp_mark_args &a) {
    const cp_members<cp_keys128> M{cp_keys128{mf_windex_view{P->windex.p, P->windex_mask, P->dhi.p, P->dlo.p, nullptr, P->nd, P->k}}, P->lo.p, P->slots.p};
    hipStream_t st = P->ctx->stream;
    const unsigned grid = cp_grid(a.n_runs, CP_WG);
    if (write) k_cp_mark<true><<<grid, CP_WG, 0, st>>>(a.bases, a.off, a.srun, a.n_seqs, a.n_runs, P->k, M, a.cnt_s, a.cnt_e, a.off_s, a.off_e, a.S, a.E);
    else k_cp_mark<false><<<grid, CP_WG, 0, st>>>(a.bases, a.off, a.srun, a.n_seqs, a.n_runs, P->k, M, a.cnt_s, a.cnt_e, a.off_s, a.off_e, a.S, a.E);
    return MF_OK;
}

extern "C" int mf_paths_create_wide(mf_ctx *ctx, mf_wcomps *c, const uint32_t *selection, uint64_t n_selection, int min_len, uint64_t max_paths, mf_paths **out) {
    mf_range rng_("mf:paths_create_wide");
    if (!ctx || !c || !out) return mf_set_error("mf_paths_create_wide: NULL argument");
    *out = nullptr;
    if (c->ctx != ctx) return mf_set_error("mf_paths_create_wide: the components belong to another context");
    MF_TRY(wcp_check_k("mf_paths_create_wide", "mf_paths_create", c->k));
    if (n_selection && !selection) return mf_set_error("mf_paths_create_wide: NULL argument");
    if (c->n >= 0xFFFFFFFFull) return mf_set_error("component-paths: %llu components (fewer than 2^32 - 1)", (unsigned long long)c->n);
    if (c->n_kmers >= 0xFFFFFFFFull) return mf_set_error("component-paths: %llu members (fewer than 2^32 - 1)", (unsigned long long)c->n_kmers);
    if (max_paths >= 0xFFFFFFFFull) return mf_set_error("component-paths: max_paths = %llu (fewer than 2^32 - 1)", (unsigned long long)max_paths);
    MF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::unique_ptr<mf_paths> P(new mf_paths());
    P->ctx = ctx; P->k = c->k; P->wide = true; P->min_len = min_len; P->max_paths = max_paths;
    std::vector<uint32_t> slot_of;
    MF_TRY(cp_slots_of(P.get(), c->n, c->sizes.data(), c->weights.data(), selection, n_selection, slot_of));
    const uint64_t ns = P->n_slots, nk = c->n_kmers;
    const int k = c->k, hb = 2 * k - 64;                   // bits of the high word, 0 .. 62
    if (nk && ns) {
        mf_buf<uint32_t> dslot, flag; mf_buf<uint64_t> rank;
        uint64_t nm = 0;
        MF_TRY(cp_select(ctx, c->comp.p, c->n, nk, slot_of, dslot, flag, rank, &nm));
        P->nm = nm;
        if (nm) {
            mf_buf<uint64_t> shi, slo, tot; mf_buf<unsigned int> bad;
            MF_TRY(shi.alloc(ctx, nm)); MF_TRY(slo.alloc(ctx, nm)); MF_TRY(P->slots.alloc(ctx, nm)); MF_TRY(tot.alloc(ctx, 1)); MF_TRY(bad.alloc(ctx, 1));
            MF_HIP(hipMemsetAsync(bad.p, 0, 4, st));
            {
                mf_buf<uint64_t> mhi, mlo, k1, g, i0, i1; mf_buf<uint32_t> ms, s1;
                MF_TRY(mhi.alloc(ctx, nm)); MF_TRY(mlo.alloc(ctx, nm)); MF_TRY(k1.alloc(ctx, nm)); MF_TRY(g.alloc(ctx, nm)); MF_TRY(i0.alloc(ctx, nm));
                MF_TRY(i1.alloc(ctx, nm)); MF_TRY(ms.alloc(ctx, nm)); MF_TRY(s1.alloc(ctx, nm));
                k_cp_wmembers<<<cp_grid(nk), 256, 0, st>>>(c->hi.p, c->lo.p, c->comp.p, dslot.p, flag.p, rank.p, nk, mhi.p, mlo.p, ms.p, i0.p);
                MF_HIP(hipGetLastError());
                // by slot, then (stable) by the low word, then by the high word: the listings of a k-mer lie together, their slots ascend
                MF_TRY(mf_sort_u32_u64(ctx, ms.p, i0.p, nm, cp_slot_bits(ns), s1.p, i1.p));            // (slot', idx') in (s1, i1)
                k_cp_gather64<<<cp_grid(nm), 256, 0, st>>>(i1.p, mlo.p, nm, g.p);
                MF_TRY(mf_sort_u64_u64(ctx, g.p, i1.p, nm, 64, k1.p, i0.p));                           // (lo'', idx'') in (k1, i0)
                if (hb) {
                    k_cp_gather64<<<cp_grid(nm), 256, 0, st>>>(i0.p, mhi.p, nm, g.p);
                    MF_TRY(mf_sort_u64_u64(ctx, g.p, i0.p, nm, hb, k1.p, i1.p));                       // (hi''', idx''') in (k1, i1)
                } else i1.swap(i0);                                                                    // (k = 32: every high word is 0; one that is not is found below)
                k_cp_gather64<<<cp_grid(nm), 256, 0, st>>>(i1.p, mhi.p, nm, shi.p);                    // the sorted triples: (shi, slo, P->slots)
                k_cp_gather64<<<cp_grid(nm), 256, 0, st>>>(i1.p, mlo.p, nm, slo.p);
                k_cp_gather32<<<cp_grid(nm), 256, 0, st>>>(i1.p, ms.p, nm, P->slots.p);
                MF_HIP(hipGetLastError());
                MF_HIP(hipStreamSynchronize(st));          // (the sort's buffers go back to the arena)
            }
            mf_buf<uint32_t> hflag; mf_buf<uint64_t> hrank;
            MF_TRY(hflag.alloc(ctx, nm)); MF_TRY(hrank.alloc(ctx, nm + 1));
            k_cp_wheads<<<cp_grid(nm), 256, 0, st>>>(shi.p, slo.p, nm, k, hflag.p, bad.p);
            MF_TRY(mf_scan<1>(ctx, hflag.p, hrank.p, nm, tot.p));
            unsigned long long nd = 0; unsigned int h_bad = 0;
            MF_HIP(hipMemcpyAsync(&nd, tot.p, 8, hipMemcpyDeviceToHost, st));
            MF_HIP(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, st));
            MF_HIP(hipStreamSynchronize(st));
            if (h_bad) return mf_set_error("component-paths: a component holds a k-mer that does not fit %d bases", k);
            P->nd = nd;
            MF_TRY(P->dhi.alloc(ctx, nd)); MF_TRY(P->dlo.alloc(ctx, nd)); MF_TRY(P->lo.alloc(ctx, nd + 1));
            k_cp_wdistinct<<<cp_grid(nm + 1), 256, 0, st>>>(shi.p, slo.p, hflag.p, hrank.p, nm, P->dhi.p, P->dlo.p, P->lo.p);
            MF_HIP(hipGetLastError());
            MF_TRY(mf_windex_build(ctx, P->dhi.p, P->dlo.p, nd, k, P->windex, &P->windex_mask));
            MF_HIP(hipGetLastError());
            MF_TRY(cp_max_listings(P.get()));               // (synchronises: the sorted listings go back to the arena)
        }
    }
    MF_HIP(hipStreamSynchronize(st));
    *out = P.release();
    return MF_OK;
}

// ---- the file form (the shape of mf_component_paths) ----
extern "C" int mf_component_paths_wide(mf_ctx *ctx, const char *components_bin, int k, const char *const *files, int nfiles, const uint32_t *selection,
                                       uint64_t n_selection, int min_len, uint64_t max_paths, const char *out_dir, uint64_t *n_components, uint64_t *n_paths) {
    mf_range rng_("mf:component_paths_wide(files)");
    if (!ctx || !components_bin || !out_dir || nfiles < 0 || (nfiles > 0 && !files)) return mf_set_error("mf_component_paths_wide: NULL argument");
    MF_TRY(wcp_check_k("mf_component_paths_wide", "mf_component_paths", k));
    mf_wcomps *c = nullptr;
    MF_TRY(mf_wcomps_load(ctx, components_bin, k, &c));      // (a file of another width or another k stops here, before anything is written)
    std::unique_ptr<mf_wcomps, void (*)(mf_wcomps *)> gc(c, mf_wcomps_destroy);
    mf_paths *P = nullptr;
    MF_TRY(mf_paths_create_wide(ctx, c, selection, n_selection, min_len, max_paths, &P));
    std::unique_ptr<mf_paths, void (*)(mf_paths *)> gp(P, mf_paths_destroy);
    for (int f = 0; f < nfiles; f++) {                     // one file resident at a time, in the order given
        mf_reads *r = nullptr;
        MF_TRY(mf_reads_load(ctx, files + f, 1, &r));
        std::unique_ptr<mf_reads, void (*)(mf_reads *)> gr(r, [](mf_reads *p) { mf_reads_destroy(p); });
        MF_TRY(mf_paths_add(P, r->d_bases, r->d_offsets, r->n, r->n_bases));
    }
    MF_TRY(mf_paths_finish(P));
    MF_TRY(mf_paths_write(P, out_dir, n_paths));
    if (n_components) *n_components = c->n;
    return MF_OK;
}
