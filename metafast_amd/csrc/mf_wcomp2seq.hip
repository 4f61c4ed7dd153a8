// mf_wcomp2seq.hip -- NO-REFERENCE EXTENSION (32 <= k <= 63): comp2seq on wide components -- the contigs of every component of a wide
// components.bin in ONE segmented unitig build.  The stages are those of mf_comp2seq.hip on 2k-bit k-mers:
//
//   rows          (component, canonical hi, canonical lo, multiplicity inside the component) of every member, sorted by (component, hi, lo):
//                 three stable radix passes that carry the member's index -- the low word, the 2k - 64 bits of the high word, the component
//                 bits --, the runs of equal triples counted (capped as the counter caps).  A row's place orders like (component, k-mer):
//                 k_ut_ends<W> keys a path by its start row's place and the ordered export sorts by it
//   pair index    open-addressed over (k-mer, component), 8-byte slots = row (low 32 bits) | tag (the hash's high 32 bits), ~0 = empty,
//                 load <= 0.5; the key words and the component are read from the row arrays behind a matching tag (as mf_windex_find); the
//                 hash is the k-mer's folded with the component.  A k-mer that is a member of several components has a slot and a row in each
//   k_wc2s_flags  U1 restricted to a component: k_w_ut_flags with every neighbour looked up as (neighbour, this row's component)
//   U2 .. U5      mf_ut_build, unchanged, with the rows' components as group ids
//
// Without split the route is one wide table of all members (mf_wide_merge_runs, shared with mf_wtable_load_kmers) and
// mf_build_unitigs_wide_device.  A member list may hold x and rc(x) (the loader asks for ascending members below 4^k, not for canonical
// ones): after canonicalisation that k-mer has multiplicity 2.
#include <algorithm>
#include <fcntl.h>
#include <map>
#include <memory>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include "mf_wc2s.h"

// members -> canonical k-mers; a member that does not fit 2k bits raises bit 0 of *flags
__global__ __launch_bounds__(256) void k_wc2s_canon(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint64_t n, int k, uint64_t *__restrict__ ohi,
                                                    uint64_t *__restrict__ olo, uint16_t *__restrict__ ones, unsigned int *__restrict__ flags) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int hb = 2 * k - 64;                                                   // bits of the high word, 0 .. 62
    uint64_t h = hi[i];
    if ((h >> hb) != 0) { atomicOr(flags, 1u); h &= (1ull << hb) - 1ull; }
    const mf_u128 x = ((mf_u128)h << 64) | (mf_u128)lo[i], r = mf_wrevcomp(x, k), c = x < r ? x : r;
    ohi[i] = (uint64_t)(c >> 64); olo[i] = (uint64_t)c;
    if (ones) ones[i] = 1;
}
__global__ void k_wc2s_iota(uint64_t *__restrict__ v, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = i;
}
__global__ void k_wc2s_gather64(const uint64_t *__restrict__ idx, const uint64_t *__restrict__ src, uint64_t n, uint64_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = src[idx[i]];
}
__global__ void k_wc2s_gather32(const uint64_t *__restrict__ idx, const uint32_t *__restrict__ src, uint64_t n, uint32_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = src[idx[i]];
}
// sorted (component, hi, lo) triples: head[i] = 1 where a run of equal triples starts
__global__ __launch_bounds__(256) void k_wc2s_heads(const uint32_t *__restrict__ comp, const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint64_t n,
                                                    uint32_t *__restrict__ head) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || comp[i] != comp[i - 1] || lo[i] != lo[i - 1] || hi[i] != hi[i - 1]) ? 1u : 0u;
}
// row r = the r-th run: its triple and where it starts
__global__ __launch_bounds__(256) void k_wc2s_rows(const uint32_t *__restrict__ comp, const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo,
                                                   const uint32_t *__restrict__ head, const uint64_t *__restrict__ idx, uint64_t n, uint64_t *__restrict__ rhi,
                                                   uint64_t *__restrict__ rlo, uint32_t *__restrict__ rcomp, uint32_t *__restrict__ rstart) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !head[i]) return;
    const uint64_t r = idx[i];
    rhi[r] = hi[i]; rlo[r] = lo[i]; rcomp[r] = comp[i]; rstart[r] = (uint32_t)i;
}
__global__ __launch_bounds__(256) void k_wc2s_counts(const uint32_t *__restrict__ rstart, uint64_t n_rows, uint64_t n, uint16_t *__restrict__ rcnt) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const uint64_t len = (r + 1 < n_rows ? (uint64_t)rstart[r + 1] : n) - (uint64_t)rstart[r];
    rcnt[r] = (uint16_t)(len > (uint64_t)MF_MAX_COUNT ? (uint64_t)MF_MAX_COUNT : len);
}

// ---- the wide pair index (wc2s_hash, wc2s_find: mf_wc2s.h)
// the rows' (k-mer, component) pairs are all different: a row takes the first empty slot of its probe sequence
__global__ __launch_bounds__(256) void k_wc2s_index_insert(unsigned long long *__restrict__ slots, uint64_t mask, const uint64_t *__restrict__ rhi,
                                                           const uint64_t *__restrict__ rlo, const uint32_t *__restrict__ rcomp, uint64_t n_rows) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const uint64_t h = wc2s_hash(rhi[r], rlo[r], rcomp[r]);
    const unsigned long long ent = (h & 0xFFFFFFFF00000000ull) | (unsigned long long)(uint32_t)r;
    uint64_t s = h & mask;
    for (;;) {                                               // (load <= 0.5: an empty slot is always there)
        if (slots[s] == WC2S_EMPTY && atomicCAS(&slots[s], WC2S_EMPTY, ent) == WC2S_EMPTY) break;
        s = (s + 1) & mask;
    }
}
// U1 restricted to a component: k_w_ut_flags (mf_wgraph.hip) per ROW, every neighbour looked up in the row's own component.  One reverse
// complement per row: rc(x[1..] + c) = (3 - c) + rc(x)[..k-2] and rc(c + x[..k-2]) = rc(x)[1..] + (3 - c), and the only shift by a run-time amount
// besides it is the one word that holds the first base's place (top); c is a constant of the unrolled loops.
__global__ __launch_bounds__(256) void k_wc2s_flags(wc2s_index ix, ut_arrays A) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const int k = A.k, tb = 2 * k - 2;                                           // the first base: bits [2k - 2, 2k), tb = 62 .. 124
    const mf_u128 top = tb >= 64 ? ((mf_u128)(1ull << (tb - 64)) << 64) : (mf_u128)(1ull << tb);
    const mf_u128 kmask = (top << 2) - 1;
    const mf_u128 x = ((mf_u128)A.ghi[i] << 64) | (mf_u128)A.gk[i];
    const mf_u128 rcx = mf_wrevcomp(x, k);
    const uint32_t comp = ix.comp[i];
    uint32_t rcode = C2S_CODE_NONE, lcode = C2S_CODE_NONE, ridx = C2S_NONE, lidx = C2S_NONE, ror = 0, lor = 0;
#pragma unroll
    for (uint32_t nuc = 0; nuc < 4; nuc++) {
        const uint32_t cn = 3u - nuc;
        const mf_u128 y = ((x << 2) | (mf_u128)nuc) & kmask;
        const mf_u128 ry = (rcx >> 2) | ((cn & 1u) ? top : (mf_u128)0) | ((cn & 2u) ? (top << 1) : (mf_u128)0);
        const mf_u128 c = y < ry ? y : ry;
        const uint32_t idx = wc2s_find(ix, c, comp);
        if (idx != C2S_NONE) {
            if (rcode == C2S_CODE_NONE) { rcode = nuc; ridx = idx; ror = (c != y); }
            else rcode = C2S_CODE_MANY;
        }
    }
#pragma unroll
    for (uint32_t nuc = 0; nuc < 4; nuc++) {
        const uint32_t cn = 3u - nuc;
        const mf_u128 y = (x >> 2) | ((nuc & 1u) ? top : (mf_u128)0) | ((nuc & 2u) ? (top << 1) : (mf_u128)0);
        const mf_u128 ry = ((rcx << 2) | (mf_u128)cn) & kmask;
        const mf_u128 c = y < ry ? y : ry;
        const uint32_t idx = wc2s_find(ix, c, comp);
        if (idx != C2S_NONE) {
            if (lcode == C2S_CODE_NONE) { lcode = nuc; lidx = idx; lor = (c != y); }
            else lcode = C2S_CODE_MANY;
        }
    }
    A.info[i] = (uint8_t)(rcode | (lcode << 3) | (ror << 6) | (lor << 7));
    if (A.pal) A.pal[i] = (uint8_t)(rcx == x);
    A.ridx[i] = ridx;
    A.lidx[i] = lidx;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
int wc2s_check_k(const char *who, int k) {
    if (k < 32 || k > 63) return mf_set_error("%s: 32 <= k <= 63 (k <= 31: the entry point without 'wide')", who);
    return MF_OK;
}
static int wc2s_member_flags(mf_ctx *ctx, const unsigned int *d_flags, int k) {
    unsigned int f = 0;
    MF_HIP(hipMemcpyAsync(&f, d_flags, 4, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    if (f & 1u) return mf_set_error("comp2seq: a component holds a k-mer that does not fit %d bases", k);
    return MF_OK;
}
int wc2s_member_count(const char *who, const mf_wcomps *c) {
    if (c->n_kmers >= 0x7FFFFFFFull) return mf_set_error("%s: %llu component k-mers (fewer than 2^31 - 1 are supported)", who, (unsigned long long)c->n_kmers);
    return MF_OK;
}
// the rows of all components, built from the member lists
int wc2s_build_rows(mf_ctx *ctx, const mf_wcomps *c, wc2s_rows &R) {
    hipStream_t st = ctx->stream;
    const uint64_t n = c->n_kmers;
    const int k = c->k, hb = 2 * k - 64;
    R.n = 0;
    if (!n) return MF_OK;
    mf_buf<uint64_t> chi, clo, k0, k1, i0, i1; mf_buf<uint32_t> c0, c1; mf_buf<unsigned int> flags;
    MF_TRY(chi.alloc(ctx, n)); MF_TRY(clo.alloc(ctx, n)); MF_TRY(k0.alloc(ctx, n)); MF_TRY(k1.alloc(ctx, n)); MF_TRY(i0.alloc(ctx, n)); MF_TRY(i1.alloc(ctx, n));
    MF_TRY(c0.alloc(ctx, n)); MF_TRY(c1.alloc(ctx, n)); MF_TRY(flags.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(flags.p, 0, 4, st));
    {
        mf_ktimer tm(ctx, "k_wc2s_rows");
        k_wc2s_canon<<<wc2s_grid(n), 256, 0, st>>>(c->hi.p, c->lo.p, n, k, chi.p, clo.p, nullptr, flags.p);
        k_wc2s_iota<<<wc2s_grid(n), 256, 0, st>>>(i0.p, n);
    }
    MF_TRY(wc2s_member_flags(ctx, flags.p, k));
    // three stable passes that carry the member's index: the low word, the high word's 2k - 64 bits, the component
    int cb = 1; while (cb < 32 && (1ull << cb) < c->n) cb++;
    MF_TRY(mf_sort_u64_u64(ctx, clo.p, i0.p, n, 64, k1.p, i1.p));                          // (lo', idx') in (k1, i1)
    if (hb) {
        k_wc2s_gather64<<<wc2s_grid(n), 256, 0, st>>>(i1.p, chi.p, n, k0.p);               // hi' in k0
        MF_TRY(mf_sort_u64_u64(ctx, k0.p, i1.p, n, hb, k1.p, i0.p));                       // (hi'', idx'') in (k1, i0)
    } else i0.swap(i1);                                                                    // (k = 32: every high word is 0)
    k_wc2s_gather32<<<wc2s_grid(n), 256, 0, st>>>(i0.p, c->comp.p, n, c0.p);
    MF_TRY(mf_sort_u32_u64(ctx, c0.p, i0.p, n, cb, c1.p, i1.p));                           // (comp''', idx''') in (c1, i1)
    k_wc2s_gather64<<<wc2s_grid(n), 256, 0, st>>>(i1.p, chi.p, n, k0.p);                   // the sorted triples: (c1, k0, k1)
    k_wc2s_gather64<<<wc2s_grid(n), 256, 0, st>>>(i1.p, clo.p, n, k1.p);
    MF_HIP(hipStreamSynchronize(st));
    chi.reset(); clo.reset(); i0.reset(); c0.reset();
    mf_buf<uint32_t> head, rstart; mf_buf<uint64_t> idx, tot;
    MF_TRY(head.alloc(ctx, n)); MF_TRY(idx.alloc(ctx, n + 1)); MF_TRY(tot.alloc(ctx, 1));
    uint64_t nr = 0;
    {
        mf_ktimer tm(ctx, "k_wc2s_rows");
        k_wc2s_heads<<<wc2s_grid(n), 256, 0, st>>>(c1.p, k0.p, k1.p, n, head.p);
        MF_TRY(mf_scan<1>(ctx, head.p, idx.p, n, tot.p));
    }
    MF_HIP(hipMemcpyAsync(&nr, tot.p, 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    MF_TRY(R.hi.alloc(ctx, nr)); MF_TRY(R.lo.alloc(ctx, nr)); MF_TRY(R.comp.alloc(ctx, nr)); MF_TRY(R.cnt.alloc(ctx, nr)); MF_TRY(rstart.alloc(ctx, nr));
    {
        mf_ktimer tm(ctx, "k_wc2s_rows");
        k_wc2s_rows<<<wc2s_grid(n), 256, 0, st>>>(c1.p, k0.p, k1.p, head.p, idx.p, n, R.hi.p, R.lo.p, R.comp.p, rstart.p);
        k_wc2s_counts<<<wc2s_grid(nr), 256, 0, st>>>(rstart.p, nr, n, R.cnt.p);
    }
    MF_HIP(hipStreamSynchronize(st));                        // (the temporaries go back to the arena below)
    R.n = nr;
    return MF_OK;
}
int wc2s_pair_index(mf_ctx *ctx, const wc2s_rows &R, mf_buf<unsigned long long> &slots, wc2s_index *ix) {
    *ix = wc2s_index{};
    if (!R.n) return MF_OK;
    uint64_t cap = 1024; while (cap < 2 * R.n) cap <<= 1;                        // load <= 0.5, as the index of a wide table (mf_wtable_ensure_index)
    MF_TRY(slots.alloc(ctx, cap));
    MF_HIP(hipMemsetAsync(slots.p, 0xFF, cap * 8, ctx->stream));
    mf_ktimer tm(ctx, "k_wc2s_index_insert");
    k_wc2s_index_insert<<<wc2s_grid(R.n), 256, 0, ctx->stream>>>(slots.p, cap - 1, R.hi.p, R.lo.p, R.comp.p, R.n);
    *ix = wc2s_index{slots.p, cap - 1, R.hi.p, R.lo.p, R.comp.p};
    return MF_OK;
}
int wc2s_flags_launch(mf_ctx *ctx, const wc2s_index &ix, const ut_arrays &A) {
    if (!A.n) return MF_OK;
    mf_ktimer tm(ctx, "k_wc2s_flags");
    k_wc2s_flags<<<wc2s_grid(A.n), 256, 0, ctx->stream>>>(ix, A);
    return MF_OK;
}
// the segmented build over the rows: pair index, restricted U1, U2 .. U5
static int wc2s_unitigs_of_rows(mf_ctx *ctx, const wc2s_rows &R, uint64_t n_comps, int k, mf_seqs **out) {
    const uint64_t nr = R.n;
    mf_buf<unsigned long long> slots;
    wc2s_index ix{};
    MF_TRY(wc2s_pair_index(ctx, R, slots, &ix));
    mf_seqs *S = nullptr;
    MF_TRY(mf_ut_build(ctx, R.lo.p, R.hi.p, R.cnt.p, nr, k, 0, nullptr, k, [&](const ut_arrays &A) -> int { return wc2s_flags_launch(ctx, ix, A); }, &S, nullptr,
                       R.comp.p));
    if (!S->d_comp) {                                        // (no rows: no sequences, but sequences of components all the same)
        void *p = nullptr;
        if (mf_alloc(ctx, 4, &p) < 0) { mf_seqs_destroy(S); return MF_ERR; }
        S->d_comp = (uint32_t *)p; S->comp_bytes = 4;
    }
    S->n_groups = std::max<uint64_t>(n_comps, 1);
    *out = S;
    return MF_OK;
}
// split absent: one wide table of all members -- distinct k-mers, count = the multiplicity over all components (capped as the counter caps)
static int wc2s_union_table(mf_ctx *ctx, const mf_wcomps *c, mf_wtable **out) {
    hipStream_t st = ctx->stream;
    const uint64_t n = c->n_kmers;
    const int k = c->k;
    auto piece = std::make_unique<mf_wtable::piece>();
    if (n) {
        mf_buf<uint64_t> chi, clo; mf_buf<uint16_t> ones; mf_buf<unsigned int> flags;
        MF_TRY(chi.alloc(ctx, n)); MF_TRY(clo.alloc(ctx, n)); MF_TRY(ones.alloc(ctx, n)); MF_TRY(flags.alloc(ctx, 1));
        MF_HIP(hipMemsetAsync(flags.p, 0, 4, st));
        {
            mf_ktimer tm(ctx, "k_wc2s_rows");
            k_wc2s_canon<<<wc2s_grid(n), 256, 0, st>>>(c->hi.p, c->lo.p, n, k, chi.p, clo.p, ones.p, flags.p);
        }
        MF_TRY(wc2s_member_flags(ctx, flags.p, k));
        MF_TRY(mf_wide_merge_runs(ctx, k, chi.p, clo.p, ones.p, n, *piece));
    }
    auto t = std::make_unique<mf_wtable>();
    t->ctx = ctx; t->k = k; t->n = piece->n; t->n_all = piece->n; t->n_occ = n;
    t->cut_thr = 0;                                          // (every entry stands for at least one member)
    t->ascending = true;
    if (piece->n) t->pieces.push_back(std::move(piece));
    *out = t.release();
    return MF_OK;
}
static int wc2s_unitigs_unsplit(mf_ctx *ctx, mf_wtable *t, mf_seqs **out) {
    mf_seqs *S = nullptr;
    MF_TRY(mf_build_unitigs_wide_device(ctx, t, 0, t->k, &S));
    void *p = nullptr;                                       // one group: every sequence has component 0
    const size_t bytes = (S->n ? S->n : 1) * 4;
    if (mf_alloc(ctx, bytes, &p) < 0) { mf_seqs_destroy(S); return MF_ERR; }
    S->d_comp = (uint32_t *)p; S->comp_bytes = bytes; S->n_groups = 1;
    if (hipMemsetAsync(p, 0, bytes, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        mf_seqs_destroy(S);
        return mf_set_error("comp2seq: hipMemsetAsync failed: %s", hipGetErrorString(hipGetLastError()));
    }
    *out = S;
    return MF_OK;
}

extern "C" int mf_wcomps_unitigs_device(mf_ctx *ctx, mf_wcomps *c, int split, mf_seqs **out) {
    mf_range rng_("mf:comp2seq_wide");
    if (!ctx || !c || !out) return mf_set_error("mf_wcomps_unitigs_device: NULL argument");
    *out = nullptr;
    if (c->ctx != ctx) return mf_set_error("mf_wcomps_unitigs_device: the components belong to another context");
    MF_TRY(wc2s_check_k("mf_wcomps_unitigs_device", c->k));
    MF_TRY(wc2s_member_count("comp2seq", c));
    MF_HIP(hipSetDevice(ctx->device));
    if (split) {
        wc2s_rows R;
        MF_TRY(wc2s_build_rows(ctx, c, R));
        return wc2s_unitigs_of_rows(ctx, R, c->n, c->k, out);
    }
    mf_wtable *t = nullptr;
    MF_TRY(wc2s_union_table(ctx, c, &t));
    const int rc = wc2s_unitigs_unsplit(ctx, t, out);
    mf_wtable_destroy(t);
    return rc;
}

// ---- the file form ----
static void wc2s_kmer_text(uint64_t hi, uint64_t lo, int k, std::string &out) {
    for (int i = 0; i < k; i++) {
        const int sh = 2 * (k - 1 - i);
        out.push_back("AGCT"[(sh >= 64 ? hi >> (sh - 64) : lo >> sh) & 3u]);
    }
}
static uint64_t wc2s_be(const uint8_t *p, int nb) { uint64_t v = 0; for (int i = 0; i < nb; i++) v = (v << 8) | p[i]; return v; }
// the wide .kmers.bin records and the .stat.txt of rows [lo, hi) (mf_wtable_write_kmers' formats)
static void wc2s_rows_text(const std::vector<uint64_t> &khi, const std::vector<uint64_t> &klo, const std::vector<uint16_t> &cnt, uint64_t lo, uint64_t hi, std::string &bin,
                           std::string &stat) {
    std::map<uint32_t, uint64_t> hist;
    bin.resize((hi - lo) * 18);
    for (uint64_t r = lo; r < hi; r++) {
        uint8_t *w = reinterpret_cast<uint8_t *>(&bin[(r - lo) * 18]);
        for (int b = 0; b < 8; b++) { w[b] = (uint8_t)(khi[r] >> (8 * (7 - b))); w[8 + b] = (uint8_t)(klo[r] >> (8 * (7 - b))); }
        w[16] = (uint8_t)(cnt[r] >> 8); w[17] = (uint8_t)cnt[r];
        hist[cnt[r]]++;
    }
    stat = "# k-mer frequency\tnumber of such k-mers\n";
    for (auto &h : hist) stat += std::to_string(h.first) + "\t" + std::to_string(h.second) + "\n";
    stat += "\n";
}

extern "C" int mf_comp2seq_wide(mf_ctx *ctx, const char *components_bin, int k, int split, const char *out_dir, uint64_t *n_files, uint64_t *n_seqs) {
    mf_range rng_("mf:comp2seq_wide(files)");
    if (!ctx || !components_bin || !out_dir) return mf_set_error("mf_comp2seq_wide: NULL argument");
    MF_TRY(wc2s_check_k("mf_comp2seq_wide", k));
    if (n_files) *n_files = 0;
    if (n_seqs) *n_seqs = 0;
    mf_wcomps *c = nullptr;
    MF_TRY(mf_wcomps_load(ctx, components_bin, k, &c));      // (a file of another width or another k stops here, before anything is written)
    std::unique_ptr<mf_wcomps, void (*)(mf_wcomps *)> gc(c, mf_wcomps_destroy);
    MF_TRY(wc2s_member_count("comp2seq", c));
    MF_HIP(hipSetDevice(ctx->device));
    const std::string od(out_dir);
    const std::string d_fa = od + "/kmers_fasta", d_km = od + "/kmer-counter-many/kmers", d_st = od + "/kmer-counter-many/stats", d_sq = od + "/seq-builder-many/sequences";
    for (const std::string *d : {&d_fa, &d_km, &d_st, &d_sq}) MF_TRY(c2s_mkdirs(*d));
    const uint64_t nc = c->n;
    auto name = [&](const std::string &dir, uint64_t i, const char *ext) { return dir + "/component" + (split ? "_" + std::to_string(i + 1) : std::string()) + ext; };
    {
        // bin2fasta: the members as the FILE lists them, not canonicalised, ">j" (split) or ">i_j" headers
        const int fd = open(components_bin, O_RDONLY);
        struct stat stc;
        if (fd < 0 || fstat(fd, &stc) != 0) { if (fd >= 0) close(fd); return mf_set_error("Can't load components: file not found (%s)", components_bin); }
        struct fd_closer { int f; ~fd_closer() { close(f); } } fdc{fd};
        uint64_t want = 4;
        for (uint64_t i = 0; i < nc; i++) want += 12 + 16 * c->sizes[i];
        if ((uint64_t)stc.st_size != want) return mf_set_error("mf_comp2seq_wide: %s changed while it was read", components_bin);
        void *map = mmap(nullptr, (size_t)want, PROT_READ, MAP_PRIVATE, fd, 0);
        if (map == MAP_FAILED) return mf_set_error("Can't load components: can't map '%s'", components_bin);
        struct unmapper { void *m; size_t n; ~unmapper() { munmap(m, n); } } um{map, (size_t)want};
        const uint8_t *p = (const uint8_t *)map;
        std::string text;
        size_t at = 4;
        for (uint64_t i = 0; i < nc; i++) {
            at += 12;
            for (uint64_t j = 0; j < c->sizes[i]; j++) {
                text += split ? ">" + std::to_string(j + 1) + "\n" : ">" + std::to_string(i + 1) + "_" + std::to_string(j + 1) + "\n";
                wc2s_kmer_text(wc2s_be(p + at, 8), wc2s_be(p + at + 8, 8), k, text);
                text.push_back('\n');
                at += 16;
            }
            if (split) { MF_TRY(c2s_write_file(name(d_fa, i, ".fasta"), text)); text.clear(); }
        }
        if (!split) MF_TRY(c2s_write_file(name(d_fa, 0, ".fasta"), text));
    }
    mf_seqs *S = nullptr;
    struct sguard { mf_seqs *&p; ~sguard() { mf_seqs_destroy(p); } } gs{S};
    if (split) {
        wc2s_rows R;
        MF_TRY(wc2s_build_rows(ctx, c, R));
        std::vector<uint64_t> khi(R.n), klo(R.n); std::vector<uint32_t> comp(R.n); std::vector<uint16_t> cnt(R.n);
        if (R.n) {
            MF_HIP(hipMemcpyAsync(khi.data(), R.hi.p, R.n * 8, hipMemcpyDeviceToHost, ctx->stream));
            MF_HIP(hipMemcpyAsync(klo.data(), R.lo.p, R.n * 8, hipMemcpyDeviceToHost, ctx->stream));
            MF_HIP(hipMemcpyAsync(comp.data(), R.comp.p, R.n * 4, hipMemcpyDeviceToHost, ctx->stream));
            MF_HIP(hipMemcpyAsync(cnt.data(), R.cnt.p, R.n * 2, hipMemcpyDeviceToHost, ctx->stream));
            MF_HIP(hipStreamSynchronize(ctx->stream));
        }
        MF_TRY(wc2s_unitigs_of_rows(ctx, R, nc, k, &S));
        std::string bin, stat;
        uint64_t r = 0;
        for (uint64_t i = 0; i < nc; i++) {
            const uint64_t lo = r;
            while (r < R.n && comp[r] == i) r++;
            wc2s_rows_text(khi, klo, cnt, lo, r, bin, stat);
            MF_TRY(c2s_write_file(name(d_km, i, ".kmers.bin"), bin));
            MF_TRY(c2s_write_file(name(d_st, i, ".stat.txt"), stat));
        }
        std::vector<uint8_t> b; std::vector<uint64_t> o; std::vector<int32_t> a, mn, mx; std::vector<uint32_t> sc;
        MF_TRY(mf_seqs_to_host_grouped(S, b, o, a, mn, mx, &sc));
        std::string text;
        uint64_t q = 0;
        for (uint64_t i = 0; i < nc; i++) {
            const uint64_t lo = q;
            while (q < S->n && sc[q] == i) q++;
            text.clear();
            c2s_seq_text(b, o, a, mn, mx, lo, q, text);
            MF_TRY(c2s_write_file(name(d_sq, i, ".seq.fasta"), text));
        }
        if (n_files) *n_files = nc;
    } else {
        mf_wtable *t = nullptr;
        MF_TRY(wc2s_union_table(ctx, c, &t));
        std::unique_ptr<mf_wtable, void (*)(mf_wtable *)> gt(t, mf_wtable_destroy);
        MF_TRY(mf_wtable_write_kmers(t, 0, name(d_km, 0, ".kmers.bin").c_str(), name(d_st, 0, ".stat.txt").c_str(), nullptr));
        MF_TRY(wc2s_unitigs_unsplit(ctx, t, &S));
        MF_TRY(mf_seqs_write_fasta(S, name(d_sq, 0, ".seq.fasta").c_str()));
        if (n_files) *n_files = 1;
    }
    if (n_seqs) *n_seqs = S->n;
    return MF_OK;
}
