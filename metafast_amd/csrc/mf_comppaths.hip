// mf_comppaths.hip -- component-paths (src/tools/ComponentPathsMain.java:82-206): the stretches of the given sequences that lie inside a
// component.  For a selected component c, a path is a maximal run of consecutive positions of ONE sequence whose canonical k-mers are
// all members of c; it is kept when its length (positions + k - 1) reaches min_len, the first max_paths per component in encounter
// order (file, record, position), printed longest first (ties in encounter order) as Sequence.printSequences prints them.
//
// The reference probes, for every sequence, one hash set per selected component: O(components x bases).  Here every position costs ONE
// lookup, whatever the number of components:
//   create   the members of the selected components as (k-mer, slot) pairs ordered by k-mer, then slot (slot = place in the
//            de-duplicated selection); an index over the DISTINCT k-mers gives the range [lo, hi) of a k-mer's listings.  Components
//            may share k-mers (seq2comp): a k-mer then has several listings, and S(p) -- the slots that list the k-mer at position p --
//            has several elements, in ascending order.  Built once, resident across the files.
//   add      k_cp_mark: one thread per run of CP_RUN positions of one sequence rolls the canonical k-mers of its positions and of
//            the one before and the one after (inside the sequence), and for every position p and slot c in S(p) decides: p STARTS a
//            run of c when c is not in S(p - 1), ENDS one when c is not in S(p + 1) (S outside the sequence is empty).  Pass 1
//            counts, the counts are scanned, pass 2 writes (slot, position) records at the scanned places: position order, no HBM
//            atomics.  Starts and ends are each sorted by slot (stable); inside a slot the i-th start and the i-th end are one run, as
//            the runs of one component cannot overlap.  Runs shorter than min_len go, the per-slot count of kept paths so far decides
//            which of the rest are within the cap, and their bases are copied (upper case) into the packed store: the file's text
//            can be released after the call.
//   finish   one stable sort by (slot, length descending); number inside the slot and byte width per record, a scan, and the writer
//            kernels format the headers (decimal numbers on the device) and copy the bases with a newline every 70.
// Nothing is truncated silently: what does not fit a 32-bit count, or HBM, is an error.
// 32 <= k <= 63 (mf_wcomppaths.hip) shares all of this but the member index and the key side of k_cp_mark: mf_cp.h.
#include "mf_cp.h"
#include "mf_roll.h"
#include <algorithm>
#include <cmath>
#include <memory>
#include <sys/stat.h>
#include <errno.h>

// ---- create: the member index over the selected components ----
__global__ void k_cp_select(const uint32_t *__restrict__ comp, const uint32_t *__restrict__ slot_of, uint64_t nk, uint32_t *__restrict__ flag) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nk) flag[j] = slot_of[comp[j]] != CP_NONE ? 1u : 0u;
}
__global__ void k_cp_members(const uint64_t *__restrict__ kmers, const uint32_t *__restrict__ comp, const uint32_t *__restrict__ slot_of,
                             const uint32_t *__restrict__ flag, const uint64_t *__restrict__ rank, uint64_t nk, uint64_t *__restrict__ mk,
                             uint32_t *__restrict__ ms) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nk && flag[j]) { mk[rank[j]] = kmers[j]; ms[rank[j]] = slot_of[comp[j]]; }
}
// the listings ordered by (k-mer, slot): flag[i] = 1 where a new k-mer starts; a k-mer that does not fit k bases raises *bad
__global__ void k_cp_heads(const uint64_t *__restrict__ mk, uint64_t nm, int k, uint32_t *__restrict__ flag, unsigned int *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nm) return;
    flag[i] = (i == 0 || mk[i] != mk[i - 1]) ? 1u : 0u;
    if (mk[i] >> (2 * k)) atomicOr(bad, 1u);
}
// the distinct k-mers and the first listing of each (lo[nd] = nm); *maxl = the most listings of one k-mer
__global__ void k_cp_distinct(const uint64_t *__restrict__ mk, const uint32_t *__restrict__ flag, const uint64_t *__restrict__ rank, uint64_t nm,
                              uint64_t *__restrict__ dk, uint32_t *__restrict__ lo) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nm) return;
    if (i == nm) { lo[rank[nm]] = (uint32_t)nm; return; }
    if (flag[i]) { dk[rank[i]] = mk[i]; lo[rank[i]] = (uint32_t)i; }
}
__global__ void k_cp_maxlist(const uint32_t *__restrict__ lo, uint64_t nd, unsigned int *__restrict__ maxl) {
    const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t v = d < nd ? lo[d + 1] - lo[d] : 0u;
    for (int o = 32; o > 0; o >>= 1) { const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64); v = w > v ? w : v; }
    if (mf_lane() == 0 && v > 1u) atomicMax(maxl, v);
}

// ---- scans of 32-bit items whose tile sums may pass 2^32 (path lengths, listings per thread): the two 16-bit halves are scanned apart ----
__global__ void k_cp_split(const uint32_t *__restrict__ in, uint64_t n, uint32_t *__restrict__ lo, uint32_t *__restrict__ hi) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const uint32_t v = in[i]; lo[i] = v & 0xFFFFu; hi[i] = v >> 16; }
}
__global__ void k_cp_join(const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi, uint64_t n1, uint64_t *__restrict__ out, uint64_t *__restrict__ total) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n1) return;
    const uint64_t v = lo[i] + (hi[i] << 16);
    out[i] = v;
    if (i == n1 - 1) *total = v;
}

// ---- add ----
// runs[i] = threads sequence i takes: ceil(max(0, len_i - k + 1) / CP_RUN); a sequence of 2^31 or more positions (or offsets that go backwards) raises *bad
__global__ void k_cp_sizes(const uint64_t *__restrict__ off, uint64_t n, int k, uint32_t *__restrict__ runs, unsigned int *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = off[i], b = off[i + 1];
    uint64_t ni = 0;
    if (b < a) atomicOr(bad, 1u);
    else if (b - a >= (uint64_t)k) ni = b - a - (uint64_t)k + 1;
    if (ni >= 0x80000000ull) { atomicOr(bad, 1u); ni = 0; }
    runs[i] = (uint32_t)((ni + CP_RUN - 1) / CP_RUN);
}

// k <= 31: s2c_roll and the index of a k-mer table (k_cp_mark: mf_cp.h)
struct cp_keys64 {
    mf_index_view ix;
    template <typename F> __device__ __forceinline__ void each(const uint8_t *__restrict__ p, uint32_t count, int k, F &&f) const {
        s2c_roll(p, count, k, [&](uint32_t i, uint64_t key) {
            uint32_t idx, val;
            const bool found = mf_index_find(ix, key, &idx, &val);
            f(i, found, idx);
        });
    }
};

// the starts and the ends, each sorted by slot: run i = (ss[i], sp[i] .. ep[i]); flag[i] = long enough; head[slot] = the slot's first run
__global__ void k_cp_pair(const uint32_t *__restrict__ ss, const uint64_t *__restrict__ sp, const uint32_t *__restrict__ es, const uint64_t *__restrict__ ep, uint64_t n,
                          int k, int64_t min_len, uint32_t *__restrict__ flag, uint32_t *__restrict__ head, unsigned int *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = ss[i];
    if (es[i] != c || ep[i] < sp[i]) atomicOr(bad, 1u);    // (cannot happen: the runs of one slot do not overlap)
    flag[i] = (int64_t)(ep[i] - sp[i]) + (int64_t)k >= min_len ? 1u : 0u;
    if (i == 0 || ss[i - 1] != c) head[c] = (uint32_t)i;
}
// rank = exclusive scan of flag: a run's place among its slot's kept runs of this batch, after the count[slot] of the batches before
__global__ void k_cp_keep(const uint32_t *__restrict__ ss, const uint32_t *__restrict__ flag, const uint64_t *__restrict__ rank, const uint32_t *__restrict__ head,
                          const unsigned long long *__restrict__ count, unsigned long long max_paths, uint64_t n, uint32_t *__restrict__ keep) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = ss[i];
    keep[i] = (flag[i] && count[c] + (rank[i] - rank[head[c]]) < max_paths) ? 1u : 0u;
}
// the slot's last run adds the slot's kept runs to its count (bounded at the cap)
__global__ void k_cp_bump(const uint32_t *__restrict__ ss, const uint64_t *__restrict__ rank, const uint32_t *__restrict__ head, uint64_t n,
                          unsigned long long *__restrict__ count, unsigned long long max_paths) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = ss[i];
    if (i + 1 < n && ss[i + 1] == c) return;
    const unsigned long long v = count[c] + (rank[i + 1] - rank[head[c]]);
    count[c] = v < max_paths ? v : max_paths;
}
__global__ void k_cp_records(const uint32_t *__restrict__ ss, const uint64_t *__restrict__ sp, const uint64_t *__restrict__ ep, const uint32_t *__restrict__ keep,
                             const uint64_t *__restrict__ rank, uint64_t n, int k, uint32_t *__restrict__ rslot, uint32_t *__restrict__ rlen, uint64_t *__restrict__ src) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const uint64_t j = rank[i];
    rslot[j] = ss[i]; rlen[j] = (uint32_t)(ep[i] - sp[i]) + (uint32_t)k; src[j] = sp[i];
}
// a wave per kept run: its bases, upper case, to the store; roff[j] = where (from the store's start)
__global__ __launch_bounds__(256) void k_cp_copy(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ src, const uint32_t *__restrict__ rlen,
                                                 const uint64_t *__restrict__ toff, uint64_t n, uint64_t base, uint8_t *__restrict__ text, uint64_t *__restrict__ roff) {
    const uint64_t j = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (j >= n) return;
    const uint8_t *__restrict__ from = bases + src[j];
    uint8_t *__restrict__ to = text + base + toff[j];
    const uint32_t len = rlen[j];
    for (uint32_t b = (uint32_t)mf_lane(); b < len; b += 64u) to[b] = from[b] & 0xDFu;
    if (mf_lane() == 0) roff[j] = base + toff[j];
}

// ---- finish ----
__global__ void k_cp_keys(const uint32_t *__restrict__ rslot, const uint32_t *__restrict__ rlen, uint64_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ idx) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) { key[j] = ((uint64_t)rslot[j] << 32) | (uint64_t)(0xFFFFFFFFu - rlen[j]); idx[j] = (uint32_t)j; }
}
__device__ __forceinline__ uint32_t cp_digits(uint64_t v) { uint32_t d = 1; while (v >= 10) { v /= 10; d++; } return d; }
__device__ __forceinline__ uint32_t cp_put(uint8_t *p, uint64_t v) {       // decimal, most significant digit first; returns the digits written
    const uint32_t d = cp_digits(v);
    for (uint32_t i = d; i-- > 0;) { p[i] = (uint8_t)('0' + v % 10); v /= 10; }
    return d;
}
__device__ __forceinline__ uint32_t cp_put_str(uint8_t *p, const char *s) { uint32_t i = 0; for (; s[i]; i++) p[i] = (uint8_t)s[i]; return i; }
__device__ __forceinline__ uint32_t cp_wdigits(int32_t w) { return w < 0 ? 1u + cp_digits((uint64_t)(-(int64_t)w)) : cp_digits((uint64_t)w); }
// ">i length=L av_weight=W min_weight=0 max_weight=0\n": 1 + 8 + 11 + 27 fixed bytes and three numbers
__device__ __forceinline__ uint32_t cp_header_len(uint64_t num, uint32_t len, int32_t w) { return 47u + cp_digits(num) + cp_digits(len) + cp_wdigits(w); }
// sorted record j (slot in the key's high half, 2^32 - 1 - length in the low one): the bytes it prints
__global__ void k_cp_widths(const uint64_t *__restrict__ key, uint64_t n, const uint64_t *__restrict__ sfirst, const int32_t *__restrict__ W, uint32_t *__restrict__ width) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t c = (uint32_t)(key[j] >> 32), len = 0xFFFFFFFFu - (uint32_t)key[j];
    width[j] = cp_header_len(j - sfirst[c] + 1, len, W[c]) + len + (len + 69u) / 70u;
}
__global__ void k_cp_slot_bytes(const uint64_t *__restrict__ ooff, const uint64_t *__restrict__ sfirst, uint64_t n1, uint64_t *__restrict__ boff) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n1) boff[c] = ooff[sfirst[c]];
}
__global__ void k_cp_write_head(const uint64_t *__restrict__ key, uint64_t n, const uint64_t *__restrict__ sfirst, const int32_t *__restrict__ W,
                                const uint64_t *__restrict__ ooff, uint8_t *__restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t c = (uint32_t)(key[j] >> 32), len = 0xFFFFFFFFu - (uint32_t)key[j];
    const int32_t w = W[c];
    uint8_t *p = out + ooff[j];
    *p++ = '>';
    p += cp_put(p, j - sfirst[c] + 1);
    p += cp_put_str(p, " length=");
    p += cp_put(p, len);
    p += cp_put_str(p, " av_weight=");
    if (w < 0) *p++ = '-';
    p += cp_put(p, (uint64_t)(w < 0 ? -(int64_t)w : (int64_t)w));
    p += cp_put_str(p, " min_weight=0 max_weight=0\n");
}
// a wave per record: the bases behind the header, a newline after every 70 and after the last
__global__ __launch_bounds__(256) void k_cp_write_bases(const uint64_t *__restrict__ key, const uint32_t *__restrict__ idx, uint64_t n, const uint64_t *__restrict__ sfirst,
                                                        const int32_t *__restrict__ W, const uint64_t *__restrict__ roff, const uint8_t *__restrict__ text,
                                                        const uint64_t *__restrict__ ooff, uint8_t *__restrict__ out) {
    const uint64_t j = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (j >= n) return;
    const uint32_t c = (uint32_t)(key[j] >> 32), len = 0xFFFFFFFFu - (uint32_t)key[j];
    const uint8_t *__restrict__ from = text + roff[idx[j]];
    uint8_t *__restrict__ to = out + ooff[j] + cp_header_len(j - sfirst[c] + 1, len, W[c]);
    for (uint32_t b = (uint32_t)mf_lane(); b < len; b += 64u) {
        to[b + b / 70u] = from[b];
        if (b % 70u == 69u || b == len - 1u) to[b + b / 70u + 1u] = '\n';
    }
}

// =============================================================================================
// host side
// =============================================================================================
// out[0 .. n] = exclusive prefix of in, *total (device) = out[n]; the items may be anything below 2^32
static int cp_scan(mf_ctx *ctx, const uint32_t *in, uint64_t *out, uint64_t n, uint64_t *total) {
    if (n <= 65536) return mf_scan<1>(ctx, in, out, n, total);               // (one workgroup, 64-bit sums)
    mf_buf<uint32_t> lo, hi; mf_buf<uint64_t> olo, ohi;
    MF_TRY(lo.alloc(ctx, n)); MF_TRY(hi.alloc(ctx, n)); MF_TRY(olo.alloc(ctx, n + 1)); MF_TRY(ohi.alloc(ctx, n + 1));
    k_cp_split<<<cp_grid(n), 256, 0, ctx->stream>>>(in, n, lo.p, hi.p);
    MF_TRY(mf_scan<1>(ctx, lo.p, olo.p, n, total));
    MF_TRY(mf_scan<1>(ctx, hi.p, ohi.p, n, total));
    k_cp_join<<<cp_grid(n + 1), 256, 0, ctx->stream>>>(olo.p, ohi.p, n + 1, out, total);
    MF_HIP(hipGetLastError());
    MF_HIP(hipStreamSynchronize(ctx->stream));             // (the halves go back to the arena)
    return MF_OK;
}
template <typename T> static int cp_grow(mf_ctx *ctx, mf_buf<T> &b, uint64_t used, uint64_t cap_now, uint64_t cap_new) {
    if (cap_new <= cap_now && b.p) return MF_OK;
    mf_buf<T> nb;
    MF_TRY(nb.alloc(ctx, cap_new));
    if (used) MF_HIP(hipMemcpyAsync(nb.p, b.p, used * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    b.swap(nb);
    return MF_OK;
}

// ---- create, the steps that see no k-mer: both widths (mf_cp.h) ----
int cp_slots_of(mf_paths *P, uint64_t n, const uint64_t *sizes, const int64_t *weights, const uint32_t *selection, uint64_t n_selection,
                std::vector<uint32_t> &slot_of) {
    mf_ctx *ctx = P->ctx;
    // the slots: the selection without its repeats, in the order given; all components in theirs
    slot_of.assign((size_t)std::max<uint64_t>(n, 1), CP_NONE);
    if (!selection) {
        for (uint64_t i = 0; i < n; i++) { slot_of[i] = (uint32_t)i; P->comp_no.push_back((uint32_t)i + 1u); }
    } else {
        for (uint64_t j = 0; j < n_selection; j++) {
            const uint32_t no = selection[j];
            if (no < 1 || (uint64_t)no > n) return mf_set_error("component-paths: there is no component %u (the file holds %llu, numbered from 1)", no, (unsigned long long)n);
            if (slot_of[no - 1] != CP_NONE) continue;
            slot_of[no - 1] = (uint32_t)P->comp_no.size();
            P->comp_no.push_back(no);
        }
    }
    const uint64_t ns = P->n_slots = P->comp_no.size();
    for (uint64_t s = 0; s < ns; s++) {
        const uint64_t size = sizes[P->comp_no[s] - 1]; const int64_t weight = weights[P->comp_no[s] - 1];
        double w = 0.0;
        if (size) {                                        // (a component without members matches nothing: its weight is never printed)
            w = floor((double)weight / (double)size + 0.5);      // Math.round
            if (!(w >= -2147483648.0 && w <= 2147483647.0))
                return mf_set_error("component-paths: the average k-mer weight of component %u does not fit a 32-bit integer", P->comp_no[s]);
        }
        P->W.push_back((int32_t)w);
    }
    MF_TRY(P->count.alloc(ctx, ns));
    MF_HIP(hipMemsetAsync(P->count.p, 0, (ns ? ns : 1) * 8, ctx->stream));
    return MF_OK;
}
int cp_select(mf_ctx *ctx, const uint32_t *d_comp, uint64_t n_comps, uint64_t nk, const std::vector<uint32_t> &slot_of, mf_buf<uint32_t> &dslot,
              mf_buf<uint32_t> &flag, mf_buf<uint64_t> &rank, uint64_t *nm) {
    hipStream_t st = ctx->stream;
    mf_buf<uint64_t> tot;
    MF_TRY(dslot.alloc(ctx, n_comps)); MF_TRY(flag.alloc(ctx, nk)); MF_TRY(rank.alloc(ctx, nk + 1)); MF_TRY(tot.alloc(ctx, 1));
    MF_HIP(hipMemcpyAsync(dslot.p, slot_of.data(), n_comps * 4, hipMemcpyHostToDevice, st));
    k_cp_select<<<cp_grid(nk), 256, 0, st>>>(d_comp, dslot.p, nk, flag.p);
    MF_TRY(mf_scan<1>(ctx, flag.p, rank.p, nk, tot.p));
    unsigned long long h = 0;
    MF_HIP(hipMemcpyAsync(&h, tot.p, 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    *nm = h;
    return MF_OK;
}
int cp_max_listings(mf_paths *P) {
    mf_ctx *ctx = P->ctx;
    hipStream_t st = ctx->stream;
    mf_buf<unsigned int> maxl;
    MF_TRY(maxl.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(maxl.p, 0, 4, st));
    k_cp_maxlist<<<cp_grid(P->nd), 256, 0, st>>>(P->lo.p, P->nd, maxl.p);
    MF_HIP(hipGetLastError());
    unsigned int h = 0;
    MF_HIP(hipMemcpyAsync(&h, maxl.p, 4, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    P->max_listings = std::max(1u, h);
    // a thread of k_cp_mark counts up to CP_RUN x listings starts in 32 bits
    if (P->max_listings >= (1u << 26)) return mf_set_error("component-paths: a k-mer is listed by %u of the selected components (fewer than 2^26)", P->max_listings);
    return MF_OK;
}

extern "C" void mf_paths_destroy(mf_paths *p) { delete p; }

extern "C" int mf_paths_create(mf_ctx *ctx, mf_comps *c, const uint32_t *selection, uint64_t n_selection, int min_len, uint64_t max_paths, mf_paths **out) {
    mf_range rng_("mf:paths_create");
    if (!ctx || !c || !out) return mf_set_error("mf_paths_create: NULL argument");
    *out = nullptr;
    if (c->ctx != ctx) return mf_set_error("mf_paths_create: the components belong to another context");
    if (c->k < 1 || c->k > 31) return mf_set_error("mf_paths_create: the components do not know their k (mf_comps_set_k), or it is not in [1,31]");
    if (n_selection && !selection) return mf_set_error("mf_paths_create: NULL argument");
    if (c->n >= 0xFFFFFFFFull) return mf_set_error("component-paths: %llu components (fewer than 2^32 - 1)", (unsigned long long)c->n);
    if (max_paths >= 0xFFFFFFFFull) return mf_set_error("component-paths: max_paths = %llu (fewer than 2^32 - 1)", (unsigned long long)max_paths);
    MF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::unique_ptr<mf_paths> P(new mf_paths());
    P->ctx = ctx; P->k = c->k; P->min_len = min_len; P->max_paths = max_paths;
    std::vector<uint32_t> slot_of;
    MF_TRY(cp_slots_of(P.get(), c->n, c->sizes.data(), c->weights.data(), selection, n_selection, slot_of));
    const uint64_t ns = P->n_slots;
    const uint64_t nk = c->n_kmers;
    if (nk && ns) {
        mf_buf<uint32_t> dslot, flag; mf_buf<uint64_t> rank, tot; mf_buf<unsigned int> scal;
        uint64_t nm = 0;
        MF_TRY(cp_select(ctx, c->d_comp, c->n, nk, slot_of, dslot, flag, rank, &nm));
        MF_TRY(tot.alloc(ctx, 1)); MF_TRY(scal.alloc(ctx, 1));
        MF_HIP(hipMemsetAsync(scal.p, 0, 4, st));
        P->nm = nm;
        if (nm) {
            mf_buf<uint64_t> mk, mk1, mk2; mf_buf<uint32_t> ms, ms1;
            MF_TRY(mk.alloc(ctx, nm)); MF_TRY(ms.alloc(ctx, nm)); MF_TRY(mk1.alloc(ctx, nm)); MF_TRY(ms1.alloc(ctx, nm));
            k_cp_members<<<cp_grid(nk), 256, 0, st>>>(c->d_kmers, c->d_comp, dslot.p, flag.p, rank.p, nk, mk.p, ms.p);
            MF_HIP(hipGetLastError());
            // by slot, then (stable) by k-mer: the listings of a k-mer lie together, their slots ascend
            MF_TRY(mf_sort_u32_u64(ctx, ms.p, mk.p, nm, cp_slot_bits(ns), ms1.p, mk1.p));
            mk.reset(); ms.reset();
            MF_TRY(mk2.alloc(ctx, nm)); MF_TRY(P->slots.alloc(ctx, nm));
            MF_TRY(mf_sort_u64_u32(ctx, mk1.p, ms1.p, nm, 64, mk2.p, P->slots.p));      // (all 64 bits: a k-mer that does not fit k bases is found below)
            mk1.reset(); ms1.reset();
            mf_buf<uint32_t> hflag; mf_buf<uint64_t> hrank;
            MF_TRY(hflag.alloc(ctx, nm)); MF_TRY(hrank.alloc(ctx, nm + 1));
            k_cp_heads<<<cp_grid(nm), 256, 0, st>>>(mk2.p, nm, P->k, hflag.p, &scal.p[0]);
            MF_TRY(mf_scan<1>(ctx, hflag.p, hrank.p, nm, tot.p));
            unsigned long long nd = 0; unsigned int h_bad = 0;
            MF_HIP(hipMemcpyAsync(&nd, tot.p, 8, hipMemcpyDeviceToHost, st));
            MF_HIP(hipMemcpyAsync(&h_bad, scal.p, 4, hipMemcpyDeviceToHost, st));
            MF_HIP(hipStreamSynchronize(st));
            if (h_bad) return mf_set_error("component-paths: a component holds a k-mer that does not fit %d bases", P->k);
            P->nd = nd;
            mf_buf<uint64_t> dk;
            MF_TRY(dk.alloc(ctx, nd)); MF_TRY(P->lo.alloc(ctx, nd + 1));
            k_cp_distinct<<<cp_grid(nm + 1), 256, 0, st>>>(mk2.p, hflag.p, hrank.p, nm, dk.p, P->lo.p);
            MF_HIP(hipGetLastError());
            MF_TRY(mf_index_build(ctx, dk.p, nullptr, nd, &P->index, &P->index_bytes));
            MF_HIP(hipGetLastError());
            MF_TRY(cp_max_listings(P.get()));               // (synchronises: dk and the sort's buffers go back to the arena)
            if (!selection && c->shared < 0) c->shared = nd < nm ? 1 : 0;       // (all members were looked at: does the member list hold a k-mer twice?)
        }
    }
    MF_HIP(hipStreamSynchronize(st));
    *out = P.release();
    return MF_OK;
}

extern "C" int mf_paths_add(mf_paths *P, const void *d_bases, const void *d_offsets, uint64_t n_seqs, uint64_t n_bases) {
    mf_range rng_("mf:paths_add");
    if (!P) return mf_set_error("mf_paths_add: NULL argument");
    if (P->finished) return mf_set_error("mf_paths_add: the paths are finished");
    if (n_seqs >= 0xFFFFFFFFull) return mf_set_error("component-paths: %llu sequences in one batch (fewer than 2^32 - 1)", (unsigned long long)n_seqs);
    if (!n_seqs) return MF_OK;
    if (!d_bases || !d_offsets) return mf_set_error("mf_paths_add: NULL argument");
    mf_ctx *ctx = P->ctx;
    MF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint8_t *bases = (const uint8_t *)d_bases;
    const uint64_t *off = (const uint64_t *)d_offsets;
    const uint64_t n = n_seqs; const int k = P->k;

    // 1. the threads every sequence takes
    mf_buf<uint32_t> runs; mf_buf<uint64_t> srun, tot; mf_buf<unsigned int> bad;
    MF_TRY(runs.alloc(ctx, n)); MF_TRY(srun.alloc(ctx, n + 1)); MF_TRY(tot.alloc(ctx, 2)); MF_TRY(bad.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(bad.p, 0, 4, st));
    k_cp_sizes<<<cp_grid(n), 256, 0, st>>>(off, n, k, runs.p, bad.p);
    MF_HIP(hipGetLastError());
    MF_TRY(cp_scan(ctx, runs.p, srun.p, n, &tot.p[0]));
    unsigned int h_bad = 0; uint64_t h_end = 0, n_runs = 0;
    MF_HIP(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, st));
    MF_HIP(hipMemcpyAsync(&h_end, off + n, 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipMemcpyAsync(&n_runs, &tot.p[0], 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    if (h_bad) return mf_set_error("component-paths: offsets that go backwards, or a sequence of 2^31 or more k-mers");
    if (h_end != n_bases) return mf_set_error("component-paths: the offsets end at %llu, n_bases = %llu", (unsigned long long)h_end, (unsigned long long)n_bases);
    if (!n_runs || !P->nm) return MF_OK;
    if (n_runs >= (1ull << 39)) return mf_set_error("component-paths: %llu k-mer positions in one batch (fewer than 2^44)", (unsigned long long)n_runs * CP_RUN);
    runs.reset();

    // 2. marking: count, scan, emit
    const cp_members<cp_keys64> M{cp_keys64{P->wide ? mf_index_view{} : mf_view(P->index)}, P->lo.p, P->slots.p};
    mf_buf<uint64_t> os, oe;
    MF_TRY(os.alloc(ctx, n_runs + 1)); MF_TRY(oe.alloc(ctx, n_runs + 1));
    {
        mf_buf<uint32_t> cs, ce;
        MF_TRY(cs.alloc(ctx, n_runs)); MF_TRY(ce.alloc(ctx, n_runs));
        {
            mf_ktimer tm(ctx, "k_cp_mark");
            if (P->wide) MF_TRY(cp_mark_wide(P, false, cp_mark_args{bases, off, srun.p, n, n_runs, cs.p, ce.p, nullptr, nullptr, cp_marks{nullptr, nullptr}, cp_marks{nullptr, nullptr}}));
            else k_cp_mark<false><<<cp_grid(n_runs, CP_WG), CP_WG, 0, st>>>(bases, off, srun.p, n, n_runs, k, M, cs.p, ce.p, nullptr, nullptr, cp_marks{nullptr, nullptr},
                                                                          cp_marks{nullptr, nullptr});
        }
        MF_HIP(hipGetLastError());
        MF_TRY(cp_scan(ctx, cs.p, os.p, n_runs, &tot.p[0]));
        MF_TRY(cp_scan(ctx, ce.p, oe.p, n_runs, &tot.p[1]));
        MF_HIP(hipStreamSynchronize(st));
    }
    uint64_t h_tot[2] = {0, 0};
    MF_HIP(hipMemcpyAsync(h_tot, tot.p, 16, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    const uint64_t nr = h_tot[0];
    if (h_tot[1] != nr) return mf_set_error("component-paths: internal error, %llu starts and %llu ends", (unsigned long long)nr, (unsigned long long)h_tot[1]);
    if (nr >= 0xFFFFFFFFull) return mf_set_error("component-paths: %llu runs in one batch (the sort takes fewer than 2^32 - 1: give the sequences in smaller batches)", (unsigned long long)nr);
    if (!nr) return MF_OK;
    mf_buf<uint32_t> ss, es; mf_buf<uint64_t> sp, ep;
    MF_TRY(ss.alloc(ctx, nr)); MF_TRY(sp.alloc(ctx, nr)); MF_TRY(es.alloc(ctx, nr)); MF_TRY(ep.alloc(ctx, nr));
    {
        mf_buf<uint32_t> us, ue; mf_buf<uint64_t> ups, upe;
        MF_TRY(us.alloc(ctx, nr)); MF_TRY(ups.alloc(ctx, nr)); MF_TRY(ue.alloc(ctx, nr)); MF_TRY(upe.alloc(ctx, nr));
        {
            mf_ktimer tm(ctx, "k_cp_mark");
            if (P->wide) MF_TRY(cp_mark_wide(P, true, cp_mark_args{bases, off, srun.p, n, n_runs, nullptr, nullptr, os.p, oe.p, cp_marks{us.p, ups.p}, cp_marks{ue.p, upe.p}}));
            else k_cp_mark<true><<<cp_grid(n_runs, CP_WG), CP_WG, 0, st>>>(bases, off, srun.p, n, n_runs, k, M, nullptr, nullptr, os.p, oe.p, cp_marks{us.p, ups.p},
                                                                         cp_marks{ue.p, upe.p});
        }
        MF_HIP(hipGetLastError());
        // 3. pairing: both lists by slot, position order kept inside a slot
        const int cb = cp_slot_bits(P->n_slots);
        MF_TRY(mf_sort_u32_u64(ctx, us.p, ups.p, nr, cb, ss.p, sp.p));
        MF_TRY(mf_sort_u32_u64(ctx, ue.p, upe.p, nr, cb, es.p, ep.p));
    }
    os.reset(); oe.reset(); srun.reset();
    mf_buf<uint32_t> flag, keep, head; mf_buf<uint64_t> rank, rank2;
    MF_TRY(flag.alloc(ctx, nr)); MF_TRY(keep.alloc(ctx, nr)); MF_TRY(head.alloc(ctx, P->n_slots)); MF_TRY(rank.alloc(ctx, nr + 1)); MF_TRY(rank2.alloc(ctx, nr + 1));
    k_cp_pair<<<cp_grid(nr), 256, 0, st>>>(ss.p, sp.p, es.p, ep.p, nr, k, P->min_len, flag.p, head.p, bad.p);
    MF_TRY(mf_scan<1>(ctx, flag.p, rank.p, nr, &tot.p[0]));
    // 4. the cap across the batches
    k_cp_keep<<<cp_grid(nr), 256, 0, st>>>(ss.p, flag.p, rank.p, head.p, P->count.p, (unsigned long long)P->max_paths, nr, keep.p);
    MF_TRY(mf_scan<1>(ctx, keep.p, rank2.p, nr, &tot.p[1]));
    k_cp_bump<<<cp_grid(nr), 256, 0, st>>>(ss.p, rank.p, head.p, nr, P->count.p, (unsigned long long)P->max_paths);
    MF_HIP(hipGetLastError());
    MF_HIP(hipMemcpyAsync(h_tot, tot.p, 16, hipMemcpyDeviceToHost, st));
    MF_HIP(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    if (h_bad) return mf_set_error("component-paths: internal error, the starts and the ends of the runs do not pair up");
    const uint64_t nkept = h_tot[1];
    if (!nkept) return MF_OK;
    if (P->n_rec + nkept >= 0xFFFFFFFFull) return mf_set_error("component-paths: %llu paths kept (fewer than 2^32 - 1)", (unsigned long long)(P->n_rec + nkept));
    // 5. the path store
    if (P->n_rec + nkept > P->rec_cap || !P->rslot.p) {
        const uint64_t cap = std::max<uint64_t>(P->n_rec + nkept, P->rec_cap + P->rec_cap / 2);
        MF_TRY(cp_grow(ctx, P->rslot, P->n_rec, P->rec_cap, cap)); MF_TRY(cp_grow(ctx, P->rlen, P->n_rec, P->rec_cap, cap)); MF_TRY(cp_grow(ctx, P->roff, P->n_rec, P->rec_cap, cap));
        P->rec_cap = cap;
    }
    mf_buf<uint64_t> src, toff;
    MF_TRY(src.alloc(ctx, nkept)); MF_TRY(toff.alloc(ctx, nkept + 1));
    k_cp_records<<<cp_grid(nr), 256, 0, st>>>(ss.p, sp.p, ep.p, keep.p, rank2.p, nr, k, P->rslot.p + P->n_rec, P->rlen.p + P->n_rec, src.p);
    MF_HIP(hipGetLastError());
    MF_TRY(cp_scan(ctx, P->rlen.p + P->n_rec, toff.p, nkept, &tot.p[0]));
    uint64_t nb = 0;
    MF_HIP(hipMemcpyAsync(&nb, &tot.p[0], 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    if (P->n_text + nb > P->text_cap || !P->text.p) {
        const uint64_t cap = std::max<uint64_t>(P->n_text + nb, P->text_cap + P->text_cap / 2);
        MF_TRY(cp_grow(ctx, P->text, P->n_text, P->text_cap, cap));
        P->text_cap = cap;
    }
    k_cp_copy<<<cp_grid(nkept * 64), 256, 0, st>>>(bases, src.p, P->rlen.p + P->n_rec, toff.p, nkept, P->n_text, P->text.p, P->roff.p + P->n_rec);
    MF_HIP(hipGetLastError());
    MF_HIP(hipStreamSynchronize(st));                      // (the caller may release the bases; this batch's buffers go back to the arena)
    P->n_rec += nkept; P->n_text += nb;
    return MF_OK;
}

extern "C" int mf_paths_finish(mf_paths *P) {
    mf_range rng_("mf:paths_finish");
    if (!P) return mf_set_error("mf_paths_finish: NULL argument");
    if (P->finished) return MF_OK;
    mf_ctx *ctx = P->ctx;
    MF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t ns = P->n_slots, nr = P->n_rec;
    std::vector<unsigned long long> cnt(ns ? ns : 1, 0);
    if (ns) MF_HIP(hipMemcpyAsync(cnt.data(), P->count.p, ns * 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    P->h_count.assign(cnt.begin(), cnt.begin() + ns);
    std::vector<uint64_t> sfirst(ns + 1, 0);
    for (uint64_t s = 0; s < ns; s++) sfirst[s + 1] = sfirst[s] + P->h_count[s];
    if (sfirst[ns] != nr) return mf_set_error("component-paths: internal error, %llu paths counted and %llu stored", (unsigned long long)sfirst[ns], (unsigned long long)nr);
    P->h_boff.assign(ns + 1, 0);
    if (nr) {
        mf_buf<uint64_t> key; mf_buf<uint32_t> idx;
        MF_TRY(key.alloc(ctx, nr)); MF_TRY(idx.alloc(ctx, nr));
        {
            mf_buf<uint64_t> k0; mf_buf<uint32_t> i0;
            MF_TRY(k0.alloc(ctx, nr)); MF_TRY(i0.alloc(ctx, nr));
            k_cp_keys<<<cp_grid(nr), 256, 0, st>>>(P->rslot.p, P->rlen.p, nr, k0.p, i0.p);
            MF_HIP(hipGetLastError());
            MF_TRY(mf_sort_u64_u32(ctx, k0.p, i0.p, nr, 32 + cp_slot_bits(ns), key.p, idx.p));      // stable: ties keep encounter order
        }
        mf_buf<uint64_t> dfirst, ooff, boff, tot; mf_buf<int32_t> dW; mf_buf<uint32_t> width;
        MF_TRY(dfirst.alloc(ctx, ns + 1)); MF_TRY(dW.alloc(ctx, ns)); MF_TRY(width.alloc(ctx, nr)); MF_TRY(ooff.alloc(ctx, nr + 1)); MF_TRY(boff.alloc(ctx, ns + 1));
        MF_TRY(tot.alloc(ctx, 1));
        MF_HIP(hipMemcpyAsync(dfirst.p, sfirst.data(), (ns + 1) * 8, hipMemcpyHostToDevice, st));
        MF_HIP(hipMemcpyAsync(dW.p, P->W.data(), ns * 4, hipMemcpyHostToDevice, st));
        k_cp_widths<<<cp_grid(nr), 256, 0, st>>>(key.p, nr, dfirst.p, dW.p, width.p);
        MF_HIP(hipGetLastError());
        MF_TRY(cp_scan(ctx, width.p, ooff.p, nr, tot.p));
        k_cp_slot_bytes<<<cp_grid(ns + 1), 256, 0, st>>>(ooff.p, dfirst.p, ns + 1, boff.p);
        MF_HIP(hipGetLastError());
        MF_HIP(hipMemcpyAsync(P->h_boff.data(), boff.p, (ns + 1) * 8, hipMemcpyDeviceToHost, st));
        MF_HIP(hipStreamSynchronize(st));
        P->out_bytes = P->h_boff[ns];
        MF_TRY(P->out.alloc(ctx, P->out_bytes));
        k_cp_write_head<<<cp_grid(nr), 256, 0, st>>>(key.p, nr, dfirst.p, dW.p, ooff.p, P->out.p);
        k_cp_write_bases<<<cp_grid(nr * 64), 256, 0, st>>>(key.p, idx.p, nr, dfirst.p, dW.p, P->roff.p, P->text.p, ooff.p, P->out.p);
        MF_HIP(hipGetLastError());
        MF_HIP(hipStreamSynchronize(st));
    }
    P->rslot.reset(); P->rlen.reset(); P->roff.reset(); P->text.reset();      // the store is printed
    P->finished = true;
    return MF_OK;
}

extern "C" int mf_paths_stats(const mf_paths *P, uint64_t *n_slots, uint64_t *n_paths, uint64_t *n_bytes, uint64_t *max_listings) {
    if (!P) return mf_set_error("paths handle is NULL");
    if ((n_paths || n_bytes) && !P->finished) return mf_set_error("mf_paths_stats: the paths are not finished");
    if (n_slots) *n_slots = P->n_slots;
    if (n_paths) *n_paths = P->n_rec;
    if (n_bytes) *n_bytes = P->out_bytes;
    if (max_listings) *max_listings = P->max_listings;
    return MF_OK;
}
extern "C" int mf_paths_slots(const mf_paths *P, uint32_t *component_no, uint64_t *n_paths, uint64_t *n_bytes, uint8_t *reached_cap) {
    if (!P) return mf_set_error("paths handle is NULL");
    if ((n_paths || n_bytes || reached_cap) && !P->finished) return mf_set_error("mf_paths_slots: the paths are not finished");
    for (uint64_t s = 0; s < P->n_slots; s++) {
        if (component_no) component_no[s] = P->comp_no[s];
        if (n_paths) n_paths[s] = P->h_count[s];
        if (n_bytes) n_bytes[s] = P->h_boff[s + 1] - P->h_boff[s];
        if (reached_cap) reached_cap[s] = P->h_count[s] == P->max_paths ? 1 : 0;      // ans[i].size() == MAX_PATHS_COUNT (:163)
    }
    return MF_OK;
}
extern "C" int mf_paths_text(const mf_paths *P, int64_t slot, uint8_t *text, uint64_t cap, uint64_t *n) {
    if (!P) return mf_set_error("paths handle is NULL");
    if (!P->finished) return mf_set_error("mf_paths_text: the paths are not finished");
    if (slot < -1 || slot >= (int64_t)P->n_slots) return mf_set_error("mf_paths_text: slot %lld of %llu", (long long)slot, (unsigned long long)P->n_slots);
    const uint64_t a = slot < 0 ? 0 : P->h_boff[slot], b = slot < 0 ? P->out_bytes : P->h_boff[slot + 1];
    if (n) *n = b - a;
    if (cap < b - a || b == a) return MF_OK;
    if (!text) return mf_set_error("mf_paths_text: NULL argument");
    MF_HIP(hipSetDevice(P->ctx->device));
    MF_HIP(hipMemcpyAsync(text, P->out.p + a, b - a, hipMemcpyDeviceToHost, P->ctx->stream));
    MF_HIP(hipStreamSynchronize(P->ctx->stream));
    return MF_OK;
}
// component-<no>.seq.fasta for every slot under out_dir (made if it is not there): the host only writes the buffer
extern "C" int mf_paths_write(const mf_paths *P, const char *out_dir, uint64_t *n_paths) {
    if (!P || !out_dir) return mf_set_error("mf_paths_write: NULL argument");
    if (!P->finished) return mf_set_error("mf_paths_write: the paths are not finished");
    if (mkdir(out_dir, 0777) != 0 && errno != EEXIST) return mf_set_error("can't create directory '%s'", out_dir);
    MF_HIP(hipSetDevice(P->ctx->device));
    const uint64_t piece = 64ull << 20;
    std::vector<uint8_t> buf;
    for (uint64_t s = 0; s < P->n_slots; s++) {
        const std::string path = std::string(out_dir) + "/component-" + std::to_string(P->comp_no[s]) + ".seq.fasta";
        FILE *f = fopen(path.c_str(), "w");
        if (!f) return mf_set_error("can't write '%s'", path.c_str());
        bool bad = false;
        for (uint64_t at = P->h_boff[s]; at < P->h_boff[s + 1] && !bad; at += piece) {
            const uint64_t m = std::min<uint64_t>(piece, P->h_boff[s + 1] - at);
            if (buf.size() < m) buf.resize(m);
            if (hipMemcpyAsync(buf.data(), P->out.p + at, m, hipMemcpyDeviceToHost, P->ctx->stream) != hipSuccess || hipStreamSynchronize(P->ctx->stream) != hipSuccess) { bad = true; break; }
            bad = fwrite(buf.data(), 1, m, f) != m;
        }
        if (fclose(f) != 0) bad = true;
        if (bad) return mf_set_error("can't write '%s'", path.c_str());
    }
    if (n_paths) *n_paths = P->n_rec;
    return MF_OK;
}

// ---- the file form (ComponentPathsMain.runImpl :82-190) ----
extern "C" int mf_component_paths(mf_ctx *ctx, const char *components_bin, int k, const char *const *files, int nfiles, const uint32_t *selection, uint64_t n_selection,
                                  int min_len, uint64_t max_paths, const char *out_dir, uint64_t *n_components, uint64_t *n_paths) {
    mf_range rng_("mf:component_paths(files)");
    if (!ctx || !components_bin || !out_dir || nfiles < 0 || (nfiles > 0 && !files)) return mf_set_error("mf_component_paths: NULL argument");
    if (k < 1 || k > 31) return mf_set_error("k must be in [1,31]");
    mf_comps *c = nullptr;
    MF_TRY(mf_comps_load(ctx, components_bin, &c));
    std::unique_ptr<mf_comps, void (*)(mf_comps *)> gc(c, [](mf_comps *p) { mf_comps_destroy(p); });
    MF_TRY(mf_comps_set_k(c, k));
    mf_paths *P = nullptr;
    MF_TRY(mf_paths_create(ctx, c, selection, n_selection, min_len, max_paths, &P));
    std::unique_ptr<mf_paths> gp(P);
    for (int f = 0; f < nfiles; f++) {                     // one file resident at a time, in the order given (:128-160)
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
