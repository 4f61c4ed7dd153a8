// mf_join.hip -- kernels and host helpers of the join core (mf_join.h; DESIGN.md section 7a, "the join core").
#include "mf_join.h"
#include <algorithm>
#include <cmath>
#include <sys/stat.h>

// ---------------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void k_stats_init(mf_uslot *__restrict__ slots, uint64_t cap, uint64_t y) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * blockDim.x) {
        ulonglong2 v; v.x = MF_EMPTY; v.y = y;
        *reinterpret_cast<ulonglong2 *>(&slots[i]) = v;
    }
}

static constexpr uint64_t MF_COLOR_FIELD_MAX = (1ull << 20) - 1;
// flags: bit 0 = a key >= 2^62, bit 1 = the table is full
template <int MODE>
__global__ __launch_bounds__(256) void k_stats_union(mf_uslot *__restrict__ slots, uint64_t mask, const uint64_t *__restrict__ keys,
                                                     const uint16_t *__restrict__ cnts, uint64_t n, int thr, uint32_t add, uint32_t S, uint32_t s,
                                                     unsigned long long *__restrict__ n_union, unsigned int *__restrict__ flags) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = cnts[i];
        if ((int)c <= thr) continue;
        const uint64_t key = keys[i];
        const mf_join_key k = mf_join_mine<true>(key, S, s, flags);
        if (!k.mine) continue;
        uint64_t p = k.h & mask;
        bool done = false;
        for (uint64_t probe = 0; probe <= mask; probe++) {
            const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long *>(&slots[p].key), (unsigned long long)MF_EMPTY,
                                                     (unsigned long long)key);
            if (old == MF_EMPTY || old == key) {
                if (old == MF_EMPTY) atomicAdd(n_union, 1ull);
                if (MODE == MF_UNION_PRESENCE) atomicAdd(&slots[p].cnt, add);
                else if (MODE == MF_UNION_SUM) { atomicAdd(&slots[p].cnt, 1u); atomicAdd(&slots[p].row, c); }
                else if (MODE == MF_UNION_COLOR) {
                    const uint32_t sh = 20u * (add & 3u);
                    const uint64_t inc = (add & 4u) ? (uint64_t)c : 1ull;
                    unsigned long long *w = reinterpret_cast<unsigned long long *>(&slots[p].cnt);
                    unsigned long long cur = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    for (;;) {
                        const uint64_t f = (cur >> sh) & MF_COLOR_FIELD_MAX;
                        const uint64_t nf = f + inc < MF_COLOR_FIELD_MAX ? f + inc : MF_COLOR_FIELD_MAX;
                        const unsigned long long nw = (cur & ~(MF_COLOR_FIELD_MAX << sh)) | (nf << sh);
                        if (nw == cur) break;
                        const unsigned long long old = atomicCAS(w, cur, nw);
                        if (old == cur) break;
                        cur = old;
                    }
                }
                else if (add == 2u) atomicAdd(&slots[p].row, c);
                else atomicAdd(&slots[p].cnt, c << (16u * add));
                done = true;
                break;
            }
            p = (p + 1) & mask;
        }
        if (!done) atomicOr(flags, 2u);
    }
}

// the occupied slots that P keeps -> (key, P's value)   (uniform trip count: every lane reaches mf_wave_reserve)
template <typename P>
__global__ __launch_bounds__(256) void k_join_read(const mf_uslot *__restrict__ slots, uint64_t cap, const P proj, uint64_t *__restrict__ okeys,
                                                   typename P::value *__restrict__ ovals, unsigned int *__restrict__ cursor) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < cap; i0 += stride) {
        const uint64_t i = i0 + threadIdx.x;
        ulonglong2 raw; raw.x = MF_EMPTY; raw.y = 0;
        if (i < cap) raw = *reinterpret_cast<const ulonglong2 *>(&slots[i]);
        const bool keep = raw.x != MF_EMPTY && proj.keep(raw);
        const uint32_t r = mf_wave_reserve(cursor, keep ? 1u : 0u);
        if (keep) { okeys[r] = raw.x; ovals[r] = proj.val(raw); }
    }
}

// run heads of the sorted values -> (value, index of its first occurrence), in any order
__global__ __launch_bounds__(256) void k_kmf_runs(const uint64_t *__restrict__ tri, uint64_t n, uint64_t *__restrict__ vals, uint64_t *__restrict__ starts,
                                                  unsigned int *__restrict__ cursor) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n; i0 += stride) {
        const uint64_t i = i0 + threadIdx.x;
        const bool head = i < n && (i == 0 || tri[i] != tri[i - 1]);
        const uint32_t r = mf_wave_reserve(cursor, head ? 1u : 0u);
        if (head) { vals[r] = tri[i]; starts[r] = i; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
static uint64_t pow2_ge(uint64_t x) { uint64_t p = 1; while (p < x) p <<= 1; return p; }

int plan_slices(mf_ctx *ctx, uint64_t total, uint32_t *S_out, uint64_t *cap_out) {
    uint32_t S = (uint32_t)std::max<int64_t>(ctx->opt_stats_slices, 0);
    auto cap_of = [&](uint32_t s) {
        const double per = (double)total / s;
        return pow2_ge((uint64_t)(2.0 * (per + 6.0 * std::sqrt(per) + 1024.0)));
    };
    if (!S) {
        size_t fr = 0, tot = 0;
        MF_HIP(hipMemGetInfo(&fr, &tot));
        const double budget = 0.4 * (double)(fr + mf_arena_idle(ctx));
        S = 1;
        while (S < 4096 && (double)cap_of(S) * sizeof(mf_uslot) > budget) S++;
    }
    *S_out = S;
    *cap_out = cap_of(S);
    if (*cap_out >= (1ull << 40)) return mf_set_error("stats join: %llu entries do not fit", (unsigned long long)total);
    return MF_OK;
}

unsigned grid_for(mf_ctx *ctx, uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->n_cu * 16)); }

int tables_total(mf_ctx *ctx, mf_table *const *t, int n, const char *what, uint64_t *total) {
    for (int j = 0; j < n; j++) {
        if (!t[j]) return mf_set_error("%s: table %d is NULL", what, j);
        if (t[j]->ctx != ctx) return mf_set_error("%s: table %d belongs to another context", what, j);
        if (total) *total += t[j]->n;
    }
    return MF_OK;
}

int file_records(const char *const *files, int n, uint64_t *total) {
    *total = 0;
    for (int j = 0; j < n; j++) {
        if (!files[j]) return mf_set_error("file %d is NULL", j);
        struct stat st;
        if (stat(files[j], &st) != 0) return mf_set_error("can't open '%s'", files[j]);
        *total += (uint64_t)st.st_size / 10;
    }
    return MF_OK;
}

int mf_join_flags(mf_ctx *ctx, const unsigned int *d_flags, const char *what) {
    unsigned int fl = 0;
    MF_HIP(hipMemcpyAsync(&fl, d_flags, 4, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    if (fl & 1u) return mf_set_error("%s: a k-mer key >= 2^62 (k-mers files hold k <= 31)", what);
    if (fl & 2u) return mf_set_error("%s: the union table of a slice is full (raise option stats_slices)", what);
    return MF_OK;
}

int mf_join_union(mf_ctx *ctx, const mf_join_get &get, int N, int b, int mode, const uint32_t *add, uint32_t S, uint32_t s, uint64_t cap,
                  mf_buf<mf_uslot> &slots, uint64_t *n_union) {
    static const decltype(&k_stats_union<MF_UNION_PRESENCE>) kernels[] = {k_stats_union<MF_UNION_PRESENCE>, k_stats_union<MF_UNION_SUM>,
                                                                          k_stats_union<MF_UNION_FIELD>, k_stats_union<MF_UNION_COLOR>};
    const auto kernel = kernels[mode];                    // (in the order of the enum)
    MF_TRY(slots.alloc(ctx, cap));
    mf_buf<unsigned long long> nu; MF_TRY(nu.alloc(ctx, 1));
    mf_buf<unsigned int> flags; MF_TRY(flags.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(nu.p, 0, 8, ctx->stream));
    MF_HIP(hipMemsetAsync(flags.p, 0, 4, ctx->stream));
    {
        mf_ktimer tm(ctx, "k_stats_init");
        k_stats_init<<<grid_for(ctx, cap), 256, 0, ctx->stream>>>(slots.p, cap, mode == MF_UNION_PRESENCE ? (uint64_t)MF_NO_ROW << 32 : 0ull);
    }
    for (int j = 0; j < N; j++)
        MF_TRY(mf_join_pass(ctx, get, j, "stats join: union pass", [&](const mf_table *t) {
            mf_ktimer tm(ctx, "k_stats_union");
            kernel<<<grid_for(ctx, t->n), 256, 0, ctx->stream>>>(slots.p, cap - 1, t->d_keys, t->d_counts, t->n, b, add[j], S, s, nu.p, flags.p);
        }));
    unsigned long long n = 0;
    MF_HIP(hipMemcpyAsync(&n, nu.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    MF_TRY(mf_join_flags(ctx, flags.p, "stats join"));
    *n_union = n;
    return MF_OK;
}

template <typename P>
int mf_join_read(mf_ctx *ctx, const mf_uslot *slots, uint64_t cap, uint64_t nu, const P &proj, mf_join_parts<uint64_t, typename P::value> &parts) {
    if (nu > MF_JOIN_CURSOR_MAX)
        return mf_set_error("%s: %llu union k-mers in one slice, at most 2^32 - 1 (raise option stats_slices)", P::tool, (unsigned long long)nu);
    uint64_t *ok = nullptr; typename P::value *ov = nullptr;
    MF_TRY(parts.add(ctx, nu, &ok, &ov));
    unsigned int m = 0;
    MF_TRY(mf_join_cursors(ctx, 1, &m, [&](unsigned int *cur) {
        mf_ktimer tm(ctx, P::timer);
        k_join_read<P><<<grid_for(ctx, cap), 256, 0, ctx->stream>>>(slots, cap, proj, ok, ov, cur);
    }));
    if (P::all && m != nu) return mf_set_error("%s: %u union entries written, %llu claimed", P::tool, m, (unsigned long long)nu);
    if (m > nu) return mf_set_error("%s: %u survivors of %llu union entries", P::tool, m, (unsigned long long)nu);
    parts.wrote(m);
    return MF_OK;
}
template int mf_join_read(mf_ctx *, const mf_uslot *, uint64_t, uint64_t, const mf_read_nsamples &, mf_join_parts<uint64_t, uint16_t> &);
template int mf_join_read(mf_ctx *, const mf_uslot *, uint64_t, uint64_t, const mf_read_kps &, mf_join_parts<uint64_t, uint16_t> &);
template int mf_join_read(mf_ctx *, const mf_uslot *, uint64_t, uint64_t, const mf_read_color &, mf_join_parts<uint64_t, uint64_t> &);
template int mf_join_read(mf_ctx *, const mf_uslot *, uint64_t, uint64_t, const mf_read_ukm &, mf_join_parts<uint64_t, uint32_t> &);
template int mf_join_read(mf_ctx *, const mf_uslot *, uint64_t, uint64_t, const mf_read_uk &, mf_join_parts<uint64_t, uint16_t> &);

int pairs_to_table(mf_ctx *ctx, mf_buf<uint64_t> &keys, mf_buf<uint16_t> &vals, uint64_t n, mf_table **out) {
    const int k = 31;
    mf_buf<uint64_t> sk; mf_buf<uint16_t> sv;
    MF_TRY(sk.alloc(ctx, n)); MF_TRY(sv.alloc(ctx, n));
    if (n) MF_TRY(mf_sort_pairs(ctx, keys.p, vals.p, n, 2 * k, sk.p, sv.p));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    const size_t kb = sk.bytes(), vb = sv.bytes();
    return mf_table_adopt(ctx, k, n, 0, sk.take(), kb, sv.take(), vb, out);
}

int empty_table(mf_ctx *ctx, mf_table **out) {
    mf_buf<uint64_t> k; mf_buf<uint16_t> v;
    MF_TRY(k.alloc(ctx, 0)); MF_TRY(v.alloc(ctx, 0));
    return pairs_to_table(ctx, k, v, 0, out);
}

int kmf_histogram(mf_ctx *ctx, mf_buf<uint64_t> &tri, uint64_t m, std::map<uint64_t, uint64_t> &hist, int bits) {
    if (!m) return MF_OK;
    mf_buf<uint64_t> st; mf_buf<uint16_t> d0, d1;
    MF_TRY(st.alloc(ctx, m)); MF_TRY(d0.alloc(ctx, m)); MF_TRY(d1.alloc(ctx, m));
    MF_HIP(hipMemsetAsync(d0.p, 0, d0.bytes(), ctx->stream));
    MF_TRY(mf_sort_pairs(ctx, tri.p, d0.p, m, bits, st.p, d1.p));
    d0.reset(); d1.reset();
    // (the run heads reuse tri: it has been sorted into st)
    mf_buf<uint64_t> starts; MF_TRY(starts.alloc(ctx, m));
    unsigned int r = 0;
    MF_TRY(mf_join_cursors(ctx, 1, &r, [&](unsigned int *cur) {
        mf_ktimer tm(ctx, "k_kmf_runs");
        k_kmf_runs<<<grid_for(ctx, m), 256, 0, ctx->stream>>>(st.p, m, tri.p, starts.p, cur);
    }));
    if (r > m) return mf_set_error("kmers-multiple-filters: %u runs in %llu triples", r, (unsigned long long)m);
    std::vector<uint64_t> hv(r), hs(r);
    if (r) {
        MF_HIP(hipMemcpyAsync(hv.data(), tri.p, (size_t)r * 8, hipMemcpyDeviceToHost, ctx->stream));
        MF_HIP(hipMemcpyAsync(hs.data(), starts.p, (size_t)r * 8, hipMemcpyDeviceToHost, ctx->stream));
        MF_HIP(hipStreamSynchronize(ctx->stream));
    }
    std::vector<uint32_t> order(r);
    for (uint32_t i = 0; i < r; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return hs[x] < hs[y]; });
    for (uint32_t i = 0; i < r; i++) {
        const uint64_t end = i + 1 < r ? hs[order[i + 1]] : m;
        hist[hv[order[i]]] += end - hs[order[i]];
    }
    return MF_OK;
}

// =============================================================================================
// Test hooks (tests/test_join_slots_gpu.py, tests/test_join_crafted_gpu.py; NOT part of the C-ABI -- not in include/metafast_hip.h; DESIGN.md
// section 7a, "The union table, as the tests pin it").  The union table slot by slot: the tests craft keys from the inverse of mf_hash64, so
// they choose every key's home slot and slice.
//   mf_debug_join_plan     plan_slices on `total` with the context's option stats_slices
//   mf_debug_join_union    mf_join_union on the caller's tables with the slice count, slice and capacity given (a power of two >= 1 -- the
//                          host never picks one below 2048) -> the cap raw 16-byte slots and n_union; an error of the pass is the production
//                          message
//   mf_debug_join_find     a slot table from the host; one thread per key: mf_join_mine<false>, then mf_join_find -> the slot,
//                          MF_JOIN_NOT_FOUND, or MF_JOIN_NOT_MINE for a key >= 2^62 or of another slice
//   mf_debug_join_read     a slot table from the host through mf_join_read with projection proj = 0 .. 4 in the order of mf_join.h
//                          (nsamples, kps, color, ukm, uk; param: thresh of kps, thr of ukm) -> m (key, value) pairs, the values widened to
//                          64 bits; keys_out and vals_out have room for nu.  nu below the number of occupied slots is refused before the
//                          launch: the read-out's piece has nu entries, and the kernel writes one per kept slot.
// =============================================================================================
static constexpr uint64_t MF_JOIN_NOT_MINE = ~0ull - 1;
static constexpr uint64_t MF_DEBUG_JOIN_MAX_CAP = 1ull << 24;

__global__ __launch_bounds__(256) void k_join_probe(const mf_uslot *__restrict__ slots, uint64_t mask, const uint64_t *__restrict__ keys, uint64_t n,
                                                    uint32_t S, uint32_t s, uint64_t *__restrict__ pos) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    const mf_join_key k = mf_join_mine<false>(key, S, s, nullptr);
    ulonglong2 raw;
    pos[i] = k.mine ? mf_join_find(slots, mask, k.h, key, &raw) : MF_JOIN_NOT_MINE;
}

static int debug_join_cap(const char *what, uint64_t cap) {
    if (cap < 1 || (cap & (cap - 1)) || cap > MF_DEBUG_JOIN_MAX_CAP)
        return mf_set_error("%s: cap = %llu is not a power of two in 1 .. 2^24", what, (unsigned long long)cap);
    return MF_OK;
}
static int debug_join_upload(mf_ctx *ctx, const mf_uslot *slots, uint64_t cap, mf_buf<mf_uslot> &d) {
    MF_TRY(d.alloc(ctx, cap));
    MF_HIP(hipMemcpyAsync(d.p, slots, cap * sizeof(mf_uslot), hipMemcpyHostToDevice, ctx->stream));
    return MF_OK;
}

extern "C" int mf_debug_join_plan(mf_ctx *ctx, uint64_t total, uint32_t *S, uint64_t *cap) {
    if (!ctx || !S || !cap) return mf_set_error("mf_debug_join_plan: NULL argument");
    MF_HIP(hipSetDevice(ctx->device));
    return plan_slices(ctx, total, S, cap);
}

extern "C" int mf_debug_join_union(mf_ctx *ctx, mf_table *const *tables, int N, int b, int mode, const uint32_t *add, uint32_t S, uint32_t s,
                                   uint64_t cap, mf_uslot *slots_out, uint64_t *n_union) {
    if (!ctx || !tables || !add || !slots_out || !n_union) return mf_set_error("mf_debug_join_union: NULL argument");
    if (N < 1) return mf_set_error("mf_debug_join_union: %d tables", N);
    if (mode < MF_UNION_PRESENCE || mode > MF_UNION_COLOR) return mf_set_error("mf_debug_join_union: mode = %d (0 .. 3)", mode);
    if (S < 1 || s >= S) return mf_set_error("mf_debug_join_union: slice %u of %u", s, S);
    MF_TRY(debug_join_cap("mf_debug_join_union", cap));
    MF_HIP(hipSetDevice(ctx->device));
    MF_TRY(tables_total(ctx, tables, N, "mf_debug_join_union", nullptr));
    mf_buf<mf_uslot> slots;
    *n_union = 0;
    MF_TRY(mf_join_union(ctx, mf_join_tables(tables), N, b, mode, add, S, s, cap, slots, n_union));
    MF_HIP(hipMemcpyAsync(slots_out, slots.p, cap * sizeof(mf_uslot), hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    return MF_OK;
}

extern "C" int mf_debug_join_find(mf_ctx *ctx, const mf_uslot *slots, uint64_t cap, const uint64_t *keys, uint64_t n, uint32_t S, uint32_t s,
                                  uint64_t *pos_out) {
    if (!ctx || !slots || (n && (!keys || !pos_out))) return mf_set_error("mf_debug_join_find: NULL argument");
    if (S < 1 || s >= S) return mf_set_error("mf_debug_join_find: slice %u of %u", s, S);
    if (n > MF_JOIN_CURSOR_MAX) return mf_set_error("mf_debug_join_find: %llu keys", (unsigned long long)n);
    MF_TRY(debug_join_cap("mf_debug_join_find", cap));
    MF_HIP(hipSetDevice(ctx->device));
    if (!n) return MF_OK;
    mf_buf<mf_uslot> d; MF_TRY(debug_join_upload(ctx, slots, cap, d));
    mf_buf<uint64_t> dk, dp; MF_TRY(dk.alloc(ctx, n)); MF_TRY(dp.alloc(ctx, n));
    MF_HIP(hipMemcpyAsync(dk.p, keys, n * 8, hipMemcpyHostToDevice, ctx->stream));
    k_join_probe<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(d.p, cap - 1, dk.p, n, S, s, dp.p);
    MF_HIP(hipMemcpyAsync(pos_out, dp.p, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    return MF_OK;
}

template <typename P>
static int debug_join_read(mf_ctx *ctx, const mf_uslot *d_slots, uint64_t cap, uint64_t nu, const P &proj, uint64_t *keys_out, uint64_t *vals_out,
                           uint64_t *m) {
    mf_join_parts<uint64_t, typename P::value> parts;
    MF_TRY(mf_join_read(ctx, d_slots, cap, nu, proj, parts));
    const uint64_t n = parts.ns.back();
    std::vector<typename P::value> v((size_t)n);
    if (n) {
        MF_HIP(hipMemcpyAsync(keys_out, parts.pk.back()->p, n * 8, hipMemcpyDeviceToHost, ctx->stream));
        MF_HIP(hipMemcpyAsync(v.data(), parts.pv.back()->p, n * sizeof(typename P::value), hipMemcpyDeviceToHost, ctx->stream));
    }
    MF_HIP(hipStreamSynchronize(ctx->stream));
    for (uint64_t i = 0; i < n; i++) vals_out[i] = (uint64_t)v[(size_t)i];
    *m = n;
    return MF_OK;
}

extern "C" int mf_debug_join_read(mf_ctx *ctx, const mf_uslot *slots, uint64_t cap, uint64_t nu, int proj, int param, uint64_t *keys_out,
                                  uint64_t *vals_out, uint64_t *m) {
    if (!ctx || !slots || !m || (nu && (!keys_out || !vals_out))) return mf_set_error("mf_debug_join_read: NULL argument");
    if (proj < 0 || proj > 4) return mf_set_error("mf_debug_join_read: proj = %d (0 .. 4)", proj);
    MF_TRY(debug_join_cap("mf_debug_join_read", cap));
    uint64_t occupied = 0;
    for (uint64_t i = 0; i < cap; i++) occupied += slots[i].key != MF_EMPTY;
    if (nu < occupied)
        return mf_set_error("mf_debug_join_read: nu = %llu, the table holds %llu entries: the read-out would write past its piece",
                            (unsigned long long)nu, (unsigned long long)occupied);
    MF_HIP(hipSetDevice(ctx->device));
    *m = 0;
    mf_buf<mf_uslot> d; MF_TRY(debug_join_upload(ctx, slots, cap, d));
    switch (proj) {
    case 0: return debug_join_read(ctx, d.p, cap, nu, mf_read_nsamples{}, keys_out, vals_out, m);
    case 1: return debug_join_read(ctx, d.p, cap, nu, mf_read_kps{param}, keys_out, vals_out, m);
    case 2: return debug_join_read(ctx, d.p, cap, nu, mf_read_color{}, keys_out, vals_out, m);
    case 3: return debug_join_read(ctx, d.p, cap, nu, mf_read_ukm{param}, keys_out, vals_out, m);
    default: return debug_join_read(ctx, d.p, cap, nu, mf_read_uk{}, keys_out, vals_out, m);
    }
}
