// mf_cp.h -- what the two widths of component-paths share (mf_comppaths.hip: k <= 31, mf_wcomppaths.hip: 32 <= k <= 63): the handle, the
// marking kernel, and the width-independent steps of create.  Everything behind the marking kernel -- pairing, the cap across batches, the
// path store, the sort, the text -- works on (slot, position) records and bytes and never sees a k-mer: it lives in mf_comppaths.hip alone,
// and mf_paths_add dispatches on the handle's width for the one launch that does.
#pragma once
#include "mf_common.h"
#include <vector>

#define CP_RUN 32                     // positions per thread of k_cp_mark
#define CP_WG 256                     // threads per workgroup: a workgroup covers CP_RUN * CP_WG = 8192 positions
#define CP_NONE 0xFFFFFFFFu

struct mf_paths {
    mf_ctx *ctx = nullptr;
    int k = 0; int64_t min_len = 0; uint64_t max_paths = 0;
    uint64_t n_slots = 0;
    std::vector<uint32_t> comp_no;                       // per slot: the component's number (from 1)
    std::vector<int32_t> W;                              // per slot: Math.round(weight / (double) size)
    uint64_t nm = 0, nd = 0; uint32_t max_listings = 0;  // listings, distinct k-mers, the most listings of one k-mer
    mf_index index; size_t index_bytes = 0;              // k <= 31: the index over the distinct k-mers
    bool wide = false;                                   // 32 <= k <= 63: the distinct k-mers as two arrays and an index of 8-byte slots over them
    mf_buf<uint64_t> dhi, dlo;                           //   (position | tag, load <= 0.5: the scheme of mf_wtable_ensure_index)
    mf_buf<unsigned long long> windex; uint64_t windex_mask = 0;
    mf_buf<uint32_t> lo, slots;
    mf_buf<unsigned long long> count;                    // per slot: paths kept so far
    uint64_t n_rec = 0, n_text = 0, rec_cap = 0, text_cap = 0;       // the path store
    mf_buf<uint32_t> rslot, rlen; mf_buf<uint64_t> roff; mf_buf<uint8_t> text;
    bool finished = false;
    std::vector<uint64_t> h_count, h_boff;               // per slot: paths; first byte of the slot's text (n_slots + 1)
    mf_buf<uint8_t> out; uint64_t out_bytes = 0;
    ~mf_paths() {
        if (index.slots) mf_release(ctx, index.slots, index_bytes);
    }
};

static inline unsigned cp_grid(uint64_t n, unsigned bs = 256) { return (unsigned)((n + bs - 1) / bs); }
static inline int cp_slot_bits(uint64_t n_slots) { int cb = 1; while (cb < 32 && (1ull << cb) < n_slots) cb++; return cb; }

// ---- create, the steps that see no k-mer (mf_comppaths.hip) ----
// the slots of a selection over n components (NULL = all), the rounded weights and the counts of P; slot_of[component] = its slot or CP_NONE
int cp_slots_of(mf_paths *P, uint64_t n, const uint64_t *sizes, const int64_t *weights, const uint32_t *selection, uint64_t n_selection,
                std::vector<uint32_t> &slot_of);
// flag[j] = member j belongs to a selected component, rank = its exclusive scan, *nm = the listings; dslot = slot_of on the device
int cp_select(mf_ctx *ctx, const uint32_t *d_comp, uint64_t n_comps, uint64_t nk, const std::vector<uint32_t> &slot_of, mf_buf<uint32_t> &dslot,
              mf_buf<uint32_t> &flag, mf_buf<uint64_t> &rank, uint64_t *nm);
// P->max_listings from P->lo[0 .. P->nd], and its limit
int cp_max_listings(mf_paths *P);

// ---- add: the one launch that sees k-mers ----
struct cp_marks { uint32_t *slot; uint64_t *pos; };
struct cp_mark_args {
    const uint8_t *bases; const uint64_t *off, *srun; uint64_t n_seqs, n_runs;
    uint32_t *cnt_s, *cnt_e; const uint64_t *off_s, *off_e; cp_marks S, E;
};
// the wide handle's launch (mf_wcomppaths.hip): write = false counts, true emits
int cp_mark_wide(const mf_paths *P, bool write, const cp_mark_args &a);

#ifdef __HIPCC__
// the members as the marking kernel sees them: KEYS rolls the canonical k-mers of a stretch and finds each among the distinct k-mers --
//   keys.each(p, count, k, f): f(i, found, idx) for the positions i = 0 .. count - 1 of p, idx = the k-mer's place among the distinct ones --
// whose listings are slots[lo[idx] .. lo[idx + 1]), ascending by slot
template <typename KEYS> struct cp_members { KEYS keys; const uint32_t *lo; const uint32_t *slots; };

// thread r: the run of CP_RUN positions it owns belongs to the last sequence s with srun[s] <= r.  WRITE = false: cnt_s[r] / cnt_e[r] =
// the starts / ends among its positions; WRITE = true: they go out at off_s[r] / off_e[r] as (slot, off[s] + position)
template <bool WRITE, typename KEYS>
__global__ __launch_bounds__(CP_WG) void k_cp_mark(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ off, const uint64_t *__restrict__ srun, uint64_t n_seqs,
                                                   uint64_t n_runs, int k, cp_members<KEYS> M, uint32_t *__restrict__ cnt_s, uint32_t *__restrict__ cnt_e,
                                                   const uint64_t *__restrict__ off_s, const uint64_t *__restrict__ off_e, cp_marks S, cp_marks E) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs) return;
    uint64_t a = 0, b = n_seqs;                            // the last s with srun[s] <= r (sequences without positions take no run: they are skipped)
    while (b - a > 1u) { const uint64_t m = a + (b - a) / 2u; if (srun[m] <= r) a = m; else b = m; }
    const uint64_t o = off[a];
    const uint32_t ni = (uint32_t)(off[a + 1] - o) - (uint32_t)k + 1u, p0 = (uint32_t)(r - srun[a]) * CP_RUN;
    const uint32_t cnt = ni - p0 < CP_RUN ? ni - p0 : CP_RUN;                 // (p0 < ni: the sequence has ceil(ni / CP_RUN) runs)
    const uint32_t first = p0 ? p0 - 1u : 0u, total = (p0 ? 1u : 0u) + cnt + (p0 + cnt < ni ? 1u : 0u);
    uint64_t ws = WRITE ? off_s[r] : 0ull, we = WRITE ? off_e[r] : 0ull;
    uint32_t ns = 0, ne = 0;
    uint32_t plo = 0, phi = 0, clo = 0, chi = 0;          // the listings of the position before (p) and of the current one (c): empty outside the sequence
    // position q with listings [clo, chi), its neighbours' [plo, phi) and [nlo, nhi): all three ascend by slot
    auto decide = [&](uint32_t q, uint32_t nlo, uint32_t nhi) {
        uint32_t jp = plo, jn = nlo;
        for (uint32_t i = clo; i < chi; i++) {
            const uint32_t c = M.slots[i];
            while (jp < phi && M.slots[jp] < c) jp++;
            while (jn < nhi && M.slots[jn] < c) jn++;
            if (!(jp < phi && M.slots[jp] == c)) {
                if (WRITE) { S.slot[ws] = c; S.pos[ws] = o + q; ws++; }
                ns++;
            }
            if (!(jn < nhi && M.slots[jn] == c)) {
                if (WRITE) { E.slot[we] = c; E.pos[we] = o + q; we++; }
                ne++;
            }
        }
    };
    M.keys.each(bases + o + first, total, k, [&](uint32_t i, bool found, uint32_t idx) {
        uint32_t nlo = 0, nhi = 0;
        if (found) { nlo = M.lo[idx]; nhi = M.lo[idx + 1]; }
        const uint32_t q = first + i - 1u;                 // the current position, if there is one yet
        if (i && q >= p0) decide(q, nlo, nhi);
        plo = clo; phi = chi; clo = nlo; chi = nhi;
    });
    if (p0 + cnt == ni) decide(ni - 1u, 0u, 0u);           // the sequence's last position: nothing follows
    if (!WRITE) { cnt_s[r] = ns; cnt_e[r] = ne; }
}
#endif
