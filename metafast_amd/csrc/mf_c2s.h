// mf_c2s.h -- what comp2seq (mf_comp2seq.hip) shares with comp2graph (mf_comp2graph.hip): the rows (component, canonical k-mer) of all
// components, the pair index over them and the per-row flags of k_c2s_flags.  The kernels stay in mf_comp2seq.hip; here are the probe
// every user of the pair index needs and the host entry points.
#pragma once
#include <string>
#include <vector>
#include "mf_common.h"
#include "mf_join.h"
#include "mf_unitig.h"

#define C2S_NONE 0xFFFFFFFFu
#define C2S_CODE_NONE 4u          // the codes of mf_unitig.hip's info byte
#define C2S_CODE_MANY 5u

static inline unsigned c2s_grid(uint64_t n) { return (unsigned)((n + 255) / 256); }

// rows sorted by (component, k-mer): row = (component, canonical k-mer, multiplicity inside the component)
struct c2s_rows { mf_buf<uint64_t> key; mf_buf<uint32_t> comp; mf_buf<uint16_t> cnt; uint64_t n = 0; };

#ifdef __HIPCC__
// ---- the pair index: slot = {k-mer, row | component << 32} (mf_uslot: cnt = row, row = component); empty = MF_EMPTY in the key word
__device__ __forceinline__ uint64_t c2s_hash(uint64_t key, uint32_t comp) { return mf_hash64(key ^ ((uint64_t)comp * 0x9E3779B97F4A7C15ULL)); }
__device__ __forceinline__ bool c2s_find(const mf_uslot *__restrict__ slots, uint64_t mask, uint64_t key, uint32_t comp, uint32_t *row) {
    uint64_t p = c2s_hash(key, comp) & mask;
    for (uint64_t probe = 0; probe <= mask; probe++) {
        const ulonglong2 raw = *reinterpret_cast<const ulonglong2 *>(&slots[p]);
        if (raw.x == key && (uint32_t)(raw.y >> 32) == comp) { *row = (uint32_t)raw.y; return true; }
        if (raw.x == MF_EMPTY) return false;
        p = (p + 1) & mask;
    }
    return false;
}
#endif

int c2s_check_k(int k);
// the rows of all components, built from the member lists (d_kmers / d_comp)
int c2s_build_rows(mf_ctx *ctx, const mf_comps *c, int k, c2s_rows &R);
// the pair index of the rows (capacity *cap, a power of two); k_c2s_flags over them into A.info / A.ridx / A.lidx / A.pal
int c2s_pair_index(mf_ctx *ctx, const c2s_rows &R, int k, mf_buf<mf_uslot> &slots, uint64_t *cap);
int c2s_flags_launch(mf_ctx *ctx, const mf_uslot *slots, uint64_t cap, const c2s_rows &R, const ut_arrays &A);
// the file form's helpers, shared with the wide tool (mf_wcomp2seq.hip): mkdir -p, a whole file written at once, and Sequence.printSequences as
// mf_seqs_write_fasta writes it for the sequences [lo, hi) numbered from 1
int c2s_mkdirs(const std::string &p);
int c2s_write_file(const std::string &path, const std::string &data);
void c2s_seq_text(const std::vector<uint8_t> &b, const std::vector<uint64_t> &o, const std::vector<int32_t> &a, const std::vector<int32_t> &mn,
                  const std::vector<int32_t> &mx, uint64_t lo, uint64_t hi, std::string &out);
