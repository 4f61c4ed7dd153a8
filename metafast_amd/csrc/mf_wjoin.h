// mf_wjoin.h -- NO-REFERENCE EXTENSION (32 <= k <= 63): the join core of the wide cohort tools (kernels and host: mf_wjoin.hip).
// The k <= 31 join (mf_join.h) claims a slot of an open-addressed table with a 64-bit atomicCAS on the key.  A 2k-bit key has two words and the
// device no 128-bit compare-and-swap, so the wide join claims nothing: per slice of the KEY RANGE the samples' entries are gathered into flat arrays,
// ordered by the two stable radix passes of mf_wide_sort_runs, and every run of equal k-mers (at most one entry per sample) is reduced by one thread.
#pragma once
#include "mf_common.h"
#include "mf_wide.h"
#include <functional>

// a sample while a pass reads it: a caller's table (borrowed) or one loaded from its file (owned); the stream is drained before an owned one goes
struct mf_wjoin_sample {
    mf_ctx *ctx; mf_wtable *t = nullptr; bool own = false;
    explicit mf_wjoin_sample(mf_ctx *c) : ctx(c) {}
    mf_wjoin_sample(const mf_wjoin_sample &) = delete;
    mf_wjoin_sample &operator=(const mf_wjoin_sample &) = delete;
    ~mf_wjoin_sample();
};
using mf_wjoin_get = std::function<int(int j, mf_wjoin_sample &)>;

// what a slice leaves: its distinct k-mers ascending, cnt = the samples that hold one, sum = the sum of their counts mod 2^16 (with weights: the sum of
// the weights of the samples that hold it), knocked = 0.  With groups (mf_wjoin_slice_union's `group`): grp = the samples of group 0, 1 and 2 that
// hold it, n0 | n1 << MF_WJOIN_GROUP_BITS | n2 << 2 * MF_WJOIN_GROUP_BITS (the presence word of the narrow three-group join, MF_STATS3_BITS of
// mf_stats.h), and sum is not filled; without groups grp stays empty
#define MF_WJOIN_GROUP_BITS 10
#define MF_WJOIN_GROUP_MAX 1023        // samples of one group: what a field of the word holds
struct mf_wjoin_union { mf_buf<uint64_t> hi, lo; mf_buf<uint16_t> cnt, sum; mf_buf<uint8_t> knocked; mf_buf<uint32_t> grp; uint64_t n = 0; };

// S slices of the key range and the room (entries) of a slice's gather buffer for `total` entries in all samples: option stats_slices forces S
int mf_wjoin_plan(mf_ctx *ctx, uint64_t total, uint32_t *S, uint64_t *cap);
// slice s of S: every entry with count > b of the n_in samples -> u.  A slice that holds more than cap entries is an error (raise stats_slices).
// weight (n_in values on the host, or NULL): sample j's entries bring weight[j] in place of their counts
// group (n_in ids in 0 ... 2 on the host, or NULL; not together with weight): sample j's entries bring group[j], and the one reduce pass counts a
// run's entries by group into u.grp -- still one gather, one sort and one reduce per slice, each sample read once.  More than MF_WJOIN_GROUP_MAX
// samples in a group, or an id above 2, is an error.
int mf_wjoin_slice_union(mf_ctx *ctx, int k, const mf_wjoin_get &get, int n_in, int b, uint32_t S, uint32_t s, uint64_t cap, mf_wjoin_union &u,
                         const uint16_t *weight = nullptr, const uint8_t *group = nullptr);
// every entry with count > b of sample t that u holds sets that k-mer's knocked byte
int mf_wjoin_knock(mf_ctx *ctx, const mf_wtable *t, int b, mf_wjoin_union &u);
// the entries with sel > thr of (hi, lo, val, sel)[n], order kept -> (ohi, olo, oval[, osel])[*m]; osel may be NULL
int mf_wjoin_select(mf_ctx *ctx, const uint64_t *hi, const uint64_t *lo, const uint16_t *val, const uint16_t *sel, uint64_t n, int thr, mf_buf<uint64_t> &ohi,
                    mf_buf<uint64_t> &olo, mf_buf<uint16_t> &oval, mf_buf<uint16_t> *osel, uint64_t *m);
// (hi, lo, cnt)[n] ascending, every count > cut -> a one-piece table; the arrays move into it
int mf_wjoin_table(mf_ctx *ctx, int k, int cut, mf_buf<uint64_t> &hi, mf_buf<uint64_t> &lo, mf_buf<uint16_t> &cnt, uint64_t n, mf_wtable **out);
// the k of a list of tables, every one checked: NULL, another context, another k.  *k = 0: no table so far; total may be NULL
int mf_wjoin_tables_check(mf_ctx *ctx, mf_wtable *const *t, int n, const char *what, int *k, uint64_t *total);
// the records (18 bytes each) of a list of wide .kmers.bin files, by their sizes
int mf_wjoin_file_records(const char *const *files, int n, uint64_t *total);

#ifdef __HIPCC__
// The slice of a k-mer: the leading 24 bits of its 2k scaled to [0, S) -- monotone in the k-mer, so a slice is a range of keys and the slices'
// ascending results, one after the other, are ascending.  hb = 2k - 64, the bits of the high word.
__device__ __forceinline__ uint32_t mf_wjoin_slice(uint64_t hi, uint64_t lo, int hb, uint32_t S) {
    const uint64_t top = hb >= 24 ? hi >> (hb - 24) : ((hi << (24 - hb)) | (lo >> (40 + hb)));
    return (uint32_t)(((top & 0xFFFFFFull) * S) >> 24);
}
#endif
