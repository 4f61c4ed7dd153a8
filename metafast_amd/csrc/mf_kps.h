// mf_kps.h -- what the two kmers-per-sample tools share: the result handle, the checks, and the row text, which does not depend on the key
// width (mf_kps.hip: k <= 31 on the hash join; mf_wkps.hip: 32 <= k <= 63 on the wide join, DESIGN.md sections 7f and 7m).
#pragma once
#include "mf_common.h"
#include <algorithm>
#include <cstdio>
#include <string>

#define MF_KPS_MAX_N 32767                // n(x) is a Java short
#define MF_KPS_MAX_WIDTH 6                // "\t" + the five digits of a uint16

// M selected k-mers x N samples.  k <= 31: keys; a wide result (wide_k = its k, 32 ... 63): hi, lo
struct mf_kps {
    mf_ctx *ctx = nullptr;
    int n_samples = 0;
    uint64_t m = 0;
    mf_buf<uint64_t> keys; mf_buf<uint16_t> ns, mat;
    int wide_k = 0;
    mf_buf<uint64_t> hi, lo;
};

// KmersPerSampleCounter.java:101, in Java int arithmetic: the product wraps, the division truncates toward zero
static inline int kps_thresh(int N, int percent) { return (int)(int32_t)((uint32_t)N * (uint32_t)percent) / 100; }
static inline unsigned kps_grid(uint64_t m) { return (unsigned)std::max<uint64_t>(1, (m + 255) / 256); }      // (m < 2^32)

// the N x M x 2 bytes of the matrix have to fit what is free now (the arena's idle regions are free to it; option kps_matrix_bytes)
int kps_matrix_fits(mf_ctx *ctx, int n, uint64_t m);

// the text of one row: buffers kept over the rows of a run
struct kps_text {
    mf_buf<uint32_t> w; mf_buf<uint64_t> off, total; mf_buf<uint8_t> out;
    int alloc(mf_ctx *ctx, uint64_t m) {
        MF_TRY(w.alloc(ctx, m)); MF_TRY(off.alloc(ctx, m + 1)); MF_TRY(total.alloc(ctx, 1));
        return out.alloc(ctx, m * MF_KPS_MAX_WIDTH);
    }
};
// row[0 .. m) -> tx.out[0 .. *bytes) = "\t" + decimal per value
int kps_format(mf_ctx *ctx, const uint16_t *row, uint64_t m, kps_text &tx, uint64_t *bytes);
// device bytes -> the file, through two halves of the context's staging memory
int kps_write(mf_ctx *ctx, const uint8_t *d_src, uint64_t bytes, FILE *f, const char *path);
// File.getName().replace(".kmers.bin", "")
std::string kps_row_name(const char *path);
// the first line of a wide result: "\t" + the k bases of (hi, lo)[i] at out[i * (k + 1)] (mf_wkps.hip)
int mf_wkps_header(mf_ctx *ctx, const uint64_t *hi, const uint64_t *lo, uint64_t m, int k, mf_buf<uint8_t> &out, uint64_t *bytes);
