// mf_wio.hip -- NO-REFERENCE EXTENSION (32 <= k <= 63): the file level of the wide path.  The reference stops at k = 31, so these formats are
// the project's own: a wide .kmers.bin is headerless, 18-byte big-endian records (int64 high word, int64 low word,
// int16 count; the words of mf_wtable_export), strictly ascending, only counts > b; a wide components.bin is mf_comps_write's layout with every
// member written as two int64 (high, low).  .stat.txt, components-stat.txt, .seq.fasta, .vec, .breadth and the matrix are the k <= 31 files.
// A headerless file cannot say how wide its records are: the loaders validate every record on the device and refuse the file by name.
// (The context's file cache holds k <= 31 objects only: a wide file is always read back from the file, and a table loaded from a file is
// ascending -- what the unitig builder needs for an output that is a function of the files alone.)
#include "mf_common.h"
#include "mf_wide.h"
#include <algorithm>
#include <fcntl.h>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

#define WREC_PER_BLOCK 256
#define WREC_BYTES 18
#define WHIST_BINS 32768
#define WHIST_LDS 1024

static unsigned wio_grid(uint64_t n, unsigned bs = 256) { return (unsigned)std::min<uint64_t>((n + bs - 1) / bs, 0x7FFFFFFFull); }

// ---------------------------------------------------------------------------------------------
// records <-> (hi, lo, count) arrays: 256 records per workgroup staged through LDS so that HBM sees whole dwords (k_records_encode, mf_io.hip);
// 256 x 18 bytes is a multiple of 4: a block's share of the image starts dword-aligned
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WREC_PER_BLOCK) void k_wrecords_encode(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, const uint16_t *__restrict__ cnts,
                                                                     uint64_t n, uint32_t *__restrict__ out) {
    __shared__ __attribute__((aligned(4))) uint8_t st[WREC_PER_BLOCK * WREC_BYTES];
    const uint64_t base = (uint64_t)blockIdx.x * WREC_PER_BLOCK, i = base + threadIdx.x;
    if (i < n) {
        const uint64_t h = hi[i], l = lo[i]; const uint32_t c = cnts[i];
        uint8_t *p = st + threadIdx.x * WREC_BYTES;
#pragma unroll
        for (int b = 0; b < 8; b++) { p[b] = (uint8_t)(h >> (8 * (7 - b))); p[8 + b] = (uint8_t)(l >> (8 * (7 - b))); }
        p[16] = (uint8_t)(c >> 8); p[17] = (uint8_t)c;
    }
    __syncthreads();
    const uint64_t nrec = n - base < WREC_PER_BLOCK ? n - base : WREC_PER_BLOCK;
    const uint32_t nw = ((uint32_t)nrec * WREC_BYTES + 3u) / 4u;                 // (the output buffer is padded to a dword)
    for (uint32_t w = threadIdx.x; w < nw; w += WREC_PER_BLOCK) out[base * WREC_BYTES / 4 + w] = reinterpret_cast<const uint32_t *>(st)[w];
}
__global__ __launch_bounds__(WREC_PER_BLOCK) void k_wrecords_decode(const uint32_t *__restrict__ raw, uint64_t n, uint64_t *__restrict__ hi, uint64_t *__restrict__ lo,
                                                                     uint16_t *__restrict__ cnts) {
    __shared__ __attribute__((aligned(4))) uint8_t st[WREC_PER_BLOCK * WREC_BYTES];
    const uint64_t base = (uint64_t)blockIdx.x * WREC_PER_BLOCK, i = base + threadIdx.x;
    const uint64_t nrec = n - base < WREC_PER_BLOCK ? n - base : WREC_PER_BLOCK;
    const uint32_t nw = ((uint32_t)nrec * WREC_BYTES + 3u) / 4u;                 // (the raw buffer is padded to a dword)
    for (uint32_t w = threadIdx.x; w < nw; w += WREC_PER_BLOCK) reinterpret_cast<uint32_t *>(st)[w] = raw[base * WREC_BYTES / 4 + w];
    __syncthreads();
    if (i < n) {
        const uint8_t *p = st + threadIdx.x * WREC_BYTES;
        uint64_t h = 0, l = 0;
#pragma unroll
        for (int b = 0; b < 8; b++) { h = (h << 8) | p[b]; l = (l << 8) | p[8 + b]; }
        hi[i] = h; lo[i] = l;
        cnts[i] = (uint16_t)(((uint32_t)p[16] << 8) | p[17]);
    }
}
// What makes a file a wide k-mers file of THIS k: every key below 4^k, canonical (not above its reverse complement), strictly above its
// predecessor (read from HBM: the rule holds across workgroups like anywhere else), a positive count.  *bad = min over the bad records of
// (record number << 3 | rule): the first bad record and the first rule it breaks.
#define WBAD_RANGE 0u
#define WBAD_CANON 1u
#define WBAD_ORDER 2u
#define WBAD_COUNT 3u
__global__ __launch_bounds__(256) void k_wrecords_validate(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, const uint16_t *__restrict__ cnts, uint64_t n, int k,
                                                           unsigned long long *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t h = hi[i], l = lo[i];
    const mf_u128 x = ((mf_u128)h << 64) | (mf_u128)l;
    const int hb = 2 * k - 64;                                                   // bits of the high word, 0 .. 62
    uint32_t rule = 0xFFu;
    if ((h >> hb) != 0) rule = WBAD_RANGE;
    else if (x > mf_wrevcomp(x, k)) rule = WBAD_CANON;
    else if (i > 0 && !((((mf_u128)hi[i - 1] << 64) | (mf_u128)lo[i - 1]) < x)) rule = WBAD_ORDER;
    else if ((int16_t)cnts[i] <= 0) rule = WBAD_COUNT;
    if (rule != 0xFFu) atomicMin(bad, ((unsigned long long)i << 3) | rule);
}
// The count histogram of a table piece (.stat.txt): 32768 bins.  Nearly every entry of a read set's table has a small count (errors: 1, the
// genome: its coverage), so a workgroup keeps the bins below 1024 in LDS (4 KB of the CU's 160: no limit on the resident workgroups) --
// ds_add_u32 without a return value, equal counts of a wave are serialised by the LDS alone -- and adds its non-empty bins to the global
// histogram once, at the end: at most 1024 device-scope atomics per workgroup instead of one per entry on a handful of addresses
// (same-address global atomics of a wave are the slow case, MI355X_MICROARCH "contention").  The few larger counts go straight to HBM.
__global__ __launch_bounds__(256) void k_whist(const uint16_t *__restrict__ cnts, uint64_t n, unsigned long long *__restrict__ hist) {
    __shared__ uint32_t bins[WHIST_LDS];
    for (uint32_t b = threadIdx.x; b < WHIST_LDS; b += blockDim.x) bins[b] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = cnts[i];
        if (c < WHIST_LDS) atomicAdd(&bins[c], 1u);
        else atomicAdd(&hist[c < WHIST_BINS ? c : WHIST_BINS - 1], 1ull);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < WHIST_LDS; b += blockDim.x) { const uint32_t v = bins[b]; if (v) atomicAdd(&hist[b], (unsigned long long)v); }
}

// ---------------------------------------------------------------------------------------------
// mf_count_reads_wide: files -> an UNCUT wide table.  The .stat.txt file wants the histogram of what the cut drops and a wide table keeps
// only n_all of it, so the cut waits for mf_wtable_write_kmers; the size limit is the uncut table's (every distinct k-mer of the
// read set in HBM at 18 bytes, < 2^32 occurrences per class of a pass) and mf_count_wide_device reports it.
// ---------------------------------------------------------------------------------------------
extern "C" int mf_count_reads_wide(mf_ctx *ctx, const char *const *files, int nfiles, int k, int min_read_len, mf_wtable **out) {
    mf_range rng_("mf:count_reads_wide(files)");
    if (!ctx || !out || nfiles < 0 || (nfiles && !files)) return mf_set_error("mf_count_reads_wide: NULL argument");
    *out = nullptr;
    if (k < 32 || k > 63) return mf_set_error("mf_count_reads_wide: 32 <= k <= 63 (k <= 31: mf_count_reads)");
    mf_reads *r = nullptr;
    MF_TRY(mf_reads_load(ctx, files, nfiles, &r));
    const void *db = nullptr, *doff = nullptr; uint64_t nr = 0, nb = 0;
    int rc = mf_reads_device_view(r, &db, &doff);
    if (rc == MF_OK) rc = mf_reads_stats(r, &nr, &nb);
    if (rc == MF_OK) rc = mf_count_wide_device(ctx, db, doff, nr, nb, k, min_read_len, out);
    mf_reads_destroy(r);
    return rc;
}

// ---------------------------------------------------------------------------------------------
// mf_wtable_write_kmers
// ---------------------------------------------------------------------------------------------
int mf_wtable_count_hist(const mf_wtable *t, std::vector<uint64_t> &hist) {
    mf_ctx *ctx = t->ctx;
    hipStream_t st = ctx->stream;
    hist.assign(WHIST_BINS, 0);
    mf_buf<unsigned long long> dh; MF_TRY(dh.alloc(ctx, WHIST_BINS));
    MF_HIP(hipMemsetAsync(dh.p, 0, WHIST_BINS * 8, st));
    for (auto &pc : t->pieces) {
        if (!pc->n) continue;
        const unsigned grid = (unsigned)std::min<uint64_t>((pc->n + 256 * 16 - 1) / (256 * 16), (uint64_t)std::max(ctx->n_cu, 1) * 8);
        k_whist<<<grid, 256, 0, st>>>(pc->cnt.p, pc->n, dh.p);
    }
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "");
    MF_HIP(hipMemcpyAsync(hist.data(), dh.p, WHIST_BINS * 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    return MF_OK;
}
extern "C" int mf_wtable_write_kmers(mf_wtable *t, int threshold, const char *kmers_bin, const char *stat_txt, uint64_t *n_good) {
    mf_range rng_("mf:write_kmers_wide(file)");
    if (!t || !kmers_bin) return mf_set_error("mf_wtable_write_kmers: NULL argument");
    mf_ctx *ctx = t->ctx;
    MF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (stat_txt && t->n_all != t->n)
        return mf_set_error("mf_wtable_write_kmers: the table was cut (%llu of %llu k-mers): it has no histogram for '%s'", (unsigned long long)t->n, (unsigned long long)t->n_all, stat_txt);
    MF_TRY(mf_wtable_ensure_ascending(t));                 // (the file is ascending whatever order the count left)
    const int fd = open(kmers_bin, O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return mf_set_error("can't write '%s'", kmers_bin);
    int rc = MF_OK;
    uint64_t written = 0;
    {
        // the records are encoded in HBM a slab at a time (option wide_write_slab, records; 2^25 = 604 MB) and stream down through the staging slots
        const uint64_t SLAB = (uint64_t)std::max<int64_t>(ctx->opt_wide_write_slab, 1);
        mf_buf<uint32_t> enc;
        for (auto &pc : t->pieces) {
            if (rc != MF_OK) break;
            mf_wtable::piece kept; const mf_wtable::piece *src = pc.get();
            if (threshold > t->cut_thr) { rc = mf_wide_compact(ctx, pc->hi.p, pc->lo.p, pc->cnt.p, pc->n, threshold, kept); src = &kept; }
            if (rc != MF_OK || !src->n) continue;
            if (!enc.p && (rc = enc.alloc(ctx, (std::min<uint64_t>(std::max<uint64_t>(t->n, 1), SLAB) * WREC_BYTES + 3) / 4 + 1)) != MF_OK) break;
            for (uint64_t i = 0; i < src->n && rc == MF_OK; i += SLAB) {
                const uint64_t m = std::min(SLAB, src->n - i);
                k_wrecords_encode<<<(unsigned)((m + WREC_PER_BLOCK - 1) / WREC_PER_BLOCK), WREC_PER_BLOCK, 0, st>>>(src->hi.p + i, src->lo.p + i, src->cnt.p + i, m, enc.p);
                rc = mf_device_to_file(ctx, enc.p, m * WREC_BYTES, fd, (off_t)(written * WREC_BYTES), kmers_bin);
                written += m;
            }
        }
    }
    if (close(fd) != 0 && rc == MF_OK) rc = mf_set_error("can't write '%s'", kmers_bin);
    MF_TRY(rc);
    if (stat_txt) {
        std::vector<uint64_t> hist;
        MF_TRY(mf_wtable_count_hist(t, hist));
        FILE *f = fopen(stat_txt, "w");
        if (!f) return mf_set_error("can't write '%s'", stat_txt);
        fprintf(f, "# k-mer frequency\tnumber of such k-mers\n");
        for (size_t v = 0; v < hist.size(); v++) if (hist[v]) fprintf(f, "%zu\t%llu\n", v, (unsigned long long)hist[v]);
        fprintf(f, "\n");
        fclose(f);
    }
    if (n_good) *n_good = written;
    return MF_OK;
}

// ---------------------------------------------------------------------------------------------
// mf_wtable_load_kmers
// ---------------------------------------------------------------------------------------------
// a file's bytes in HBM as they are (the staged upload; one pageable copy where there is no staging memory)
static int upload_whole(mf_ctx *ctx, int fd, size_t n, const char *path, uint8_t *d_dst) {
    int urc = mf_upload_file(ctx, fd, n, d_dst);
    if (urc == 1) {
        std::vector<char> buf(n);
        size_t got = 0;
        while (got < n) { const ssize_t r = pread(fd, buf.data() + got, n - got, (off_t)got); if (r <= 0) break; got += (size_t)r; }
        if (got != n) return mf_set_error("short read on '%s'", path);
        MF_HIP(hipMemcpyAsync(d_dst, buf.data(), n, hipMemcpyHostToDevice, ctx->stream));
        MF_HIP(hipStreamSynchronize(ctx->stream));
        urc = 0;
    }
    return urc;
}
__global__ void k_wio_iota(uint64_t *__restrict__ v, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = i;
}
__global__ void k_wio_gather64(const uint64_t *__restrict__ idx, const uint64_t *__restrict__ src, uint64_t n, uint64_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = src[idx[i]];
}
__global__ void k_wio_gather_pair(const uint64_t *__restrict__ idx, const uint64_t *__restrict__ lo, const uint16_t *__restrict__ cnt, uint64_t n, uint64_t *__restrict__ olo,
                                  uint16_t *__restrict__ ocnt) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const uint64_t j = idx[i]; olo[i] = lo[j]; ocnt[i] = cnt[j]; }
}
__global__ void k_wio_heads(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint64_t n, uint32_t *__restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = (i == 0 || hi[i] != hi[i - 1] || lo[i] != lo[i - 1]) ? 1u : 0u;
}
// the segmented saturating sum: the head of a run of equal k-mers (at most one entry per file) adds the run up
__global__ void k_wio_sum_runs(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, const uint16_t *__restrict__ cnt, const uint32_t *__restrict__ flag,
                               const uint64_t *__restrict__ idx, uint64_t n, uint64_t *__restrict__ ohi, uint64_t *__restrict__ olo, uint16_t *__restrict__ ocnt) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    uint32_t s = cnt[i];
    for (uint64_t j = i + 1; j < n && !flag[j]; j++) { s += cnt[j]; if (s > (uint32_t)MF_MAX_COUNT) s = (uint32_t)MF_MAX_COUNT; }
    const uint64_t o = idx[i];
    ohi[o] = hi[i]; olo[o] = lo[i]; ocnt[o] = (uint16_t)(s > (uint32_t)MF_MAX_COUNT ? (uint32_t)MF_MAX_COUNT : s);
}
// (hi, lo, cnt)[n] in any order -> r: the entries ascending in (hi, lo), the head of every run of equal k-mers flagged, idx = the run an entry
// stands in.  Two stable passes -- the low word, then the high word's 2k - 64 bits -- that carry the entry's index (what mf_wide_merge_runs
// sums up, and the wide join of mf_wjoin.hip reduces)
int mf_wide_sort_runs(mf_ctx *ctx, int k, const uint64_t *hi, const uint64_t *lo, const uint16_t *cnt, uint64_t n, mf_wide_runs &r) {
    hipStream_t st = ctx->stream;
    r.n_runs = 0;
    if (!n) return MF_OK;
    const int hb = 2 * k - 64;
    mf_buf<uint64_t> k0, k1, i0, i1;
    MF_TRY(k0.alloc(ctx, n)); MF_TRY(k1.alloc(ctx, n)); MF_TRY(i0.alloc(ctx, n)); MF_TRY(i1.alloc(ctx, n));
    k_wio_iota<<<wio_grid(n), 256, 0, st>>>(i0.p, n);
    MF_TRY(mf_sort_u64_u64(ctx, lo, i0.p, n, 64, k1.p, i1.p));                             // (lo', idx') in (k1, i1)
    if (hb) {
        k_wio_gather64<<<wio_grid(n), 256, 0, st>>>(i1.p, hi, n, k0.p);                    // hi' in k0
        MF_TRY(mf_sort_u64_u64(ctx, k0.p, i1.p, n, hb, k1.p, i0.p));                       // (hi'', idx'') in (k1, i0)
    } else i0.swap(i1);                                                                    // (k = 32: every high word is 0)
    MF_TRY(r.lo.alloc(ctx, n)); MF_TRY(r.cnt.alloc(ctx, n));
    k_wio_gather_pair<<<wio_grid(n), 256, 0, st>>>(i0.p, lo, cnt, n, r.lo.p, r.cnt.p);
    if (!hb) { MF_HIP(hipMemsetAsync(k1.p, 0, n * 8, st)); }
    r.hi.swap(k1);
    mf_buf<uint64_t> tot;
    MF_TRY(r.flag.alloc(ctx, n)); MF_TRY(r.idx.alloc(ctx, n + 1)); MF_TRY(tot.alloc(ctx, 1));
    k_wio_heads<<<wio_grid(n), 256, 0, st>>>(r.hi.p, r.lo.p, n, r.flag.p);
    MF_TRY(mf_scan<1>(ctx, r.flag.p, r.idx.p, n, tot.p));
    MF_HIP(hipMemcpyAsync(&r.n_runs, tot.p, 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    return MF_OK;
}
// (hi, lo, cnt)[n] in any order -> out: the distinct k-mers ascending, each with the saturating sum of its entries' counts: the saturating sum of
// every run of equal k-mers that mf_wide_sort_runs leaves (mf_wtable_load_kmers over several files; comp2seq's table of all members, mf_wcomp2seq.hip)
int mf_wide_merge_runs(mf_ctx *ctx, int k, const uint64_t *hi, const uint64_t *lo, const uint16_t *cnt, uint64_t n, mf_wtable::piece &out) {
    hipStream_t st = ctx->stream;
    out.n = 0;
    if (!n) return MF_OK;
    mf_wide_runs r;
    MF_TRY(mf_wide_sort_runs(ctx, k, hi, lo, cnt, n, r));
    const uint64_t nd = r.n_runs;
    MF_TRY(out.hi.alloc(ctx, nd)); MF_TRY(out.lo.alloc(ctx, nd)); MF_TRY(out.cnt.alloc(ctx, nd));
    k_wio_sum_runs<<<wio_grid(n), 256, 0, st>>>(r.hi.p, r.lo.p, r.cnt.p, r.flag.p, r.idx.p, n, out.hi.p, out.lo.p, out.cnt.p);
    MF_HIP(hipStreamSynchronize(st));
    out.n = nd;
    return MF_OK;
}
static const char *wbad_text(uint32_t rule) {
    switch (rule) {
        case WBAD_RANGE: return "the k-mer is not below 4^k";
        case WBAD_CANON: return "the k-mer is above its reverse complement (not canonical)";
        case WBAD_ORDER: return "the k-mer is not above its predecessor (the file must be strictly ascending)";
        default: return "the count is not positive";
    }
}
extern "C" int mf_wtable_load_kmers(mf_ctx *ctx, const char *const *files, int nfiles, int freq_threshold, int k, mf_wtable **out) {
    mf_range rng_("mf:load_kmers_wide(file)");
    if (!ctx || !out || nfiles < 0 || (nfiles && !files)) return mf_set_error("mf_wtable_load_kmers: NULL argument");
    *out = nullptr;
    if (k < 32 || k > 63) return mf_set_error("mf_wtable_load_kmers: 32 <= k <= 63 (k <= 31: mf_table_load_kmers)");
    MF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<int> fds((size_t)nfiles, -1);
    std::vector<uint64_t> recs((size_t)nfiles, 0);
    struct closer { std::vector<int> &f; ~closer() { for (int d : f) if (d >= 0) close(d); } } closer_{fds};
    uint64_t total = 0;
    for (int i = 0; i < nfiles; i++) {
        fds[(size_t)i] = open(files[i], O_RDONLY);
        struct stat stf;
        if (fds[(size_t)i] < 0 || fstat(fds[(size_t)i], &stf) != 0) return mf_set_error("can't open '%s'", files[i]);
        if ((uint64_t)stf.st_size % WREC_BYTES)
            return mf_set_error("Can't load wide k-mers file '%s': size %llu is not a multiple of the 18-byte record (k = %d)", files[i], (unsigned long long)stf.st_size, k);
        recs[(size_t)i] = (uint64_t)stf.st_size / WREC_BYTES;
        total += recs[(size_t)i];
    }
    auto piece = std::make_unique<mf_wtable::piece>();
    MF_TRY(piece->hi.alloc(ctx, total)); MF_TRY(piece->lo.alloc(ctx, total)); MF_TRY(piece->cnt.alloc(ctx, total));
    mf_buf<unsigned long long> bad; MF_TRY(bad.alloc(ctx, 1));
    uint64_t at = 0;
    for (int i = 0; i < nfiles; i++) {
        const uint64_t m = recs[(size_t)i];
        if (!m) continue;
        mf_buf<uint32_t> raw; MF_TRY(raw.alloc(ctx, (m * WREC_BYTES + 3) / 4 + 1));
        MF_TRY(upload_whole(ctx, fds[(size_t)i], m * WREC_BYTES, files[i], reinterpret_cast<uint8_t *>(raw.p)));
        MF_HIP(hipMemsetAsync(bad.p, 0xFF, 8, st));
        k_wrecords_decode<<<(unsigned)((m + WREC_PER_BLOCK - 1) / WREC_PER_BLOCK), WREC_PER_BLOCK, 0, st>>>(raw.p, m, piece->hi.p + at, piece->lo.p + at, piece->cnt.p + at);
        k_wrecords_validate<<<wio_grid(m), 256, 0, st>>>(piece->hi.p + at, piece->lo.p + at, piece->cnt.p + at, m, k, bad.p);
        unsigned long long b = 0;
        MF_HIP(hipMemcpyAsync(&b, bad.p, 8, hipMemcpyDeviceToHost, st));
        MF_HIP(hipStreamSynchronize(st));
        if (b != ~0ull)
            return mf_set_error("Can't load wide k-mers file '%s': record %llu: %s (k = %d; is this a file of another k?)", files[i], b >> 3, wbad_text((uint32_t)(b & 7u)), k);
        at += m;
    }
    piece->n = total;
    // records with count <= freq_threshold are dropped, file by file, before anything is summed (IOUtils.loadKmers' rule carried over)
    if (freq_threshold >= 1 && total) {
        auto kept = std::make_unique<mf_wtable::piece>();
        MF_TRY(mf_wide_compact(ctx, piece->hi.p, piece->lo.p, piece->cnt.p, total, freq_threshold, *kept));
        piece = std::move(kept);
    }
    // several files (seq-builder): ascending order over all of them, the counts of equal k-mers added up
    if (nfiles > 1 && piece->n) {
        auto sum = std::make_unique<mf_wtable::piece>();
        MF_TRY(mf_wide_merge_runs(ctx, k, piece->hi.p, piece->lo.p, piece->cnt.p, piece->n, *sum));
        piece = std::move(sum);
    }
    auto t = std::make_unique<mf_wtable>();
    t->ctx = ctx; t->k = k; t->n = piece->n; t->n_all = piece->n; t->n_occ = 0;
    t->cut_thr = std::max(0, freq_threshold);                // (every record of a valid file has a positive count)
    t->ascending = true;
    if (piece->n) t->pieces.push_back(std::move(piece));
    *out = t.release();
    return MF_OK;
}

// ---------------------------------------------------------------------------------------------
// wide components.bin: int32 number of components; per component int32 size, int64 weight, size x (int64 high word, int64 low word); big-endian
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_wcomps_encode(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, const uint64_t *__restrict__ koff,
                                                       const uint64_t *__restrict__ foff, const long long *__restrict__ weights, uint32_t n_comp, uint32_t *__restrict__ raw) {
    if (blockIdx.x == 0 && threadIdx.x == 0) raw[0] = __builtin_bswap32(n_comp);
    for (uint32_t c = blockIdx.x; c < n_comp; c += gridDim.x) {
        const uint64_t w0 = foff[c] / 4, k0 = koff[c], sz = koff[c + 1] - k0;
        if (threadIdx.x == 0) {
            const unsigned long long w = (unsigned long long)weights[c];
            raw[w0] = __builtin_bswap32((uint32_t)sz); raw[w0 + 1] = __builtin_bswap32((uint32_t)(w >> 32)); raw[w0 + 2] = __builtin_bswap32((uint32_t)w);
        }
        for (uint64_t j = threadIdx.x; j < sz; j += blockDim.x) {
            const uint64_t h = hi[k0 + j], l = lo[k0 + j];
            uint32_t *o = raw + w0 + 3 + 4 * j;
            o[0] = __builtin_bswap32((uint32_t)(h >> 32)); o[1] = __builtin_bswap32((uint32_t)h);
            o[2] = __builtin_bswap32((uint32_t)(l >> 32)); o[3] = __builtin_bswap32((uint32_t)l);
        }
    }
}
// ... and back; *bad = min over the bad members of (member number << 3 | rule): not below 4^k, or not above its predecessor inside the component
__global__ __launch_bounds__(256) void k_wcomps_decode(const uint32_t *__restrict__ raw, const uint64_t *__restrict__ foff, const uint64_t *__restrict__ koff, uint32_t n_comp,
                                                       int k, uint64_t *__restrict__ hi, uint64_t *__restrict__ lo, uint32_t *__restrict__ comp, unsigned long long *__restrict__ bad) {
    const int hb = 2 * k - 64;
    for (uint32_t c = blockIdx.x; c < n_comp; c += gridDim.x) {
        const uint64_t w0 = foff[c] / 4 + 3, k0 = koff[c], sz = koff[c + 1] - k0;
        for (uint64_t j = threadIdx.x; j < sz; j += blockDim.x) {
            const uint32_t *p = raw + w0 + 4 * j;
            const uint64_t h = ((uint64_t)__builtin_bswap32(p[0]) << 32) | __builtin_bswap32(p[1]), l = ((uint64_t)__builtin_bswap32(p[2]) << 32) | __builtin_bswap32(p[3]);
            hi[k0 + j] = h; lo[k0 + j] = l; comp[k0 + j] = c;
            uint32_t rule = 0xFFu;
            if ((h >> hb) != 0) rule = WBAD_RANGE;
            else if (j > 0) {
                const uint64_t ph = ((uint64_t)__builtin_bswap32(p[-4]) << 32) | __builtin_bswap32(p[-3]), pl = ((uint64_t)__builtin_bswap32(p[-2]) << 32) | __builtin_bswap32(p[-1]);
                if (!(ph < h || (ph == h && pl < l))) rule = WBAD_ORDER;
            }
            if (rule != 0xFFu) atomicMin(bad, ((unsigned long long)(k0 + j) << 3) | rule);
        }
    }
}
extern "C" int mf_wcomps_write(const mf_wcomps *c, const char *components_bin, const char *stat_txt) {
    mf_range rng_("mf:write_components_wide(file)");
    if (!c || !components_bin) return mf_set_error("mf_wcomps_write: NULL argument");
    mf_ctx *ctx = c->ctx;
    if (c->n >= 0x7FFFFFFFull) return mf_set_error("components: too many components for the file format");
    MF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t n = c->n, nk = c->n_kmers;
    std::vector<uint64_t> koff(n + 1, 0), foff(n + 1, 0);
    foff[0] = 4;
    for (uint64_t i = 0; i < n; i++) {
        if (c->sizes[i] >= 0x7FFFFFFFull) return mf_set_error("components: a component too large for the file format");
        koff[i + 1] = koff[i] + c->sizes[i]; foff[i + 1] = foff[i] + 12 + 16 * c->sizes[i];
    }
    if (koff[n] != nk) return mf_set_error("components: sizes do not add up to the member list");
    const uint64_t total = foff[n];
    mf_buf<uint32_t> raw; MF_TRY(raw.alloc(ctx, total / 4 + 1));
    if (n) {
        mf_buf<uint64_t> dko, dfo; mf_buf<long long> dw;
        MF_TRY(dko.alloc(ctx, n + 1)); MF_TRY(dfo.alloc(ctx, n + 1)); MF_TRY(dw.alloc(ctx, n));
        MF_HIP(hipMemcpyAsync(dko.p, koff.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
        MF_HIP(hipMemcpyAsync(dfo.p, foff.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
        MF_HIP(hipMemcpyAsync(dw.p, c->weights.data(), n * 8, hipMemcpyHostToDevice, st));
        k_wcomps_encode<<<(unsigned)std::min<uint64_t>(n, 65535), 256, 0, st>>>(c->hi.p, c->lo.p, dko.p, dfo.p, dw.p, (uint32_t)n, raw.p);
        MF_HIP(hipStreamSynchronize(st));
    } else {
        const uint32_t zero = 0;
        MF_HIP(hipMemcpyAsync(raw.p, &zero, 4, hipMemcpyHostToDevice, st));
        MF_HIP(hipStreamSynchronize(st));
    }
    const int fd = open(components_bin, O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return mf_set_error("can't write '%s'", components_bin);
    int rc = mf_device_to_file(ctx, raw.p, total, fd, 0, components_bin);
    if (close(fd) != 0 && rc == MF_OK) rc = mf_set_error("can't write '%s'", components_bin);
    MF_TRY(rc);
    if (stat_txt) {
        FILE *f = fopen(stat_txt, "w");
        if (!f) return mf_set_error("can't write '%s'", stat_txt);
        fprintf(f, "# component.no\tcomponent.size\tcomponent.weight\tusedFreqThreshold\n");
        for (uint64_t i = 0; i < n; i++)
            fprintf(f, "%llu\t%llu\t%lld\t%d\n", (unsigned long long)(i + 1), (unsigned long long)c->sizes[i], (long long)c->weights[i], c->thr[i]);
        fclose(f);
    }
    return MF_OK;
}
extern "C" int mf_wcomps_load(mf_ctx *ctx, const char *components_bin, int k, mf_wcomps **out) {
    mf_range rng_("mf:load_components_wide(file)");
    if (!ctx || !components_bin || !out) return mf_set_error("mf_wcomps_load: NULL argument");
    *out = nullptr;
    if (k < 32 || k > 63) return mf_set_error("mf_wcomps_load: 32 <= k <= 63 (k <= 31: mf_comps_load)");
    const int fd = open(components_bin, O_RDONLY);
    struct stat stc;
    if (fd < 0 || fstat(fd, &stc) != 0) { if (fd >= 0) close(fd); return mf_set_error("Can't load components: file not found (%s)", components_bin); }
    struct fd_closer { int f; ~fd_closer() { close(f); } } fdc{fd};
    const size_t n = (size_t)stc.st_size;
    if (n < 4 || n % 4) return mf_set_error("Can't load wide components file '%s': %zu bytes is not a components file", components_bin, n);
    // the host walks the component headers (one every 12 + 16 x size bytes) through a mapping of the file; the bytes go to HBM as they are
    void *map = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
    if (map == MAP_FAILED) return mf_set_error("Can't load components: can't map '%s'", components_bin);
    struct unmapper { void *m; size_t n; ~unmapper() { munmap(m, n); } } um{map, n};
    const uint8_t *p = (const uint8_t *)map;
    auto be32 = [&](size_t o) { return ((uint32_t)p[o] << 24) | ((uint32_t)p[o + 1] << 16) | ((uint32_t)p[o + 2] << 8) | (uint32_t)p[o + 3]; };
    const int32_t cnt = (int32_t)be32(0);
    if (cnt < 0) return mf_set_error("Can't load wide components file '%s': negative number of components", components_bin);
    auto C = std::make_unique<mf_wcomps>();
    C->ctx = ctx; C->k = k; C->n = (uint64_t)cnt;
    C->sizes.reserve((size_t)cnt); C->weights.reserve((size_t)cnt);
    std::vector<uint64_t> foff((size_t)cnt + 1, 0), koff((size_t)cnt + 1, 0);
    size_t at = 4;
    for (int32_t i = 0; i < cnt; i++) {
        if (at + 12 > n) return mf_set_error("Can't load wide components file '%s': the file ends inside the header of component %d (k = %d; is this a file of another k?)", components_bin, i + 1, k);
        const int32_t sz = (int32_t)be32(at);
        const uint64_t w = ((uint64_t)be32(at + 4) << 32) | be32(at + 8);
        if (sz < 0 || (uint64_t)sz * 16 > n - at - 12)
            return mf_set_error("Can't load wide components file '%s': component %d has size %d, more than the file holds (k = %d; is this a file of another k?)", components_bin, i + 1, sz, k);
        C->sizes.push_back((uint64_t)sz); C->weights.push_back((int64_t)w);
        foff[(size_t)i] = at; koff[(size_t)i + 1] = koff[(size_t)i] + (uint64_t)sz;
        at += 12 + (size_t)sz * 16;
    }
    foff[(size_t)cnt] = at;
    if (at != n) return mf_set_error("Can't load wide components file '%s': %zu bytes after the last component (k = %d; is this a file of another k?)", components_bin, n - at, k);
    C->thr.assign((size_t)cnt, 0);
    const uint64_t nk = koff[(size_t)cnt];
    if (nk >= 0xFFFFFFFFull) return mf_set_error("components: too many k-mers");
    C->n_kmers = nk;
    MF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    MF_TRY(C->hi.alloc(ctx, nk)); MF_TRY(C->lo.alloc(ctx, nk)); MF_TRY(C->comp.alloc(ctx, nk));
    if (nk) {
        mf_buf<uint32_t> raw; MF_TRY(raw.alloc(ctx, n / 4 + 2));
        mf_buf<uint64_t> dfo, dko; MF_TRY(dfo.alloc(ctx, (size_t)cnt + 1)); MF_TRY(dko.alloc(ctx, (size_t)cnt + 1));
        mf_buf<unsigned long long> bad; MF_TRY(bad.alloc(ctx, 1));
        MF_TRY(upload_whole(ctx, fd, n, components_bin, reinterpret_cast<uint8_t *>(raw.p)));
        MF_HIP(hipMemcpyAsync(dfo.p, foff.data(), ((size_t)cnt + 1) * 8, hipMemcpyHostToDevice, st));
        MF_HIP(hipMemcpyAsync(dko.p, koff.data(), ((size_t)cnt + 1) * 8, hipMemcpyHostToDevice, st));
        MF_HIP(hipMemsetAsync(bad.p, 0xFF, 8, st));
        k_wcomps_decode<<<(unsigned)std::min<uint64_t>((uint64_t)cnt, 65535), 256, 0, st>>>(raw.p, dfo.p, dko.p, (uint32_t)cnt, k, C->hi.p, C->lo.p, C->comp.p, bad.p);
        unsigned long long b = 0;
        MF_HIP(hipMemcpyAsync(&b, bad.p, 8, hipMemcpyDeviceToHost, st));
        MF_HIP(hipStreamSynchronize(st));
        if (b != ~0ull)
            return mf_set_error("Can't load wide components file '%s': member %llu: %s (k = %d; is this a file of another k?)", components_bin, b >> 3,
                                (b & 7u) == WBAD_RANGE ? "the k-mer is not below 4^k" : "the k-mer is not above its predecessor inside the component", k);
    }
    *out = C.release();
    return MF_OK;
}

// (mf_features_wide and the other file forms of the wide features: mf_wfeatures.hip)
