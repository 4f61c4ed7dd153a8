// mf_comp2seq.hip -- comp2seq: the contigs of every component of a components.bin in ONE segmented unitig build.
//
// Replaces ComponentsToSequences (src/tools/ComponentsToSequences.java:41-76): bin2fasta -cf ... [--split], kmer-counter-many -b 0 on the
// FASTA files it wrote, seq-builder-many -b 0 -l k on their .kmers.bin files -- with --split a count -> index -> unitig run per component,
// a few dozen launches each over a few thousand keys.  Here all components go through the builder together:
//
//   rows          (component, canonical k-mer, multiplicity inside the component) of every member, sorted by (component, k-mer): two
//                 stable radix sorts of the member list, the runs of equal pairs counted (capped as the counter caps)
//   pair index    open-addressed, 16-byte slots {k-mer, component << 32 | row}, hashed on the k-mer's mix folded with the component:
//                 a k-mer that is a member of several components has a slot (and a row) in each
//   k_c2s_flags   U1 of mf_unitig.hip restricted to a component: a neighbour exists only if (neighbour, this row's component) is in the
//                 pair index
//   U2 .. U5      mf_ut_build, unchanged: it works on row ids; the paths come back with the component of their start row and the
//                 ordered export groups them by it
//
// Without --split the route is one ordinary table of all members (mf_table_from_device_pairs) and mf_build_unitigs_device.
#include "mf_c2s.h"
#include "mf_parse.h"
#include <errno.h>

int mf_table_from_device_pairs(mf_ctx *ctx, const uint64_t *d_keys, const uint16_t *d_vals, uint64_t n, int k, mf_table **out);

// members -> canonical k-mers; a member that does not fit 2k bits raises bit 0 of *flags
__global__ __launch_bounds__(256) void k_c2s_canon(const uint64_t *__restrict__ kmers, uint64_t n, int k, uint64_t *__restrict__ out, uint16_t *__restrict__ ones,
                                                   unsigned int *__restrict__ flags) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t x = kmers[i];
    if (x >> (2 * k)) { atomicOr(flags, 1u); x &= (1ull << (2 * k)) - 1ull; }
    out[i] = mf_canon(x, k);
    if (ones) ones[i] = 1;
}
// sorted (component, k-mer) pairs: head[i] = 1 where a run of equal pairs starts
__global__ __launch_bounds__(256) void k_c2s_heads(const uint32_t *__restrict__ comp, const uint64_t *__restrict__ key, uint64_t n, uint32_t *__restrict__ head) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || comp[i] != comp[i - 1] || key[i] != key[i - 1]) ? 1u : 0u;
}
// row r = the r-th run: its pair and where it starts
__global__ __launch_bounds__(256) void k_c2s_rows(const uint32_t *__restrict__ comp, const uint64_t *__restrict__ key, const uint32_t *__restrict__ head,
                                                  const uint64_t *__restrict__ idx, uint64_t n, uint64_t *__restrict__ rkey, uint32_t *__restrict__ rcomp,
                                                  uint32_t *__restrict__ rstart) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !head[i]) return;
    const uint64_t r = idx[i];
    rkey[r] = key[i]; rcomp[r] = comp[i]; rstart[r] = (uint32_t)i;
}
__global__ __launch_bounds__(256) void k_c2s_counts(const uint32_t *__restrict__ rstart, uint64_t n_rows, uint64_t n, uint16_t *__restrict__ rcnt) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const uint64_t len = (r + 1 < n_rows ? (uint64_t)rstart[r + 1] : n) - (uint64_t)rstart[r];
    rcnt[r] = (uint16_t)(len > (uint64_t)MF_MAX_COUNT ? (uint64_t)MF_MAX_COUNT : len);
}

// ---- the pair index: slot = {k-mer, row | component << 32} (mf_uslot: cnt = row, row = component); empty = MF_EMPTY in the key word
// the rows' pairs are all different: a row takes the first empty slot of its probe sequence, nobody has to be recognised
__global__ __launch_bounds__(256) void k_c2s_index_insert(mf_uslot *__restrict__ slots, uint64_t mask, const uint64_t *__restrict__ rkey, const uint32_t *__restrict__ rcomp,
                                                          uint64_t n_rows, unsigned int *__restrict__ flags) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const uint64_t key = rkey[r];
    const uint32_t comp = rcomp[r];
    uint64_t p = c2s_hash(key, comp) & mask;
    for (uint64_t probe = 0; probe <= mask; probe++) {
        if (atomicCAS(reinterpret_cast<unsigned long long *>(&slots[p].key), (unsigned long long)MF_EMPTY, (unsigned long long)key) == (unsigned long long)MF_EMPTY) {
            slots[p].cnt = (uint32_t)r; slots[p].row = comp;
            return;
        }
        p = (p + 1) & mask;
    }
    atomicOr(flags, 2u);                                     // (full: never with the capacity the host picks)
}
// U1 restricted to a component: what k_ut_flags (mf_unitig.hip) does per table entry, per ROW -- getRightNucleotide / getLeftNucleotide
// (HashMapOperations.java:13-47) in the map of the row's own component
__global__ __launch_bounds__(256) void k_c2s_flags(const mf_uslot *__restrict__ slots, uint64_t mask, const uint32_t *__restrict__ rcomp, ut_arrays A) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const int k = A.k;
    const uint64_t kmask = (1ull << (2 * k)) - 1;
    const uint64_t x = A.gk[i];
    const uint32_t comp = rcomp[i];
    uint32_t rcode = C2S_CODE_NONE, lcode = C2S_CODE_NONE, ridx = C2S_NONE, lidx = C2S_NONE, ror = 0, lor = 0;
#pragma unroll
    for (uint32_t nuc = 0; nuc < 4; nuc++) {
        const uint64_t y = ((x << 2) | nuc) & kmask;                 // ShortKmer.shiftRight
        const uint64_t ry = mf_revcomp(y, k);
        const uint64_t c = y < ry ? y : ry;
        uint32_t idx;
        if (c2s_find(slots, mask, c, comp, &idx)) {
            if (rcode == C2S_CODE_NONE) { rcode = nuc; ridx = idx; ror = (c != y); }
            else rcode = C2S_CODE_MANY;
        }
    }
#pragma unroll
    for (uint32_t nuc = 0; nuc < 4; nuc++) {
        const uint64_t y = (x >> 2) | ((uint64_t)nuc << (2 * k - 2));   // ShortKmer.shiftLeft
        const uint64_t ry = mf_revcomp(y, k);
        const uint64_t c = y < ry ? y : ry;
        uint32_t idx;
        if (c2s_find(slots, mask, c, comp, &idx)) {
            if (lcode == C2S_CODE_NONE) { lcode = nuc; lidx = idx; lor = (c != y); }
            else lcode = C2S_CODE_MANY;
        }
    }
    A.info[i] = (uint8_t)(rcode | (lcode << 3) | (ror << 6) | (lor << 7));
    if (A.pal) A.pal[i] = (uint8_t)(mf_revcomp(x, k) == x);
    A.ridx[i] = ridx;
    A.lidx[i] = lidx;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
int c2s_check_k(int k) {
    if (k <= 0) return mf_set_error("The size of k-mer must be at least 1.");                 // KmersCounterMain.java:66-73
    if (k > 31) return mf_set_error("The size of k-mer must be no more than 31.");
    return MF_OK;
}
static int c2s_member_flags(mf_ctx *ctx, const unsigned int *d_flags, int k) {
    unsigned int f = 0;
    MF_HIP(hipMemcpyAsync(&f, d_flags, 4, hipMemcpyDeviceToHost, ctx->stream));
    MF_HIP(hipStreamSynchronize(ctx->stream));
    if (f & 1u) return mf_set_error("comp2seq: a component holds a k-mer that does not fit %d bases", k);
    if (f & 2u) return mf_set_error("comp2seq: internal error, the pair index is full");
    return MF_OK;
}
// the rows of all components, built from the member lists (d_kmers / d_comp), never from the components' own k-mer index
int c2s_build_rows(mf_ctx *ctx, const mf_comps *c, int k, c2s_rows &R) {
    hipStream_t st = ctx->stream;
    const uint64_t n = c->n_kmers;
    R.n = 0;
    if (!n) return MF_OK;
    if (n >= 0x7FFFFFFFull) return mf_set_error("comp2seq: %llu component k-mers (fewer than 2^31 - 1 are supported)", (unsigned long long)n);
    mf_buf<uint64_t> canon, k1, k2, idx, tot; mf_buf<uint32_t> c1, c2, head, rstart; mf_buf<unsigned int> flags;
    MF_TRY(canon.alloc(ctx, n)); MF_TRY(k1.alloc(ctx, n)); MF_TRY(c1.alloc(ctx, n)); MF_TRY(k2.alloc(ctx, n)); MF_TRY(c2.alloc(ctx, n));
    MF_TRY(flags.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(flags.p, 0, 4, st));
    {
        mf_ktimer tm(ctx, "k_c2s_rows");
        k_c2s_canon<<<c2s_grid(n), 256, 0, st>>>(c->d_kmers, n, k, canon.p, nullptr, flags.p);
    }
    MF_TRY(c2s_member_flags(ctx, flags.p, k));
    // two stable passes: by k-mer, then by component
    int cb = 1; while (cb < 32 && (1ull << cb) < c->n) cb++;
    MF_TRY(mf_sort_u64_u32(ctx, canon.p, c->d_comp, n, 2 * k, k1.p, c1.p));
    MF_TRY(mf_sort_u32_u64(ctx, c1.p, k1.p, n, cb, c2.p, k2.p));
    canon.reset(); k1.reset(); c1.reset();
    MF_TRY(head.alloc(ctx, n)); MF_TRY(idx.alloc(ctx, n + 1)); MF_TRY(tot.alloc(ctx, 1));
    uint64_t nr = 0;
    {
        mf_ktimer tm(ctx, "k_c2s_rows");
        k_c2s_heads<<<c2s_grid(n), 256, 0, st>>>(c2.p, k2.p, n, head.p);
        MF_TRY(mf_scan<1>(ctx, head.p, idx.p, n, tot.p));
    }
    MF_HIP(hipMemcpyAsync(&nr, tot.p, 8, hipMemcpyDeviceToHost, st));
    MF_HIP(hipStreamSynchronize(st));
    MF_TRY(R.key.alloc(ctx, nr)); MF_TRY(R.comp.alloc(ctx, nr)); MF_TRY(R.cnt.alloc(ctx, nr)); MF_TRY(rstart.alloc(ctx, nr));
    {
        mf_ktimer tm(ctx, "k_c2s_rows");
        k_c2s_rows<<<c2s_grid(n), 256, 0, st>>>(c2.p, k2.p, head.p, idx.p, n, R.key.p, R.comp.p, rstart.p);
        k_c2s_counts<<<c2s_grid(nr), 256, 0, st>>>(rstart.p, nr, n, R.cnt.p);
    }
    MF_HIP(hipStreamSynchronize(st));                        // (the temporaries go back to the arena below)
    R.n = nr;
    return MF_OK;
}
// the pair index of the rows; *cap_out = its slots (a power of two)
int c2s_pair_index(mf_ctx *ctx, const c2s_rows &R, int k, mf_buf<mf_uslot> &slots, uint64_t *cap_out) {
    hipStream_t st = ctx->stream;
    const uint64_t nr = R.n;
    mf_buf<unsigned int> flags;
    uint64_t cap = 1024; while (cap < 2 * nr) cap <<= 1;     // load <= 0.5, as the HBM index of a table (mf_index_build)
    *cap_out = cap;
    if (nr) {
        MF_TRY(slots.alloc(ctx, cap)); MF_TRY(flags.alloc(ctx, 1));
        MF_HIP(hipMemsetAsync(slots.p, 0xFF, cap * sizeof(mf_uslot), st));       // every key word = MF_EMPTY
        MF_HIP(hipMemsetAsync(flags.p, 0, 4, st));
        {
            mf_ktimer tm(ctx, "k_c2s_index_insert");
            k_c2s_index_insert<<<c2s_grid(nr), 256, 0, st>>>(slots.p, cap - 1, R.key.p, R.comp.p, nr, flags.p);
        }
        MF_TRY(c2s_member_flags(ctx, flags.p, k));
    }
    return MF_OK;
}
int c2s_flags_launch(mf_ctx *ctx, const mf_uslot *slots, uint64_t cap, const c2s_rows &R, const ut_arrays &A) {
    mf_ktimer tm(ctx, "k_c2s_flags");
    k_c2s_flags<<<c2s_grid(R.n), 256, 0, ctx->stream>>>(slots, cap - 1, R.comp.p, A);
    return MF_OK;
}
// the segmented build over the rows: pair index, restricted U1, U2 .. U5
static int c2s_unitigs_of_rows(mf_ctx *ctx, const c2s_rows &R, uint64_t n_comps, int k, mf_seqs **out) {
    const uint64_t nr = R.n;
    mf_buf<mf_uslot> slots;
    uint64_t cap = 0;
    MF_TRY(c2s_pair_index(ctx, R, k, slots, &cap));
    mf_seqs *S = nullptr;
    MF_TRY(mf_ut_build(ctx, R.key.p, nullptr, R.cnt.p, nr, k, 0, nullptr, k, [&](const ut_arrays &A) -> int {
        return c2s_flags_launch(ctx, slots.p, cap, R, A);
    }, &S, nullptr, R.comp.p));
    if (!S->d_comp) {                                        // (no rows: no sequences, but sequences of components all the same)
        void *p = nullptr;
        if (mf_alloc(ctx, 4, &p) < 0) { mf_seqs_destroy(S); return MF_ERR; }
        S->d_comp = (uint32_t *)p; S->comp_bytes = 4;
    }
    S->n_groups = std::max<uint64_t>(n_comps, 1);
    *out = S;
    return MF_OK;
}
// --split absent: one table of all members -- distinct k-mers, count = the multiplicity over all components (capped as the counter caps)
static int c2s_union_table(mf_ctx *ctx, const mf_comps *c, int k, mf_table **out) {
    hipStream_t st = ctx->stream;
    const uint64_t n = c->n_kmers;
    mf_buf<uint64_t> canon; mf_buf<uint16_t> ones; mf_buf<unsigned int> flags;
    MF_TRY(canon.alloc(ctx, n)); MF_TRY(ones.alloc(ctx, n)); MF_TRY(flags.alloc(ctx, 1));
    MF_HIP(hipMemsetAsync(flags.p, 0, 4, st));
    if (n) {
        mf_ktimer tm(ctx, "k_c2s_rows");
        k_c2s_canon<<<c2s_grid(n), 256, 0, st>>>(c->d_kmers, n, k, canon.p, ones.p, flags.p);
    }
    MF_TRY(c2s_member_flags(ctx, flags.p, k));
    MF_TRY(mf_table_from_device_pairs(ctx, canon.p, ones.p, n, k, out));
    (*out)->n_occ = n;
    return MF_OK;
}
static int c2s_unitigs_unsplit(mf_ctx *ctx, mf_table *t, int k, mf_seqs **out) {
    mf_seqs *S = nullptr;
    MF_TRY(mf_build_unitigs_device(ctx, t, 0, k, &S));
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
static int c2s_comps_k(const mf_comps *c, int *k) {
    if (c->k == 0) return mf_set_error("mf_comps_unitigs_device: these components do not know their k (they were loaded from a file): mf_comps_set_k first");
    MF_TRY(c2s_check_k(c->k));
    *k = c->k;
    return MF_OK;
}

extern "C" int mf_comps_set_k(mf_comps *c, int k) {
    if (!c) return mf_set_error("comps is NULL");
    MF_TRY(c2s_check_k(k));
    if (c->k != 0 && c->k != k) return mf_set_error("mf_comps_set_k: k = %d, the components were built with k = %d", k, c->k);
    c->k = k;
    return MF_OK;
}

extern "C" int mf_comps_unitigs_device(mf_ctx *ctx, mf_comps *c, int split, mf_seqs **out) {
    mf_range rng_("mf:comp2seq");
    if (!ctx || !c || !out) return mf_set_error("mf_comps_unitigs_device: NULL argument");
    *out = nullptr;
    if (c->ctx != ctx) return mf_set_error("mf_comps_unitigs_device: the components belong to another context");
    int k = 0;
    MF_TRY(c2s_comps_k(c, &k));
    MF_HIP(hipSetDevice(ctx->device));
    if (split) {
        c2s_rows R;
        MF_TRY(c2s_build_rows(ctx, c, k, R));
        return c2s_unitigs_of_rows(ctx, R, c->n, k, out);
    }
    mf_table *t = nullptr;
    MF_TRY(c2s_union_table(ctx, c, k, &t));
    const int rc = c2s_unitigs_unsplit(ctx, t, k, out);
    mf_table_destroy(t);
    return rc;
}

// ---- the file form ----
int c2s_mkdirs(const std::string &p) {
    std::string cur;
    for (size_t i = 0; i <= p.size(); i++) {
        if ((i == p.size() || p[i] == '/') && !cur.empty() && mkdir(cur.c_str(), 0777) != 0 && errno != EEXIST) return mf_set_error("can't create directory %s", cur.c_str());
        if (i < p.size()) cur.push_back(p[i]);
    }
    return MF_OK;
}
int c2s_write_file(const std::string &path, const std::string &data) {
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return mf_set_error("can't write '%s'", path.c_str());
    const bool bad = data.size() && fwrite(data.data(), 1, data.size(), f) != data.size();
    if (fclose(f) != 0 || bad) return mf_set_error("can't write '%s'", path.c_str());
    return MF_OK;
}
static void c2s_kmer_text(uint64_t km, int k, std::string &out) {       // ShortKmer.toString (itmo!/dna/kmers/ShortKmer.java:153-160)
    for (int i = 0; i < k; i++) out.push_back("AGCT"[(km >> (2 * (k - 1 - i))) & 3u]);
}
// Sequence.printSequences as mf_seqs_write_fasta writes it, for the sequences [lo, hi) numbered from 1
void c2s_seq_text(const std::vector<uint8_t> &b, const std::vector<uint64_t> &o, const std::vector<int32_t> &a, const std::vector<int32_t> &mn,
                         const std::vector<int32_t> &mx, uint64_t lo, uint64_t hi, std::string &out) {
    char hdr[128];
    for (uint64_t i = lo; i < hi; i++) {
        const uint64_t len = o[i + 1] - o[i];
        snprintf(hdr, sizeof hdr, ">%llu length=%llu av_weight=%d min_weight=%d max_weight=%d\n", (unsigned long long)(i - lo + 1), (unsigned long long)len, a[i], mn[i], mx[i]);
        out += hdr;
        const char *q = reinterpret_cast<const char *>(b.data()) + o[i];
        uint64_t j = 0;
        while ((j + 1) * 70 < len) { out.append(q + j * 70, 70); out.push_back('\n'); j++; }
        out.append(q + j * 70, len - j * 70); out.push_back('\n');
    }
}
// the .kmers.bin records and the .stat.txt of rows [lo, hi) (mf_table_write_kmers' formats)
static void c2s_rows_text(const std::vector<uint64_t> &key, const std::vector<uint16_t> &cnt, uint64_t lo, uint64_t hi, std::string &bin, std::string &stat) {
    std::map<uint32_t, uint64_t> hist;
    bin.resize((hi - lo) * 10);
    for (uint64_t r = lo; r < hi; r++) {
        uint8_t *w = reinterpret_cast<uint8_t *>(&bin[(r - lo) * 10]);
        be_put(w, key[r], 8); be_put(w + 8, cnt[r], 2);
        hist[cnt[r]]++;
    }
    stat = "# k-mer frequency\tnumber of such k-mers\n";
    for (auto &h : hist) stat += std::to_string(h.first) + "\t" + std::to_string(h.second) + "\n";
    stat += "\n";
}

extern "C" int mf_comp2seq(mf_ctx *ctx, const char *components_bin, int k, int split, const char *out_dir, uint64_t *n_files, uint64_t *n_seqs) {
    mf_range rng_("mf:comp2seq(files)");
    if (!ctx || !components_bin || !out_dir) return mf_set_error("mf_comp2seq: NULL argument");
    MF_TRY(c2s_check_k(k));
    if (n_files) *n_files = 0;
    if (n_seqs) *n_seqs = 0;
    mf_comps *c = nullptr;
    MF_TRY(mf_comps_load(ctx, components_bin, &c));
    struct guard { mf_comps *p; ~guard() { mf_comps_destroy(p); } } gc{c};
    if (c->k != 0 && c->k != k) return mf_set_error("mf_comp2seq: k = %d, the components of %s were built with k = %d", k, components_bin, c->k);
    MF_HIP(hipSetDevice(ctx->device));
    const std::string od(out_dir);
    const std::string d_fa = od + "/kmers_fasta", d_km = od + "/kmer-counter-many/kmers", d_st = od + "/kmer-counter-many/stats", d_sq = od + "/seq-builder-many/sequences";
    for (const std::string *d : {&d_fa, &d_km, &d_st, &d_sq}) MF_TRY(c2s_mkdirs(*d));
    // bin2fasta (src/tools/BinaryToFasta.java:120-170): the members as the FILE lists them, not canonicalised, ">j" (split) or ">i_j" headers
    raw_file img;
    if (read_file_parallel(components_bin, img, ctx->host_threads) < 0) return mf_set_error("Can't load components: file not found (%s)", components_bin);
    std::vector<uint64_t> sizes, foff, koff; std::vector<int64_t> weights;
    const uint8_t *p = reinterpret_cast<const uint8_t *>(img.data());
    MF_TRY(comps_walk_headers(p, img.size(), sizes, weights, foff, koff));
    const uint64_t nc = sizes.size();
    if (nc != c->n || koff[nc] != c->n_kmers) return mf_set_error("mf_comp2seq: %s changed while it was read", components_bin);
    auto name = [&](const std::string &dir, uint64_t i, const char *ext) { return dir + "/component" + (split ? "_" + std::to_string(i + 1) : std::string()) + ext; };
    {
        std::string text;
        for (uint64_t i = 0; i < nc; i++) {
            for (uint64_t j = 0; j < sizes[i]; j++) {
                text += split ? ">" + std::to_string(j + 1) + "\n" : ">" + std::to_string(i + 1) + "_" + std::to_string(j + 1) + "\n";
                c2s_kmer_text(be_get(p + foff[i] + 8 * j, 8), k, text);
                text.push_back('\n');
            }
            if (split) { MF_TRY(c2s_write_file(name(d_fa, i, ".fasta"), text)); text.clear(); }
        }
        if (!split) MF_TRY(c2s_write_file(name(d_fa, 0, ".fasta"), text));
    }
    mf_seqs *S = nullptr;
    struct sguard { mf_seqs *&p; ~sguard() { mf_seqs_destroy(p); } } gs{S};
    if (split) {
        // kmer-counter-many -b 0 and seq-builder-many -b 0 -l k of every component: the sorted rows, in one host pass
        c2s_rows R;
        MF_TRY(c2s_build_rows(ctx, c, k, R));
        std::vector<uint64_t> key(R.n); std::vector<uint32_t> comp(R.n); std::vector<uint16_t> cnt(R.n);
        if (R.n) {
            MF_HIP(hipMemcpyAsync(key.data(), R.key.p, R.n * 8, hipMemcpyDeviceToHost, ctx->stream));
            MF_HIP(hipMemcpyAsync(comp.data(), R.comp.p, R.n * 4, hipMemcpyDeviceToHost, ctx->stream));
            MF_HIP(hipMemcpyAsync(cnt.data(), R.cnt.p, R.n * 2, hipMemcpyDeviceToHost, ctx->stream));
            MF_HIP(hipStreamSynchronize(ctx->stream));
        }
        MF_TRY(c2s_unitigs_of_rows(ctx, R, nc, k, &S));
        std::string bin, stat;
        uint64_t r = 0;
        for (uint64_t i = 0; i < nc; i++) {
            const uint64_t lo = r;
            while (r < R.n && comp[r] == i) r++;
            c2s_rows_text(key, cnt, lo, r, bin, stat);
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
        mf_table *t = nullptr;
        MF_TRY(c2s_union_table(ctx, c, k, &t));
        struct tguard { mf_table *p; ~tguard() { mf_table_destroy(p); } } gt{t};
        MF_TRY(mf_table_write_kmers(t, 0, name(d_km, 0, ".kmers.bin").c_str(), name(d_st, 0, ".stat.txt").c_str(), nullptr));
        MF_TRY(c2s_unitigs_unsplit(ctx, t, k, &S));
        MF_TRY(mf_seqs_write_fasta(S, name(d_sq, 0, ".seq.fasta").c_str()));
        if (n_files) *n_files = 1;
    }
    if (n_seqs) *n_seqs = S->n;
    return MF_OK;
}
