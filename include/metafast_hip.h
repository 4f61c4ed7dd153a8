/*
 * metafast_hip.h -- C-ABI of the MI355X-native MetaFast hot path
 * (libmetafast_hip.so; hand-written HIP for gfx950 behind plain C entry points).
 *
 * The reference (ctlab/metafast) is pure Java and has NO FFI: its seams for this
 * path are Java static methods called from Tool.runImpl on the main thread.  Each
 * entry point below replaces one of those seams and cites it.  The reference-side
 * binding a maintainer would add (JNI natives forwarding 1:1) is in INTEGRATION.md.
 *
 * Citations:  src/...  = /root/reference/src/...
 *             itmo!/.. = /root/reference/lib/itmo-assembler-src.jar!/ru/ifmo/genetics/..
 *
 * Conventions
 *  - every call returns int: 0 = ok, <0 = error; mf_last_error() returns a
 *    thread-local message (mirrors the Java side's checked ExecutionFailedException,
 *    itmo!/utils/tool/Tool.java:450-463).
 *  - handles are opaque and CALLER-OWNED; free with the matching *_destroy.
 *  - calls are made from one host thread, block until the result is complete and
 *    parallelise internally on the GPU (reference: callee spawns P threads and joins
 *    on a latch, src/io/IOUtils.java:846-862).
 *  - "d_" pointers are device (HBM) pointers valid on the ctx's device; everything
 *    else is host memory.  No torch / C++ types cross this boundary.
 *  - there is NO CPU fallback: without a usable GPU mf_ctx_create fails.
 *
 * k-mer encoding (itmo!/dna/DnaTools.java:31,46-64; itmo!/dna/kmers/ShortKmer.java:54-71):
 *   A=0 G=1 C=2 T=3, first base in the most significant used bits, canonical =
 *   min(forward, reverse-complement); k in [1,31]; counts saturate at 32767.
 */
#ifndef METAFAST_HIP_H
#define METAFAST_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MF_OK 0
#define MF_ERR (-1)
#define MF_MAX_COUNT 32767        /* itmo!/utils/NumUtils.java:21-26 (short saturation) */

typedef struct mf_ctx   mf_ctx;    /* device + stream + workspace                           */
typedef struct mf_table mf_table;  /* canonical k-mer -> saturating count (BigLong2ShortHashMap) */
typedef struct mf_seqs  mf_seqs;   /* unitigs with weights (Deque<Sequence>)                */
typedef struct mf_comps mf_comps;  /* connected components (List<ConnectedComponent>)       */
typedef struct mf_dcc   mf_dcc;    /* one rank's part of the distributed component cutter   */
typedef struct mf_reads mf_reads;  /* the reads of a list of files, in HBM (NamedSource<Dna>) */
typedef struct mf_kps mf_kps;      /* the k-mer x sample abundance table of a cohort (mf_kmers_per_sample_tables, ..._wide_tables) */

const char *mf_last_error(void);
const char *mf_version(void);

/* ---- context ---------------------------------------------------------------------- */
/* host_threads plays the role of -p/--available-processors (Tool.java:61-143) for the host
 * side parsers; GPU parallelism is fixed by the device. */
int  mf_ctx_create(int device, int host_threads, mf_ctx **out);
void mf_ctx_destroy(mf_ctx *ctx);
/* Devices this process sees (no context is made).  The reference's drivers loop over all libraries in one process
 * (src/tools/KmersCounterForManyFilesMain.java:80-108, SeqBuilderForManyFilesMain.java:82-94, FeaturesCalculatorMain.java:137-162);
 * a host that wants one library per GPU makes one context per device, each driven by a thread of its own. */
int  mf_device_count(void);
int  mf_device_memory(int device, uint64_t *total_bytes);
int  mf_ctx_device(const mf_ctx *ctx);
/* A context is used by ONE thread at a time; HIP's current device belongs to the thread, so a thread other than the one that made
 * the context calls this before its first call on it. */
int  mf_ctx_bind_thread(mf_ctx *ctx);
/* Use an existing HIP stream (hipStream_t as void*) for all launches instead of the ctx-owned one;
 * NULL = the device's default (null) stream. The caller keeps ownership. */
int  mf_ctx_set_stream(mf_ctx *ctx, void *hip_stream);
/* Tuning / test knobs, e.g. "l1_bits", "l2_bits", "part_target", "scatter_staged", "profile". */
int  mf_ctx_set_option(mf_ctx *ctx, const char *name, int64_t value);
int  mf_ctx_synchronize(mf_ctx *ctx);
/* Release cached workspace back to the driver. */
int  mf_ctx_trim(mf_ctx *ctx);
/* ... only `want` bytes of it, smallest idle regions first (a host that shares the device with the library and is short of
 * memory: a region the library has to allocate again costs about 35 ms per GiB).  *freed may be NULL. */
int  mf_ctx_trim_bytes(mf_ctx *ctx, uint64_t want, uint64_t *freed);
/* Per-kernel HIP-event timings accumulated while option "profile"=1.
 * Returns number of launches of `kernel` since the last reset; *total_ms = summed duration. */
int64_t mf_ctx_kernel_time(mf_ctx *ctx, const char *kernel, double *total_ms);
/* Writes "name\tlaunches\ttotal_ms\tmax_launch_ms\n" lines for every timed kernel into buf (NUL-terminated). */
int  mf_ctx_kernel_report(mf_ctx *ctx, char *buf, uint64_t cap);
int  mf_ctx_reset_timers(mf_ctx *ctx);
/* Counters and gauges by name: "slice_restarts" (counting runs that threw their slices away and started over with more because a
 * buffer found no place in HBM), "device_parsed_files" / "device_parser_stepped_back" (read files the device parser took / left to
 * the host readers), "unitig_doublings" (unitig runs whose long paths went through the doubled jump words), "wide_hashed_entries" /
 * "wide_big_entries" (k = 32..63: entries of large buckets ordered through the LDS hash tables / sorted aside), "hipmalloc_calls",
 * "hipmalloc_bytes", "hipmalloc_us", "arena_bytes", "arena_idle_bytes", "streamed_counts" / "streamed_counts_stepped_back" (counts of read
 * files that ran while the files crossed PCIe / that started so and were done again from the whole files).  < 0: unknown name. */
int64_t mf_ctx_stat(mf_ctx *ctx, const char *name);

/* ---- A1-A4  reads -> canonical k-mer counts ---------------------------------------- */
/* (round 6: plain FASTA / FASTQ files of 512 MB and more are counted WHILE they cross PCIe -- option "stream_count", mf_stream.hip: the reference's
 * reader feeds its workers while it reads, src/io/ReadsDispatcher.java:34-53 -- with the same table as a result) */
/* replaces IOUtils.loadReads (src/io/IOUtils.java:772-803), called from
 * KmersCounterMain.runImpl (src/tools/KmersCounterMain.java:77) with min_read_len=0 and from
 * ComponentCutterMain.runImpl (src/tools/ComponentCutterMain.java:81) with min_read_len=l.
 * Files are FASTA/FASTQ by extension, optionally compressed (.gz, .bz2; itmo!/io/ReadersUtils.java:27-54,
 * FastaGZReader.java, FastqGZReader.java, FastaBZ2Reader.java) or .binq (BinqReader.java); reads with N (FASTA)
 * or any phred-0 base (FASTQ) are dropped (FastaReader.java:53-76, FastaReaderFromXQSource.java:66-70).
 * All files go into ONE table (paired files are summed). */
int mf_count_reads(mf_ctx *ctx, const char *const *files, int nfiles, int k, int min_read_len,
                   mf_table **out);
/* The same load, keeping only the k-mers with count > threshold: KmersCounterMain.runImpl (src/tools/KmersCounterMain.java:77-99)
 * is loadReads followed by printKmers(hm, maximalBadFrequency, ...), which writes the entries with value > threshold only
 * (src/io/IOUtils.java:52-60).  The cut is made inside the counting kernels (mf_count_device_above), so a sample with more
 * than 2^32 distinct k-mers never exists as an uncut table; mf_table_write_kmers / mf_table_hist on the result give the same
 * .kmers.bin / .stat.txt as on the uncut table for every threshold >= this one.  *n_distinct_all (may be NULL) = distinct
 * k-mers before the cut (the "k-mers found" log line, KmersCounterMain.java:101-103). */
int mf_count_reads_above(mf_ctx *ctx, const char *const *files, int nfiles, int k, int min_read_len, int threshold,
                         mf_table **out, uint64_t *n_distinct_all);
/* The readers alone: ReadersUtils.readDnaLazy (itmo!/io/ReadersUtils.java:81-102) over a list of files -- FastaReader.java:53-104,
 * FastqReader.java:53-115 + FastaReaderFromXQSource.java:66-70, their .gz / .bz2 forms, BinqReader.java -- into the (bases, offsets)
 * layout mf_count_device takes (upper-case A / C / G / T; reads with N or a phred-0 base are not there).  Plain FASTA / FASTQ files
 * are parsed on the device (option "device_parse", mf_dparse.hip); the files that parser is not sure about, and every error, go
 * through the host readers. */
int  mf_reads_load(mf_ctx *ctx, const char *const *files, int nfiles, mf_reads **out);
void mf_reads_destroy(mf_reads *r);
int  mf_reads_stats(const mf_reads *r, uint64_t *n_reads, uint64_t *n_bases);
int  mf_reads_device_view(const mf_reads *r, const void **d_bases, const void **d_offsets);
int  mf_reads_export(const mf_reads *r, uint8_t *bases, uint64_t *offsets);      /* bases[n_bases], offsets[n_reads + 1] */
/* Same, for reads already resident in HBM: d_bases = concatenated ASCII bases (ACGT, either case,
 * no N), d_offsets = uint64[n_reads+1] with offsets[0]=0, offsets[n_reads]=n_bases.  d_bases must
 * be 16-byte aligned and readable up to the next multiple of 16 bytes.  This is the device half of
 * ReadsLoadWorker.process (src/io/IOUtils.java:756-768). */
int mf_count_device(mf_ctx *ctx, const void *d_bases, const void *d_offsets, uint64_t n_reads,
                    uint64_t n_bases, int k, int min_read_len, mf_table **out);
/* Same counting pass, but only the k-mers with count > threshold are kept (what KmersCounterMain hands on: IOUtils.printKmers
 * writes the entries with value > maximalBadFrequency, src/io/IOUtils.java:52-60; src/tools/KmersCounterMain.java:99) -- the
 * rejected entries are dropped inside the counting kernels instead of being written out and filtered afterwards.
 * *n_distinct_all (may be NULL) = number of distinct k-mers before the cut (BigLong2ShortHashMap.size()). */
int mf_count_device_above(mf_ctx *ctx, const void *d_bases, const void *d_offsets, uint64_t n_reads,
                          uint64_t n_bases, int k, int min_read_len, int threshold, mf_table **out,
                          uint64_t *n_distinct_all);
void mf_table_destroy(mf_table *t);
/* BigLong2ShortHashMap.size() and the sum of all (saturated) values */
int mf_table_stats(const mf_table *t, uint64_t *n_distinct, uint64_t *n_total);
/* k-mer occurrences fed into the table by the call that built it (N_occ) */
int mf_table_occurrences(const mf_table *t, uint64_t *n_occ);
/* Records the counting pass moved through its radix partitions to build this table: super-k-mer records of 16 bytes
 * (padding included) on the default path for k >= 20, else one 8-byte record per k-mer occurrence; 0 for tables that
 * were loaded or filtered.  Measurement only (bench.py prices the kernels' algorithmic bytes with it). */
int mf_table_records(const mf_table *t, uint64_t *n_records, int *record_bytes);
/* QuickQuantitativeStatistics of IOUtils.printKmers (src/io/IOUtils.java:45-71; itmo!/statistics/
 * QuickQuantitativeStatistics.java:38-72): hist[c] = number of distinct k-mers with count c over ALL k-mers that were
 * counted, c = 0 .. MF_MAX_COUNT (hist must hold MF_MAX_COUNT + 1 entries).  A table that comes out of
 * mf_count_device_above / mf_table_filter has remembered the k-mers the cut dropped, so this is what the .stat.txt of
 * the uncut table would hold. */
int mf_table_hist(const mf_table *t, uint64_t *hist);
/* Copies entries with count > threshold to host arrays in ASCENDING KEY order (the reference's
 * iteration order is thread-count dependent, BigLong2ShortHashMap.java:216-253, so callers must
 * not rely on it).  Call with cap=0 to get *n only. */
int mf_table_export(const mf_table *t, int threshold, uint64_t *keys, uint16_t *counts,
                    uint64_t cap, uint64_t *n);
/* Device view (unsorted, dense): uint64 keys[n], uint16 counts[n]. */
int mf_table_device_view(const mf_table *t, const void **d_keys, const void **d_counts, uint64_t *n);
/* Long2ShortHashMap.get (itmo!/structures/map/Long2ShortHashMap.java:160-175) for a batch of host
 * keys: values[i] = count or -1.  Builds the HBM open-addressed index on first use. */
int mf_table_lookup(mf_table *t, const uint64_t *keys, uint64_t n, int32_t *values);
/* Releases the table's lookup index (built on first use by the unitig builder, the features step and mf_table_lookup; rebuilt
 * when it is needed again).  The reference keeps one map per library alive at a time (KmersCounterForManyFilesMain.java:80-108);
 * a rank that holds several samples' tables drops each index between the sample's seq-builder and features steps.
 * Safe whenever no library call on this table is running (one calling thread): the views of a table that the library makes for
 * itself (a cut that keeps every entry) live inside the call that made them; a handle that came out of the context's file cache
 * (option file_cache: the same table under several handles, mf_table::refs) rebuilds the index when its next user needs it. */
int mf_table_drop_index(mf_table *t);

/* ---- NO-REFERENCE EXTENSION: 32 <= k <= 63 ----------------------------------------------------
 * The reference rejects k > 31 (src/tools/KmersCounterMain.java:66-73: one Java long per k-mer); BASELINE.json's config 4 has a
 * k = 63 leg.  These entry points replace nothing and take part in no parity claim: canonical counts of 2k-bit k-mers (two
 * 64-bit words, first base most significant, canonical = the smaller of the k-mer and its reverse complement, counts saturate
 * at 32767, reads shorter than max(k, min_read_len) give nothing) -- the k <= 31 definitions carried over; checked against
 * oracle/mf_oracle.c:or_count_wide (unsigned __int128).  Input as for mf_count_device. */
typedef struct mf_wtable mf_wtable;
int  mf_count_wide_device(mf_ctx *ctx, const void *d_bases, const void *d_offsets, uint64_t n_reads, uint64_t n_bases, int k,
                          int min_read_len, mf_wtable **out);
void mf_wtable_destroy(mf_wtable *t);
int  mf_wtable_stats(const mf_wtable *t, uint64_t *n_distinct, uint64_t *n_occ, int *k);
/* ascending k-mers as (high word, low word) + counts; NULL arrays: only *n */
int  mf_wtable_export(const mf_wtable *t, uint64_t *keys_hi, uint64_t *keys_lo, uint16_t *counts, uint64_t capacity, uint64_t *n);
/* the table where it is: it lies in HBM in *n_pieces pieces (one per pass over the reads), ascending inside a piece and piece after piece;
 * piece i: device pointers to its high words, low words (uint64) and counts (uint16), *n entries.  Valid until mf_wtable_destroy. */
int  mf_wtable_pieces(const mf_wtable *t, uint32_t *n_pieces);
int  mf_wtable_piece_view(const mf_wtable *t, uint32_t i, const void **d_keys_hi, const void **d_keys_lo, const void **d_counts, uint64_t *n);
/* ... "counted + graphed" for 32 <= k <= 63 (round 6; mf_wgraph.hip): the rest of the path on 2k-bit k-mers, same definitions as for
 * k <= 31 (the entry points named in brackets), checked against oracle/mf_oracle_wide.c = the pinned oracle's text compiled for 128-bit
 * keys.  A wide table is ascending, so a k-mer's place in it is a 32-bit vertex id that orders like the k-mer: only the neighbour
 * look-up sees 128-bit keys, everything after it is the k <= 31 machinery on ids. */
/* [mf_count_device_above] the count with the cut count > threshold inside the pass; *n_distinct_all (may be NULL) = distinct k-mers before it */
int  mf_count_wide_device_above(mf_ctx *ctx, const void *d_bases, const void *d_offsets, uint64_t n_reads, uint64_t n_bases, int k,
                                int min_read_len, int threshold, mf_wtable **out, uint64_t *n_distinct_all);
/* [mf_table_filter] the entries with count > threshold as a new table */
int  mf_wtable_filter(const mf_wtable *t, int threshold, mf_wtable **out);
/* [mf_table_drop_index] */
int  mf_wtable_drop_index(mf_wtable *t);
/* [mf_table_lookup] values[i] = count of the k-mer (keys_hi[i], keys_lo[i]) or -1; builds the lookup index on first use */
int  mf_wtable_lookup(mf_wtable *t, const uint64_t *keys_hi, const uint64_t *keys_lo, uint64_t n, int32_t *values);
/* [mf_build_unitigs_device] src/algo/AddSequencesShiftingRightTask.java:40-123 on 2k-bit k-mers; the result is an ordinary mf_seqs */
int  mf_build_unitigs_wide_device(mf_ctx *ctx, mf_wtable *t, int freq_threshold, int min_len, mf_seqs **out);
/* [mf_cut_components_device] src/algo/ComponentsBuilder.java:58-270; the cutter table = mf_count_wide_device over the unitigs with
 * min_read_len = l.  Components ordered as for k <= 31 (thr asc, weight desc, size desc, smallest k-mer asc), k-mers ascending inside */
typedef struct mf_wcomps mf_wcomps;
int  mf_cut_components_wide_device(mf_ctx *ctx, mf_wtable *cutter, int b1, int b2, mf_wcomps **out);
void mf_wcomps_destroy(mf_wcomps *c);
int  mf_wcomps_stats(const mf_wcomps *c, uint64_t *n_comp, uint64_t *n_kmers);
/* sizes[n], weights[n], thr[n], kmer_offsets[n + 1], the k-mers' high and low words [n_kmers]; any array may be NULL */
int  mf_wcomps_export(const mf_wcomps *c, uint64_t *sizes, int64_t *weights, int32_t *thr, uint64_t *kmer_offsets, uint64_t *kmers_hi,
                      uint64_t *kmers_lo);
/* [mf_features_device] vec[c] = sum of the sample's counts > threshold over the component's k-mers, breadth[c] = found / size */
int  mf_features_wide_device(mf_ctx *ctx, mf_wcomps *c, mf_wtable *sample, int threshold, int64_t *vec, double *breadth);
/* [mf_features_device_selected / mf_features_reads_device(_selected)] the other two inputs of features-calculator on wide components
 * (mf_wfeatures.hip), the k <= 31 definitions word for word on 2k-bit k-mers (oracle/mf_oracle_core.inc: or_features_selected,
 * or_features_reads_selected, compiled for 128-bit keys).  k is the components' own.  A component is summed over its member LISTINGS: a
 * k-mer that two components list is read once for each.  selected (NULL: no selection): only the listings whose k-mer has a value > 0 in
 * that table take part -- in vec, in found and in the denominator of breadth = found / cnt, which is 0.0 / 0.0 = NaN for a component
 * with no such listing; a negative threshold makes absent k-mers count as found.  Reads form: every position of every read of >= k bases
 * whose canonical k-mer is a member adds 1 to it, in 64 bits -- a k-mer seen 40 000 times counts 40 000, where a sample table holds 32767;
 * reads shorter than k give nothing, no reads give vec = 0 and breadth = 0 / cnt; d_bases are ASCII letters of either case without
 * alignment or slack demands (a run of positions reads its own bases only), d_offsets as for mf_count_device; offsets that go backwards
 * or do not end at n_bases are errors.  Errors carry the entry point's name: NULL arguments, a handle of another context, a sample or
 * selected table of another k, k outside 32 ... 63, 2^32 - 1 or more members.  No components: MF_OK, nothing written.  The file forms
 * load the components with mf_wcomps_load(k) first (nothing is written before it has accepted the file, and an empty one is the
 * reference's "No components were found" error), take the files of ONE library through mf_reads_load or one wide .kmers.bin uncut,
 * and write .vec / .breadth as for k <= 31.  mf_ctx_stat("wf_run"): the read positions one thread takes. */
int  mf_features_wide_device_selected(mf_ctx *ctx, mf_wcomps *c, mf_wtable *sample, mf_wtable *selected, int threshold, int64_t *vec,
                                      double *breadth);
int  mf_features_reads_wide_device(mf_ctx *ctx, mf_wcomps *c, const void *d_bases, const void *d_offsets, uint64_t n_reads,
                                   uint64_t n_bases, int threshold, int64_t *vec, double *breadth);
int  mf_features_reads_wide_device_selected(mf_ctx *ctx, mf_wcomps *c, const void *d_bases, const void *d_offsets, uint64_t n_reads,
                                            uint64_t n_bases, mf_wtable *selected, int threshold, int64_t *vec, double *breadth);
/* ... and its files (mf_wio.hip).  No reference format exists for k > 31; these are the project's own:
 *   wide .kmers.bin     headerless, 18-byte big-endian records: int64 high word, int64 low word, int16 count (the words of
 *                       mf_wtable_export); strictly ascending in (high, low); only records with count > threshold
 *   wide components.bin the layout of mf_comps_write with every member k-mer written as two int64 (high, low)
 *   .stat.txt, components-stat.txt, .seq.fasta, .vec, .breadth: the k <= 31 files
 * A headerless file cannot say how wide its records are, so the loaders check every record on the device (the size is a multiple of
 * the record; every k-mer < 4^k, canonical, strictly above its predecessor; counts positive) and refuse a file that fails by name,
 * with the number of its first bad record. */
/* [mf_count_reads] the files' reads counted UNCUT (the histogram of .stat.txt covers what the cut of the writer drops, and a wide table does
 * not keep it): every distinct k-mer of the read set must fit in HBM, the limit of mf_count_wide_device */
int  mf_count_reads_wide(mf_ctx *ctx, const char *const *files, int nfiles, int k, int min_read_len, mf_wtable **out);
/* [mf_table_write_kmers] records with count > threshold, ascending whatever order the count left the table in (it is ordered in place);
 * stat_txt (may be NULL): the histogram of ALL entries of the table, an error for a table that was cut.  Context option
 * "wide_write_slab": records encoded in HBM at a time */
int  mf_wtable_write_kmers(mf_wtable *t, int threshold, const char *kmers_bin, const char *stat_txt, uint64_t *n_good);
/* [mf_table_load_kmers] records with count <= freq_threshold dropped; one file: one ascending piece, no sort; several files: a k-mer gets the
 * sum of its counts, saturating at 32767 */
int  mf_wtable_load_kmers(mf_ctx *ctx, const char *const *files, int nfiles, int freq_threshold, int k, mf_wtable **out);
/* [mf_table_write_kmers_filtered] the records of t with count > threshold whose k-mer has a value > filter_threshold in `filter` (absent: 0),
 * in the format and order of mf_wtable_write_kmers; *n_written (may be NULL) = records.  Both tables of one context and one k; the filter
 * gets its lookup index (mf_wtable_lookup's), t is ordered in place. */
int  mf_wtable_write_kmers_filtered(mf_wtable *t, int threshold, mf_wtable *filter, int filter_threshold, const char *kmers_bin,
                                    uint64_t *n_written);
/* [mf_unique_kmers_multi_tables] the same definition on (high, low) keys (mf_wjoin.hip): cnt(x), sum(x) wrapped to a Java short, an x that a
 * filter table holds with count > b knocked out, *n_union = distinct keys of the inputs, out[i - min_samples] = the records (x, sum(x)) with
 * sum(x) > b and cnt(x) >= i as ascending wide tables, the list ending with the first empty one (included); out and counts sized as there.
 * The join sorts and reduces per slice of the KEY RANGE (option "stats_slices" forces their number; the result is the same for every number);
 * a slice that does not fit its share of HBM is an error that names the option.  Errors as there (min_samples > max_samples with the
 * reference's message, max_bad < 0, more than 32767 inputs), and: a NULL table, a table of another context, tables of different k -- each
 * names the list and the table's number.  Tables in any order (fresh from the count or loaded) are taken as they are. */
int  mf_unique_kmers_multi_wide_tables(mf_ctx *ctx, mf_wtable *const *inputs, int n_inputs, mf_wtable *const *filters, int n_filters,
                                       int max_bad, int min_samples, int max_samples, mf_wtable **out, int *n_out, uint64_t *n_union,
                                       uint64_t *counts);
/* [mf_unique_kmers_multi] wide .kmers.bin files, each loaded with mf_wtable_load_kmers(file, max_bad), one sample resident at a time (a file
 * is read once per slice) -> <out_dir>/filtered_<i>.kmers.bin, wide records.  32 <= k <= 63. */
int  mf_unique_kmers_multi_wide(mf_ctx *ctx, const char *const *in_files, int n_inputs, const char *const *filter_files, int n_filters,
                                int max_bad, int k, int min_samples, int max_samples, const char *out_dir, int *n_out, uint64_t *n_union,
                                uint64_t *counts);
/* [mf_kmers_per_sample_tables] the same definition on (high, low) keys (mf_wkps.hip): the candidates are the k-mers some sample
 * (the first included) holds with count > max_bad, n(x) = the samples j >= 1 (count_first != 0: j >= 0) that do, selected: n(x) >= thresh =
 * n * percent / 100 in Java int arithmetic (thresh <= 0: every candidate, thresh > n: none).  *out = an mf_kps handle (below, with the narrow
 * tool): the M selected k-mers ascending in (high, low), their n(x), the n x M row-major uint16 matrix of the samples' counts (0 = absent or
 * count <= max_bad).  mf_kps_destroy, mf_kps_stats, mf_kps_row_text and mf_kps_header_text (its k must be the tables' k) take the handle;
 * mf_kps_export and mf_kps_device_view hold one word a k-mer and refuse it by name: mf_kps_export_wide and mf_kps_device_view_wide are its
 * forms (and refuse a handle of k <= 31).  The union sorts and reduces per slice of the key range (option "stats_slices"; the result is the
 * same for every number).  Errors, each named and none a write out of bounds: n < 1 or n > 32767; a NULL table, a table of another
 * context, tables of different k, k outside 32 ... 63; a sample or a slice of 2^31 or more entries (raise stats_slices); 2^32 - 1 or more
 * selected k-mers (raise -perc); a matrix of n x M x 2 bytes that does not fit the free device memory (raise -perc, or use the file form).
 * Tables in any order (fresh from the count, in several pieces, or loaded) are taken as they are. */
int  mf_kmers_per_sample_wide_tables(mf_ctx *ctx, mf_wtable *const *tables, int n, int max_bad, int percent, int count_first, mf_kps **out);
/* device pointers, valid until the destroy: uint64 high[M], uint64 low[M], uint16 n(x)[M], uint16 matrix[n][M]; any may be NULL */
int  mf_kps_device_view_wide(const mf_kps *r, const void **d_hi, const void **d_lo, const void **d_nsamples, const void **d_matrix);
/* host copies: hi[M], lo[M], nsamples[M], matrix[n * M]; any may be NULL */
int  mf_kps_export_wide(const mf_kps *r, uint64_t *hi, uint64_t *lo, uint16_t *nsamples, uint16_t *matrix);
/* [mf_kmers_per_sample] the file form on wide .kmers.bin files, max_bad = 0: every load is mf_wtable_load_kmers(file, 1, 0, k), one sample
 * resident at a time -- loaded, gathered, formatted, downloaded and written before the next; the matrix is never resident and every file
 * is read twice (once more per further slice).  out_txt as there: "\t" + the k bases per selected k-mer, then per file its name with
 * every ".kmers.bin" removed and "\t" + count per selected k-mer.  32 <= k <= 63; *n_kmers (may be NULL) = M. */
int  mf_kmers_per_sample_wide(mf_ctx *ctx, const char *const *files, int n, int k, int percent, int count_first, const char *out_txt,
                              uint64_t *n_kmers);
/* [mf_stats_kmers_tables] the same definition on (high, low) keys (mf_wstats.hip), samples numbered A first, then B: sample j holds
 * x iff its count of x is > max_bad; counters[9] (MF_STATS_COUNTERS) as there; chi = the chi-squared survivors with value 1, group_a / group_b =
 * the kept k-mers with the Java (short)(int) of their mean, all three ascending wide tables.  A group table's values are any 16 bits: 0 and
 * values >= 0x8000 occur and are held as the uint16 they are (mf_wtable_export gives them as they are).  The union sorts and reduces per slice of
 * the key range with weights (A = 1, B = 0: the weighted sum is n1A), the chi-squared and Mann-Whitney decisions are the host tables and the row
 * kernels of the narrow tool; option "stats_slices" forces the number of slices and the result is the same for every number.  Errors, each named
 * and none a write out of bounds: na < 1 or nb < 1, na + nb > 1024, p_chi2 outside [0, 1], max_bad < 0; a NULL table, a table of another
 * context, tables of different k, k outside 32 ... 63; a sample or a slice of 2^31 or more entries, a slice that overflows its buffer, a
 * slice's matrix of survivors x samples x 2 bytes that does not fit the free device memory (each: raise stats_slices).  Tables in any order
 * (fresh from the count, in several pieces, or loaded) are taken as they are. */
int  mf_stats_kmers_wide_tables(mf_ctx *ctx, mf_wtable *const *a, int na, mf_wtable *const *b, int nb, int max_bad, double p_chi2, double p_mw,
                                mf_wtable **chi, mf_wtable **group_a, mf_wtable **group_b, uint64_t *counters);
/* [mf_stats_kmers] the file form on wide .kmers.bin files: every load is mf_wtable_load_kmers(file, 1, 0, k) (the loader checks every record:
 * a file lists no k-mer twice), one sample resident at a time, each file read twice per slice -> <out_dir>/filtered_chisquared.kmers.bin +
 * .stat.txt, filtered_groupA.kmers.bin, filtered_groupB.kmers.bin, wide records, ascending.  The group files are written at threshold -1,
 * every record as in the narrow tool: such a file may hold records with a value <= 0, which mf_wtable_load_kmers refuses by design (`view
 * --wide-kmers` reads them on the host).  32 <= k <= 63; counters may be NULL. */
int  mf_stats_kmers_wide(mf_ctx *ctx, const char *const *a_files, int na, const char *const *b_files, int nb, int max_bad, int k, double p_chi2,
                         double p_mw, const char *out_dir, uint64_t *counters);
/* [mf_kmers_samples_count_tables / mf_kmers_samples_count] n(x) = the samples that hold x with count > max_bad, for every x with n(x) > 0, as an
 * ascending wide table: the union's sample count with no further pass.  At most 32767 samples.  Library calls only: the command-line tool
 * kmers-samples-counter stays at k <= 31. */
int  mf_kmers_samples_count_wide_tables(mf_ctx *ctx, mf_wtable *const *t, int n, int max_bad, mf_wtable **out);
int  mf_kmers_samples_count_wide(mf_ctx *ctx, const char *const *files, int n, int max_bad, int k, const char *kmers_bin, const char *stat_txt,
                                 uint64_t *n_kmers);
/* [mf_stats_kmers3_tables] the same definition on (high, low) keys (mf_wstats.hip), samples numbered A, then B, then C: sample j
 * holds x iff its count of x is > max_bad; counters[10] (MF_STATS3_COUNTERS) as there; chi = the chi-squared survivors with value 1, group_a /
 * group_b / group_c = the kept k-mers with the Java (short)(int) of their mean (any 16 bits, as in mf_stats_kmers_wide_tables), all four
 * ascending wide tables.  One union per slice of the key range carries the three per-group sample counts of a k-mer as one word of three
 * 10-bit fields (a run of equal k-mers is counted by group in the reduce pass; a weighted 16-bit sum cannot hold three counts); the
 * chi-squared and Mann-Whitney decisions are the host tables and the three-group row kernels of the narrow tool; option "stats_slices" forces
 * the number of slices and the result is the same for every number.  Errors, each named and none a write out of bounds: a group with no
 * sample, na + nb + nc > 1024, p_chi2 outside [0, 1], max_bad < 0; a NULL table, a table of another context, tables of different k, k outside
 * 32 ... 63; the join's slice errors and a slice's matrix that does not fit (each: raise stats_slices).  On an error no table is returned.
 * Library calls only: the command-line tool stats-kmers-3 stays at k <= 31, with or without --wide-kmers. */
int  mf_stats_kmers3_wide_tables(mf_ctx *ctx, mf_wtable *const *a, int na, mf_wtable *const *b, int nb, mf_wtable *const *c, int nc, int max_bad,
                                 double p_chi2, double p_mw, mf_wtable **chi, mf_wtable **group_a, mf_wtable **group_b, mf_wtable **group_c,
                                 uint64_t *counters);
/* [mf_stats_kmers3] the file form on wide .kmers.bin files, as mf_stats_kmers_wide: every load is mf_wtable_load_kmers(file, 1, 0, k), one
 * sample resident at a time -> <out_dir>/filtered_chisquared.kmers.bin + .stat.txt, filtered_group{A,B,C}.kmers.bin, wide records, ascending,
 * the group files at threshold -1 (values are Java shorts: 0 and >= 0x8000 occur).  32 <= k <= 63; counters may be NULL. */
int  mf_stats_kmers3_wide(mf_ctx *ctx, const char *const *a_files, int na, const char *const *b_files, int nb, const char *const *c_files, int nc,
                          int max_bad, int k, double p_chi2, double p_mw, const char *out_dir, uint64_t *counters);
/* [mf_kmers_grouped_count_tables] on wide tables: for every k-mer x of `kmers` the number of tables of each group (CD, UC, nonIBD; a group
 * may be empty, at most 1022 tables in one) whose count of x is > max_bad.  *n = the entries of `kmers`, whatever `cap` is; with cap >= *n,
 * (hi, lo)[0 .. *n) = the k-mers in ascending order and counts[i] = cd << 32 | uc << 16 | nonibd; with a smaller cap nothing is written (cap = 0
 * with NULL arrays asks for the number alone).  `kmers` is put in ascending order, in one piece, if it is not.  With no k-mer in `kmers` the
 * groups are not read at all. */
int  mf_kmers_grouped_count_wide_tables(mf_ctx *ctx, mf_wtable *kmers, mf_wtable *const *cd, int n_cd, mf_wtable *const *uc, int n_uc,
                                        mf_wtable *const *nonibd, int n_nonibd, int max_bad, uint64_t *hi, uint64_t *lo, uint64_t *counts,
                                        uint64_t cap, uint64_t *n);
/* [mf_kmers_grouped_count] the file form on wide .kmers.bin files: kmers = mf_wtable_load_kmers(kmers_files, n, 0, k), the group files loaded
 * one at a time -> out_txt: the line "Kmer\tcd_count\tuc_count\tnonibd_count", then one line per k-mer in ascending (hi, lo) order, its k
 * bases (A G C T = 0 1 2 3, the first base in the highest bits) and the three counts.  32 <= k <= 63; *n_kmers (may be NULL) = lines written. */
int  mf_kmers_grouped_count_wide(mf_ctx *ctx, const char *const *kmers_files, int n_kmers_files, const char *const *cd_files, int n_cd,
                                 const char *const *uc_files, int n_uc, const char *const *nonibd_files, int n_nonibd, int max_bad, int k,
                                 const char *out_txt, uint64_t *n_kmers);
/* [mf_comps_write / mf_comps_load] on load the members must be < 4^k and ascending inside a component */
int  mf_wcomps_write(const mf_wcomps *c, const char *components_bin, const char *stat_txt);
int  mf_wcomps_load(mf_ctx *ctx, const char *components_bin, int k, mf_wcomps **out);
/* [mf_features] both files loaded, mf_features_wide_device, .vec / .breadth as for k <= 31 */
int  mf_features_wide(mf_ctx *ctx, const char *components_bin, const char *kmers_bin, int k, int threshold, const char *vec_path,
                      const char *breadth_path);
/* [mf_features_selected / mf_features_reads(_selected)] the file forms of the calls above */
int  mf_features_wide_selected(mf_ctx *ctx, const char *components_bin, const char *kmers_bin, int k, int threshold, mf_wtable *selected,
                               const char *vec_path, const char *breadth_path);
int  mf_features_reads_wide(mf_ctx *ctx, const char *components_bin, const char *const *files, int nfiles, int k, int threshold,
                            const char *vec_path, const char *breadth_path);
int  mf_features_reads_wide_selected(mf_ctx *ctx, const char *components_bin, const char *const *files, int nfiles, int k, int threshold,
                                     mf_wtable *selected, const char *vec_path, const char *breadth_path);
/* [mf_comps_unitigs_device / mf_comp2seq] comp2seq on wide components (mf_wcomp2seq.hip): the semantics of the k <= 31 entry points on
 * 2k-bit k-mers.  split != 0: per component the unitigs (threshold 0, minimal length k) of its canonical k-mers, each weighted with its
 * multiplicity in the member list, a neighbour counting only inside the SAME component, all components in one pass; split == 0: the
 * unitigs of the one table of all members (count = multiplicity over all components, capped at 32767).  The components know their k
 * (mf_wcomps_load takes it).  A member list may hold x and rc(x): that k-mer then has multiplicity 2.  The result is an ordinary mf_seqs
 * for mf_seqs_components / mf_seqs_export / mf_seqs_write_fasta, in (component, canonical start k-mer, strand) order.  Fewer than
 * 2^31 - 1 members.  The file form writes mf_comp2seq's layout under out_dir with WIDE .kmers.bin records; nothing is written before
 * mf_wcomps_load has accepted the file. */
int  mf_wcomps_unitigs_device(mf_ctx *ctx, mf_wcomps *c, int split, mf_seqs **out);
int  mf_comp2seq_wide(mf_ctx *ctx, const char *components_bin, int k, int split, const char *out_dir, uint64_t *n_files,
                      uint64_t *n_seqs);
/* [mf_comps_graph_device / mf_comp2graph] comp2graph on wide components (mf_wcomp2graph.hip): the semantics of the k <= 31 entry points
 * on 2k-bit k-mers, rule for rule -- names <n>_i<c>, paths ascending by (canonical start k-mer, strand as walked) then isolated cycles, the
 * printed strand never above its reverse complement in string order, L lines ascending by (from, sign, to, sign), a palindromic k-mer
 * (even k) as two S lines with its links counted twice, a hairpin ending its segment with a link to itself; a member list that holds x
 * and rc(x) gives one row, drawn once.  Values: no samples -- every member 1; coverage == 0 -- the number of tables that hold the k-mer
 * with a count > 0; coverage != 0 -- the summed count, bounded at 32767.  A sample table of another k or another context is an error.
 * The result is an ordinary mf_gfa, declared below, for mf_gfa_text / mf_gfa_stats / mf_gfa_destroy.  Fewer than 2^31 - 1 members,
 * 2^31 - 1 segments, 2^32 - 1 components.  The file form keeps one wide .kmers.bin resident at a time (coverage: one load of all files);
 * nothing is written before mf_wcomps_load has accepted the file and the text is complete. */
struct mf_gfa;
int  mf_wcomps_graph_device(mf_ctx *ctx, mf_wcomps *c, mf_wtable *const *samples, int n_samples, int coverage, struct mf_gfa **out);
int  mf_comp2graph_wide(mf_ctx *ctx, const char *components_bin, int k, const char *const *kmers_files, int n_files, int coverage,
                        const char *out_gfa, uint64_t *n_components, uint64_t *n_segments, uint64_t *n_links);
/* [mf_comps_from_sequences_device / mf_seq2comp] seq2comp on 2k-bit k-mers (mf_wseq2comp.hip): the semantics of the k <= 31 entry points
 * word for word -- one component per sequence in sequence order, members the distinct canonical k-mers, size their number, weight
 * max(0, L - k + 1), thr 0, a sequence shorter than k an empty component -- with the members ASCENDING in (hi, lo) inside every component
 * on the device, as every mf_wcomps has them.  32 <= k <= 63; the limits and their messages are the narrow tool's (n_seqs, members and the
 * k-mers of one sequence below 2^32 - 1; offsets that go backwards or do not end at n_bases are errors).  Sequences of up to
 * mf_ctx_stat("ws2c_lds_max") k-mers are sorted in LDS, longer ones by three pair sorts; options "s2c_lds" and "s2c_batch_pairs" and stat
 * "s2c_sort_batches" as for k <= 31.  The file form keeps one file resident at a time, writes components_bin through mf_wcomps_write and
 * the three-column stat_txt (may be NULL) itself; nothing is written when an argument is refused. */
int  mf_wcomps_from_sequences_device(mf_ctx *ctx, const void *d_bases, const void *d_offsets, uint64_t n_seqs, uint64_t n_bases, int k,
                                     mf_wcomps **out);
int  mf_seq2comp_wide(mf_ctx *ctx, const char *const *files, int nfiles, int k, const char *components_bin, const char *stat_txt,
                      uint64_t *n_components, uint64_t *per_file);

/* ---- A5/A6 .kmers.bin / .stat.txt --------------------------------------------------- */
/* replaces IOUtils.printKmers (src/io/IOUtils.java:45-71; KmersCounterMain.java:99): 10-byte
 * big-endian records (int64 k-mer, int16 count) for count > threshold, ascending key order;
 * histogram of ALL counts to stat_txt (may be NULL). */
int mf_table_write_kmers(const mf_table *t, int threshold, const char *kmers_bin,
                         const char *stat_txt, uint64_t *n_good);
/* replaces IOUtils.filterAndPrintKmers (src/io/IOUtils.java:101-123; KmersFilter.java:107): the
 * records of `t` with count > threshold whose k-mer has a value > filter_threshold in `filter`
 * (absent = 0), same record format and order as mf_table_write_kmers. */
int mf_table_write_kmers_filtered(const mf_table *t, int threshold, mf_table *filter, int filter_threshold,
                                  const char *kmers_bin, uint64_t *n_good);
/* replaces IOUtils.loadKmers (src/io/IOUtils.java:369-401; SeqBuilderMain.java:80): keeps records
 * with freq > freq_threshold; duplicate k-mers across files are summed with saturation. */
int mf_table_load_kmers(mf_ctx *ctx, const char *const *files, int nfiles, int freq_threshold, int k,
                        mf_table **out);
/* In-HBM equivalent of write_kmers + load_kmers: new table with the entries whose count > threshold. */
int mf_table_filter(const mf_table *t, int threshold, mf_table **out);
/* Build a table from host (key,count) arrays (insert-or-add with saturation). */
int mf_table_from_host(mf_ctx *ctx, const uint64_t *keys, const uint16_t *counts, uint64_t n, int k,
                       mf_table **out);

/* ---- A7/A8  unitigs ---------------------------------------------------------------- */
/* replaces SequencesFinders.thresholdStrategy (src/algo/SequencesFinders.java:13-31 ->
 * AddSequencesShiftingRightTask.java:40-123) over k-mers with count > freq_threshold, keeping
 * sequences with length >= min_len, including the reference's start/end emission rule
 * (:101-121) under which a path may be emitted 0, 1 or 2 times. */
int  mf_build_unitigs_device(mf_ctx *ctx, mf_table *t, int freq_threshold, int min_len, mf_seqs **out);
void mf_seqs_destroy(mf_seqs *s);
int  mf_seqs_stats(const mf_seqs *s, uint64_t *n_seqs, uint64_t *total_len);
/* Device view: ASCII bases concatenated + uint64 offsets[n+1] (same layout mf_count_device takes),
 * int32 avg/min/max weights per sequence. */
int  mf_seqs_device_view(const mf_seqs *s, const void **d_bases, const void **d_offsets,
                         const void **d_avg, const void **d_min, const void **d_max,
                         uint64_t *n_seqs, uint64_t *n_bases);
/* Host copy: bases[total_len], offsets[n+1], avg/min/max[n]; sequences ordered by
 * (canonical start k-mer, strand) for reproducibility (reference order is a thread race). */
int  mf_seqs_export(const mf_seqs *s, uint8_t *bases, uint64_t *offsets, int32_t *avg, int32_t *mn,
                    int32_t *mx);
/* Sequence.printSequences (src/structures/Sequence.java:26-37): ">i length=L av_weight=A
 * min_weight=m max_weight=M", 70 columns (FastaDedicatedWriter.java:15,33-49). */
int  mf_seqs_write_fasta(const mf_seqs *s, const char *seq_fasta);
/* One call = SeqBuilderMain.runImpl (src/tools/SeqBuilderMain.java:78-160): histogram file
 * `distribution` (:84-98,170-176; may be NULL) + unitigs to seq_fasta. */
int  mf_build_unitigs(mf_ctx *ctx, mf_table *t, int k, int freq_threshold, int min_len,
                      const char *seq_fasta, const char *distribution, uint64_t *n_seq);

/* ---- A9-A11  component cutter ------------------------------------------------------- */
/* replaces ComponentsBuilder.splitStrategy (src/algo/ComponentsBuilder.java:24-32,58-270) on the
 * cutter table (k-mers of every emitted unitig of every sample): connected components over the 8
 * canonical neighbours (src/algo/KmerOperations.java:9-26), size window [b1,b2], oversize
 * components re-split on value >= thr+1.  Components are ordered by (thr asc, weight desc,
 * size desc, min k-mer asc); k-mers inside a component ascending. */
int  mf_cut_components_device(mf_ctx *ctx, mf_table *cutter, int b1, int b2, mf_comps **out);
void mf_comps_destroy(mf_comps *c);
int  mf_comps_stats(const mf_comps *c, uint64_t *n_comp, uint64_t *n_kmers);
/* Host copy: sizes[n], weights[n], thr[n], kmer_offsets[n+1], kmers[n_kmers]. */
int  mf_comps_export(const mf_comps *c, uint64_t *sizes, int64_t *weights, int32_t *thr,
                     uint64_t *kmer_offsets, uint64_t *kmers);
/* ConnectedComponent.saveComponents (src/structures/ConnectedComponent.java:80-93) +
 * components-stat file (ComponentsBuilder.java:146-152; may be NULL). */
int  mf_comps_write(const mf_comps *c, const char *components_bin, const char *stat_txt);
/* ConnectedComponent.loadComponents (:95-122) */
int  mf_comps_load(mf_ctx *ctx, const char *components_bin, mf_comps **out);
/* One call = ComponentCutterMain.runImpl :92-108 */
int  mf_cut_components(mf_ctx *ctx, mf_table *cutter, int k, int b1, int b2,
                       const char *components_bin, const char *stat_txt, uint64_t *n_comp);
/* comp2seq (src/tools/ComponentsToSequences.java:41-76: bin2fasta, kmer-counter-many -b 0, seq-builder-many -b 0 -l k; mf_comp2seq.hip).
 * split != 0: the contigs of every component by itself -- the unitigs (threshold 0, minimal length k) of the component's canonical
 * k-mers, each weighted with its multiplicity in the component's member list, a neighbour counting only when it is a member of the SAME
 * component; a k-mer that is a member of several components takes part in each.  All components are built in one pass.  split == 0: the
 * unitigs of the one table of all members (count = multiplicity over all components).  k <= 31; components that were loaded from a
 * file do not know their k: mf_comps_set_k states it (an error where the components know another one). */
int  mf_comps_set_k(mf_comps *c, int k);
int  mf_comps_unitigs_device(mf_ctx *ctx, mf_comps *c, int split, mf_seqs **out);
/* The component index of every sequence, in the order of mf_seqs_export -- which, for these sequences, is (component, oriented start
 * k-mer); all 0 where split was 0; an error for sequences of another producer.  *n (may be NULL) = the number of sequences; nothing
 * is written when capacity is below it. */
int  mf_seqs_components(const mf_seqs *s, uint32_t *comp, uint64_t capacity, uint64_t *n);
/* File form, the reference's layout under out_dir (i = 1, 2, ... in the file's order; without split one file set, no suffix):
 *   kmers_fasta/component[_<i>].fasta                       the members as the file lists them (BinaryToFasta.java:120-170)
 *   kmer-counter-many/kmers/component[_<i>].kmers.bin       records as mf_table_write_kmers writes them, ascending k-mers
 *   kmer-counter-many/stats/component[_<i>].stat.txt
 *   seq-builder-many/sequences/component[_<i>].seq.fasta    as mf_seqs_write_fasta, numbered from 1 in every file
 * Every component gets its four files.  *n_files = file sets written, *n_seqs = sequences in all (either may be NULL). */
int  mf_comp2seq(mf_ctx *ctx, const char *components_bin, int k, int split, const char *out_dir,
                 uint64_t *n_files, uint64_t *n_seqs);
/* comp2graph (src/tools/ComponentsToGraph.java:70-130, src/algo/Comp2Graph.java, src/io/GFAWriter.java; mf_comp2graph.hip): the compacted
 * de Bruijn graph of every component as GFA text, all components in one pass.  Per component all S lines, then all L lines; components
 * in their order, an empty one contributes nothing.  A segment is a maximal path whose inner links are the only way out of one k-mer and
 * the only way into the next, inside the component; it is printed on the strand that is not above its reverse complement in string
 * order (LN = its bases, KC = the values of its k-mers + (k - 1) x the value of the printed strand's last k-mer).  L lines as
 * GFAWriter.printEdge: every adjacency from both sides.  Where the reference's names follow the iteration order of a hash map, these are
 * fixed: segment <n>_i<c>, c = the component's position, n = 1, 2, ... inside the component -- paths (walked from the end whose
 * canonical k-mer is smaller) ascending by (canonical start k-mer, strand of the start k-mer as walked: canonical first),
 * then isolated cycles, each opened at its smallest canonical k-mer (numeric order of the 2-bit code A0 G1 C2 T3) on that k-mer's
 * canonical strand, with a link from its end to its start; L lines ascending by (from, from sign, to, to sign), '+' before '-'.
 * Values: no samples -- every k-mer 1; coverage == 0 -- the number of samples that hold the k-mer; coverage != 0 -- its summed count over
 * the samples, bounded at 32767 (IOUtils.loadKmers, threshold 0).  k <= 31 (mf_comps_set_k for components loaded from a file). */
typedef struct mf_gfa mf_gfa;
int  mf_comps_graph_device(mf_ctx *ctx, mf_comps *c, mf_table *const *samples, int n_samples, int coverage, mf_gfa **out);
void mf_gfa_destroy(mf_gfa *g);
/* any may be NULL: segments (a palindromic k-mer's two S lines count once), L lines, opened cycles, bytes of text */
int  mf_gfa_stats(const mf_gfa *g, uint64_t *n_segments, uint64_t *n_links, uint64_t *n_cycles, uint64_t *n_bytes);
/* *n (may be NULL) = the bytes of the text, whatever cap is; nothing is written when cap is below it */
int  mf_gfa_text(const mf_gfa *g, uint8_t *text, uint64_t cap, uint64_t *n);
/* File form: components_bin + optional .kmers.bin files (one resident at a time) -> out_gfa.  The counts may be NULL. */
int  mf_comp2graph(mf_ctx *ctx, const char *components_bin, int k, const char *const *kmers_files, int n_files, int coverage,
                   const char *out_gfa, uint64_t *n_components, uint64_t *n_segments, uint64_t *n_links);

/* seq2comp (src/tools/SequencesToComponents.java:61-103, src/algo/ComponentFromSequence.java:24-30; mf_seq2comp.hip): sequences a user
 * already has -- a gene catalogue, marker contigs, filtered .seq.fasta files of comp2seq -- as components, so that features-calculator
 * counts one feature per sequence.  Every sequence gives ONE component, in the order of the sequences: its members are the distinct
 * canonical k-mers of the sequence, size = their number, weight = the k-mer occurrences max(0, L - k + 1).  A sequence shorter than k
 * gives a component of size 0 and weight 0 (its position is its feature index; its breadth is 0.0 / 0.0 = NaN, its vector entry 0).
 * Components may share k-mers (a common stretch, a sequence given twice): the features calls credit such a k-mer to every component
 * that lists it, as the reference does.  Deviations, as sets and in size and weight the components are the reference's: inside one
 * file the reference appends the components in the order its thread pool finishes, here they come in file order, then record order;
 * the reference lists a component's k-mers in first-occurrence order, here they ascend, as in every components.bin of this library.
 * Device form: the (bases, offsets) layout of mf_count_device / mf_reads_device_view; the result is an ordinary mf_comps -- k set, thr 0,
 * no index yet -- for mf_comps_export, mf_comps_write, mf_features_device*, mf_comps_unitigs_device, mf_comps_graph_device.
 * 1 <= k <= 31, n_seqs < 2^32 - 1, a sequence of fewer than 2^32 - 1 k-mers, fewer than 2^32 - 1 members in all: anything beyond is an
 * error, never a truncated result.  Sequences of up to mf_ctx_stat("s2c_lds_max") k-mers build their sets in LDS, longer ones are
 * sorted; option "s2c_lds" = 0 sorts all of them (same result), "s2c_batch_pairs" bounds the k-mer occurrences sorted together. */
int  mf_comps_from_sequences_device(mf_ctx *ctx, const void *d_bases, const void *d_offsets, uint64_t n_seqs, uint64_t n_bases, int k,
                                    mf_comps **out);
/* File form: the files one at a time, in the order given, through the readers of mf_reads_load (records with N or a phred-0 base are
 * not there) -> components_bin (ConnectedComponent format) and stat_txt (may be NULL): "# component.no\tcomponent.size\tcomponent.weight"
 * and one line per component, numbered from 1 -- three columns, not the cutter's four.  *n_components (may be NULL) = components in
 * all, per_file[nfiles] (may be NULL) = components of each file. */
int  mf_seq2comp(mf_ctx *ctx, const char *const *files, int nfiles, int k, const char *components_bin, const char *stat_txt,
                 uint64_t *n_components, uint64_t *per_file);

/* component-paths (src/tools/ComponentPathsMain.java:82-206; mf_comppaths.hip): which stretches of the given sequences lie inside a
 * component.  Every selected component is looked at by itself: a path is a maximal run of consecutive positions of ONE sequence whose
 * canonical k-mers are all members of the component -- the sequence's own text [first, first + positions + k - 1), forward as given,
 * upper case.  Runs never join across two sequences; a sequence shorter than k has no positions; components that share k-mers
 * (seq2comp) each get the shared stretch, and each run goes on by itself where the other ends.  A path is kept when its length is at
 * least min_len; per component the first max_paths kept paths in encounter order (call of mf_paths_add, sequence, position) stay,
 * the rest are dropped; the kept ones are printed longest first, ties in encounter order, as Sequence.printSequences prints them:
 * ">i length=L av_weight=W min_weight=0 max_weight=0", i from 1, the bases in lines of 70; W = Math.round(weight / (double) size) =
 * floor(x + 0.5) of the component (an error where it does not fit a signed 32-bit integer; the reference's cast wraps around).  Every
 * position costs one lookup in an index over the members of the selected components, whatever their number (the reference: one hash
 * set per component and sequence).
 * Device form: mf_paths_create (the components must know their k: mf_comps_set_k; selection: component numbers from 1, NULL = all of
 * them; a number twice counts once, a number below 1 or above the count is an error; slot = place in the de-duplicated selection, in
 * the order given), mf_paths_add once per batch of sequences (the (bases, offsets) layout of mf_count_device; the batch may be
 * released afterwards: the kept paths' bases are copied into a store on the device), mf_paths_finish, then the counts and the text.
 * A thread of the marking kernel takes mf_ctx_stat("cp_run") consecutive positions of one sequence, a workgroup "cp_block".
 * Limits, each an error and never a truncated result: 1 <= k <= 31; fewer than 2^32 - 1 components, members, sequences per batch, runs
 * per batch, kept paths and max_paths; a sequence of fewer than 2^31 k-mers; fewer than 2^26 selected components that list one k-mer;
 * the store and the text must find room in HBM. */
typedef struct mf_paths mf_paths;
int  mf_paths_create(mf_ctx *ctx, mf_comps *c, const uint32_t *selection, uint64_t n_selection, int min_len, uint64_t max_paths,
                     mf_paths **out);
int  mf_paths_add(mf_paths *p, const void *d_bases, const void *d_offsets, uint64_t n_seqs, uint64_t n_bases);
int  mf_paths_finish(mf_paths *p);
void mf_paths_destroy(mf_paths *p);
/* any may be NULL: slots, kept paths and bytes of text over all slots (these two after mf_paths_finish), the most selected components
 * that list one k-mer (1: the selected components share no k-mer) */
int  mf_paths_stats(const mf_paths *p, uint64_t *n_slots, uint64_t *n_paths, uint64_t *n_bytes, uint64_t *max_listings);
/* per slot, arrays of n_slots entries, any may be NULL: the component's number, its kept paths, the bytes of its text, and whether
 * its count reached max_paths (the reference warns then: "keeping only first ... of them"); all but the first after mf_paths_finish */
int  mf_paths_slots(const mf_paths *p, uint32_t *component_no, uint64_t *n_paths, uint64_t *n_bytes, uint8_t *reached_cap);
/* the text of one slot, or of all slots one after the other (slot = -1): *n (may be NULL) = its bytes, whatever cap is; nothing is
 * written when cap is below it */
int  mf_paths_text(const mf_paths *p, int64_t slot, uint8_t *text, uint64_t cap, uint64_t *n);
/* out_dir/component-<no>.seq.fasta for every slot, an empty file where a component has no path; out_dir is made if it is not there.
 * *n_paths (may be NULL) = paths written */
int  mf_paths_write(const mf_paths *p, const char *out_dir, uint64_t *n_paths);
/* File form: components_bin + the sequence files, one resident at a time, in the order given, through the readers of mf_reads_load
 * (records with N or a phred-0 base are not there) -> out_dir.  selection as for mf_paths_create; the driver passes max_paths = 10^6
 * (MAX_PATHS_COUNT).  *n_components (may be NULL) = components in the file, *n_paths (may be NULL) = paths written. */
int  mf_component_paths(mf_ctx *ctx, const char *components_bin, int k, const char *const *files, int nfiles, const uint32_t *selection,
                        uint64_t n_selection, int min_len, uint64_t max_paths, const char *out_dir, uint64_t *n_components,
                        uint64_t *n_paths);
/* NO-REFERENCE EXTENSION, 32 <= k <= 63 (mf_wcomppaths.hip): component-paths on wide components, the semantics of the k <= 31 entry
 * points on 2k-bit k-mers word for word.  mf_paths_create_wide gives the SAME handle type (the components know their k): mf_paths_add,
 * mf_paths_finish, mf_paths_stats, mf_paths_slots, mf_paths_text, mf_paths_write and mf_paths_destroy work on it unchanged -- the handle
 * remembers its width, and only the marking kernel's look at a k-mer differs (a 128-bit roll, an index of 8-byte slots over the distinct
 * members as two word arrays).  The selection's rules, the errors and their texts, the rounding of weight / size, the cap and the limits
 * are those of mf_paths_create.  The file form loads through mf_wcomps_load (a file of another width or another k is its error), keeps
 * one sequence file resident at a time, and writes nothing before the components file has been accepted. */
int  mf_paths_create_wide(mf_ctx *ctx, mf_wcomps *c, const uint32_t *selection, uint64_t n_selection, int min_len, uint64_t max_paths,
                          mf_paths **out);
int  mf_component_paths_wide(mf_ctx *ctx, const char *components_bin, int k, const char *const *files, int nfiles,
                             const uint32_t *selection, uint64_t n_selection, int min_len, uint64_t max_paths, const char *out_dir,
                             uint64_t *n_components, uint64_t *n_paths);

/* ---- A9-A11 on several GPUs: every rank owns a shard of the cutter table ---------------------
 * The cutter table and the components step join ALL samples (ComponentCutterMain.runImpl,
 * src/tools/ComponentCutterMain.java:78-114; ComponentsBuilder.run, src/algo/ComponentsBuilder.java:58-153).
 * With one process per GPU, rank r owns the k-mers whose minimizer-partition hash starts with r
 * (world = power of two <= 64).  The library does the per-rank work on device buffers; the caller moves
 * the buffers between the ranks (torch.distributed over RCCL in metafast_amd/pipeline.py; any
 * all-to-all / all-gather will do).  All d_* pointers are device memory of the ctx's GPU.
 *
 *   table:    all-gather of the unitigs -> mf_count_device_shard                   (the shard)
 *   once:     mf_dcc_create; mf_dcc_queries + _fill -> all-to-all -> mf_dcc_answer -> all-to-all back
 *             -> mf_dcc_set_answers
 *   level t:  mf_dcc_level_local + mf_dcc_pairs_fill -> all-to-all -> mf_dcc_pairs_complete
 *             -> all-gather -> mf_dcc_merge + mf_dcc_stats_fill -> all-gather -> mf_dcc_classify
 *             (+ mf_dcc_kept_fill: every rank derives ALL kept components and the number of oversize ones from
 *             the gathered records -- nothing more to exchange; stop when there is no oversize component)
 *   end:      mf_dcc_minkeys -> all-reduce (min); mf_dcc_members + _fill -> all-gather -> mf_dcc_finish: the same mf_comps on every rank,
 *             identical to mf_cut_components_device on the merged table.                              */
/* rank's shard of the table of ALL the given sequences (every rank passes the same input, the unitigs of all samples):
 * the k-mers whose minimizer-partition hash starts with `rank`.  k >= 20. */
int  mf_count_device_shard(mf_ctx *ctx, const void *d_bases, const void *d_offsets, uint64_t n_seqs, uint64_t n_bases,
                           int k, int min_len, int rank, int world, mf_table **out);
/* base[world + 1]: global id of each rank's first vertex (prefix sums of the shard sizes; total < 2^32).
 * The shard must outlive the handle. */
int  mf_dcc_create(mf_ctx *ctx, mf_table *shard, int rank, int world, const uint32_t *base, mf_dcc **out);
void mf_dcc_destroy(mf_dcc *d);
/* the world size the handle was created with (the length of the per-rank count arrays below) */
int  mf_dcc_world(const mf_dcc *d);
/* neighbours in other shards: counts[world] (host), then the 16-byte queries grouped by owner */
int  mf_dcc_queries(mf_dcc *d, uint64_t *counts);
int  mf_dcc_queries_fill(mf_dcc *d, void *d_queries);
/* owner side: n queries -> n 16-byte answers, same order */
int  mf_dcc_answer(mf_dcc *d, const void *d_queries, uint64_t n, void *d_answers);
/* the answers to this rank's queries, in the order the queries were written */
int  mf_dcc_set_answers(mf_dcc *d, const void *d_answers, uint64_t n);
/* one threshold level (ComponentsBuilder.java:86-150): union-find inside the shard; counts[world] = 8-byte half
 * pairs (edges to fragments of HIGHER ranks) for each owner, then the half pairs themselves */
int  mf_dcc_level_local(mf_dcc *d, uint64_t *counts);
int  mf_dcc_pairs_fill(mf_dcc *d, void *d_pairs);
/* owner side, in place: half pairs -> (own fragment root, other fragment root), global ids.  An entry (0xFFFFFFFF, 0xFFFFFFFF) is no pair: it is
 * skipped here and by mf_dcc_merge, so that exchanges of a fixed capacity can pad their slices instead of announcing their sizes first. */
int  mf_dcc_pairs_complete(mf_dcc *d, void *d_pairs, uint64_t n);
/* ALL ranks' completed pairs -> global root of each own fragment; *n_stats = components this rank has vertices of, then
 * its share of each: 16-byte records (global root u32, size u32, weight u64) */
int  mf_dcc_merge(mf_dcc *d, const void *d_pairs, uint64_t n, uint64_t *n_stats);
int  mf_dcc_stats_fill(mf_dcc *d, void *d_stats);
/* ALL ranks' records in rank order (seg_first[world + 1], host: rank r's are [seg_first[r], seg_first[r + 1]); this rank's own
 * are [own_first, own_first + own_n)) -> classification of every own vertex at threshold thr (size window [b1, b2]);
 * n_kept / n_big: the kept / oversize components of the level over ALL ranks -- the same on every rank, which holds every
 * component's records --; then the kept ones' 16-byte records (root u32, size u32, weight u64), all of them, in no
 * particular order (sort by root for an order every rank agrees on) */
int  mf_dcc_classify(mf_dcc *d, const void *d_stats, uint64_t n, const uint64_t *seg_first, uint64_t own_first, uint64_t own_n,
                     int b1, int b2, int thr, uint64_t *n_kept, uint64_t *n_big);
int  mf_dcc_kept_fill(mf_dcc *d, void *d_kept);
/* members of kept components among this rank's k-mers, all levels: k-mers u64[n], global roots u32[n] */
int  mf_dcc_members(mf_dcc *d, uint64_t *n);
int  mf_dcc_members_fill(mf_dcc *d, void *d_kmers, void *d_roots);
/* smallest member k-mer of each kept component among this rank's k-mers (0x7FFF...F: none) -> d_min u64[n_kept];
 * the caller takes the minimum over the ranks (it breaks ties in the components' order) */
int  mf_dcc_minkeys(mf_dcc *d, const uint32_t *kept_root, uint64_t n_kept, void *d_min);
/* The same members grouped by component: 8 bytes per member on the wire -- k-mers u64[n_members], sorted by component, and
 * (root u32, count u32) runs [n_runs] -- instead of 12; mf_dcc_finish_grouped takes ALL ranks' k-mers (rank order) and runs
 * (rank order) */
int  mf_dcc_members_grouped(mf_dcc *d, uint64_t *n_members, uint64_t *n_runs);
int  mf_dcc_members_grouped_fill(mf_dcc *d, void *d_kmers, void *d_runs);
int  mf_dcc_finish_grouped(mf_dcc *d, const void *d_kmers, uint64_t n_members, const void *d_runs, uint64_t n_runs,
                           const uint32_t *kept_root, const uint32_t *kept_size, const int64_t *kept_weight,
                           const int32_t *kept_thr, const uint64_t *kept_minkey, uint64_t n_kept, mf_comps **out);
/* ALL ranks' members + all levels' kept components (host arrays) -> components, ordered as above */
int  mf_dcc_finish(mf_dcc *d, const void *d_kmers, const void *d_roots, uint64_t n_members, const uint32_t *kept_root,
                   const uint32_t *kept_size, const int64_t *kept_weight, const int32_t *kept_thr,
                   const uint64_t *kept_minkey, uint64_t n_kept, mf_comps **out);

/* ---- the exchanges of the multi-GPU path, behind this boundary (round 6; mf_comm.hip) ----------------------
 * The reference is one JVM (ComponentCutterMain.runImpl, src/tools/ComponentCutterMain.java:78-114, joins all libraries in one map; IOUtils.run,
 * src/io/IOUtils.java:846-862, waits for its threads on a latch).  With a library per GPU the join is an exchange.  A communicator gives every rank
 * three primitives on buffers in HBM -- a gather of a few host integers, an all-gather and an all-to-all of slices whose sizes all ranks know --
 * over one of three transports, and the calls below run the path's exchange steps on it (on the context's stream and workspace):
 *   local     the ranks are THREADS of one process, a context each (metafast.sh --devices a,b,...): a rank copies its slice straight into every
 *             peer's receive buffer (peer access over xGMI; a device-to-device copy where two ranks share a GPU) -- the direct all-gather of a
 *             fully connected xGMI node, no ring;
 *   rccl      one process per GPU: librccl looked up at run time; slices travel as grouped ncclSend / ncclRecv pairs;
 *   external  the host's own primitives (MPI under a Java host; torch.distributed in this repository's tests).
 * One calling thread per communicator; every rank makes the same calls in the same order.  MF_ERR_TOGETHER: some rank could not do its part
 * and ALL ranks return this from the same call (mf_last_error names the ranks) -- the caller may take another route on all of them, e.g.
 * mf_comm_gather_sequences + mf_count_device + mf_cut_components_device everywhere. */
#define MF_ERR_TOGETHER (-2)
typedef struct mf_comm mf_comm;
/* n communicators for n threads of this process, out[r] for the thread that drives ctxs[r] */
int  mf_comm_create_local(mf_ctx *const *ctxs, int n, mf_comm **out);
/* one process per GPU: rank 0 makes an id (128 bytes) and hands it to the others by the host's own means; all ranks then create together */
int  mf_comm_rccl_id(void *id128);
int  mf_comm_create_rccl(mf_ctx *ctx, const void *id128, int rank, int world, mf_comm **out);
/* the host's primitives; all sizes in bytes, known to every rank; device pointers of the context's GPU; < 0 = failure.  The library has
 * synchronised its stream before a call and reads the result on that stream after it: the primitive returns when the data has arrived.
 *   gather_ints(user, vals[n], n, out[world * n])                       rank r's vals at out[r * n]
 *   all_gather(user, d_send, d_recv, bytes[world])                      rank r's bytes[r] bytes at d_recv + sum(bytes[:r]), on every rank
 *   all_to_all(user, d_send, send_bytes[world], d_recv, recv_bytes[world])   d_send grouped by destination, d_recv by source */
typedef struct mf_comm_ops {
    int (*gather_ints)(void *user, const int64_t *vals, int n, int64_t *out);
    int (*all_gather)(void *user, const void *d_send, void *d_recv, const uint64_t *bytes);
    int (*all_to_all)(void *user, const void *d_send, const uint64_t *send_bytes, void *d_recv, const uint64_t *recv_bytes);
} mf_comm_ops;
int  mf_comm_create_external(mf_ctx *ctx, int rank, int world, const mf_comm_ops *ops, void *user, mf_comm **out);
void mf_comm_destroy(mf_comm *c);
int  mf_comm_rank(const mf_comm *c);
int  mf_comm_world(const mf_comm *c);
const char *mf_comm_kind(const mf_comm *c);                  /* "local" / "rccl" / "external" */
/* "collectives", "bytes_in" (received), "us" (host time inside the exchanges) since the last reset; < 0: unknown name */
int64_t mf_comm_stat(const mf_comm *c, const char *name);
int  mf_comm_reset_stats(mf_comm *c);
/* the primitives themselves (tests; hosts that have more to exchange) */
int  mf_comm_gather_ints(mf_comm *c, const int64_t *vals, int n, int64_t *out);
int  mf_comm_all_gather(mf_comm *c, const void *d_send, void *d_recv, const uint64_t *bytes_per_rank);
int  mf_comm_all_to_all(mf_comm *c, const void *d_send, const uint64_t *send_bytes, void *d_recv, const uint64_t *recv_bytes);
/* Every rank's sequences (its libraries' unitigs: the layout of mf_seqs_device_view / mf_reads_device_view) on every rank, rank after rank:
 * IOUtils.loadReads over the .seq.fasta files of ALL libraries (src/tools/ComponentCutterMain.java:81).  The result is read with
 * mf_reads_stats / mf_reads_device_view and freed with mf_reads_destroy. */
int  mf_comm_gather_sequences(mf_comm *c, const void *d_bases, const void *d_offsets, uint64_t n_seqs, uint64_t n_bases, mf_reads **all);
/* One call = ComponentCutterMain.runImpl :81-108 over all ranks: the sequences are gathered, every rank counts the k-mers it owns
 * (mf_count_device_shard) and the exchange protocol of the sharded cutter above (mf_dcc_*) runs inside: the SAME components on every rank,
 * identical to mf_cut_components_device on the table of all sequences.  world = a power of two <= 64, 20 <= k <= 31. */
int  mf_cut_components_sharded(mf_comm *c, const void *d_bases, const void *d_offsets, uint64_t n_seqs, uint64_t n_bases, int k, int min_len,
                               int b1, int b2, mf_comps **out);
/* File form, every rank: its libraries' .seq.fasta files in (nfiles may be 0), rank 0 writes components.bin and the components-stat file
 * (ComponentCutterMain.runImpl :92-108), every rank keeps the components for the features step of its own libraries (option file_cache). */
int  mf_cut_components_sharded_files(mf_comm *c, const char *const *seq_files, int nfiles, int k, int min_len, int b1, int b2,
                                     const char *components_bin, const char *stat_txt, uint64_t *n_comp);
/* ... on a shard the caller has counted (NULL: this rank has none -- all ranks return MF_ERR_TOGETHER); info (may be NULL): [0] threshold levels,
 * [1] this rank's neighbour queries, [2] members over all ranks, [3] vertices over all ranks */
int  mf_cut_components_of_shard(mf_comm *c, mf_table *shard, int k, int b1, int b2, mf_comps **out, uint64_t *info);
/* The feature vectors of all ranks' samples, rank after rank, on every rank (the rows DistanceMatrixCalculatorMain reads back from the .vec files,
 * src/tools/DistanceMatrixCalculatorMain.java:125-138): rows = this rank's int64[n_rows][n_comp] (host); all_rows (host; NULL: only the count)
 * takes capacity_rows rows. */
int  mf_features_allgather(mf_comm *c, const int64_t *rows, uint64_t n_rows, uint64_t n_comp, int64_t *all_rows, uint64_t capacity_rows,
                           uint64_t *n_all_rows);

/* ---- A12  features ------------------------------------------------------------------ */
/* replaces FeaturesCalculatorMain: hm.put(kmer,0) for component k-mers (:97-103), presence pass
 * over the sample's records (IOUtils.calculatePresenceForKmers, src/io/IOUtils.java:577-597) and
 * buildAndPrintVector (:169-236): vec[c] = sum of counts > threshold, breadth[c] = found/size. */
int  mf_features_device(mf_ctx *ctx, mf_comps *c, const mf_table *sample, int threshold,
                        int64_t *vec, double *breadth);
/* File form: components.bin + <name>.kmers.bin -> <name>.vec / <name>.breadth (either may be NULL) */
int  mf_features(mf_ctx *ctx, const char *components_bin, const char *kmers_bin, int k, int threshold,
                 const char *vec_path, const char *breadth_path);

/* --use-reads-for-calculating-features (FeaturesCalculatorMain.java:117-131 + IOUtils.calculatePresenceForReads /
 * ReadsPresenceWorker, src/io/IOUtils.java:806-834): the features of a sample straight from its READS -- every k-mer of
 * every read that is a component k-mer adds 1 (64-bit counts, no saturation; reads shorter than k give nothing), then
 * vec[c] = sum of the counts > threshold, breadth[c] = found / size.  Device form: reads resident in HBM (layout of
 * mf_count_device); file form: FASTA / FASTQ (.gz) files of ONE library, output as mf_features. */
int mf_features_reads_device(mf_ctx *ctx, mf_comps *c, const void *d_bases, const void *d_offsets, uint64_t n_reads,
                             uint64_t n_bases, int k, int threshold, int64_t *vec, double *breadth);
int mf_features_reads(mf_ctx *ctx, const char *components_bin, const char *const *files, int nfiles, int k, int threshold,
                      const char *vec_path, const char *breadth_path);

/* --selected (FeaturesCalculatorMain.java:55-57 the parameter, :113-116 selected = IOUtils.loadKmers(selectedKmers, 0, ...),
 * :193-203 its use in buildAndPrintVector): with a table of selected k-mers only the component k-mers with
 * selected.getWithZero(kmer) > 0 enter vec[c], kmersFound AND kmersCount, so breadth[c] = found / (selected k-mers of c) and a
 * component without a selected k-mer gets 0.0 / 0.0 = NaN ("NaN" in the .breadth file, Double.toString).  `selected` is a table of
 * the same context, e.g. mf_table_load_kmers(ctx, files, n, 0, k, &selected); NULL = no selection (the calls above). */
int mf_features_device_selected(mf_ctx *ctx, mf_comps *c, const mf_table *sample, mf_table *selected, int threshold,
                                int64_t *vec, double *breadth);
int mf_features_selected(mf_ctx *ctx, const char *components_bin, const char *kmers_bin, int k, int threshold, mf_table *selected,
                         const char *vec_path, const char *breadth_path);
int mf_features_reads_device_selected(mf_ctx *ctx, mf_comps *c, const void *d_bases, const void *d_offsets, uint64_t n_reads,
                                      uint64_t n_bases, int k, mf_table *selected, int threshold, int64_t *vec, double *breadth);
int mf_features_reads_selected(mf_ctx *ctx, const char *components_bin, const char *const *files, int nfiles, int k, int threshold,
                               mf_table *selected, const char *vec_path, const char *breadth_path);

/* ---- group comparison: the multi-sample join (pipelines 3 and 5 of the reference's Pipelines.md; mf_stats.hip on mf_join.hip) ------
 * Each k-mer of the union of N samples gets its row of per-sample presence / counts and a decision is made over the row.  Keys are the
 * 64-bit values of the tables / files (below 2^62, as for any k <= 31; a larger one is an error); result tables have k = 31 and come in
 * ascending key order.  Option "stats_slices" (mf_ctx_set_option) forces the number of hash slices of the key space (0: as many as
 * free HBM asks for); the result does not depend on it.
 *
 * StatsKmersFinder.runImpl (src/tools/StatsKmersFinder.java:89-297), samples numbered A first, then B; b = --maximal-bad-frequence:
 * sample j holds x iff its count of x is > b; chi-squared test on (n1A, n1B) at p_chi2, then (p_mw > 0) Mann-Whitney on
 * v_j = (c_j * M) / F_j (F_j = sum of sample j's counts, M = sum of all F_j / N), the kept k-mers to group A or B with
 * (short)(int)mean.  chi = the chi-squared survivors with value 1.  counters[9] (MF_STATS_COUNTERS): k-mers, scarce, present in all,
 * unique, rejected by chi-squared, rejected by Mann-Whitney, group A, group B, unique left (the reference's log lines :284-296).
 * 1 <= |A|, 1 <= |B|, |A| + |B| <= 1024. */
#define MF_STATS_COUNTERS 9
int mf_stats_kmers_tables(mf_ctx *ctx, mf_table *const *a, int na, mf_table *const *b, int nb, int max_bad, double p_chi2, double p_mw,
                          mf_table **chi, mf_table **group_a, mf_table **group_b, uint64_t *counters);
/* File form (the CLI's): .kmers.bin files of the two groups (duplicate records of a k-mer in one file: presence = some record > b, count =
 * saturating sum, F_j = sum of all records > 0, IOUtils.loadKmersFreq) -> <out_dir>/filtered_chisquared.kmers.bin + .stat.txt,
 * filtered_groupA.kmers.bin, filtered_groupB.kmers.bin; counters may be NULL. */
int mf_stats_kmers(mf_ctx *ctx, const char *const *a_files, int na, const char *const *b_files, int nb, int max_bad, double p_chi2, double p_mw,
                   const char *out_dir, uint64_t *counters);
/* KmersSamplesCounter.runImpl (src/tools/KmersSamplesCounter.java:69-140): n(x) = number of samples whose count of x is > max_bad, for
 * every x with n(x) > 0; at most 32767 samples. */
int mf_kmers_samples_count_tables(mf_ctx *ctx, mf_table *const *t, int n, int max_bad, mf_table **out);
/* File form: -> kmers_bin (records (x, n(x))) and stat_txt (histogram of n, may be NULL); *n_kmers (may be NULL) = records written */
int mf_kmers_samples_count(mf_ctx *ctx, const char *const *files, int n, int max_bad, int k, const char *kmers_bin, const char *stat_txt,
                           uint64_t *n_kmers);
/* StatsKmers3GroupsFinder.runImpl (src/tools/StatsKmers3GroupsFinder.java:92-377), samples numbered A, then B, then C: as
 * mf_stats_kmers_tables with the three-group chi-squared test on (n1A, n1B, n1C) (2 degrees of freedom; the threshold is the closed form
 * -2 ln(p_chi2) where the reference runs a numeric solver) and, for p_mw > 0, three Mann-Whitney tests (A, B), (B, C), (A, C): a k-mer is
 * kept when any of them gives p < p_mw.  A kept k-mer goes to A if mean(A) is greater than both other means, else to B if mean(B) is,
 * else to C.  counters[10] (MF_STATS3_COUNTERS): k-mers, scarce, present in all, unique (present in one group only), rejected by
 * chi-squared, rejected by Mann-Whitney, group A, group B, group C, unique left (the reference's log lines :329-339).
 * 1 <= |A|, |B|, |C|, |A| + |B| + |C| <= 1024. */
#define MF_STATS3_COUNTERS 10
int mf_stats_kmers3_tables(mf_ctx *ctx, mf_table *const *a, int na, mf_table *const *b, int nb, mf_table *const *c, int nc, int max_bad,
                           double p_chi2, double p_mw, mf_table **chi, mf_table **group_a, mf_table **group_b, mf_table **group_c,
                           uint64_t *counters);
/* File form: as mf_stats_kmers -> <out_dir>/filtered_chisquared.kmers.bin + .stat.txt, filtered_group{A,B,C}.kmers.bin */
int mf_stats_kmers3(mf_ctx *ctx, const char *const *a_files, int na, const char *const *b_files, int nb, const char *const *c_files, int nc,
                    int max_bad, double p_chi2, double p_mw, const char *out_dir, uint64_t *counters);
/* SpecificKmersFinder.runImpl (src/tools/SpecificKmersFinder.java:65-245), samples numbered A first, then B; every sample is read at
 * threshold 0 and the decision is made on its RAW counts c_j(x) (absent = 0).  Per k-mer x of the union, in the reference's order:
 * unique (held by one group only) is counted; x is scarce when the count of the FIRST sample that holds it is <= ceil(N * 0.05) -- a
 * count against a bound made from the number of samples, reproduced as it is --; else the two-group chi-squared test on (n1A, n1B) at
 * p_chi2 (1 degree of freedom), which an x that EVERY sample holds passes whatever its statistic; then (p_mw > 0) Mann-Whitney on the raw
 * counts, x is dropped when p > p_mw (kept at p == p_mw); the kept go to A with (short)(int)mean(A) when mean(A) > mean(B), else to B
 * with (short)(int)mean(B).  No chi-squared list is written.  counters[MF_SPECIFIC_COUNTERS], indexed by the enum below (the log lines
 * :202-216).  1 <= |A|, 1 <= |B|, |A| + |B| <= 1024; a key >= 2^62 is an error. */
#define MF_SPECIFIC_COUNTERS 8
enum { MF_SPECIFIC_TOTAL = 0, MF_SPECIFIC_UNIQUE = 1, MF_SPECIFIC_SCARCE = 2, MF_SPECIFIC_SKIP_CHI2 = 3, MF_SPECIFIC_SKIP_MW = 4,
       MF_SPECIFIC_UNIQUE_LEFT = 5, MF_SPECIFIC_GROUP_A = 6, MF_SPECIFIC_GROUP_B = 7 };
int mf_specific_kmers_tables(mf_ctx *ctx, mf_table *const *a, int na, mf_table *const *b, int nb, double p_chi2, double p_mw,
                             mf_table **group_a, mf_table **group_b, uint64_t *counters);
/* File form: each file loaded like IOUtils.loadKmers([file], 0) -> <out_dir>/filtered_groupA.kmers.bin, filtered_groupB.kmers.bin in
 * ascending key order (the reference's order is its hash map's); counters may be NULL. */
int mf_specific_kmers(mf_ctx *ctx, const char *const *a_files, int na, const char *const *b_files, int nb, double p_chi2, double p_mw,
                      const char *out_dir, uint64_t *counters);
/* SpecificKmers3GroupsFinder.runImpl (src/tools/SpecificKmers3GroupsFinder.java:70-280): mf_stats_kmers3_tables at threshold 0 with these
 * differences -- the chi-squared threshold is the quantile of 1 degree of freedom, not 2; no chi-squared list; F_j = the sum of sample
 * j's (bounded) counts and M = (sum of all F_j) / N in integer arithmetic; v_j = (c_j * M) / F_j for a sample that holds x and 0 for one
 * that does not (no NaN from an empty sample); unique left = kept and held by one group only.  counters[MF_SPECIFIC3_COUNTERS] in the
 * order of MF_STATS3_COUNTERS. */
#define MF_SPECIFIC3_COUNTERS 10
int mf_specific_kmers3_tables(mf_ctx *ctx, mf_table *const *a, int na, mf_table *const *b, int nb, mf_table *const *c, int nc, double p_chi2,
                              double p_mw, mf_table **group_a, mf_table **group_b, mf_table **group_c, uint64_t *counters);
/* File form -> <out_dir>/filtered_group{A,B,C}.kmers.bin */
int mf_specific_kmers3(mf_ctx *ctx, const char *const *a_files, int na, const char *const *b_files, int nb, const char *const *c_files, int nc,
                       double p_chi2, double p_mw, const char *out_dir, uint64_t *counters);
/* KmersGroupedSamplesCounter.runImpl (src/tools/KmersGroupedSamplesCounter.java:82-190): for every k-mer x of `kmers` the number of
 * tables of each group (CD, UC, nonIBD; a group may be empty, at most 1022 tables in one) whose count of x is > max_bad.  *n = the
 * entries of `kmers`, whatever `cap` is; with cap >= *n, keys[0 .. *n) = the k-mers in ASCENDING order (the reference's order is its hash
 * map's) and counts[i] = cd << 32 | uc << 16 | nonibd, the packing of mf_kmers_multiple_filters_tables; with a smaller cap nothing is
 * written (cap = 0 with NULL arrays asks for the number alone).  A key >= 2^62 in any table is an error. */
int mf_kmers_grouped_count_tables(mf_ctx *ctx, mf_table *kmers, mf_table *const *cd, int n_cd, mf_table *const *uc, int n_uc,
                                  mf_table *const *nonibd, int n_nonibd, int max_bad, uint64_t *keys, uint64_t *counts, uint64_t cap,
                                  uint64_t *n);
/* File form: kmers = IOUtils.loadKmers(kmers_files, 0) (the k-mers with some record > 0; one listed more than once comes once), every group
 * file loaded at max_bad -> out_txt: the line "Kmer\tcd_count\tuc_count\tnonibd_count", then one line per k-mer in ascending key order,
 * the k-mer as ShortKmer.toString prints it at this k and the three counts.  1 <= k <= 31; *n_kmers (may be NULL) = lines written. */
int mf_kmers_grouped_count(mf_ctx *ctx, const char *const *kmers_files, int n_kmers_files, const char *const *cd_files, int n_cd,
                           const char *const *uc_files, int n_uc, const char *const *nonibd_files, int n_nonibd, int max_bad, int k,
                           const char *out_txt, uint64_t *n_kmers);

/* KmersPerSampleCounter.runImpl (src/tools/KmersPerSampleCounter.java:56-157; mf_kps.hip): the k-mer x sample abundance table of a cohort.
 * n(x) = the number of samples j >= 1 whose count of x is > max_bad -- sample 0 is NOT counted (count_first = 0, the reference: its first
 * file's map is the accumulator and is zeroed before it is iterated, :82-96; count_first != 0 counts it like the others); a k-mer that
 * only sample 0 holds has n = 0 and is still a candidate.  Selected: n(x) >= thresh = n * percent / 100 in Java int arithmetic
 * (truncation toward zero; percent may be negative or above 100), so thresh <= 0 selects the whole union.  The result holds the M
 * selected k-mers in ASCENDING order (the reference's order is its hash map's), their n(x), and the n x M row-major matrix of the
 * samples' counts (0 = absent or count <= max_bad).  Errors: n < 1 or n > 32767, a key >= 2^62, 2^32 - 1 or more selected k-mers, more
 * than 2^32 - 1 union k-mers in one hash slice, and a matrix of n x M x 2 bytes that does not fit the free device memory (select fewer
 * k-mers with a higher percent, or use the file form). */
int  mf_kmers_per_sample_tables(mf_ctx *ctx, mf_table *const *tables, int n, int max_bad, int percent, int count_first, mf_kps **out);
void mf_kps_destroy(mf_kps *r);
int  mf_kps_stats(const mf_kps *r, uint64_t *n_kmers, int *n_samples);                 /* either may be NULL */
/* device pointers, valid until the destroy: uint64 keys[M], uint16 n(x)[M], uint16 matrix[n][M]; any may be NULL */
int  mf_kps_device_view(const mf_kps *r, const void **d_keys, const void **d_nsamples, const void **d_matrix);
/* host copies: keys[M], nsamples[M], matrix[n * M]; any may be NULL */
int  mf_kps_export(const mf_kps *r, uint64_t *keys, uint16_t *nsamples, uint16_t *matrix);
/* The text of the reference's file, formatted on the device: the first line without its newline ("\t" + ShortKmer.toString at this k per
 * selected k-mer, M * (k + 1) bytes) and one sample's line without name and newline ("\t" + decimal count per selected k-mer, at most
 * 6 M bytes).  *n = the bytes of the text, whatever cap is; nothing is written when cap is below it. */
int  mf_kps_header_text(const mf_kps *r, int k, uint8_t *text, uint64_t cap, uint64_t *n);
int  mf_kps_row_text(const mf_kps *r, int sample, uint8_t *text, uint64_t cap, uint64_t *n);
/* File form, max_bad = 0 (every load is IOUtils.loadKmers(file, 0): records with a value > 0, duplicate records of a k-mer summed with
 * saturation) -> out_txt (selected_kmers_<percent>.txt): the line of k-mers, then one line per file in argument order -- the file's name
 * with every ".kmers.bin" removed, then "\t" + count per selected k-mer.  Streams: a sample is loaded, gathered, formatted and written
 * before the next, the matrix is never resident and every file is read twice.  1 <= k <= 31; *n_kmers (may be NULL) = M. */
int  mf_kmers_per_sample(mf_ctx *ctx, const char *const *files, int n, int k, int percent, int count_first, const char *out_txt,
                         uint64_t *n_kmers);

/* ---- set operations over cohorts on the same join (pipelines 2 and 3 of the reference's Pipelines.md; mf_kmersets.hip) -------------
 * Keys, slices and result tables as above; b = max_bad >= 0 (a negative one is an error); the counts of the tables are 1 .. MF_MAX_COUNT.
 *
 * UniqueKmersMultipleSamplesFinder.runImpl (src/tools/UniqueKmersMultipleSamplesFinder.java:84-185): over the inputs' entries with
 * count > b, cnt(x) = number of inputs that hold x and sum(x) = the sum of their counts WRAPPED to a Java short ((short)(a + b), not a
 * saturating add: 3 x 20000 -> -5536); an x that a filter table holds with count > b while sum(x) > b is knocked out (sum(x) := 0);
 * *n_union = distinct keys of the inputs, knocked-out ones included.  For i = min_samples, min_samples + 1, ... max_samples: out[i -
 * min_samples] = the records (x, sum(x)) with sum(x) > b and cnt(x) >= i, counts[i - min_samples] = their number; the list ends with the
 * first empty table (included).  *n_out = tables returned (each to be destroyed by the caller); out and counts must hold
 * min(max_samples, max(min_samples, n_inputs + 1)) - min_samples + 1 entries.  Errors: min_samples > max_samples (the reference's
 * message), more than 32767 inputs (cnt is a Java short), a key >= 2^62 in an input or a filter table (every filter table is read,
 * whatever the inputs hold), more than 2^32 - 1 union k-mers in one hash slice (raise "stats_slices"). */
int mf_unique_kmers_multi_tables(mf_ctx *ctx, mf_table *const *inputs, int n_inputs, mf_table *const *filters, int n_filters, int max_bad,
                                 int min_samples, int max_samples, mf_table **out, int *n_out, uint64_t *n_union, uint64_t *counts);
/* File form: .kmers.bin files, each loaded like IOUtils.loadKmers(file, b) (duplicate records of a k-mer in one file: saturating sum of
 * those > b) -> <out_dir>/filtered_<i>.kmers.bin for the i above */
int mf_unique_kmers_multi(mf_ctx *ctx, const char *const *in_files, int n_inputs, const char *const *filter_files, int n_filters, int max_bad,
                          int k, int min_samples, int max_samples, const char *out_dir, int *n_out, uint64_t *n_union, uint64_t *counts);
/* UniqueKmersFinder.runImpl (src/tools/UniqueKmersFinder.java:73-144): the inputs are POOLED into one map -- pooled(x) = the sum of the
 * inputs' counts of x that are > b, bounded at 32767 (IOUtils.loadKmers over all files: the threshold is per record, the add saturates);
 * an x that a filter table holds with count > b is zeroed.  *out = the records (x, pooled(x)) that are left, *n_pooled = the size of the
 * pooled map, zeroed k-mers included (hm.size()).  b >= 0; at most 32767 inputs; a key >= 2^62 in any table is an error. */
int mf_unique_kmers_tables(mf_ctx *ctx, mf_table *const *inputs, int n_inputs, mf_table *const *filters, int n_filters, int max_bad,
                           mf_table **out, uint64_t *n_pooled);
/* File form -> kmers_bin and stat_txt (may be NULL: IOUtils.printKmers of the pooled map at b -- the histogram counts the zeroed k-mers
 * under 0); *n_good (may be NULL) = records written, *n_pooled may be NULL.  1 <= k <= 31. */
int mf_unique_kmers(mf_ctx *ctx, const char *const *in_files, int n_inputs, const char *const *filter_files, int n_filters, int max_bad, int k,
                    const char *kmers_bin, const char *stat_txt, uint64_t *n_pooled, uint64_t *n_good);
/* IOUtils.MultipleFiltersAndPrintKmers (src/io/IOUtils.java:125-213) for one input table: every entry (x, v) with v > b gets the triple
 * (cd(x), uc(x), nonibd(x)) of the three filter tables' counts (entries with count > 0; absent = 0); *kept = the entries with a non-zero
 * triple.  The distinct triples, packed cd << 32 | uc << 16 | nonibd, come in ascending order (Triple.compareTo) with the number of
 * entries of each.  *n_triples = the number of ALL distinct triples (<= entries of `table`), whatever `cap` is; only the first
 * min(cap, *n_triples) are written to triples / triple_counts, so a caller that finds *n_triples > cap calls again with a larger cap
 * (cap = entries of `table` always suffices; cap = 0 with NULL arrays asks for the number alone).  found_kept[2] = entries with
 * v > b, entries kept.  Errors: a key >= 2^62 in any of the four tables, an input of more than 2^32 - 1 entries. */
int mf_kmers_multiple_filters_tables(mf_ctx *ctx, mf_table *table, mf_table *cd, mf_table *uc, mf_table *nonibd, int max_bad, mf_table **kept,
                                     uint64_t *triples, uint64_t *triple_counts, uint64_t cap, uint64_t *n_triples, uint64_t *found_kept);
/* File form (KmersMultipleFilters.runImpl, src/tools/KmersMultipleFilters.java:77-133): the three filter tables are
 * IOUtils.loadKmers(list, 0) of their file lists (a list may be empty), built once; input j (loaded at threshold b) ->
 * out_kmers[j] and the triples' histogram out_stats[j] (out_stats or an entry of it may be NULL); found_kept (may be NULL) gets
 * 2 * n_inputs values: found and kept of each input. */
int mf_kmers_multiple_filters(mf_ctx *ctx, const char *const *in_files, int n_inputs, const char *const *cd_files, int n_cd,
                              const char *const *uc_files, int n_uc, const char *const *nonibd_files, int n_nonibd, int max_bad, int k,
                              const char *const *out_kmers, const char *const *out_stats, uint64_t *found_kept);

/* ---- colored metagenomic features (pipeline 4 of the reference's Pipelines.md; mf_color.hip, mf_ctable.hip, mf_cc.hip) ------------
 * mf_ctable: k-mer -> 64-bit value (BigLong2LongHashMap), ascending keys, resident in HBM.  The values of kmers-color are three 20-bit
 * fields, class c in bits 20c .. 20c + 19. */
typedef struct mf_ctable mf_ctable;
/* host pairs in any order; the values of a key that comes more than once are added, saturating at 2^63 - 1; a value with the sign bit
 * set and a key that does not fit 2k bits are errors */
int  mf_ctable_from_host(mf_ctx *ctx, const uint64_t *keys, const uint64_t *values, uint64_t n, int k, mf_ctable **out);
/* IOUtils.loadLongKmers (src/io/IOUtils.java:260-281): files of 16-byte big-endian (k-mer, value) records; a record is kept iff its
 * value is > min_value (one with the sign bit set never is); the kept values of a key are added, saturating at 2^63 - 1 */
int  mf_ctable_load(mf_ctx *ctx, const char *const *files, int nfiles, int64_t min_value, int k, mf_ctable **out);
int  mf_ctable_stats(const mf_ctable *t, uint64_t *n, int *k);
/* keys[n], values[n] in ascending key order; cap = 0: *n only */
int  mf_ctable_export(const mf_ctable *t, uint64_t *keys, uint64_t *values, uint64_t cap, uint64_t *n);
/* IOUtils.printKmers of a long map at threshold 0 (src/tools/ColorKmersMain.java:126-135): the 16-byte records in ascending key order and
 * the .stat.txt over the distinct values (may be NULL); *n_written may be NULL */
int  mf_ctable_write(const mf_ctable *t, const char *kmers_bin, const char *stat_txt, uint64_t *n_written);
void mf_ctable_destroy(mf_ctable *t);
/* ColorKmersMain.runImpl (src/tools/ColorKmersMain.java:89-136, src/algo/ColoredKmerOperations.java): every sample whose count of x is
 * > max_bad adds 1 (count_values != 0: its count) to the field of its class in x's packed value, each add saturating at 2^20 - 1.
 * classes[n] in {0, 1, 2}; at most 1024 samples; keys below 2^62. */
int  mf_kmers_color_tables(mf_ctx *ctx, mf_table *const *t, const int *classes, int n, int max_bad, int count_values, mf_ctable **out);
/* File form: each .kmers.bin loaded like IOUtils.loadKmers([file], max_bad) -> kmers_bin + stat_txt (may be NULL) */
int  mf_kmers_color(mf_ctx *ctx, const char *const *files, const int *classes, int n, int max_bad, int count_values, int k,
                    const char *kmers_bin, const char *stat_txt, uint64_t *n_kmers);
/* ColoredComponentsBuilder (src/algo/ColoredComponentsBuilder.java:85-124, 250-280), default and --separate modes: colour of a value =
 * the first c in 0, 1, 2 with (double)f_c / (f_0 + f_1 + f_2) >= perc, else neutral (ColoredKmerOperations.getColor).  separate != 0:
 * for each colour the connected components (8 neighbours, src/algo/KmerOperations.java:9-26) of the k-mers of that colour; else the
 * components of (colour c or neutral) that hold a k-mer of colour c, neutral k-mers included.  out[n_groups]: one mf_comps per colour
 * (size = weight = k-mers; ordered by size descending, then smallest k-mer; k-mers ascending inside), counts[n_groups] (may be NULL)
 * their numbers.  A k-mer whose colour is >= n_groups is an error. */
int  mf_colored_components_device(mf_ctx *ctx, const mf_ctable *t, int k, int n_groups, int separate, double perc, mf_comps **out,
                                  uint64_t *counts);
/* File form (ColoredComponentMain.runImpl, src/tools/ColoredComponentMain.java:83-119; the reference passes k as min_value) ->
 * <out_dir>/components_color_<c>.bin for c < n_groups and stat_txt (may be NULL) */
int  mf_colored_components(mf_ctx *ctx, const char *const *files, int nfiles, int k, int64_t min_value, int n_groups, int separate,
                           double perc, const char *out_dir, const char *stat_txt, uint64_t *counts);

/* ---- NO-REFERENCE EXTENSION: pipeline 4 for 32 <= k <= 63 (mf_wcolor.hip, mf_wgraph.hip) ------------------------------
 * mf_wctable: 2k-bit k-mer (high word, low word) -> 64-bit value, ascending, resident in HBM.  Its file is the wide colored_kmers.kmers.bin:
 * headerless, 24-byte big-endian records -- int64 high word, int64 low word, int64 value.  The calls mirror mf_ctable_*; a call of either
 * family refuses a handle of the other by name (both handles begin with their context and k, and k tells them apart; the build asserts that
 * layout).  The two destroy calls return nothing and cannot refuse: given a handle of the other family, mf_ctable_destroy and
 * mf_wctable_destroy touch nothing of it and return -- the handle stays valid and is still to be released by its own family's call. */
typedef struct mf_wctable mf_wctable;
/* [mf_ctable_from_host] host triples in any order; the values of a k-mer that comes more than once are added, saturating at 2^63 - 1; a value
 * with the sign bit set and a k-mer that does not fit 2k bits are errors.  32 <= k <= 63 */
int  mf_wctable_from_host(mf_ctx *ctx, const uint64_t *hi, const uint64_t *lo, const uint64_t *values, uint64_t n, int k, mf_wctable **out);
/* [mf_ctable_load] files of 24-byte records, parsed and merged on the host; a record is kept iff its value is > min_value (signed: one with
 * the sign bit set never is); the kept values of a k-mer are added, saturating at 2^63 - 1.  A file whose size is no multiple of 24 is an
 * error that names the file and the record size, a k-mer that does not fit 2k bits one that names the file. */
int  mf_wctable_load(mf_ctx *ctx, const char *const *files, int nfiles, int64_t min_value, int k, mf_wctable **out);
int  mf_wctable_stats(const mf_wctable *t, uint64_t *n, int *k);
/* hi[n], lo[n], values[n] in ascending order of the k-mer; cap = 0: *n only */
int  mf_wctable_export(const mf_wctable *t, uint64_t *hi, uint64_t *lo, uint64_t *values, uint64_t cap, uint64_t *n);
/* [mf_ctable_write] the 24-byte records with value > 0 in ascending order and the .stat.txt over the distinct values in the narrow writer's
 * format (may be NULL); *n_written may be NULL */
int  mf_wctable_write(const mf_wctable *t, const char *kmers_bin, const char *stat_txt, uint64_t *n_written);
void mf_wctable_destroy(mf_wctable *t);
/* [mf_kmers_color_tables] the same definition on (high, low) keys: every sample whose count of x is > max_bad adds 1 (count_values != 0: its
 * count) to the 20-bit field of its class in x's packed value, each add clamped at 2^20 - 1; no limit on the key.  Per slice of the key range
 * (option "stats_slices" forces the number; the result is the same for every number) the wide join's union lists the slice's distinct k-mers,
 * then every sample is read a second time and each entry adds into its k-mer's row, found by binary search, with a 64-bit compare-and-swap.
 * Errors, decided on the host before any launch: a class outside 0 ... 2, more than 1024 samples, max_bad < 0, a NULL table, a table of
 * another context, tables of different k, k outside 32 ... 63; from the join core, with the tool's name in front: a sample or a slice of 2^31
 * or more entries, a slice that overflows its buffer (raise stats_slices).  Tables in any order and in several pieces are taken as they are. */
int  mf_kmers_color_wide_tables(mf_ctx *ctx, mf_wtable *const *t, const int *classes, int n, int max_bad, int count_values, mf_wctable **out);
/* [mf_kmers_color] the file form on wide .kmers.bin files: every load is mf_wtable_load_kmers(file, 1, 0, k), one sample resident at a time,
 * each file read twice per slice -> kmers_bin (24-byte records) + stat_txt (may be NULL).  32 <= k <= 63; *n_kmers (may be NULL) = the
 * records written. */
int  mf_kmers_color_wide(mf_ctx *ctx, const char *const *files, const int *classes, int n, int max_bad, int count_values, int k,
                         const char *kmers_bin, const char *stat_txt, uint64_t *n_kmers);
/* [mf_colored_components_device] on an mf_wctable: the values are classified by the narrow tool's kernel, the k-mers become a one-piece
 * ascending wide table whose counts are the colour codes, the adjacency is the wide cutter's (mf_cut_components_wide_device) and the
 * per-colour passes are the narrow tool's on vertex ids.  out[n_groups]: one mf_wcomps per colour (size = weight = k-mers; size descending,
 * then smallest k-mer; members ascending); colours above 2 give empty components; counts[n_groups] may be NULL.  k must be the table's.
 * A k-mer whose colour is >= n_groups is an error that prints the k-mer as its k bases.  Fewer than 2^32 - 1 k-mers; n_groups 1 ... 64. */
int  mf_colored_components_wide_device(mf_ctx *ctx, const mf_wctable *t, int k, int n_groups, int separate, double perc, mf_wcomps **out,
                                       uint64_t *counts);
/* [mf_colored_components] the file form: mf_wctable_load(files, min_value) -> <out_dir>/components_color_<c>.bin for c < n_groups, each an
 * ordinary wide components.bin (mf_wcomps_write), and stat_txt (may be NULL), the narrow tool's four columns.  On an error nothing is written. */
int  mf_colored_components_wide(mf_ctx *ctx, const char *const *files, int nfiles, int k, int64_t min_value, int n_groups, int separate,
                                double perc, const char *out_dir, const char *stat_txt, uint64_t *counts);

/* ---- A13  Bray-Curtis ---------------------------------------------------------------- */
/* replaces DistanceMatrixCalculatorMain.brayCurtisDistance (src/tools/DistanceMatrixCalculatorMain.java:
 * 140-152): d = sum|a-b| / sum(|a|+|b|) on raw vectors; vecs is row-major [n_samples][n_comp]. */
int  mf_bray_curtis(const int64_t *vecs, int n_samples, int n_comp, double *out_matrix);

/* ---- synthetic reads (bench / tests) ---------------------------------- */
/* Fills d_bases[n_reads*read_len] (ASCII) and d_offsets[n_reads+1] with the deterministic,
 * integer-only generator described in DESIGN.md (128-genome pool with shared repeats, log-normal
 * abundances, strand flips, 0.5 % substitutions, no N).  The host mirror mf_synth_reads_host
 * produces the identical bytes on the CPU. */
int  mf_synth_reads_device(mf_ctx *ctx, uint64_t seed, int sample, uint64_t first_read, uint64_t n_reads,
                           int read_len, uint64_t genome_scale_bp, void *d_bases, void *d_offsets);
int  mf_synth_reads_host(uint64_t seed, int sample, uint64_t first_read, uint64_t n_reads, int read_len,
                         uint64_t genome_scale_bp, uint8_t *bases, uint64_t *offsets);
/* the same with the substitution rate as a parameter: sub_per_16384 substitutions per 16384 bases (82 = the 0.5 % above,
 * 164 = 1 %: BASELINE.json config 5, "generator scaled: pool 2 Gbp, error 1 %") */
int  mf_synth_reads_device_ex(mf_ctx *ctx, uint64_t seed, int sample, uint64_t first_read, uint64_t n_reads,
                              int read_len, uint64_t genome_scale_bp, int sub_per_16384, void *d_bases, void *d_offsets);
int  mf_synth_reads_host_ex(uint64_t seed, int sample, uint64_t first_read, uint64_t n_reads, int read_len,
                            uint64_t genome_scale_bp, int sub_per_16384, uint8_t *bases, uint64_t *offsets);

#ifdef __cplusplus
}
#endif
#endif
