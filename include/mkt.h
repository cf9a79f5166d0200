/*
 * include/mkt.h -- C ABI of libmkt_hip.so, the MI355X (gfx950) implementation of Microcket's
 * sam2pairs hot path.  Plain C: opaque handle, POD structs, caller-visible pointers and sizes,
 * int return codes, no exceptions, no torch types.
 *
 * What it replaces (paths relative to the reference tree):
 *   src/sam2pairs/sam2pairs.cpp:23-228  main(): argv, batch loop, stdout/.sam writes, .log
 *   src/sam2pairs/pairutil.h:136-177    load_batch(): per-line filter + QNAME run-length grouping
 *   src/sam2pairs/pairutil.h:63-126     cigar2segment()
 *   src/sam2pairs/pairutil.h:180-208    check_integrity_{1,2}_seg()
 *   src/sam2pairs/flash2pairs.h:17-155  flash2pairs()
 *   src/sam2pairs/unc2pairs.h:16-358    unc2pairs()
 * The reference has no library boundary of its own: its plugin surface is the process contract
 * of bin/sam2pairs (argv / stdin / stdout / <prefix>.<mode>.sam / <prefix>.<mode>2pairs.log,
 * microcket:479,483,501,505).  The drop-in for THAT surface is the `sam2pairs` executable built
 * from microcket_amd/csrc/sam2pairs_main.cpp, which is a thin host loop over this ABI.
 * INTEGRATION.md shows both bindings.
 *
 * Threading: one context per GPU and per input stream; a context is not thread-safe.
 * Every entry point fails with MKT_E_NO_DEVICE when no HIP device is usable: there is no CPU path.
 */
#ifndef MKT_H
#define MKT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MKT_ABI_VERSION 9

enum { MKT_MODE_FLASH = 0, MKT_MODE_UNC = 1 };           /* argv[2], sam2pairs.cpp:59-67 */

enum {
    MKT_OK = 0,
    MKT_E_ARG = -1,          /* bad argument */
    MKT_E_NO_DEVICE = -2,    /* no usable HIP device / kernel image not loadable */
    MKT_E_HIP = -3,          /* a HIP call failed (mkt_last_error has the text) */
    MKT_E_NOMEM = -4,
    MKT_E_CAPACITY = -5,     /* a QNAME group does not fit the block buffer */
    MKT_E_KERNEL = -6,       /* the kernel reported an internal error bit */
    MKT_E_STATE = -7,        /* call order violated (e.g. submit after finish) */
    MKT_E_IO = -8,           /* a temporary file could not be created, written or read (the error text names it) */
    MKT_E_FORMAT = -9,       /* a BGZF file or a deflate stream is refused (mkt_bgzf_error names the reason and the block's offset) */
    MKT_E_RANGE = -10        /* more than an object is built for (the pair statistics' table of more than 2048 names) */
};

/* tile geometry selection (tests force the small-tile build to exercise every slow path) */
enum { MKT_TILES_AUTO = 0, MKT_TILES_FAST = 1, MKT_TILES_SMALL = 2 };

typedef struct mkt_params {
    int32_t mode;              /* MKT_MODE_*                                   argv[2] */
    float min_mapped_ratio;    /* float32, as (float)atof(argv[5])             sam2pairs.cpp:41 */
    int32_t min_mapq;          /* atoi(argv[6]); compared unsigned             sam2pairs.cpp:44, pairutil.h:157 */
    int32_t write_sam;         /* 0: argv[7] starts with N/n/0                 sam2pairs.cpp:47 */
    int32_t ref_threads;       /* argv[4] (>= 2): only the logged selfCircle depends on it (quirk Q2) */
    int32_t device;            /* HIP device ordinal */
    uint64_t block_bytes;      /* streaming path: bytes of SAM text per kernel pass, 0 = default (64 MiB); < 2 GiB - 64 KiB */
    int32_t tiles;             /* MKT_TILES_* */
    int32_t ordered;           /* 1: outputs in input order (deterministic bytes); 0 (default): any order, like the
                                * reference, whose worker threads fwrite concurrently (sam2pairs.cpp:154,175) */
    uint32_t extensions;       /* MKT_EXT_* bits; 0 (default) = exactly the reference's behaviour and outputs */
    uint32_t reserved2;
} mkt_params;

/* Extensions.  NOT in the reference's sam2pairs (its only duplicate removal works on FASTQ,
 * src/preprocess/krmdup.cpp:151-213): default off, they never change stdout / .sam / .log, parity is unpinned.
 * MKT_EXT_KEYS makes the kernels also emit one key record per reported pair (chr1,pos1,chr2,pos2,strand1,strand2),
 * kept on the device in input order; mkt_ext_dedup / mkt_ext_chrstat work on those after the end of the input. */
enum { MKT_EXT_KEYS = 1,
       MKT_EXT_LANES = 2 };    /* with MKT_EXT_KEYS: the read's sequencing lane (QNAME field 4) is part of the duplicate key, i.e. duplicates
                                * never span lanes -- the driver's -b, which runs one krmdup per lane (microcket:421-451) */

/* The 8 counters of <prefix>.<mode>2pairs.log in file order (sam2pairs.cpp:211-218), plus totals. */
typedef struct mkt_stats {
    uint32_t lowMap, manyHits, unpaired, selfCircle, trans, cis10K, cis1K, cis0;
    uint32_t selfCircle_all;   /* every self-circle, before the thread-0 mask of quirk Q2 */
    uint32_t reserved;
    uint64_t groups;           /* K: surviving QNAME groups, including the last one (never classified, quirk Q1) */
    uint64_t pairs;            /* .pairs lines */
    uint64_t pair_bytes, sam_bytes;
    uint64_t lines_in, bytes_in, blocks;
} mkt_stats;

typedef struct mkt_out {
    const char* pairs; size_t pairs_len;   /* ready .pairs bytes (stdout of bin/sam2pairs) */
    const char* sam;   size_t sam_len;     /* ready <prefix>.<mode>.sam bytes */
} mkt_out;

/* HIP-event timing of the kernels launched by a context (for bench.py's roofline object) */
typedef struct mkt_timing {
    double tile_kernel_ms;     /* sum over launches of the fused tile kernel */
    uint64_t tile_launches;
    uint64_t tile_bytes;       /* SAM bytes those launches consumed */
    double other_ms;           /* memset + finish kernels */
    uint64_t tiles;            /* tiles processed */
    uint64_t deferred_tiles;   /* of those, tiles the lean kernel left to the generic kernel */
} mkt_timing;

/* how often a context had to run blocks again, by the cause it repaired first (tests read this to prove that an input took the
 * path they are about).  Streaming path: every cause; resident path (mkt_sync): geometry only, everything else is an error. */
typedef struct mkt_replays {
    uint64_t geometry;         /* line table overflown: next smaller tile geometry */
    uint64_t pairs_cap;        /* .pairs region too small: buffer grown */
    uint64_t sam_cap;          /* .sam region too small: buffer grown */
    uint64_t sc_cap;           /* self-circle slices or the run's lists too small: grown */
    uint64_t jobs_rerun;       /* blocks launched again: the failed one and every block queued behind it */
} mkt_replays;

typedef struct mkt_ctx mkt_ctx;

int mkt_abi_version(void);
const char* mkt_strerror(int code);
const char* mkt_last_error(const mkt_ctx* ctx);     /* ctx may be NULL: last create error */
int mkt_device_count(void);

int mkt_create(const mkt_params* p, mkt_ctx** out);
void mkt_destroy(mkt_ctx* ctx);

/* ---- streaming path: host bytes in, host bytes out (what the sam2pairs executable uses) -------
 * mkt_submit takes the next bytes of the SAM stream in any chunking; `last` != 0 ends the input.
 * The path is a pipeline: a full block (block_bytes, cut on a QNAME-group boundary) is queued on the GPU -- H2D copy,
 * kernels, output gather -- and the call returns; a worker thread inside the library takes the results in input order,
 * copies the outputs back and publishes what is final (everything except the newest group, see quirk Q1).  Reading the
 * next block, the PCIe copies in both directions, the kernels and the consumer's writes all overlap.  A kernel-side
 * problem (e.g. an output buffer guess that was too small, a line table overflow) is repaired by re-running the affected
 * blocks; what cannot be repaired is reported by the next call on the context (mkt_last_error has the text).
 *
 * mkt_drain (non-blocking) hands back, as one contiguous copy, every output byte published so far; the pointers stay
 * valid until the next drain call.  mkt_finish waits for the pipeline, so submit .. finish .. drain from ONE thread
 * always sees everything.
 * mkt_drain_wait is the zero-copy form for a dedicated consumer thread (the executable's writer): it blocks until a
 * chunk of output is published and hands out pointers into the pinned staging buffer it was copied to (valid until the
 * next mkt_drain_wait call, which gives the buffer back: a slow consumer throttles the pipeline); *done = 1 with empty
 * ranges once mkt_finish has run and everything was handed out.  One thread may call mkt_drain_wait while another one
 * feeds the context; no other concurrent use of a context is allowed. */
int mkt_submit(mkt_ctx* ctx, const char* bytes, size_t n, int last);
int mkt_drain(mkt_ctx* ctx, mkt_out* out);
int mkt_drain_wait(mkt_ctx* ctx, mkt_out* out, int* done);
/* The same without the intermediate copy: mkt_input_window hands out the free part of the context's pinned input block
 * (*cap > 0 bytes at *buf; a full block is processed first); the caller reads the next bytes of the SAM stream straight
 * into it (read / pread, several threads if it likes) and commits them with mkt_submit_window.  Do not mix with
 * mkt_submit inside one window. */
int mkt_input_window(mkt_ctx* ctx, char** buf, size_t* cap);
int mkt_submit_window(mkt_ctx* ctx, size_t n, int last);

/* ---- resident path: text already in HBM (bench.py, multi-GPU shards) --------------------------
 * The block must start on a QNAME-group boundary, end on a line end, be < 2 GiB - 64 KiB and 16-byte
 * aligned, and the memory must be readable up to the next multiple of 16 bytes past its end
 * (the kernels load whole 16-byte vectors); d_text must stay valid until mkt_sync.  Output bytes stay on the device (fetch them
 * with mkt_fetch_last_block) and results accumulate in the context exactly as for mkt_submit.
 * The call is asynchronous on the context's stream. */
int mkt_submit_device(mkt_ctx* ctx, const void* d_text, size_t n);
int mkt_sync(mkt_ctx* ctx);
int mkt_fetch_last_block(mkt_ctx* ctx, char* pairs, size_t pairs_cap, size_t* pairs_len,
                         char* sam, size_t sam_cap, size_t* sam_len);

/* ---- end of input ------------------------------------------------------------------------------
 * drop_last != 0: this context saw the end of the whole input, so its last surviving group is
 * dropped (quirk Q1).  For a sharded run only the shard holding the input's end passes 1.
 * group_offset / total_groups place the shard's groups in the whole input for quirk Q2
 * (single context: pass 0, 0 and the library uses its own count). */
int mkt_finish(mkt_ctx* ctx, int drop_last, uint64_t group_offset, uint64_t total_groups, mkt_stats* st);
/* formats the 8-line log exactly as sam2pairs.cpp:211-218; returns bytes written */
int mkt_format_log(const mkt_stats* st, char* out, size_t cap);

/* forget everything seen so far (counters, pending group, outputs) but keep the device buffers:
 * the context is ready for a new input stream */
int mkt_reset(mkt_ctx* ctx);

int mkt_get_timing(const mkt_ctx* ctx, mkt_timing* t);
int mkt_reset_timing(mkt_ctx* ctx);      /* clears mkt_replays as well; mkt_reset clears neither */
int mkt_get_replays(const mkt_ctx* ctx, mkt_replays* r);

/* ---- synthetic inputs (stand-in for util/simulation + BWA) ------------------------
 * Generates groups [first_group, first_group + n_groups) of the seeded data set straight into
 * device memory owned by the context; *d_text stays valid until the next mkt_synth_device call or
 * mkt_destroy.  profile: 0 unc, 1 flash, 2 stress; genome: 0 hg38, 1 mm10. */
int mkt_synth_device(mkt_ctx* ctx, uint64_t seed, int profile, int genome, int read_len, int lanes,
                     uint64_t first_group, uint64_t n_groups, int tail_group,
                     const void** d_text, size_t* n_bytes);
int mkt_copy_to_host(mkt_ctx* ctx, const void* d_src, void* dst, size_t n);
/* host text -> a device buffer owned by the context (16-byte aligned, lives until mkt_destroy): a block for mkt_submit_device */
int mkt_device_text(mkt_ctx* ctx, const char* bytes, size_t n, const void** d_text);

/* A whole synthetic data set resident in HBM, cut into group-aligned blocks (bench.py's workload:
 * 100 M read pairs = ~92 GB of SAM text on one MI355X).  Blocks are 16-byte aligned. */
typedef struct mkt_dataset mkt_dataset;
int mkt_dataset_create(mkt_ctx* ctx, uint64_t seed, int profile, int genome, int read_len, int lanes,
                       uint64_t first_group, uint64_t n_groups, uint64_t groups_per_block, int tail_group,
                       mkt_dataset** out);
int mkt_dataset_info(const mkt_dataset* ds, uint64_t* n_blocks, uint64_t* total_bytes, uint64_t* total_groups);
int mkt_dataset_block(const mkt_dataset* ds, uint64_t i, const void** d_text, size_t* n_bytes, uint64_t* n_groups);
void mkt_dataset_destroy(mkt_dataset* ds);

/* Pairs-level duplicate marking: a reported pair is a duplicate when an EARLIER reported pair (input order) has the
 * same key.  flags (may be NULL) receives one byte per reported pair in input order (1 = duplicate).
 * drop_last as in mkt_finish.  Requires MKT_EXT_KEYS. */
int mkt_ext_dedup(mkt_ctx* ctx, int drop_last, uint64_t* total, uint64_t* dups, uint8_t* flags, size_t flags_cap);
/* Sharded duplicate marking (one context per GPU): the key space is exchanged by the caller (RCCL all-gather through
 * torch.distributed in microcket_amd/shard.py) and marked with the same kernels.
 *   mkt_ext_chr_names   the context's chromosome-name table as "slot\tname\n" lines (slots are per context);
 *   mkt_ext_keys_fetch  the context's key records (24 bytes each: k0, k1, ordinal; see mkt_core.h KeyRec) in input order;
 *   mkt_ext_dedup_keys  duplicate flags for ANY key array in input order (e.g. the concatenation of all shards with
 *                       chromosome slots rewritten to ids that are the same on every rank). */
int mkt_ext_chr_names(mkt_ctx* ctx, char* out, size_t cap, size_t* len);
int mkt_ext_keys_fetch(mkt_ctx* ctx, int drop_last, void* keys, size_t cap_bytes, uint64_t* n);
int mkt_ext_dedup_keys(mkt_ctx* ctx, const void* keys, uint64_t n, uint8_t* flags, uint64_t* dups);
/* The same for sharded runs as an xGMI design: every key record travels to rank mix64(key) % world, so equal keys meet on
 * one GPU (microcket_amd/shard.py: dedup_exchange drives it with three all_to_all_single calls on DEVICE buffers over RCCL).
 *   mkt_ext_keys_device   the context's key list where it lies in HBM (input order);
 *   mkt_ext_partition     rewrites chromosome slots through lut (8192 entries, host; from the exchanged name tables; NULL:
 *                         keep) and writes the records grouped by destination rank, in input order inside every group, to the
 *                         device buffer d_send (24 bytes per record); counts[r] = records for rank r (world <= 16);
 *   mkt_ext_dedup_device  duplicate flags (device, one byte per record) for n key records lying in device memory, first
 *                         in buffer order wins;
 *   mkt_ext_unpartition   flags that came back in d_send order -> the context's input order (host buffer `flags`, may be
 *                         NULL); *dups = duplicates among this context's pairs. */
int mkt_ext_keys_device(mkt_ctx* ctx, int drop_last, const void** d_keys, uint64_t* n);
int mkt_ext_partition(mkt_ctx* ctx, int drop_last, const uint16_t* lut, uint32_t world, void* d_send, uint64_t* counts);
int mkt_ext_dedup_device(mkt_ctx* ctx, const void* d_keys, uint64_t n, uint8_t* d_flags, uint64_t* dups);
int mkt_ext_unpartition(mkt_ctx* ctx, const uint8_t* d_flags_part, uint8_t* flags, size_t flags_cap, uint64_t* dups);
/* The whole exchange for `world` contexts of ONE process (one per GPU; shard r = ctxs[r], contiguous ranges of the input in rank
 * order; last_rank holds the input's end: its last group is dropped, quirk Q1): partition, device-to-device copies between the
 * contexts' GPUs (hipMemcpyPeerAsync: xGMI between two GPUs of a node), marking, flags back.  totals[r] / dups[r]: reported pairs /
 * duplicates of shard r; flags[r] (may be NULL): its flags in input order.  This is what bin/sam2pairs uses with MKT_DEVICES. */
int mkt_ext_dedup_multi(mkt_ctx** ctxs, uint32_t world, uint32_t last_rank, uint64_t* totals, uint64_t* dups, uint8_t** flags, const size_t* flags_cap);

/* Per-chromosome contact counts of the reported pairs: lines "chrA\tchrB\tcount\n" sorted bytewise by (chrA, chrB). */
int mkt_ext_chrstat(mkt_ctx* ctx, int drop_last, char* out, size_t cap, size_t* len);

/* ---- .pairs text in the driver's order ----------------------------------------------------
 * The stage behind sam2pairs is `LANG=C sort -k2,2d -k4,4d -k3,3n -k5,5n` and, to pool the stitched and the unstitched
 * mode, `sort -m` with the same keys (microcket:480,484,502,506,514).  A sorter takes whole .pairs lines in any
 * order and any number of pieces (host or device memory), sorts them on the GPU by (chr1 and chr2 in dictionary order
 * -- blanks and alphanumerics only --, pos1, pos2 numerically, then the whole line bytewise) and hands the text back:
 * byte for byte what the system's sort prints.  One sorter fed with both modes' pairs replaces sort + sort -m. */
typedef struct mkt_sorter mkt_sorter;
int mkt_sorter_create(int device, mkt_sorter** out);
void mkt_sorter_destroy(mkt_sorter* s);
const char* mkt_sorter_error(const mkt_sorter* s);
int mkt_sorter_add(mkt_sorter* s, const char* bytes, size_t n);            /* host bytes (copied before the call returns) */
int mkt_sorter_add_device(mkt_sorter* s, const void* d_bytes, size_t n);   /* device bytes */
int mkt_sorter_sort(mkt_sorter* s, uint64_t* lines, uint64_t* bytes);
int mkt_sorter_fetch(mkt_sorter* s, uint64_t off, char* out, size_t n);    /* sorted bytes [off, off + n) */

/* ---- FASTQ duplicate removal: the reference's krmdup / krmdup.pipe ---------------------------------
 * Replaces src/preprocess/krmdup.cpp:88-227 and krmdup.pipe.cpp:80-205: interleaved paired-end FASTQ in; out the pairs whose
 * 64-bit key (2 bits per base over seq1[hskip1, hskip1 + keylen1) and seq2[hskip2, hskip2 + keylen2), C=0 A=1 T=2 G=3)
 * was not seen before -- first seen wins, one key set per first key base, output order and the Total / Uniq / Dup / Discard
 * counters exactly as the reference's -- either as read-1 and read-2 records (krmdup) or interleaved (krmdup.pipe).  The
 * drop-ins for the process contract are bin/krmdup and bin/krmdup.pipe (microcket_amd/csrc/krmdup_main.cpp). */
typedef struct mkt_rmdup mkt_rmdup;
int mkt_rmdup_create(int device, mkt_rmdup** out);
void mkt_rmdup_destroy(mkt_rmdup* r);
const char* mkt_rmdup_error(const mkt_rmdup* r);
/* STREAMING form (what bin/krmdup[.pipe] use; any input size): begin, then push the bytes as they arrive.  The input is worked off in
 * SEGMENTS of whole 2^16-pair batches -- the reference's own batches (krmdup.cpp:19, 330-364), so the output order is the reference's --
 * as soon as MKT_RMDUP_SEGMENT_MB (default 256) of text are buffered: only that much FASTQ text is resident, plus 9 bytes per read pair
 * seen so far (its key and bucket) and a hash set of pair ordinals (4 bytes per slot, load <= 1/2) -- "first seen wins" holds across
 * segments.  A push that worked off a segment reports what it left in the outputs (out_bytes; fetch before the next push). */
int mkt_rmdup_begin(mkt_rmdup* r, uint32_t hskip1, uint32_t keylen1, uint32_t hskip2, uint32_t keylen2, int interleaved);
int mkt_rmdup_push(mkt_rmdup* r, const char* bytes, size_t n, int final, uint64_t out_bytes[2]);
int mkt_rmdup_stats(const mkt_rmdup* r, uint64_t stats[4] /* total, uniq, dup, discard so far */);
/* RESIDENT form (inputs that fit HBM; kept for callers of ABI <= 8): add everything, then run = ONE segment over all of it */
int mkt_rmdup_reserve(mkt_rmdup* r, size_t bytes);                   /* optional: room for that much FASTQ text up front */
int mkt_rmdup_add(mkt_rmdup* r, const char* bytes, size_t n);       /* the next bytes of the FASTQ stream (host; copied) */
int mkt_rmdup_run(mkt_rmdup* r, uint32_t hskip1, uint32_t keylen1, uint32_t hskip2, uint32_t keylen2, int interleaved,
                  uint64_t stats[4] /* total, uniq, dup, discard */, uint64_t out_bytes[2]);
int mkt_rmdup_fetch(mkt_rmdup* r, int which /* 0: read 1 or the interleaved stream, 1: read 2 */, uint64_t off, char* out, size_t n);

/* ---- read stitching: the driver's `flash ... -To -c - | perl deal.flash.pl - PREFIX` (microcket:405-408, 430-438) ----------------
 * Interleaved paired-end FASTQ in (8 lines per pair, as bin/krmdup.pipe writes it); out, in INPUT order, four streams:
 *   MKT_STITCH_TAB   FLASH's tab-delimited lines: "tag \t seq \t qual" for a combined pair, "tag \t seq1 \t qual1 \t seq2 \t qual2" else
 *   MKT_STITCH_EXT   PREFIX.ext.fq: every combined pair as "@tag \n seq \n + \n qual \n"
 *   MKT_STITCH_CUT1 / MKT_STITCH_CUT2   PREFIX.cut.read1.fq / .cut.read2.fq: every uncombined pair whose read 1 has at least
 *                    min_size + cut_tail bases (only read 1 is tested), the last cut_tail characters cut from all four strings
 * and the counters of PREFIX.stitch.stat.  The definition (restated in tests/stitchdef.py, pinned to FLASH v1.2.11 and deal.flash.pl
 * by tests/golden/stitch_golden.json); qualities are Phred values, byte - phred_offset:
 *   reading      letters are upper-cased, anything outside ACGT becomes N, and is written that way; the tag is read 1's header without
 *                '@' and without white space at its end.  A combined pair's is cut at its LAST '/' if it has one ("a/1" -> "a",
 *                "d/1 x y" -> "d", "b 1:N:0:ACGT" and "e_1" stay whole); an uncombined pair's only loses a "/1" or "/2" at its very end
 *                ("a/1" -> "a", but "d/1 x y", "a/3" and "x/y" stay whole)
 *   orientation  read 2 is reverse-complemented, its qualities reversed
 *   candidates   offsets i = max(0, n1 - n2) .. n1 - min_overlap into read 1, overlap length n1 - i, in this order
 *   scoring      a position where either base is N is uncalled; eff = overlap - uncalled, mm = called positions that differ, mq = the
 *                sum of min(q1, q2) over those; a candidate counts only if eff >= min_overlap
 *   comparing    in float32: sl = min(eff, max_overlap), d = mm / sl, qs = mq / sl; the best starts at d = x + 1, qs = 0 and is replaced
 *                when d <= best_d && (d < best_d || qs < best_qs); best_d > x after the scan: not combined.  So the first candidate
 *                with the smallest (d, qs) wins.  Every d and qs is a fraction with a denominator <= max_overlap, and only d < 2 and
 *                qs < 93 * 2 ever decide: two different ones differ by at least 1 / max_overlap^2, more than a float32 step (2^-16 below
 *                256) for max_overlap <= MKT_STITCH_MAX_M = 255.  In that range the kernels' cross-multiplied integer comparison is the
 *                same decision, and a larger max_overlap is refused; `d > x` is taken from a table of the float32 quotients themselves.
 *   combining    read 1 before the offset | the overlap | the rest of the reverse-complemented read 2; in the overlap equal bases keep the
 *                base with max(q1, q2), different bases get max(|q1 - q2|, 2) and the base of the higher quality, on a tie read 2's
 *                unless that is N
 *   cutting      a string shorter than cut_tail (only read 2 can be) keeps 2 * length - cut_tail characters or none: Perl's substr
 *                with a negative length
 * The program itself writes its tab lines in blocks of 35 per kind, so its stream alternates between runs of combined and uncombined
 * lines even with one thread (and has no defined order with several); each kind by itself is in input order, which is all that
 * deal.flash.pl's files show.  Out of scope: outie pairs (-O), the other output formats, histograms.
 * Limits, each MKT_E_ARG with a message that names the pair, never a truncation: reads of 1 .. MKT_STITCH_MAX_READ bases, sequence
 * and quality of equal length, quality bytes in phred_offset .. phred_offset + 93, whole pairs (a line count that is no multiple of 8
 * at the end of the input is an error); 1 <= min_overlap <= max_overlap <= MKT_STITCH_MAX_M, 0 <= max_mismatch_density <= 1,
 * phred_offset 0 .. 127, cut_tail and min_size below 2^16.
 * The input is worked off in segments of whole pairs (mkt_stitch_segment_pairs, default 2^20; MKT_STITCH_SEGMENT_PAIRS), a record
 * may be split anywhere between pushes; the outputs are the same bytes whatever the pieces and the segment size.
 *   mkt_stitch_check   the argument check of mkt_stitch_begin without a device: MKT_OK, or MKT_E_ARG with the message in msg
 *   mkt_stitch_push    the next bytes (may be none); final != 0 ends the input.  out_bytes = what this push left in the four streams
 *                      (fetch before the next push), zeros when no segment was worked off
 *   mkt_stitch_timing  ms (HIP events) of the segments so far: line index, scoring, sizes and their scans, writing */
#define MKT_STITCH_MAX_READ 512
#define MKT_STITCH_MAX_M 255
enum { MKT_STITCH_TAB = 0, MKT_STITCH_EXT = 1, MKT_STITCH_CUT1 = 2, MKT_STITCH_CUT2 = 3 };
typedef struct mkt_stitch mkt_stitch;
int mkt_stitch_create(int device, mkt_stitch** out);
void mkt_stitch_destroy(mkt_stitch* s);
const char* mkt_stitch_error(const mkt_stitch* s);
int mkt_stitch_check(uint32_t min_overlap, uint32_t max_overlap, double max_mismatch_density, uint32_t phred_offset, uint32_t cut_tail, uint32_t min_size,
                     char* msg, size_t msg_cap);
int mkt_stitch_segment_pairs(mkt_stitch* s, uint64_t pairs);        /* before begin; at least 1 */
int mkt_stitch_begin(mkt_stitch* s, uint32_t min_overlap, uint32_t max_overlap, double max_mismatch_density, uint32_t phred_offset, uint32_t cut_tail,
                     uint32_t min_size);
int mkt_stitch_push(mkt_stitch* s, const char* bytes, size_t n, int final, uint64_t out_bytes[4]);
int mkt_stitch_fetch(mkt_stitch* s, int which /* MKT_STITCH_* */, uint64_t off, char* out, size_t n);
int mkt_stitch_stats(const mkt_stitch* s, uint64_t* total, uint64_t* combined, uint64_t* uncombined, uint64_t* pass);
int mkt_stitch_timing(const mkt_stitch* s, double* index_ms, double* score_ms, double* scan_ms, double* write_ms);

/* ---- adapter and quality trimming: the driver's `ktrim -k KIT -t T -o PREFIX -1 R1 -2 R2 -c` (microcket:371, 405, 413, 430, 444) ------
 * Paired FASTQ in (two streams, or one interleaved stream), out in input order
 *   MKT_TRIM_INTERLEAVED   what the program writes to stdout with -c: read 1's record, then read 2's, of every pair kept
 *   MKT_TRIM_READ1 / MKT_TRIM_READ2   PREFIX.read1.fq / PREFIX.read2.fq, what it writes without -c
 * and the six counters of PREFIX.trim.log.  The definition (restated in tests/ktrimdef.py, pinned to Ktrim 1.6.0's paired-end route by
 * tests/golden/ktrim_golden.json).  Bytes are compared as they stand: lower case never equals upper case, N equals only N.
 *   common length  n = min(len1, len2); all four strings of the pair are cut to n
 *   quality        a cycle passes when its byte is >= phred + min_qual in both reads.  k = the largest i + 1, i >= min_size - 1, for
 *                  which the `window` cycles i - window + 1 .. i all pass (a window that would begin before cycle 0 does not pass).
 *                  No such i: the pair is dropped.  The four strings are cut to k.
 *   seeds          every position at which the first 3 letters of adapter 1 stand in read 1, or the first 3 of adapter 2 in read 2,
 *                  wholly inside the k cycles; ascending, each position once
 *   verification   at a seed p: L = min(k - p, adapter length), limit = ceil(float32(L) * float32(mismatch)) (float32 throughout).
 *                  Read 1's [p, p + L) differs from adapter 1's first L letters in at most `limit` places AND read 2's from adapter
 *                  2's.  Nothing else is compared (the reads are not compared with each other).  The first seed that verifies wins
 *                  and counts as "Aadaptor": p >= min_size keeps p cycles, otherwise the pair is dropped, and is a dimer when p <= 1.
 *   tail           only when no seed verifies.  With i = k - 2, of the six conditions  r1[i] == a1[0], r1[i+1] == a1[1], r2[i] == a2[0],
 *                  r2[i+1] == a2[1], revcomp(r1[5], r2[i-6]), revcomp(r2[5], r1[i-6])  at most one fails: a tail hit, i cycles are kept
 *                  (dropped when i < min_size).  Otherwise with i = k - 1, of  r1[i] == a1[0], r2[i] == a2[0], revcomp(r1[5], r2[i-6]),
 *                  revcomp(r2[5], r1[i-6]), revcomp(r1[6], r2[i-7]), revcomp(r2[6], r1[i-7])  at most one fails: a tail hit, i cycles.
 *                  revcomp(x, y) holds for (A,T), (C,G), (G,C), (T,A) only.
 *   adapters       kit: illumina | nextera | transposase | bgi in the program's spellings; it wins over adapter1 / adapter2.  Without
 *                  a kit: adapter1 (and adapter2, default adapter1), cut to their common length, 8 .. 64 letters; neither: illumina.
 *   output         header lines whole, the third line is "+"
 * The float32 limit is tabulated on the host for L = 0 .. 64; the kernels work in integers.
 * Deliberately different from the program, which damages such records and exits 0: here each is MKT_E_ARG with a message that names
 * the pair (counted from 0), never a truncation: sequence and quality of different lengths; a header line longer than
 * MKT_TRIM_MAX_HEADER or a read longer than MKT_TRIM_MAX_READ (the program's line buffers); a record without '@' or '+'; a quality byte
 * outside phred .. 126; at the end of the input a line count that is no multiple of 4, or streams of different pair counts.
 * Not accepted although the program accepts them (unpinned or meaningless): phred, min_qual and window of 0 are refused by the program
 * too (exit 12), min_size below 10 too (exit 11); mismatch outside 0 .. 1; the CLIP kit.  A pair with more than 128 seeds overruns the
 * program's seed list; here the rule above holds for any number.
 * The input is worked off in segments of whole pairs (mkt_trim_segment_pairs, default 2^20; MKT_TRIM_SEGMENT_PAIRS); the bytes do not
 * depend on the segment size or on where the pushes are cut.
 *   mkt_trim_check     the argument check of mkt_trim_begin without a device: MKT_OK, or MKT_E_ARG with the message in msg
 *   mkt_trim_push      the next bytes of both streams (either may be none), cut anywhere; with opts.interleaved_input one interleaved
 *                      stream in bytes1 and n2 = 0.  final != 0 ends the input.  out_bytes = what this push left in the three streams
 *   mkt_trim_fetch     a range of one of them (valid until the next push)
 *   mkt_trim_timing    ms (HIP events) of the segments so far: line indexes, decisions, sizes and their scans, writing */
#define MKT_TRIM_MAX_READ 510
#define MKT_TRIM_MAX_HEADER 126
#define MKT_TRIM_MIN_ADAPTER 8
#define MKT_TRIM_MAX_ADAPTER 64
enum { MKT_TRIM_INTERLEAVED = 0, MKT_TRIM_READ1 = 1, MKT_TRIM_READ2 = 2 };
typedef struct mkt_trim_opts {
    const char* adapter1;      /* NULL: by kit */
    const char* adapter2;      /* NULL: adapter1 */
    const char* kit;           /* NULL: by adapter1 / adapter2, or illumina */
    uint32_t min_size, phred, min_qual, window;
    double mismatch;
    int interleaved_input;
} mkt_trim_opts;
typedef struct mkt_trim mkt_trim;
void mkt_trim_default_opts(mkt_trim_opts* o);      /* illumina, 36, 33, 20, 5, 0.125, two streams */
int mkt_trim_create(int device, mkt_trim** out);
void mkt_trim_destroy(mkt_trim* t);
const char* mkt_trim_error(const mkt_trim* t);
int mkt_trim_check(const mkt_trim_opts* o, char* msg, size_t msg_cap);
int mkt_trim_segment_pairs(mkt_trim* t, uint64_t pairs);        /* before begin; at least 1 */
int mkt_trim_begin(mkt_trim* t, const mkt_trim_opts* o);
int mkt_trim_push(mkt_trim* t, const char* bytes1, size_t n1, const char* bytes2, size_t n2, int final, uint64_t out_bytes[3]);
int mkt_trim_fetch(mkt_trim* t, int which /* MKT_TRIM_* */, uint64_t off, char* out, size_t n);
int mkt_trim_stats(const mkt_trim* t, uint64_t* total, uint64_t* dropped, uint64_t* adapter, uint64_t* tailhit, uint64_t* dimer, uint64_t* pass);
int mkt_trim_timing(const mkt_trim* t, double* index_ms, double* decide_ms, double* scan_ms, double* write_ms);

/* ---- the .sam -> BAM tail of the pipeline -----------------------------------------------------------
 * Replaces microcket:533-540: `cat header flash.sam unc.sam | samtools view -b | samtools sort -o valid.bam; samtools index`.
 * SAM text in (leading '@' lines = the header, then alignment lines), out a BGZF-compressed BAM -- records in input order
 * (sorted = 0: `samtools view -b`) or in coordinate order with @HD SO:coordinate and a .bai index (sorted = 1: view | sort,
 * index).  level 0 stores the blocks, 1 deflates them on the GPU with LZ77 + the fixed Huffman codes, >= 2 with codes built per block.  Formats follow the
 * SAM/BAM specification (hts-specs SAMv1 4.1, 4.2, 5.2) and RFC 1951 / 1952; samtools ships with the reference only as a
 * prebuilt binary that is never run, so byte parity with it is unpinned.  No .bai is made (bai_bytes = 0) when a
 * reference is longer than 2^29 bases, the limit of that format.  Drop-in for the process contract:
 * bin/sam2bam (microcket_amd/csrc/sam2bam_main.cpp). */
typedef struct mkt_bam mkt_bam;
int mkt_bam_create(int device, mkt_bam** out);
void mkt_bam_destroy(mkt_bam* b);
const char* mkt_bam_error(const mkt_bam* b);
const char* mkt_bam_note(const mkt_bam* b);                                /* after a successful run: why no index was made ("" otherwise) */
int mkt_bam_add(mkt_bam* b, const char* bytes, size_t n);                  /* the next bytes of the SAM stream (host; copied) */
int mkt_bam_add_device(mkt_bam* b, const void* d_bytes, size_t n);         /* alignment lines already on the device */
int mkt_bam_reserve(mkt_bam* b, size_t bytes);                             /* optional: room for that much alignment text up front */
int mkt_bam_window(mkt_bam* b, char** buf, size_t* cap);                   /* a pinned 64 MiB host buffer for the next bytes of the stream ... */
int mkt_bam_commit(mkt_bam* b, size_t n);                                  /* ... its first n bytes are those bytes (copied asynchronously; two buffers alternate) */
int mkt_bam_run(mkt_bam* b, int sorted, int level, uint64_t* records, uint64_t* bam_bytes, uint64_t* bai_bytes);
int mkt_bam_read(mkt_bam* b, int which, uint64_t off, size_t n, const char** ptr);  /* result bytes through the pinned buffers; *ptr valid until the next call but one */
int mkt_bam_fetch(mkt_bam* b, int which /* 0: the BAM, 1: the BAI */, uint64_t off, char* out, size_t n);
/* Out-of-core mode, for inputs larger than HBM (samtools sort's sorted runs + merge).  Called before the first byte.  run_bytes:
 * alignment text per run (0: off -- the single pass above; MKT_BAM_RUNS_AUTO: the single pass while it fits the GPU, runs from where the
 * text or the rest of the pass would not).  Sorted: every run is sorted on the GPU and written to <tmp_prefix>.runs / <tmp_prefix>.keys, which are removed
 * again (only when this object created them) on success, on every error return and in mkt_bam_destroy; mkt_bam_pull then merges the runs on the GPU window by window.
 * Input order (sorted = 0): no temporary files; pieces of the BAM are ready while the input arrives (pull them between adds).
 * sorted / level must equal those given to mkt_bam_run.  The result equals the single-pass result byte for byte, BAI included.
 * Until a run is cut (input within the budget) the single pass runs.  With runs, mkt_bam_run reports bam_bytes = 0 (sorted) and
 * bai_bytes = 0: mkt_bam_stats has both after the last piece. */
#define MKT_BAM_RUNS_AUTO (~(uint64_t)0)
int mkt_bam_spill(mkt_bam* b, uint64_t run_bytes, const char* tmp_prefix, int sorted, int level);
int mkt_bam_pull(mkt_bam* b, const char** ptr, size_t* n);                /* the next piece of the BAM (<= 64 MiB, pinned; *n = 0: none now / the end after run) */
int mkt_bam_stats(const mkt_bam* b, uint64_t stats[5] /* runs, temporary bytes written, peak device bytes held, BAM bytes so far, BAI bytes */);

/* surviving QNAME groups seen so far (synchronises the context's stream); sharded runs exchange
 * these counts before mkt_finish */
int mkt_group_count(mkt_ctx* ctx, uint64_t* groups);

/* ---- pairs -> binned contact matrix at several resolutions (the driver's last stage, microcket:520-554) -------------------
 * What `juicer_tools pre -r ...` and `cooler cload pairix` spend their time on: the sparse binned matrix.  The .hic container is
 * defined at the end of this file, behind mkt_matrix_hic; the .cool container and zoomify are out of scope; parity with those tools
 * is unpinned.  Bin drop-in: bin/pairs2matrix.
 * Balancing (iterative correction) of each resolution's matrix is defined below, behind mkt_matrix_balance, and the expected
 * (distance decay) tables and observed / expected values behind mkt_matrix_expected.
 *
 * Definition.  chromsizes: lines name<TAB>length (anno/<genome>.info; empty and '#' lines ignored); FILE ORDER IS BIN ORDER.
 * For a resolution r >= 1: chromosome i of length L_i owns n_i = ceil(L_i / r) bins, off_i = n_0 + .. + n_(i-1), nbins = sum n_i;
 * bin(chr_i, pos) = off_i + (pos - 1) / r for the 1-based positions of a .pairs line (columns 2-5: chrA posA chrB posB).
 * A pair is SKIPPED (counted, never binned, never an error) when a chromosome is not in the table or a position is 0 or > L_i.
 * Every other pair adds 1 to cell (min(b1, b2), max(b1, b2)) -- decided on bin ids, not on the order of the text's two sides.
 * Result: the non-empty cells (bin1, bin2, count) strictly ascending in (bin1, bin2); it depends on the multiset of pairs only
 * (input order, chunking and the route the pairs came by never change a byte); sum(count) + skipped == pairs.
 *
 * Limits (MKT_E_ARG / MKT_E_CAPACITY with a message): 1 .. 16 resolutions per object; nbins < 2^32 at every resolution; fewer than
 * 2^32 pairs per object (counts are uint32_t); names of 1 .. 63 bytes, at most 8192 of them, none twice; lengths < 2^32.
 *
 * The table and the resolutions are fixed at create time (mkt_matrix_error(NULL): why the last create failed).  Pairs arrive by
 * any mix of the add forms; only 16 bytes per pair stay on the device, the text of one add call is resident during that call only.
 *   mkt_matrix_add         .pairs text from the host in ANY chunking (a partial last line is carried to the next call; '#' lines
 *                          are ignored).  Lines with fewer than five columns or a non-decimal position make mkt_matrix_run fail.
 *   mkt_matrix_add_device  whole lines already on the device
 *   mkt_matrix_add_keys    the reported pairs of a context created with MKT_EXT_KEYS on the same device (drop_last as in
 *                          mkt_finish); skip_flags (may be NULL): one byte per reported pair in input order, e.g. what
 *                          mkt_ext_dedup returns -- flagged pairs are left out (not counted as pairs): the matrix without duplicates
 *   mkt_matrix_run         bins everything added so far at every resolution; pairs / skipped: the totals.  More pairs may be added
 *                          and run called again.
 *   mkt_matrix_info        nbins (valid before run), cells and bytes of COO text of resolution res_index
 *   mkt_matrix_fetch       cells [first, first + n) as arrays (any of the three may be NULL)
 *   mkt_matrix_fetch_text  bytes [off, off + n) of the lines "bin1<TAB>bin2<TAB>count\n", made on the device: what
 *                          `cooler load -f coo <chromsizes>:<r>` reads
 *   mkt_matrix_timing      device time (ms, HIP events) the last run spent on resolution res_index */
typedef struct mkt_matrix mkt_matrix;
int mkt_matrix_create(int device, const char* chromsizes, size_t len, const uint32_t* resolutions, uint32_t n_res, mkt_matrix** out);
void mkt_matrix_destroy(mkt_matrix* m);
const char* mkt_matrix_error(const mkt_matrix* m);
int mkt_matrix_add(mkt_matrix* m, const char* bytes, size_t n);
int mkt_matrix_add_device(mkt_matrix* m, const void* d_bytes, size_t n);
int mkt_matrix_add_keys(mkt_matrix* m, mkt_ctx* ctx, int drop_last, const uint8_t* skip_flags, size_t n_flags);
int mkt_matrix_run(mkt_matrix* m, uint64_t* pairs, uint64_t* skipped);
int mkt_matrix_info(const mkt_matrix* m, uint32_t res_index, uint64_t* nbins, uint64_t* nnz, uint64_t* text_bytes);
int mkt_matrix_fetch(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, uint32_t* bin1, uint32_t* bin2, uint32_t* count);
int mkt_matrix_fetch_text(mkt_matrix* m, uint32_t res_index, uint64_t off, char* out, size_t n);
int mkt_matrix_timing(const mkt_matrix* m, uint32_t res_index, double* ms);

/* ---- matrix balancing: iterative correction (ICE) of one resolution's cells, on the GPU -----------------------------------
 * The definition is this project's own, modelled on the genome-wide `cooler balance`; parity with cooler is UNPINNED (cooler is not
 * run anywhere here; in particular its convergence criterion may differ in scale from the one below -- it was not compared).
 * tests/balancedef.py restates the definition in numpy.  All arithmetic is float64.
 *
 * Definition, for the cells (bin1 <= bin2, count) of one resolution, nbins, and the per-chromosome bin ranges [off_i, off_i + n_i):
 *  1. USED cells: bin2 - bin1 >= ignore_diags (global bin ids).  marg(x)[k] = sum of x over used cells with bin1 == k + sum of x
 *     over used cells with bin2 == k (a diagonal cell counts twice; that only matters when ignore_diags == 0).
 *  2. bias = 1 for every bin.  min_nnz > 0: bias = 0 where marg(1) < min_nnz.  m = marg(count * bias[bin1] * bias[bin2]).
 *     min_count > 0: bias = 0 where m < min_count.
 *  3. mad_max > 0: within each chromosome's bin range m is divided by the median of its positive entries (a range with none is
 *     left alone); lg = log(m[m > 0]); cut = exp(median(lg) - mad_max * median(|lg - median(lg)|)); bias = 0 where m < cut.
 *     A median of an even number of values is the mean of the two middle ones.
 *  4. for it = 1 .. max_iters: m = marg(count * bias[bin1] * bias[bin2]); nz = m[m != 0]; nz empty: every weight is NaN, scale and
 *     var are NaN, stop (not converged).  mean = mean(nz); var = population variance of nz / mean (scale-free);
 *     m /= mean; m[m == 0] = 1; bias /= m; var < tol: converged, stop.
 *  5. weight = bias / sqrt(mean) with the last mean; bins with bias == 0 get NaN.  iterations = the last it, scale = the last mean,
 *     masked = the number of NaN weights.  The balanced value of a cell is count * weight[bin1] * weight[bin2].
 * Out of scope: cis_only / trans_only (per-chromosome loops), KR / VC vectors, the .cool container.  What follows the
 * weights (expected tables, balanced and observed / expected values of the cells) is defined below, behind mkt_matrix_expected; a
 * per-cell TEXT dump of those values stays out of scope.
 *
 * Determinism: no floating-point atomics anywhere; every sum has a fixed shape that depends on (nbins, cells) only, so the weights
 * are the same bits from call to call, process to process and whatever route the pairs came by.  Against the numpy restatement
 * the mask, the iteration count and the stopping decision are identical and the weights agree to summation-order rounding.
 *
 *   mkt_balance_opts_default   ignore_diags 2, min_nnz 10, min_count 0, mad_max 5.0, tol 1e-5, max_iters 200
 *   mkt_matrix_balance         valid after mkt_matrix_run (MKT_E_STATE before); opts NULL = the defaults; MKT_E_ARG with a message for
 *                              a bad index, a negative or NaN option, max_iters == 0 or a non-zero reserved.  stats may be NULL.
 *                              The filters of steps 2-3 run on the host from one nbins-sized copy; step 4 stays on the device.
 *                              Cells and COO text are untouched; a later mkt_matrix_run (or add) discards the weights.
 *   mkt_matrix_fetch_weights   weights [first, first + n) of resolution res_index (MKT_E_STATE "balance first" without them)
 *   mkt_matrix_balance_timing  device time (ms, HIP events) of the last balance of res_index: the one-time setup (row pointers and the
 *                              transposed copy, 8 bytes per cell, kept until the next run; 0 when it was reused) and the whole
 *                              iteration loop of step 4: the host looks at the device's state once per 4 iterations, so up to 3
 *                              iterations of empty launches behind the last one and the looks themselves are in iter_ms.  Like
 *                              mkt_matrix_timing it takes a const handle: a bad index is MKT_E_ARG without a message.
 * Limit: fewer than 2^32 cells per resolution (MKT_E_CAPACITY with a message; implied today by the matrix stage's own limit of fewer
 * than 2^32 pairs per object). */
typedef struct mkt_balance_opts {
    int32_t ignore_diags;
    int32_t min_nnz;
    double min_count;
    double mad_max;
    double tol;
    int32_t max_iters;
    uint32_t reserved;       /* 0 */
} mkt_balance_opts;
typedef struct mkt_balance_stats {
    uint32_t iterations;
    int32_t converged;       /* 0 / 1 */
    double var;              /* of the last iteration */
    double scale;            /* the last mean */
    uint64_t masked;         /* NaN weights */
} mkt_balance_stats;
void mkt_balance_opts_default(mkt_balance_opts* o);
int mkt_matrix_balance(mkt_matrix* m, uint32_t res_index, const mkt_balance_opts* opts, mkt_balance_stats* stats);
int mkt_matrix_fetch_weights(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, double* out);
int mkt_matrix_balance_timing(const mkt_matrix* m, uint32_t res_index, double* setup_ms, double* iter_ms);

/* ---- expected contacts: distance decay per chromosome and genome-wide, trans block means, observed / expected values ------------
 * What `juicer_tools pre` keeps next to the counts (an expected-value vector per resolution) and what cooltools `expected-cis` /
 * `expected-trans` compute.  The definition is this project's own, modelled on those; parity with cooltools and juicer is UNPINNED
 * (neither is run anywhere here).  tests/expecteddef.py restates the definition in numpy.  All arithmetic is float64.
 *
 * Definition, for the cells (bin1 <= bin2, count) of one resolution, nbins, the chromosome ranges [off_c, off_c + n_c) and use_weights:
 *  1. valid(k).  use_weights == 0: every bin is valid and w[k] = 1.  use_weights == 1: w = the weights of the last mkt_matrix_balance
 *     of that resolution, valid(k) = w[k] is not NaN (without weights: MKT_E_STATE "balance first").
 *  2. v = ((double)count * w[bin1]) * w[bin2]: two float64 multiplications in this order.  A cell is USED when both bins are valid.
 *  3. CIS table, exactly nbins rows: row off_c + d is (chromosome c, diagonal d), 0 <= d < n_c.
 *     n_valid = #{i in [off_c, off_c + n_c - d): valid(i) and valid(i + d)}; count_sum (uint64, exact) = sum of count over the used
 *     cells with both bins in c and bin2 - bin1 == d; balanced_sum = the sum of v over the same cells.  No diagonal is left out:
 *     consumers drop the first ignore_diags rows themselves.
 *  4. TRANS table, one row per chromosome pair a < b in file order, row a * (2 * n_chr - a - 1) / 2 + (b - a - 1):
 *     n_valid = nvalid_a * nvalid_b (valid bins of a times valid bins of b), count_sum and balanced_sum over the used cells of the
 *     block, expected = balanced_sum / n_valid, NaN when n_valid == 0.
 *  5. GENOME-WIDE table, one row per d in [0, max n_c): N[d], C[d], S[d] = the cis rows added over the chromosomes IN FILE ORDER
 *     (done on the host); expected[d] = S[d] / N[d], NaN when N[d] == 0.
 *  6. SMOOTHED expected, group edges in integers only: diagonal 0 is a group of its own; after it e_0 = 1,
 *     e_(j+1) = e_j + max(1, e_j >> 3) (1 .. 8, 9, .., 16, 18, 20, 22, 24, 27, 30, 33, 37, ..), group j = [e_j, e_(j+1)) clipped to the
 *     table.  expected_smooth[d] = (sum of S over d's group) / (sum of N over d's group), both sums in ascending d; NaN when the sum
 *     of N is 0.
 *  7. Per-cell VALUES in cell order: MKT_VALUE_BALANCED is v; MKT_VALUE_OE is v / expected[bin2 - bin1] for a cis cell and
 *     v / expected(block) for a trans cell; MKT_VALUE_OE_SMOOTH the same with expected_smooth for cis cells.  A cell with a masked
 *     bin is NaN.  A used cell's divisor is > 0 (its own v is in S), so a used cell is finite.
 *
 * Determinism: no floating-point atomics; every float64 sum has a shape fixed by (nbins, cells) only (a fixed number of lanes with a
 * fixed stride and a fixed tree per segment, long segments in fixed chunks), so tables and values are the same bits from call to call,
 * process to process and whatever route the pairs came by (add, add_device, add_keys).  Against the numpy restatement the integers
 * and the NaN pattern are identical and the float sums agree to summation-order rounding.
 *
 *   mkt_expected_opts_default         use_weights 1
 *   mkt_matrix_expected               valid after mkt_matrix_run (MKT_E_STATE before; with use_weights == 1 also before
 *                                     mkt_matrix_balance of that resolution); opts NULL = the defaults; MKT_E_ARG with a message for a
 *                                     bad index, use_weights other than 0 / 1 or a non-zero reserved.  info may be NULL.  The tables stay
 *                                     resident (with a host mirror for the fetches) until the cells or the weights go away: a later
 *                                     mkt_matrix_run, add or mkt_matrix_balance of that resolution discards them.
 *   mkt_matrix_fetch_expected_cis / _trans / _genome   rows [first, first + n) of a table; any output pointer may be NULL.
 *                                     MKT_E_STATE without tables, MKT_E_ARG with a message for a bad index or range.
 *   mkt_matrix_fetch_values           values of cells [first, first + n) in the order of mkt_matrix_fetch.  OE and OE_SMOOTH need the
 *                                     tables; BALANCED needs only the weights (it follows the tables' use_weights when there are tables:
 *                                     with use_weights == 0 it is the count as a double).  MKT_E_ARG for a bad kind or range.
 *   mkt_matrix_expected_timing        device time (ms, HIP events) of the last mkt_matrix_expected of res_index: the one-time grouping of
 *                                     the cells by segment (12 bytes per cell, kept until the next run; 0 when it was reused) and the
 *                                     sums (validity bits, n_valid, the segment sums).  A bad index is MKT_E_ARG without a message.
 * Out of scope: a per-cell text dump, per-chromosome smoothing, the .cool container.
 * Limit: bits of (nbins + trans rows) + bits of the cell count <= 64 (MKT_E_CAPACITY with a message). */
typedef struct mkt_expected_opts { int32_t use_weights; uint32_t reserved; /* 0 */ } mkt_expected_opts;
typedef struct mkt_expected_info { uint64_t cis_rows, trans_rows, genome_rows; uint32_t n_chrom, smooth_groups; } mkt_expected_info;
void mkt_expected_opts_default(mkt_expected_opts* o);
int mkt_matrix_expected(mkt_matrix* m, uint32_t res_index, const mkt_expected_opts* opts, mkt_expected_info* info);
int mkt_matrix_fetch_expected_cis(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, uint64_t* n_valid, uint64_t* count_sum, double* balanced_sum);
int mkt_matrix_fetch_expected_trans(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, uint64_t* n_valid, uint64_t* count_sum, double* balanced_sum, double* expected);
int mkt_matrix_fetch_expected_genome(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, uint64_t* n_valid, uint64_t* count_sum, double* balanced_sum, double* expected,
                                     double* expected_smooth);
#define MKT_VALUE_BALANCED 0
#define MKT_VALUE_OE 1
#define MKT_VALUE_OE_SMOOTH 2
int mkt_matrix_fetch_values(mkt_matrix* m, uint32_t res_index, int kind, uint64_t first, uint64_t n, double* out);
int mkt_matrix_expected_timing(const mkt_matrix* m, uint32_t res_index, double* setup_ms, double* sums_ms);

/* ---- loop calling: donut enrichment of every cell against its local neighbourhood, FDR thresholds, clustering --------------------
 * The last hot loop of the Hi-C toolchain: what the reference's own benchmarking runs on its .hic files (HiCCUPS at 10 kb).  The
 * definition is this project's own, modelled on HiCCUPS (Rao et al. 2014); parity with juicer_tools is UNPINNED (it is not run
 * anywhere here).  tests/loopsdef.py restates the definition in numpy.  All arithmetic is float64.
 *
 * Inputs, for one resolution: the cells (bin1 <= bin2, count), the chromosome ranges [off_c, off_c + n_c) and the state of the last
 * mkt_matrix_expected: its use_weights, w[k] and valid(k), E[d] = the genome-wide expected_smooth, v = ((double)count * w[bin1]) * w[bin2].
 * Options (mkt_loops_opts): peak p, window, window_max, min_ll_count, min_dist, max_dist (0 = none), fdr, cluster_radius.
 *  1. CANDIDATE cell (i, j): both bins in one chromosome c, both valid, min_dist <= j - i (and j - i <= max_dist when that is set).
 *     A candidate is TESTED when step 4 leaves every region defined and step 5 leaves every r_R <= 512.
 *  2. KEPT positions of an offset (a, b): (i + a, j + b) with both bins inside c's range, both valid and (j + b) - (i + a) >= 1.
 *     Regions for a window w:   DONUT  max(|a|, |b|) <= w, not (|a| <= p and |b| <= p), a != 0, b != 0
 *                               LL     1 <= a <= w, -w <= b <= -1, not (a <= p and b >= -p)           (towards the diagonal)
 *                               H      |a| <= 1, p < |b| <= w
 *                               V      p < |a| <= w, |b| <= 1
 *  3. WINDOW: w = window; while Csum_LL(w) < min_ll_count and w < window_max: w += 1.  Csum_LL = the exact integer sum of the counts of
 *     the stored cells at LL's kept positions.  All four regions use the final w, which is reported per cell.
 *  4. Per region R: Bsum_R = the sum of v over the stored cells at kept positions, Esum_R = the sum of E[(j + b) - (i + a)] over ALL kept
 *     positions.  Esum_R == 0 or no kept position: the region is UNDEFINED (status MKT_LOOP_UNDEFINED, r_R = e_R = NaN).
 *     e_R = (Bsum_R / Esum_R) * E[j - i]; the raw expected r_R = e_R / (w[i] * w[j]).
 *  5. CHUNKS: 28 edges, edge_k = ldexp(C[k % 3], k / 3) with C = {1.0, 1.2599210498948732, 1.5874010519681994} as those decimal
 *     literals (edge_27 = 512).  chunk_R = the smallest k with r_R <= edge_k, by comparisons only.  r_R > 512 (or not a number) in any
 *     region: status MKT_LOOP_OVER, counted, not tested.  The chunk of an undefined or over region is reported as 255.
 *  6. HISTOGRAM H_R[k][x] (uint64) = the tested cells with chunk_R == k and min(count, 2047) == x.
 *  7. THRESHOLDS, on the host, per (R, k) with lambda = edge_k: pmf_0 = exp(-lambda), pmf_x = (pmf_(x-1) * lambda) / x, cdf_x ascending,
 *     Q(0) = 1, Q(x) = max(0, 1 - cdf_(x-1)); n = sum_x H, O(x) = sum_(x' >= x) H; T_R[k] = the smallest x >= 1 with O(x) > 0 and
 *     n * Q(x) <= fdr * O(x); 2048 when there is none.
 *  8. ENRICHED: a tested cell with count >= T_R[chunk_R] for all four R.
 *  9. LOOPS: enriched cells of one chromosome are linked when max(|d bin1|, |d bin2|) <= cluster_radius; a loop is a connected component:
 *     its peak cell (the largest count, ties to the smallest cell index) with count, window and the four r_R, the number of cells and
 *     the bounding box.  Loops ascend by peak cell index.  (Done on the host: enriched cells are few.)
 * Out of scope: HiCCUPS's post-filter ratio thresholds, merging across resolutions, per-chromosome expected, a .hic reader.
 *
 * Determinism: no floating-point atomics (the histogram's are integers); a region's sums are formed by a fixed number of lanes, each
 * taking the rows a = -w + lane, + lanes, .. in ascending b, and a fixed shuffle tree: the same bits from call to call, process to
 * process and whatever route the pairs came by.  Against the numpy restatement (which adds in ascending (a, b)) Csum_LL, the window,
 * the kept positions and integer-valued Bsum are identical; Esum, e_R and r_R agree to summation-order rounding.
 *
 *   mkt_loops_opts_default        peak 2, window 5, window_max 20, min_ll_count 16, min_dist 8, max_dist 0, fdr 0.1, cluster_radius 2
 *   mkt_matrix_loops              valid after mkt_matrix_expected of that resolution (MKT_E_STATE "expected first" without tables, and
 *                                 before mkt_matrix_run); opts NULL = the defaults; MKT_E_ARG with a message for a bad index, a negative
 *                                 option, window <= peak, window_max < window or > 20, fdr outside (0, 1) or NaN, or a non-zero reserved.
 *                                 info may be NULL.  A later mkt_matrix_run, add, balance or expected of that resolution discards the results.
 *   mkt_matrix_fetch_loop_cells   per-cell results of cells [first, first + n) in the order of mkt_matrix_fetch; any pointer may be NULL;
 *                                 chunk, kept, r, e, bsum and esum hold 4 values per cell (DONUT, LL, H, V).  A cell that is no candidate
 *                                 has window 0, chunks 255, NaN and zeros.
 *   mkt_matrix_fetch_loop_hist    H as [4][28][2048] uint64
 *   mkt_matrix_fetch_loop_thresholds   T as [4][28] uint32
 *   mkt_matrix_fetch_loops        loops [first, first + n)
 *   mkt_matrix_loops_timing       device time (ms, HIP events) of the neighbourhood pass (both launches), the histogram and the flagging
 *                                 of the last mkt_matrix_loops of res_index.  A bad index is MKT_E_ARG without a message.
 * Memory: 151 bytes per cell stay resident with the results (7 GB for 46.5 M cells), non-candidates included; 104 of them are the
 * intermediate values (csum_ll, kept, bsum, esum, e) that mkt_matrix_fetch_loop_cells hands out for checking. */
#define MKT_LOOP_NONE 0        /* not a candidate */
#define MKT_LOOP_TESTED 1
#define MKT_LOOP_UNDEFINED 2
#define MKT_LOOP_OVER 3
typedef struct mkt_loops_opts {
    int32_t peak, window, window_max, min_ll_count, min_dist, max_dist;
    double fdr;
    int32_t cluster_radius;
    uint32_t reserved;       /* 0 */
} mkt_loops_opts;
typedef struct mkt_loops_info {
    uint64_t cells, candidates, tested, undefined, over;
    uint64_t grew;           /* candidates whose window is larger than opts.window */
    uint64_t at_max;         /* ... that stopped at window_max with Csum_LL < min_ll_count */
    uint64_t enriched, loops;
} mkt_loops_info;
typedef struct mkt_loop {
    uint64_t cell;           /* index of the peak cell in the order of mkt_matrix_fetch */
    uint32_t bin1, bin2, count, window, n_cells;
    uint32_t box[4];         /* min bin1, max bin1, min bin2, max bin2 of the component */
    uint32_t reserved;
    double r[4];             /* raw expected of the peak: DONUT, LL, H, V */
} mkt_loop;
void mkt_loops_opts_default(mkt_loops_opts* o);
int mkt_matrix_loops(mkt_matrix* m, uint32_t res_index, const mkt_loops_opts* opts, mkt_loops_info* info);
int mkt_matrix_fetch_loop_cells(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, uint8_t* status, uint8_t* window, uint8_t* chunk, double* r,
                                uint8_t* enriched, uint64_t* csum_ll, uint16_t* kept, double* bsum, double* esum, double* e);
int mkt_matrix_fetch_loop_hist(mkt_matrix* m, uint32_t res_index, uint64_t* hist);
int mkt_matrix_fetch_loop_thresholds(mkt_matrix* m, uint32_t res_index, uint32_t* thresholds);
int mkt_matrix_fetch_loops(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, mkt_loop* out);
int mkt_matrix_loops_timing(const mkt_matrix* m, uint32_t res_index, double* pass_ms, double* hist_ms, double* flag_ms);

/* ---- compartments: the leading eigenvectors of each chromosome's cis observed / expected - 1 matrix ------------------------------
 * What `juicer_tools eigenvector` and cooltools `eigs-cis` compute from the .hic / .cool.  The definition is this project's own,
 * modelled on cooltools eigs-cis; parity with cooltools and juicer_tools is UNPINNED (neither is run anywhere here).
 * tests/eigsdef.py restates the definition in numpy.  All arithmetic is float64.
 *
 * Inputs, for one resolution: the cells, the chromosome ranges [off_c, off_c + n_c) and the state of the last mkt_matrix_expected: its
 * use_weights, w[k] and valid(k), E[d] = the genome-wide expected_smooth, v = ((double)count * w[bin1]) * w[bin2].
 * Options (mkt_eigs_opts): n_eigs (1 .. 4), ignore_diags, clip, min_good, tol, max_iters; an optional phasing track p[nbins] (NaN = no value).
 *  1. GOOD bin of chromosome c: valid(k) and at least one stored cell (k, j) or (j, k) with j in c, valid(j) and |j - k| >= ignore_diags.
 *     n_good(c) counts them.  A chromosome with n_good < max(min_good, 9) is SKIPPED: eigenvalues NaN, vector entries NaN,
 *     iterations 0, converged 0.
 *  2. MATRIX A_c (symmetric, n_c x n_c, never formed on the GPU): for good i, j in c with |i - j| >= ignore_diags A[i][j] = oe - 1,
 *     where oe = v / E[|i - j|] for a stored cell, replaced by min(oe, clip) when clip > 0, and oe = 0 for an absent cell.  Every other
 *     entry is 0.  Equivalently A = S - (g g^T - B): S holds oe at the stored eligible positions, g is the 0/1 good indicator and
 *     B[i][j] = g_i g_j for |i - j| < ignore_diags, so (A x)_i = (S x)_i - g_i (g^T x) + g_i sum_{|i - j| < ignore_diags, j in c} g_j x_j.
 *  3. EIGENPAIRS: the n_eigs eigenpairs of A_c largest in |lambda|, in descending |lambda|; each vector has unit 2-norm over the good
 *     bins and is NaN elsewhere.  A chromosome is CONVERGED when every reported pair has ||A x - lambda x||_2 <= tol * |lambda_1| as
 *     computed on the device; otherwise the iteration stops after max_iters sweeps with converged = 0 and the pairs it has are still
 *     reported, normalised.  The procedure: a block of 8 columns, X_0 a fixed integer hash of (bin - off_c, column) zeroed on the
 *     other bins and orthonormalised; per iteration ONE sweep Y = A X, H = X^T Y (8 x 8 per chromosome), Rayleigh-Ritz
 *     H = S Theta S^T by a cyclic Jacobi with a fixed number of sweeps, Ritz vectors X S, residual columns Y S - X S Theta, the next
 *     X = orth(Y S).  A chromosome that is done freezes (a device-side flag per chromosome).
 *  4. ORIENTATION.  With a track: when sum x_i (p_i - pbar) over the good bins with a value (pbar their mean) is negative, the vector is
 *     flipped.  Without a track, or when that sum is exactly 0 or has no terms: the entry of largest |x_i| (ties to the lowest bin)
 *     is made positive.
 * An absent cell counts as -1: where the cis matrix is mostly empty the leading vector is the all-ones direction with
 * lambda ~ -n_good.  Compartments are meant for resolutions where cis is dense (100 kb .. 1 Mb).
 * Out of scope: percentile clipping (it needs a selection), per-arm views, trans eigenvectors, Pearson-correlation (juicer-style)
 * vectors, Lanczos.  (The saddle tables that judge the vectors are mkt_matrix_saddle below.)
 *
 * Determinism: no floating-point atomics; a row's sum is formed by a fixed number of lanes with a fixed stride and a fixed shuffle
 * tree (rows of more than 1024 cells: one workgroup, the four wave sums added in wave order); the per-chromosome dot products use
 * fixed chunks of 256 bins whose partial sums are added in chunk order; the 8 x 8 step runs on the host in a fixed order.  Everything
 * depends on (nbins, cells, options) only: the same bits from call to call, process to process and whatever route the pairs came by.
 *
 *   mkt_eigs_opts_default       n_eigs 3, ignore_diags 2, min_good 9, max_iters 300, tol 1e-8, clip 0 (none)
 *   mkt_matrix_eigs             valid after mkt_matrix_expected of that resolution (MKT_E_STATE "expected first" without tables); opts
 *                               NULL = the defaults; phasing: nbins doubles or NULL; MKT_E_ARG with a message for a bad index, n_eigs
 *                               outside 1 .. 4, a negative option, tol not inside (0, 1) or NaN, a NaN or negative clip or a non-zero
 *                               reserved.  info may be NULL.  A later mkt_matrix_run, add, balance or expected of that resolution
 *                               discards the results; loops and eigenvectors of one resolution do not disturb each other.
 *   mkt_matrix_fetch_eigvecs    vector k (0 .. n_eigs - 1) for bins [first, first + n)
 *   mkt_matrix_fetch_eigvals    chromosomes [first_chrom, first_chrom + n): lambda and resid as [n][n_eigs] (resid = the device's
 *                               ||A x - lambda x||_2), n_good, iterations, converged; any pointer may be NULL
 *   mkt_matrix_eigs_apply       y = A x for all chromosomes at once through the sweep kernel of the iteration: x and y are
 *                               [nbins][ncols], 1 <= ncols <= 8; x is used as given on good bins and treated as 0 elsewhere; y is 0 on
 *                               the other bins and on skipped chromosomes.  Needs the tables like mkt_matrix_eigs; keeps no result.
 *   mkt_matrix_eigs_timing      of the last mkt_matrix_eigs of res_index (ms, HIP events): the setup (row pointers and transposed copy
 *                               when no balance built them, good flags, X_0), the sweeps alone, and the rest of the iteration loop
 *                               (reductions, the 8 x 8 step on the host with its copies).  A bad index is MKT_E_ARG without a message. */
typedef struct mkt_eigs_opts {
    int32_t n_eigs, ignore_diags, min_good, max_iters;
    double tol, clip;
    uint32_t reserved;       /* 0 */
} mkt_eigs_opts;
typedef struct mkt_eigs_info { uint32_t n_chrom, solved, converged, skipped, max_iterations; } mkt_eigs_info;
void mkt_eigs_opts_default(mkt_eigs_opts* o);
int mkt_matrix_eigs(mkt_matrix* m, uint32_t res_index, const mkt_eigs_opts* opts, const double* phasing, mkt_eigs_info* info);
int mkt_matrix_fetch_eigvecs(mkt_matrix* m, uint32_t res_index, uint32_t k, uint64_t first, uint64_t n, double* out);
int mkt_matrix_fetch_eigvals(mkt_matrix* m, uint32_t res_index, uint32_t first_chrom, uint32_t n, double* lambda, double* resid, uint32_t* n_good,
                             uint32_t* iterations, uint8_t* converged);
int mkt_matrix_eigs_apply(mkt_matrix* m, uint32_t res_index, const mkt_eigs_opts* opts, const double* x, uint32_t ncols, double* y);
int mkt_matrix_eigs_timing(const mkt_matrix* m, uint32_t res_index, double* setup_ms, double* sweep_ms, double* small_ms);

/* ---- domains: the diamond insulation score of every bin at up to four nested windows, and the boundaries called from it -----------
 * What cooltools `insulation` computes from a .cool (Crane et al. 2015): the analysis the reference's own benchmarking runs on its
 * .hic files besides loops.  The definition is this project's own, modelled on cooltools insulation; parity with cooltools is
 * UNPINNED (it is not run anywhere here).  tests/insuldef.py restates the definition in numpy.  All floating point is float64.
 *
 * Inputs, for one resolution: the cells (bin1 <= bin2, count), the chromosome ranges [off_c, off_c + n_c) and use_weights: with 0
 * every bin is valid and w = 1; with 1 w is the weights of the last mkt_matrix_balance and valid(k) means w[k] is not NaN.
 * v = ((double)count * w[bin1]) * w[bin2]: two multiplications in this order, never fused with the addition that follows.
 * Options (mkt_insulation_opts): n_windows (1 .. 4), window[4] in bins (strictly ascending, each 1 .. 1024), ignore_diags,
 * use_weights, min_frac_valid, min_strength.
 *  1. POSITIONS of bin i in chromosome c for a window W: (a, b) = (i - p, i + q) with 0 <= p, q < W, p + q >= ignore_diags, a >= off_c and
 *     b < off_c + n_c.  A position is KEPT when valid(a) and valid(b) (valid(i) itself is not asked for).
 *     n_full(W) = #{(p, q): 0 <= p, q < W, p + q >= ignore_diags}: the unclipped count, the same for every i.
 *  2. Per (i, W): n_valid (uint64) = the kept positions; csum (uint64, exact) = the sum of count over the stored cells at kept
 *     positions; bsum = the sum of v over the same cells.  An absent cell at a kept position adds 0 and still counts in n_valid.
 *  3. SCORE = bsum / (double)n_valid; NaN when n_full == 0, n_valid == 0 or (double)n_valid < min_frac_valid * (double)n_full.  With
 *     the default min_frac_valid the clipped diamonds at chromosome ends are therefore NaN; with min_frac_valid = 0 they are scored.
 *  4. NORMALISATION, on the host, per chromosome and window: mean_c = the sum, in ascending bin order, of the scores that are finite
 *     and > 0, divided by their number; L[i] = log2(score[i] / mean_c), NaN when the score is NaN or 0 or the chromosome has no such
 *     score.
 *  5. MINIMA, on the host: inside a chromosome a SEGMENT is a maximal run of consecutive bins with finite L.  A plateau [s, e] of equal
 *     value x inside a segment is a minimum when s - 1 and e + 1 are in the segment and both hold values > x; it is reported at bin s.
 *  6. STRENGTH of a minimum: walk left from s - 1 while in the segment and L[j] >= x and take the largest value seen, the same to the
 *     right from e + 1; strength = min(left, right) - x.  NaN on every bin that is not a reported minimum.
 *  7. BOUNDARY: a minimum with strength >= min_strength.
 * Out of scope: Otsu / Li automatic thresholds, min_dist_bad_bin, per-arm views, merging boundaries across windows, a dense or
 * sliding-sum path.
 *
 * Determinism: no floating-point atomics.  The summation order of bsum, with W_max the largest window: G lanes own bin i, G = 64 for
 * X >= 48, 32 for X >= 24, 16 for X >= 12, else 8, where X = W_max when the matrix holds at least one cell per bin and W_max / 2
 * (integer) otherwise.  Lane l takes the rows a = i - p for p = l, l + G, l + 2 G, .. (p < W_max, a >= off_c), each row's stored cells
 * in ascending b, and adds every v to its partial sum of the cell's SHELL k = the smallest k with max(p, q) < window[k], starting
 * from 0.0.  Per shell the lanes are added by the tree lane l += lane l + d for d = G / 2, G / 4, .. 1; window k's bsum is then
 * shell 0 + shell 1 + .. + shell k, added in that order.  n_valid and csum are integers (n_valid from a prefix count of the valid
 * bins, never through a float).  G, the stride, the tree and the order depend on (nbins, cells, options) only: the same bits from
 * call to call, process to process and by every route (add, add_device, add_keys).  Against the numpy restatement (which adds in
 * ascending (a, b)) n_valid, csum, the NaN pattern and integer-valued bsum are identical; other bsum agree to summation-order
 * rounding.  Asking for several windows at once may round bsum differently from asking for one (the shells).
 *
 *   mkt_insulation_opts_default   n_windows 3, window {5, 10, 25}, ignore_diags 2, use_weights 1, min_frac_valid 0.66, min_strength 0.2
 *   mkt_matrix_insulation         valid after mkt_matrix_run (MKT_E_STATE before it) and, with use_weights 1, after mkt_matrix_balance of
 *                                 that resolution (MKT_E_STATE "balance first"); opts NULL = the defaults; MKT_E_ARG with a message
 *                                 for a bad index, n_windows outside 1 .. 4, windows not strictly ascending or outside 1 .. 1024, a
 *                                 negative ignore_diags, use_weights not 0 / 1, min_frac_valid outside [0, 1] or NaN, a negative or NaN
 *                                 min_strength or a non-zero reserved.  info may be NULL.  A later mkt_matrix_run, add or balance of
 *                                 that resolution discards the results; expected tables, loops, eigenvectors and insulation of one
 *                                 resolution do not disturb each other.
 *   mkt_matrix_fetch_insulation   window k (0 .. n_windows - 1) for bins [first, first + n); any pointer may be NULL; MKT_E_ARG with
 *                                 a message for k >= n_windows or a bad range
 *   mkt_matrix_insulation_timing  of the last mkt_matrix_insulation of res_index (ms, HIP events): the setup (the copy of the weights,
 *                                 the prefix count on the host and its upload; 0 without weights) and the sweep.  A bad index is
 *                                 MKT_E_ARG without a message. */
typedef struct mkt_insulation_opts {
    int32_t n_windows;
    int32_t window[4];       /* bins; the first n_windows are used */
    int32_t ignore_diags, use_weights;
    uint32_t reserved;       /* 0 */
    double min_frac_valid, min_strength;
} mkt_insulation_opts;
typedef struct mkt_insulation_info {
    uint64_t defined[4];     /* per window: bins with a finite log2 score */
    uint64_t minima[4], boundaries[4];
    uint32_t n_chrom, reserved;
} mkt_insulation_info;
void mkt_insulation_opts_default(mkt_insulation_opts* o);
int mkt_matrix_insulation(mkt_matrix* m, uint32_t res_index, const mkt_insulation_opts* opts, mkt_insulation_info* info);
int mkt_matrix_fetch_insulation(mkt_matrix* m, uint32_t res_index, uint32_t k, uint64_t first, uint64_t n, uint64_t* n_valid, uint64_t* csum, double* bsum,
                                double* score, double* log2_score, double* strength, uint8_t* boundary);
int mkt_matrix_insulation_timing(const mkt_matrix* m, uint32_t res_index, double* setup_ms, double* sweep_ms);

/* ---- pileups: the average contact map in a small window around a list of features; aggregate peak analysis (APA) ------------------
 * The step that judges the calls: with the called loops as the list it is `juicer_tools apa`, with the insulation boundaries the
 * on-diagonal pileup of `cooltools pileup` / coolpup.py, with a user's pairs of anchors a comparison of matrices at known features.
 * The definition is this project's own, modelled on those; parity with juicer_tools and cooltools is UNPINNED (neither is run anywhere
 * here).  tests/piledef.py restates the definition in numpy.  All floating point is float64.
 *
 * Inputs, for one resolution: the cells (bin1 <= bin2, count), the chromosome ranges [off_c, off_c + n_c) and the state of the last
 * mkt_matrix_expected: its use_weights, w[k] and valid(k), the genome-wide expected[d] and expected_smooth[d];
 * v = ((double)count * w[bin1]) * w[bin2].  n features (a_f, b_f) as global bin ids in the order given; duplicates are allowed.
 * Options (mkt_pileup_opts): flank (1 .. 32, side S = 2 * flank + 1), corner (1 .. flank), kind (MKT_VALUE_BALANCED, MKT_VALUE_OE or
 * MKT_VALUE_OE_SMOOTH), ignore_diags, edges (0 / 1), min_dist, max_dist (0 = none).
 *  1. STATUS of a feature: MKT_PILE_TRANS when the anchors lie in different chromosomes; else MKT_PILE_DIST when b - a < min_dist, or
 *     b - a > max_dist when that is set; else MKT_PILE_EDGE when edges == 0 and some bin of a +- flank or b +- flank leaves the
 *     chromosome's range; else MKT_PILE_USED.  Only USED features contribute.  a > b or a bin >= nbins is MKT_E_ARG with a message that
 *     names the feature, and nothing is computed.
 *  2. POSITIONS: (p, q) with -flank <= p, q <= flank denotes i = a + p, j = b + q.  The matrix is symmetric: the cell looked up is
 *     (min(i, j), max(i, j)) and d = |j - i|.  A position is KEPT when both bins are inside the chromosome, both are valid and
 *     d >= ignore_diags.
 *  3. VALUE of a stored cell at a kept position: v for BALANCED, v / expected[d] for OE, v / expected_smooth[d] for OE_SMOOTH: one IEEE
 *     division, never fused, no reciprocal approximation.  A stored cell with two valid bins has a divisor > 0 (expected, step 7).
 *  4. Per position over the used features: n[p][q] (uint64) = the features where the position is kept; csum[p][q] (uint64, exact) = the
 *     sum of count over the stored cells at kept positions; vsum[p][q] = the sum of the values over the same cells.  An absent cell at
 *     a kept position adds nothing and still counts in n.  mean = vsum / (double)n, NaN when n == 0.
 *  5. SUMMATION ORDER of vsum, which is part of the definition: chunk c holds the features [256 c, 256 c + 256) by their index as given
 *     (features that are not used keep their slots); T_c[p][q] starts from 0.0 and takes the values of the chunk's used features in
 *     ascending index; vsum starts from 0.0 and takes T_0, T_1, .. in ascending c.  No floating-point atomics.  The result is the same
 *     bits from call to call, process to process and by every route (add, add_device, add_keys), and the same bits as
 *     tests/piledef.py, which adds in this same order.
 *  6. SCORES, on the host, from mean.  Boxes of corner x corner positions: LL p in [flank - corner + 1, flank], q in
 *     [-flank, -flank + corner - 1] (the corner towards the diagonal, as in the loops stage); UL p low, q low; UR p low, q high; LR p
 *     high, q high.  mean_B = the sum of the finite mean over the box in ascending (p, q), divided by their number; NaN when there are
 *     none.  peak = mean[0][0]; p2ll = peak / mean_LL, p2ul, p2ur, p2lr the same; p2m = peak / (the mean of the finite values at all
 *     positions but (0, 0)); z_ll = (peak - mean_LL) / sd_LL, sd_LL = the square root of the sum of (x - mean_LL)^2 in ascending (p, q)
 *     over (k - 1), NaN with fewer than two finite values.
 * Out of scope: shifted or random controls, rescaled (variable-size) features, by-strand or by-distance splitting, trans pileups,
 * per-feature snippets, a .hic / .cool reader.
 *
 *   mkt_pileup_opts_default         flank 10, corner 6, kind OE_SMOOTH, ignore_diags 2, edges 0, min_dist 0, max_dist 0
 *   mkt_matrix_pileup               valid after mkt_matrix_expected of that resolution (MKT_E_STATE "expected first" without tables,
 *                                   "pileup before run" before mkt_matrix_run); opts NULL = the defaults; n == 0 is allowed (all counts
 *                                   zero, mean and scores NaN).  MKT_E_ARG with a message for a bad index, flank outside 1 .. 32, corner
 *                                   outside 1 .. flank, a bad kind, a negative option, edges not 0 / 1, max_dist set and below min_dist,
 *                                   a non-zero reserved, a bad feature (step 1) or NULL bins with n > 0; MKT_E_CAPACITY for n >= 2^32.
 *                                   info may be NULL.  A refused call leaves the previous results alone.  A later mkt_matrix_run, add,
 *                                   balance or expected of that resolution discards the results; loops, eigenvectors, insulation and
 *                                   pileup of one resolution do not disturb each other.  Features go to the device in batches of 4096
 *                                   chunks (2^20 features), so the partial sums take at most 4096 * S^2 * 20 bytes whatever n is; the
 *                                   bits do not depend on the batch.
 *   mkt_matrix_fetch_pileup         n, csum, vsum, mean as [side][side], row p, column q (index [p + flank][q + flank]); any may be NULL
 *   mkt_matrix_fetch_pileup_status  the MKT_PILE_* of features [first, first + n); MKT_E_ARG with a message for a bad range
 *   mkt_matrix_pileup_timing        of the last mkt_matrix_pileup of res_index (ms, HIP events, added over the batches): the setup (the
 *                                   upload of the features and their statuses) and the sweep (the chunk kernel and the fold).  A bad
 *                                   index is MKT_E_ARG without a message; 0, 0 without results. */
#define MKT_PILE_USED 1
#define MKT_PILE_TRANS 2
#define MKT_PILE_EDGE 3
#define MKT_PILE_DIST 4
typedef struct mkt_pileup_opts {
    int32_t flank, corner, kind, ignore_diags, edges, min_dist, max_dist;
    uint32_t reserved;       /* 0 */
} mkt_pileup_opts;
typedef struct mkt_pileup_info {
    uint64_t features, used, trans, edge, dist;
    uint32_t side, chunks;
    double peak, p2ll, p2ul, p2ur, p2lr, p2m, z_ll;
} mkt_pileup_info;
void mkt_pileup_opts_default(mkt_pileup_opts* o);
int mkt_matrix_pileup(mkt_matrix* m, uint32_t res_index, const uint32_t* bin1, const uint32_t* bin2, uint64_t n, const mkt_pileup_opts* opts, mkt_pileup_info* info);
int mkt_matrix_fetch_pileup(mkt_matrix* m, uint32_t res_index, uint64_t* n, uint64_t* csum, double* vsum, double* mean);
int mkt_matrix_fetch_pileup_status(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, uint8_t* status);
int mkt_matrix_pileup_timing(const mkt_matrix* m, uint32_t res_index, double* setup_ms, double* sweep_ms);

/* ---- saddle tables and compartment strength: what judges the compartment eigenvectors -------------------------------------------------
 * Bins are ranked by a track (an eigenvector of mkt_matrix_eigs, or any caller's values) and cut into Q groups; the mean observed /
 * expected of every pair of groups is tabulated and reduced to one number, the compartment strength (AA + BB over AB).  The definition
 * is this project's own, modelled on cooltools `saddle`; parity with cooltools is UNPINNED (it is not run anywhere here).
 * tests/saddledef.py restates the definition in numpy.  All floating point is float64.
 *
 * Inputs, for one resolution: the cells (bin1 <= bin2, count) in the order of mkt_matrix_fetch, the chromosome ranges
 * [off_c, off_c + n_c) and the state of the last mkt_matrix_expected: its use_weights, w[k] and valid(k), the genome-wide expected[d] and
 * expected_smooth[d] and the trans expected of a block; v = ((double)count * w[bin1]) * w[bin2].  A track t[nbins] of doubles: NaN means
 * no value, +-inf are ordinary values.  Options (mkt_saddle_opts): n_groups Q (2 .. 64), trim_lo, trim_hi (basis points, >= 0,
 * trim_lo + trim_hi < 10000), contact (0 cis, 1 trans), kind (MKT_VALUE_OE or MKT_VALUE_OE_SMOOTH; only the cis divisor differs),
 * min_diag, max_diag (cis; 0 = no upper limit), corner (0 = max(1, Q / 5), else 1 .. Q / 2).
 *  1. GROUPS, on the host, integers only.  The candidates are the bins with valid(k) and a non-NaN t[k], ordered by t ascending; ties go
 *     to the lower bin, and -0.0 == 0.0 is a tie.  With T candidates, lo = T * trim_lo / 10000 and hi = T * trim_hi / 10000 (integer
 *     division); the candidates of rank r in [lo, T - hi) are kept, K = T - hi - lo of them, and get g = (r - lo) * Q / K.  Every other
 *     bin gets g = 255 (none).  K < Q leaves some groups empty; K == 0 is not an error (every table entry is zero, the means and scores
 *     are NaN).  Per group: the number of its bins and the track values of its lowest and of its highest rank (NaN for an empty group).
 *  2. A stored cell (i, j, count), i <= j, is USED when both bins have a group and, cis: both lie in one chromosome, min_diag <= j - i,
 *     and j - i <= max_diag when that is set; trans: they lie in different chromosomes.  Its value x = v / expected[j - i] (or
 *     expected_smooth[j - i]) for cis, v / expected(block) for trans: one IEEE division, never fused, no reciprocal approximation.  Its
 *     entry is the unordered pair (min(g_i, g_j), max(g_i, g_j)).
 *  3. SUMMATION ORDER, which is part of the definition: chunk c is the stored cells [4096 c, 4096 c + 4096) (cells that are not used
 *     keep their slots); T_c[entry] starts from +0.0 and takes the values of the chunk's used cells of that entry in ascending cell
 *     index; vsum[entry] starts from +0.0 and takes T_0, T_1, .. in ascending c.  nnz (the used cells) and csum (the sum of their
 *     counts) are exact uint64.  No floating-point atomics.  The order depends on the cells alone: the same bits from call to call,
 *     process to process and by every route (add, add_device, add_keys), and the same bits as tests/saddledef.py.
 *  4. POSITIONS: n[entry] (uint64, exact) = the pairs of bins (i <= j) that would be used if stored (an absent cell is a zero of the map
 *     and counts in the mean): cis, in one chromosome with the diagonal in range and both bins grouped; trans, in different chromosomes
 *     and both grouped.
 *  5. TABLES, each [Q][Q] and symmetric (S[a][b] = S[b][a] = the unordered entry): n, nnz, csum, vsum and mean = vsum / (double)n, the
 *     quiet NaN when n == 0.
 *  6. SCORES, on the host, never fused, for k = 1 .. Q / 2: the vsum (in doubles) and the n (in uint64) of each block are added over
 *     the unordered entries a <= b in ascending (a, b), row-major: BB(k) the entries with b < k, AA(k) those with a >= Q - k, AB(k)
 *     those with a < k and b >= Q - k.  strength[k] = ((BBs + AAs) / (double)(BBn + AAn)) / (ABs / (double)ABn),
 *     aa_ab[k] = (AAs / AAn) / (ABs / ABn), bb_ab[k] likewise.  A division by zero gives the quiet NaN, and every NaN is the one quiet
 *     NaN.  The info carries the three at k = corner.
 * Out of scope: per-chromosome or per-arm views, group edges given as values or quantiles of the genome-wide distribution (`vrange`,
 * `qrange` of cooltools), the saddle plot itself, saddles of several tracks at once.
 *
 *   mkt_saddle_opts_default           n_groups 50, trim 250 / 250, contact 0, kind OE, min_diag 2, max_diag 0, corner 0
 *   mkt_matrix_saddle                 valid after mkt_matrix_expected of that resolution (MKT_E_STATE "expected first" without tables,
 *                                     "saddle before run" before mkt_matrix_run); opts NULL = the defaults.  MKT_E_ARG with a message for
 *                                     a bad index, n_groups outside 2 .. 64, a negative trim or trim_lo + trim_hi >= 10000, a bad contact,
 *                                     kind or corner, a negative diagonal, max_diag set and below min_diag, a non-zero reserved or a NULL
 *                                     track.  info may be NULL.  A refused call leaves the previous results alone.  A later
 *                                     mkt_matrix_run, add, balance or expected of that resolution discards the results; loops,
 *                                     eigenvectors, insulation, pileup and saddle of one resolution do not disturb each other.  The partial
 *                                     tables of all chunks are resident at once (chunks * Q (Q + 1) / 2 * 8 bytes): MKT_E_NOMEM otherwise.
 *   mkt_matrix_fetch_saddle           n, nnz, csum, vsum, mean as [Q][Q]; any may be NULL
 *   mkt_matrix_fetch_saddle_groups    the group byte of bins [first, first + n); MKT_E_ARG with a message for a bad range
 *   mkt_matrix_fetch_saddle_edges     per group [Q]: its bins, the track value of its lowest and highest rank; any may be NULL
 *   mkt_matrix_fetch_saddle_profile   strength, aa_ab, bb_ab as [Q / 2], index k - 1; any may be NULL
 *   mkt_matrix_saddle_timing          of the last mkt_matrix_saddle of res_index (ms): the setup (on the host: the groups, the positions,
 *                                     the copy of the weights and the upload of the groups; wall time) and the sweep (the chunk kernel
 *                                     and the fold; HIP events).  A bad index is MKT_E_ARG without a message; 0, 0 without results. */
#define MKT_SADDLE_NONE 255
typedef struct mkt_saddle_opts {
    int32_t n_groups, trim_lo, trim_hi, contact, kind, min_diag, max_diag, corner;
    uint32_t reserved;       /* 0 */
} mkt_saddle_opts;
typedef struct mkt_saddle_info {
    uint64_t candidates, kept, cells_used;
    uint32_t n_groups, chunks, corner, reserved;
    double strength, aa_ab, bb_ab;
} mkt_saddle_info;
void mkt_saddle_opts_default(mkt_saddle_opts* o);
int mkt_matrix_saddle(mkt_matrix* m, uint32_t res_index, const mkt_saddle_opts* opts, const double* track, mkt_saddle_info* info);
int mkt_matrix_fetch_saddle(mkt_matrix* m, uint32_t res_index, uint64_t* n, uint64_t* nnz, uint64_t* csum, double* vsum, double* mean);
int mkt_matrix_fetch_saddle_groups(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, uint8_t* group);
int mkt_matrix_fetch_saddle_edges(mkt_matrix* m, uint32_t res_index, uint64_t* bins, double* lo, double* hi);
int mkt_matrix_fetch_saddle_profile(mkt_matrix* m, uint32_t res_index, double* strength, double* aa_ab, double* bb_ab);
int mkt_matrix_saddle_timing(const mkt_matrix* m, uint32_t res_index, double* setup_ms, double* sweep_ms);

/* ---- replicate comparison: the stratum-adjusted correlation coefficient (SCC) of two matrices ---------------------------------------------
 * Do two contact maps agree?  Both are smoothed with a box filter and correlated diagonal by diagonal (stratum by stratum); the
 * correlations are combined with weights into one number per chromosome and one for the genome.  The definition is this project's own,
 * modelled on HiCRep (Yang et al. 2017); parity with HiCRep and hicreppy is UNPINNED (neither is run anywhere here).  Out of scope:
 * HiCRep's rank-based variance weights (they need a sort per stratum; MKT_SCC_WEIGHT_VAR below uses the plain variances) and the
 * down-sampling of both maps to equal depth, which is a separate step (count_a and count_b of the info show a depth imbalance).
 * tests/sccdef.py restates the definition in numpy.  All floating point is float64; nothing is fused.
 *
 * Inputs: two matrix objects A and B on one device with equal chromosome tables (names and lengths, in order), a resolution index in
 * each naming the same resolution r, both run.  A and B may be the same object.  Options (mkt_scc_opts): h (0 .. 16: the half width of
 * the filter), min_diag, max_diag (0 <= min_diag <= max_diag; max_diag 0 = every diagonal of the longest chromosome), use_weights (0,
 * 1), weighting (MKT_SCC_WEIGHT_N, MKT_SCC_WEIGHT_VAR), min_n (>= 2), slab_rows (0 = the library chooses, else a positive multiple of
 * 256: how many rows of a chromosome are resident as a dense band at a time; the results do not depend on it), reserved (0).
 *  1. JOINT VALIDITY.  use_weights 0: every bin is jointly valid and the value of a cell is (double)count.  use_weights 1 (both
 *     resolutions balanced, MKT_E_STATE otherwise): bin k is jointly valid when its weight is NaN neither in A nor in B; the value in A
 *     is ((double)count * wA[bin1]) * wA[bin2], in B the same with wB.
 *  2. FULL MATRICES, per chromosome c of n_c bins, indices relative to the chromosome: F_A[i][j] = F_A[j][i] = the value of A's stored
 *     cell (min, max), 0.0 when the cell is absent or one of the bins is not jointly valid; F_B likewise.  Cells of other chromosomes
 *     and trans cells never enter.
 *  3. SMOOTHING.  nv(a, b) = the jointly valid bins with relative index in [max(a, 0), min(b, n_c - 1)].
 *     R[i'][j] = F[i'][j - h] + F[i'][j - h + 1] + .. + F[i'][j + h], added left to right, terms outside [0, n_c) being 0.0;
 *     W[i][j] = R[i - h][j] + .. + R[i + h][j] in ascending i', rows outside the chromosome being 0.0;
 *     x(i, j) = W_A[i][j] / (double)(nv(i - h, i + h) * nv(j - h, j + h)), y(i, j) the same from B.
 *  4. STRATA.  For d in [min_diag, max_diag] and i in [0, n_c - d) the position (i, i + d) is a CANDIDATE when both bins are jointly
 *     valid, and USED when it is a candidate and x != 0 || y != 0 (as in HiCRep, a position that is zero in both maps is left out).
 *  5. SUMS per stratum (c, d): n_cand and n (the candidates and the used positions, exact uint64) and Sx, Sy, Sxx, Syy, Sxy, the sums of
 *     x, y, x * x, y * y, x * y over the used positions, every product rounded on its own.  SUMMATION ORDER, which is part of the
 *     definition: chunk q holds the positions with i in [256 q, 256 q + 256), an unused slot or a slot past the end holding 0.0;
 *     inside a chunk, for half = 128, 64, .., 1: s[k] = s[k] + s[k + half] for k < half; then the chunks are added in ascending q.
 *     No floating-point atomics: the same bits from call to call, by every route and for every slab_rows, and the same bits as
 *     tests/sccdef.py.
 *  6. SCORES per stratum, on the host, in this order of operations: mx = Sx / n, my = Sy / n, vx = Sxx / n - mx * mx,
 *     vy = Syy / n - my * my, cv = Sxy / n - mx * my.  The stratum is SCORED when n >= min_n, vx > 0x1p-40 * (Sxx / n) and
 *     vy > 0x1p-40 * (Syy / n).  Then rho = cv / sqrt(vx * vy) and the weight w = (double)n (WEIGHT_N) or n * sqrt(vx * vy)
 *     (WEIGHT_VAR).  A stratum that is not scored has rho = NaN and w = 0.
 *  7. PER CHROMOSOME: num_c = the sum of w * rho and den_c = the sum of w over the scored strata in ascending d;
 *     scc_c = num_c / den_c, NaN when no stratum is scored.
 *  8. GENOME-WIDE: scc = (the sum of num_c) / (the sum of den_c) over the chromosomes in table order, NaN when nothing is scored.
 *     Every NaN is the one quiet NaN.
 *  9. The strata table has n_chrom * (max_diag - min_diag + 1) rows, chromosome-major; a stratum with d >= n_c has n = 0 and is not
 *     scored.
 * 10. Exchanging A and B exchanges x and y (Sx with Sy, Sxx with Syy, count_a with count_b) and changes nothing else, bit for bit.
 *
 *   mkt_scc_opts_default           h 5, min_diag 0, max_diag 0, use_weights 0, weighting MKT_SCC_WEIGHT_N, min_n 3, slab_rows 0
 *   mkt_matrix_scc                 opts NULL = the defaults; info may be NULL.  MKT_E_ARG with a message (on a) for a bad index, unequal
 *                                  resolutions or chromosome tables, different devices, an option out of range, a non-zero reserved
 *                                  word, b NULL; MKT_E_STATE "scc before run" when either object has not been run, and with use_weights
 *                                  when either resolution has no weights; MKT_E_NOMEM with a message when the two bands do not fit at
 *                                  the smallest slab (or at the slab_rows given), or when the partial sums of a chromosome (its chunks
 *                                  * strata * 56 bytes) do not.  Everything is checked before anything is changed and the results
 *                                  are built aside: a refused or failed call leaves the previous results alone.  The results live on
 *                                  a at res_a and are a snapshot: a later change of b leaves them alone; a later mkt_matrix_run, add
 *                                  or balance of a discards them.  The info: n_chrom, strata (per chromosome), the totals of candidates
 *                                  and of used positions, the scored strata, count_a and count_b (the sum of the counts of the stored
 *                                  cis cells with both bins jointly valid and min_diag <= bin2 - bin1 <= max_diag, of A and of B) and scc.
 *   mkt_matrix_fetch_scc_strata    rows [first, first + n) of the strata table; any pointer may be NULL; MKT_E_ARG with a message for a
 *                                  bad range
 *   mkt_matrix_fetch_scc_chrom     per chromosome [first, first + n): scc_c, num_c, den_c and the scored strata; any may be NULL
 *   mkt_matrix_scc_timing          of the last mkt_matrix_scc of res_index (ms, HIP events, added over the slabs): the fill (zeroing and
 *                                  scattering the bands) and the sweep (with the fold).  A bad index is MKT_E_ARG without a message;
 *                                  0, 0 without results. */
#define MKT_SCC_WEIGHT_N 0
#define MKT_SCC_WEIGHT_VAR 1
typedef struct mkt_scc_opts {
    int32_t h, min_diag, max_diag, use_weights, weighting, min_n, slab_rows;
    uint32_t reserved[3];    /* 0 */
} mkt_scc_opts;
typedef struct mkt_scc_info {
    uint32_t n_chrom, strata;
    uint64_t candidates, used, scored, count_a, count_b;
    double scc;
} mkt_scc_info;
void mkt_scc_opts_default(mkt_scc_opts* o);
int mkt_matrix_scc(mkt_matrix* a, uint32_t res_a, mkt_matrix* b, uint32_t res_b, const mkt_scc_opts* opts, mkt_scc_info* info);
int mkt_matrix_fetch_scc_strata(mkt_matrix* a, uint32_t res_a, uint64_t first, uint64_t n, uint64_t* n_cand, uint64_t* n_used, double* sx, double* sy, double* sxx,
                                double* syy, double* sxy, double* rho, double* w);
int mkt_matrix_fetch_scc_chrom(mkt_matrix* a, uint32_t res_a, uint64_t first, uint64_t n, double* scc, double* num, double* den, uint64_t* n_scored);
int mkt_matrix_scc_timing(const mkt_matrix* a, uint32_t res_a, double* fill_ms, double* sweep_ms);

/* ---- viewpoint contact profiles (a virtual 4C): one chromosome against the rest of the genome -----------------------------------------------
 * The contacts between one chromosome (the VIEWPOINT, e.g. a viral episome such as chrEBV) and a set of PARTNER chromosomes, the two sides
 * binned at two different sizes, which the square matrices cannot express.  This is the reference's util/analyze.EBV (its two Perl
 * scripts): with origin 0 and second_side_only 1 the three texts made from these results are theirs byte for byte (tests/golden/
 * viewpoint_golden.json holds their output; tests/viewpointdef.py restates the definition).  Integers only on the device.
 *
 * Input: the resident pair records of a matrix object that has been run: table index and 1-based position of the two sides of every
 * pair, in the order the sides were added (.pairs columns 2, 3 and 4, 5).  The resolutions of the object play no part.
 * Options (mkt_viewpoint_opts):
 *   viewpoint          table index of the viewpoint chromosome
 *   partner_mask       one byte per chromosome of the table, non-zero = partner; NULL = every chromosome but the viewpoint.  The byte of
 *                      the viewpoint itself must be 0 (cis profiles from a sub-range of a chromosome are out of scope).
 *   vbin, pbin         bin sizes in bp of the viewpoint side and of the partner side, each at least 1
 *   origin             0: bin = pos / size, the reference's int(pos / bin) on the 1-based position; 1: bin = (pos - 1) / size, the
 *                      convention of the matrices
 *   second_side_only   0: a pair matches when one side is on the viewpoint and the other on a partner, whichever is which;
 *                      1: the reference's rule, the viewpoint must be the second side as stored and the partner the first
 *   min_count          at least 1: the smallest count of a cell of the partner track
 *   hotspot_ratio      in [0, 1)
 *   reserved           0
 * A record the matrix stage skipped (unknown chromosome, position 0 or past the length) or that is no pair never matches.  DEVIATION:
 * the Perl scripts have no table and count such pairs.
 * Results (counts exact uint32, totals uint64); they depend on the multiset of records only, with second_side_only 0 not on which side of
 * a pair was written first either; input order, chunking and the route (add, add_device, add_keys) never change a byte:
 *   total              the matching pairs
 *   LINK TABLE         the non-empty cells (viewpoint bin, partner chromosome, partner bin, count), strictly ascending in that order
 *   VIEWPOINT TRACK    dense counts of the viewpoint bins 0 .. the largest occupied one; length 0 when nothing matched.  DEVIATION: the
 *                      Perl prints one line of zeros and warnings then.
 *   PARTNER TRACK      the cells (partner chromosome, partner bin, count) with count >= min_count, ascending by (chromosome NAME bytewise,
 *                      bin): the order of `LC_ALL=C sort -k1,1 -k2,2n`
 * HOTSPOT CUT, on the host: over the distinct counts v of the link table in descending order, accum += v * (links with count v); at the
 * first v where accum > (uint64)((double)total * hotspot_ratio) (">", not ">=") min_loop = v + 1; a min_loop above the largest count becomes
 * the largest count.  0 without links.
 * LINKS TEXT (csrc/mkt_viewpoint.h, vp_links_text): the links with count >= min_loop in the bytewise order of the text
 * "<viewpoint bin>\t<hs name>\t<partner bin>" in decimal (so 10 sorts before 2), hs name = the chromosome name with its first "chr",
 * wherever it stands, replaced by "hs"; each as  hs0 \t i * vbin * 5000 \t i * vbin * 5000 + vbin * 5000 \t <hs name> \t j * pbin \t
 * j * pbin + pbin \t thickness=<t>p  with t = (int)(log((double)count) / log(2.0)) in doubles through the C library (not a bit length).
 * A viewpoint chromosome whose last bin end, bins * vbin * 5000, does not stay below 2^63 is refused (MKT_E_ARG).
 *
 *   mkt_viewpoint_opts_default        vbin 200, pbin 1000000, origin 0, second_side_only 0, min_count 1, hotspot_ratio 0.01, mask NULL
 *   mkt_matrix_viewpoint              opts NULL = the defaults (viewpoint 0); info may be NULL.  MKT_E_STATE "viewpoint before run" before
 *                                     mkt_matrix_run.  MKT_E_ARG with a message for a viewpoint outside the table or inside its own mask, a
 *                                     bin size of 0, an origin or second_side_only that is not 0 or 1, min_count 0, a ratio outside [0, 1),
 *                                     a non-zero reserved word; MKT_E_CAPACITY for 2^32 bins or more on either side; MKT_E_NOMEM when the
 *                                     dense tracks (4 bytes per bin of either side) do not fit half of the free memory.  Everything is
 *                                     checked before anything changes and the results are built aside: a refused or failed call leaves the
 *                                     previous results alone.  A later mkt_matrix_add or run discards them; the analyses of the resolutions
 *                                     and this one do not disturb each other.
 *   mkt_matrix_fetch_viewpoint_links     links [first, first + n); any pointer may be NULL; MKT_E_ARG with a message for a bad range
 *   mkt_matrix_fetch_viewpoint_track     bins [first, first + n) of the viewpoint track
 *   mkt_matrix_fetch_viewpoint_partners  cells [first, first + n) of the partner track (those with count >= min_count)
 *   mkt_matrix_viewpoint_timing       of the last mkt_matrix_viewpoint (ms, HIP events): the two scans of the records, and the sort with the
 *                                     run-length passes.  0, 0 without results. */
typedef struct mkt_viewpoint_opts {
    const uint8_t* partner_mask;
    double hotspot_ratio;
    uint32_t viewpoint, vbin, pbin, min_count;
    int32_t origin, second_side_only;
    uint32_t reserved[2];    /* 0 */
} mkt_viewpoint_opts;
typedef struct mkt_viewpoint_info {
    uint64_t total, links, links_kept, partner_cells, partner_cells_kept;
    uint32_t min_loop, viewpoint_bins;
} mkt_viewpoint_info;
void mkt_viewpoint_opts_default(mkt_viewpoint_opts* o);
int mkt_matrix_viewpoint(mkt_matrix* m, const mkt_viewpoint_opts* opts, mkt_viewpoint_info* info);
int mkt_matrix_fetch_viewpoint_links(mkt_matrix* m, uint64_t first, uint64_t n, uint32_t* vbin, uint32_t* chrom, uint32_t* pbin, uint32_t* count);
int mkt_matrix_fetch_viewpoint_track(mkt_matrix* m, uint64_t first, uint64_t n, uint32_t* count);
int mkt_matrix_fetch_viewpoint_partners(mkt_matrix* m, uint64_t first, uint64_t n, uint32_t* chrom, uint32_t* pbin, uint32_t* count);
int mkt_matrix_viewpoint_timing(const mkt_matrix* m, double* scan_ms, double* sort_ms);

/* ---- the .hic container: every resolution of the object in one file (the driver's `juicer_tools pre ... $sid.hic`, microcket:529) ----------
 * The file definition is this project's own, modelled on hic format version 8; tests/hicdef.py restates it in pure Python (struct and
 * zlib only: a builder and a parser that accounts for every byte).  PARITY with juicer_tools, straw and Juicebox is UNPINNED: none of them
 * is run.  All integers are little-endian; "string" is bytes followed by a NUL.
 *
 * HEADER   "HIC\0" | int32 version = 8 | int64 footerPosition | string genomeId | int32 nAttributes = 1: string "software", string
 *          "microcket-mi355x" | int32 nChrs, per chromosome of the table in file order: string name, int32 length | int32 nBpRes, the
 *          object's bin sizes in DESCENDING order (zoom index = position in this list; the same bin size twice is MKT_E_ARG) |
 *          int32 nFragRes = 0.  DEVIATION: the ALL pseudo-chromosome and its whole-genome matrix are NOT written, so chromosome index k is
 *          table index k.
 * BODY     for every chromosome pair c1 <= c2 (table index) with at least one cell at ANY resolution, ascending in (c1, c2), a matrix
 *          record: int32 c1, int32 c2, int32 nRes (every resolution, also one without cells), per resolution in header order:
 *          string "BP" | int32 zoomIndex | float32 sumCounts (the exact integer sum of the pair's counts at this resolution, converted
 *          once, round to nearest even) | float32 0, 0, 0 (occupied cells, stddev, percent95: not computed) | int32 binSize | int32
 *          blockBinCount bb | int32 blockColumnCount = max(L_c1, L_c2) / binSize / bb + 1 (integer divisions) | int32 blockCount | per
 *          non-empty block, ascending blockNumber: int32 blockNumber, int64 position, int32 sizeBytes.
 *          The blocks of the matrix follow its record immediately, in the order of the index (resolution by resolution).
 * BLOCK    a cell (bin1, bin2) of the genome-wide matrix has x = bin1 - off_c1, y = bin2 - off_c2 (cis: x <= y);
 *          blockNumber = (y / bb) * blockColumnCount + x / bb.  Payload: int32 nRecords | int32 xOff = (x / bb) * bb | int32 yOff =
 *          (y / bb) * bb | uint8 useShort (1 if and only if every count of the block is <= 32767) | uint8 matrixType = 1 (list of rows; the
 *          dense type 2 is never written) | int16 rowCount | per distinct y, ascending: int16 y - yOff, int16 recordCount, and per record
 *          of the row, ascending x: int16 x - xOff, then int16 count (useShort) or float32 count (round to nearest even).
 *          On disk a block is one zlib stream (RFC 1950) of the payload: 78 9C, the payload cut into pieces of at most 65280 bytes, each
 *          piece deflate block(s) with BFINAL = 0 that end on a byte (a coded piece is closed by an empty stored block 000, padding,
 *          00 00 FF FF; a piece that does not shrink is one stored block), then 03 00 and the Adler-32, big-endian.  level: 0 stored
 *          pieces, 1 fixed codes, 2 codes built per piece (the LZ77 + Huffman stage of mkt_bam, the same greedy one-pass parse).
 * FOOTER   at footerPosition: int32 nBytes (the bytes of the footer behind this field: everything up to the end of the vector index, the
 *          vectors themselves not counted) | int32 nEntries, per matrix record: string "c1_c2" (decimal), int64 position, int32 size
 *          (record plus its blocks) | int32 nExpectedValueVectors = 0 | int32 nNormExpectedValueVectors = 0 | int32 nNormVectors, per
 *          vector: string type (norm_label) | int32 chrIdx | string "BP" | int32 binSize | int64 position | int32 nBytes.
 * VECTORS  behind the index, in its order: int32 nValues = n_i, float64 values.  With norm = 1 every resolution that holds balancing weights
 *          when mkt_matrix_hic is called gets one vector per chromosome (resolutions in header order, chromosomes in table order).  .hic
 *          vectors DIVIDE: v = 1 / w, one IEEE division; the NaN 0x7FF8000000000000 where the weight is NaN (a masked bin).  Expected-value
 *          vectors are not written.
 * Nothing lies between these parts and the file ends with the last vector (or the index).  The bytes depend on the multiset of pairs,
 * the weights and the options only.
 * Limits: block_bins 1 .. 32767 (MKT_E_ARG); chromosome lengths below 2^31, block numbers below 2^31, a deflated block, a matrix record
 * with its blocks and a vector below 2^31 bytes (MKT_E_CAPACITY); always with a message, never a truncated file.
 *
 *   mkt_hic_opts_default    block_bins 1000, level 2, norm 1, genome_id NULL (""), norm_label NULL ("ICE")
 *   mkt_matrix_hic          opts NULL = the defaults; info may be NULL.  MKT_E_STATE "hic before run" before mkt_matrix_run.  The file stays
 *                           in device memory until the next add or run; a later balance does not change it.
 *   mkt_matrix_fetch_hic    bytes [off, off + n) of the file; MKT_E_ARG with a message for a range past its end
 *   mkt_matrix_hic_timing   of the last mkt_matrix_hic, per resolution index of the object (ms, HIP events): the sort with the head flags
 *                           and their scan; tables, sizes and serialisation; deflate; placing the streams in the file */
typedef struct mkt_hic_opts {
    const char* genome_id;
    const char* norm_label;
    uint32_t block_bins;
    int32_t level, norm;
    uint32_t reserved;                    /* 0 */
} mkt_hic_opts;
typedef struct mkt_hic_info {
    uint64_t file_bytes, matrices, blocks, float_blocks, pieces;
    uint64_t raw_bytes, deflated_bytes;   /* the payloads; their zlib streams */
} mkt_hic_info;
void mkt_hic_opts_default(mkt_hic_opts* o);
int mkt_matrix_hic(mkt_matrix* m, const mkt_hic_opts* opts, mkt_hic_info* info);
int mkt_matrix_fetch_hic(mkt_matrix* m, uint64_t off, char* out, size_t n);
int mkt_matrix_hic_timing(const mkt_matrix* m, uint32_t res_index, double* sort_ms, double* serialise_ms, double* deflate_ms, double* pack_ms);

/* ---- pair-level concordance of two .pairs texts (the reference's benchmarking/check.consistency.pl) on the GPU --------------------
 * Two texts A and B of tab-separated lines  id c1 p1 c2 p2 [more ...]  are joined on the exact bytes of id, and every line gets a
 * class.  No chromosome table: chromosome names are compared as bytes.  Independent of mkt_matrix.
 *
 * LINES   a line that starts with '#' is skipped (class 0); a last line without a newline counts; p1 and p2 are decimal integers in
 *         [0, 2^31).  A data line with fewer than five fields or a position that is not such an integer is refused: MKT_E_ARG, the
 *         message names the file (A or B) and the 1-based line.  max_dist 0 means 200.
 * DISTRIBUTION, per side, every data line counted (repeats of an id too): trans if c1 and c2 differ as bytes; else d = |p2 - p1|:
 *         d > 10000 cis>10K, d < 1000 cis<1K, anything else cis 1-10K.
 * JOIN    of several A lines with one id the LAST is the value, the earlier ones are superseded.  B lines are taken in file order: if
 *         the id has an A value that no earlier B line has claimed, the B line claims it, and the two are CONSISTENT if, with D =
 *         max_dist, either  a.c1 == b.c1, |a.p1 - b.p1| < D, a.c2 == b.c2, |a.p2 - b.p2| < D  (straight)  or  a.c1 == b.c2,
 *         |a.p1 - b.p2| < D, a.c2 == b.c1, |a.p2 - b.p1| < D  (swapped) holds, both comparisons strict, else DISCORDANT.  Every other B
 *         line is B-only (a second B line of a claimed id too, whatever it holds); unclaimed A values are A-only.
 * CLASSES one byte per input line.  A side: 0 comment, 1 superseded, 2 A-only, 3 consistent, 4 discordant.  B side: 0 comment,
 *         2 B-only, 3 consistent, 4 discordant.
 * REPORT  the script's stdout: "Using Distance: D", "Loading file A: <name> ...", "Loading file B: <name> ..." and an empty line; then
 *         A_only = a_only + discordant, B_only = b_only + discordant, Consistent, #Disconcordant and the two distributions, every count
 *         divided by 1e6 and printed with %.15g (3 is 3e-06, 0 is 0, 1234567 is 1.234567).
 * TEXT    (want_lines) in B's file order one line  I \t id \t A's c1 p1 c2 p2 \t vs \t B's c1 p1 c2 p2  per discordant B line and one
 *         line  B \t id \t c1 p1 c2 p2  per B-only line; behind all of them one line  A \t id \t c1 p1 c2 p2  per A-only value, in
 *         ascending line number (the script walks a hash there).  Fields are copied as text: 007 stays 007.
 * The classes, counters and bytes depend on the two texts and max_dist only: not on the route (host or device bytes, any chunking of
 * add), not on hash_bits, and they are the same on every call.  Integers only.
 * Both texts stay on the device; together they hold at most 2^32 - 1 lines (MKT_E_CAPACITY with a message beyond; MKT_E_NOMEM with a
 * message when device memory does not suffice).
 *
 *   mkt_paircmp_add / _add_device   side 0 = A, 1 = B; repeatable, a chunk need not end at a line end; host bytes are copied before the
 *                                   call returns
 *   mkt_paircmp_opts_default        max_dist 200, want_lines 1, hash_bits 0
 *   mkt_paircmp_run                 opts NULL = the defaults; info may be NULL; repeatable with other options on the same texts.
 *                                   hash_bits 0: ids are keyed by the full 95-bit hash; 1 .. 32: by that many bits only, a TEST KNOB that
 *                                   forces different ids onto one key (such runs are resolved on the host by exact string grouping;
 *                                   info.host_runs counts them; nothing else may change).  MKT_E_ARG for hash_bits > 32 or a non-zero
 *                                   reserved word.
 *   mkt_paircmp_fetch_classes       the class bytes of lines [first, first + n) of one side (MKT_E_STATE before run)
 *   mkt_paircmp_fetch_lines         bytes [off, off + n) of the text of the last run
 *   mkt_paircmp_report              host only, no handle: the report into out (cap bytes, NUL-terminated); returns its length without
 *                                   the NUL, or -1 when cap is too small
 *   mkt_paircmp_timing              of the last run, ms from HIP events: line index and parse; radix passes; join (the host's share
 *                                   included) and the class counts; the text */
typedef struct mkt_paircmp mkt_paircmp;
typedef struct mkt_paircmp_opts {
    uint32_t max_dist, want_lines, hash_bits;
    uint32_t reserved[5];                 /* 0 */
} mkt_paircmp_opts;
typedef struct mkt_paircmp_info {
    uint64_t lines[2], data_lines[2];     /* per side: all lines; those that are no comment */
    uint64_t distinct_a;                  /* different ids in A = A-only + consistent + discordant */
    uint64_t consistent, discordant, a_only, b_only;
    uint64_t dist[2][4];                  /* per side: cis<1K, cis 1-10K, cis>10K, trans */
    uint64_t host_runs;                   /* runs of one key with different ids, resolved on the host */
    uint64_t lines_bytes;                 /* bytes of the text (0 without want_lines) */
} mkt_paircmp_info;
int mkt_paircmp_create(int device, mkt_paircmp** out);
void mkt_paircmp_destroy(mkt_paircmp* p);
const char* mkt_paircmp_error(const mkt_paircmp* p);
int mkt_paircmp_add(mkt_paircmp* p, int side, const char* bytes, size_t n);
int mkt_paircmp_add_device(mkt_paircmp* p, int side, const void* d_bytes, size_t n);
void mkt_paircmp_opts_default(mkt_paircmp_opts* o);
int mkt_paircmp_run(mkt_paircmp* p, const mkt_paircmp_opts* opts, mkt_paircmp_info* info);
int mkt_paircmp_fetch_classes(mkt_paircmp* p, int side, uint64_t first, uint64_t n, uint8_t* out);
int mkt_paircmp_fetch_lines(mkt_paircmp* p, uint64_t off, char* out, size_t n);
long mkt_paircmp_report(const mkt_paircmp_info* info, uint32_t max_dist, const char* name_a, const char* name_b, char* out, size_t cap);
int mkt_paircmp_timing(const mkt_paircmp* p, double* parse_ms, double* sort_ms, double* join_ms, double* emit_ms);

/* ---- final.pairs.gz and its pairix index final.pairs.gz.px2 (the driver's `bgzip -c final.pairs > final.pairs.gz; pairix final.pairs.gz`) ----
 * The definition is what the reference's bin/bgzip (1.17) and bin/pairix (0.3.7) write; tests/px2def.py states it in Python and
 * tests/golden/px2_golden.json records their output.  Independent of mkt_matrix.
 *
 * GZ      BGZF (SAMv1 4.1): the text in blocks of 0xff00 bytes, each a gzip member with its CRC-32 and ISIZE, then the 28-byte EOF
 *         block.  The text is compressed as it is: no newline is added.  (bgzip itself puts the leading '#' lines into a block of
 *         their own and ends every block at a line end; the index does not depend on where blocks are cut, see OFFSETS.)
 * LINES   a line that starts with '#' is counted and not indexed, wherever it stands; it belongs to the chunk in front of it.  A last
 *         line without a newline is a line.  Every other line is a record of tab-separated columns  id chr1 pos1 chr2 pos2 ...  : the 4DN
 *         `pairs` preset, the only one offered.  Only chr1, pos1 and chr2 are read.
 * NAMES   the pair "chr1|chr2" of a record, compared as bytes; the name table lists them in order of first appearance (no order of
 *         the names is asked for: chr2|chr2 may stand in front of chr1|chr1).
 * BINS    pairix indexes the single base [pos1 - 1, pos1) (pos1 0 counts as 1), which always fits the finest of its six levels
 *         (windows of 2^15, 2^18, ... 2^30 positions; first bins 4681, 585, 73, 9, 1, 0): bin = 4681 + ((pos1 - 1) >> 15).  This is
 *         not tabix's 14-bit scheme.  The formula goes on past 2^30: pos1 = 2^31 - 1 has bin 70216.  The linear window is the same
 *         2^15 positions, so a name's linear index has ((largest pos1 - 1) >> 15) + 1 entries.
 * CHUNKS  a chunk {beg, end} of a bin runs from the start of the first record of a run of records with one name and one bin to the
 *         start of the first record of the next run, or to the end of the text.  pairix joins two chunks of one bin when the first ends
 *         in the block in which the second begins (tabix's rule); in a file that is accepted this never happens, because a (name,
 *         bin) is a single run.  So every bin holds exactly one chunk.
 * LINEAR  entry w of a name is the begin of the chunk of window w; a window without a record repeats the entry before it; windows in
 *         front of the name's first record hold 0.
 * OFFSETS virtual offsets, coffset << 16 | offset in block, of the reader that has consumed the text up to there: a position at which
 *         a block ends is offset 0 of the NEXT block, and the end of the text is offset 0 of the EOF block.
 * PX2     itself BGZF.  Uncompressed, little-endian:  "PX2.004\1", int32 n_ref, uint64 lines (all of them, '#' lines too), int32 3 (the
 *         preset), 2 3 3 (columns of chr1, begin, end), 4 5 5 (of chr2), bytes 09 '|' 00 00 (delimiter, region separator), int32 '#',
 *         int32 0 (lines to skip), int32 l_nm, the names each with a NUL; then PER NAME  int32 n_bin, n_bin x { uint32 bin, int32
 *         n_chunk, n_chunk x { uint64 beg, uint64 end } }, int32 n_intv, n_intv x uint64.  pairix writes the bins of a name in the
 *         order of a hash walk; this project writes them ascending.  A text without a record has n_ref 0 and l_nm 0 and ends there.
 * REFUSED with MKT_E_ARG and a message that begins "line N:" (1-based, all lines counted), the smallest such N, nothing being written:
 *         a record with fewer than five columns (an empty line too; pairix fails there as well); a pos1 that is empty, holds another
 *         byte than a digit, has more than ten digits or exceeds 2^31 - 1 (pairix reads it with strtol into an int32 and writes an
 *         index that is wrong or refuses the file as unsorted); a pos1 smaller than that of the record before it in the same pair
 *         (pairix: "the file out of order"); a pair that reappears after another (pairix: "the chromosome blocks not continuous").
 * QUERIES are answered by the reader below (mkt_bgzf_query).  pairix's reader answers a region of which the first range lies below 2^30
 *         only: records behind that are indexed and never returned.
 * Both files depend on the text and the level only: not on how `add` was fed, and they are the same bytes on every call.  Integers only,
 * no atomics.  The text, its compressed blocks (64 KiB each) and 28 bytes per line are resident; fewer than 2^32 - 1 lines
 * (MKT_E_CAPACITY beyond, MKT_E_NOMEM with a message when device memory does not suffice).
 *
 *   mkt_pairsgz_add            repeatable; a piece need not end at a line end; the bytes are copied before the call returns
 *   mkt_pairsgz_opts_default   level 1, preset MKT_PAIRSGZ_PRESET_PAIRS
 *   mkt_pairsgz_run            opts NULL = the defaults; info may be NULL; repeatable.  level: 0 stored, 1 the fixed code, 2 a code per
 *                              block (both files).  MKT_E_ARG for another level or preset, a non-zero reserved word, a refused text.
 *   mkt_pairsgz_fetch_gz / _fetch_px2   bytes [off, off + n) of the two files of the last run (MKT_E_STATE unless it succeeded)
 *   mkt_pairsgz_timing         of the last run, ms from HIP events: deflate and pack of the text; line index; the per-line kernel; names
 *                              and chunks (scans, the name table, the host's check for a reappearing pair); the index and its deflate */
#define MKT_PAIRSGZ_PRESET_PAIRS 0u
typedef struct mkt_pairsgz mkt_pairsgz;
typedef struct mkt_pairsgz_opts {
    int32_t level;
    uint32_t preset;
    uint32_t reserved[6];                 /* 0 */
} mkt_pairsgz_opts;
typedef struct mkt_pairsgz_info {
    uint64_t lines, records;              /* all lines; those that do not start with '#' */
    uint64_t names, bins, chunks;         /* pairs; (name, bin) entries; their chunks (one each) */
    uint64_t blocks;                      /* BGZF blocks of the text, without the EOF block */
    uint64_t gz_bytes, px2_bytes;
} mkt_pairsgz_info;
int mkt_pairsgz_create(int device, mkt_pairsgz** out);
void mkt_pairsgz_destroy(mkt_pairsgz* p);
const char* mkt_pairsgz_error(const mkt_pairsgz* p);
int mkt_pairsgz_add(mkt_pairsgz* p, const char* bytes, size_t n);
void mkt_pairsgz_opts_default(mkt_pairsgz_opts* o);
int mkt_pairsgz_run(mkt_pairsgz* p, const mkt_pairsgz_opts* opts, mkt_pairsgz_info* info);
int mkt_pairsgz_fetch_gz(mkt_pairsgz* p, uint64_t off, char* out, size_t n);
int mkt_pairsgz_fetch_px2(mkt_pairsgz* p, uint64_t off, char* out, size_t n);
int mkt_pairsgz_timing(const mkt_pairsgz* p, double ms[5]);

/* ---- reading BGZF back: final.pairs.gz (and any other BGZF file, sam2bam's BAM included, as bytes) inflated on the GPU ----
 * The definition of the format is SAMv1 4.1 and RFC 1951; tests/px2def.py (bgzf_blocks) and tests/inflatedef.py state in Python what is
 * accepted and what is refused.  Independent of mkt_pairsgz and mkt_matrix.
 *
 * FILE     a sequence of gzip members, each  1f 8b 08 04 | mtime xfl os | XLEN = 6 | 'B' 'C' 02 00 BSIZE | deflate | CRC-32 ISIZE .  Anything
 *          else is refused with the file offset of the member: other magic bytes, a plain gzip member (no extra field: "not BGZF"), another
 *          extra field, a BSIZE that runs past the file (a truncated file), a BSIZE below 26, an ISIZE above 65536.  The empty EOF block
 *          may stand anywhere and need not be there; info.has_eof says whether the file ends with one.
 * TEXT     the inflated members one behind the other: member k begins at the sum of the ISIZE in front of it.
 * DEFLATE  stored, fixed and dynamic blocks, any number per member.  REFUSED, each with a reason of its own: block type 3; a stored block
 *          whose NLEN is not the complement of LEN or that has non-zero bits up to its byte boundary; more than 286 literal/length or 30
 *          distance codes; an over-subscribed or incomplete code (code-length, literal/length, distance; one distance code of length 1 and
 *          no distance code at all are accepted); no end-of-block code; a repeat at the first length or past the last; length symbols 286,
 *          287 and distance symbols 30, 31; a match without a distance code; a bit pattern that is no code; a distance that reaches before
 *          the member's own first byte; output longer or shorter than ISIZE; a stream that runs past its member; bytes or non-zero
 *          bits behind the final block; a CRC-32 that differs from the footer.  zlib's tolerated oddities are not accepted.
 * SAFETY   a malformed file ends in MKT_E_FORMAT, never in a fault: every read is bounded to the member, every write to the member's
 *          ISIZE bytes of the text, every loop by the bits left in the member.
 * LIMITS   resident only: the compressed bytes and the whole text are held in device memory at once (MKT_E_NOMEM with a message when
 *          they do not fit; no streaming in batches).  BGZF only, no plain gzip.  A BAM inflates to its bytes: mkt_bamtext below decodes them.
 *          bin/pairscmp and bin/pairsbgz still refuse .gz names; `pairsgunzip a.pairs.gz | pairscmp - b.pairs` is the route.
 * The text depends on the file only: integers, no atomics.
 *
 * REGION QUERIES through the file's .px2: what `pairix file.pairs.gz REGION ...` prints (pairix 0.3.7, preset pairs; tests/pairsquerydef.py
 * states it in Python on top of tests/px2def.py query, tests/golden/pairsquery_golden.json records pairix's answers).  A query needs add and
 * load_index, not run: only the members the index points to are inflated.  After a run that succeeded the resident text is used and
 * nothing is inflated; both routes give the same bytes, the same on every call (integers only, no atomics).
 * REGION   A[:b-e]|B[:b-e], 1-based inclusive, commas allowed in a number.  [b1, e1) and [b2, e2) are 0-based half-open: b - 1 (b = 0
 *          counts as b = 1, as pairix answers it) and e.  A side without a range is [0, 2^30).  e1 is clipped to 2^30 (pairix's reader; e2
 *          is not); b1 >= e1 answers nothing.  The pair A|B is compared as bytes against the name table; an absent pair answers nothing.
 *          `*` as one side (no range) is every name whose other side is the chromosome given, in the order of the name table.  With
 *          autoflip (`pairix -a`) a pair A|B that is absent while B|A is present is answered as B:range2|A:range1.
 *          REFUSED with MKT_E_ARG and a message "region R: why" (R the index in the batch, from 0): no '|' (a one-sided query on a 2D
 *          file is not offered) or more than one, b > e, a bound that is not 1 to 18 digits, an empty chromosome, *|*, a range on *.
 *          pairix itself answers some of these (it reads a bound with strtol) and ends a call at a pair that is absent while its flip
 *          is present; neither is reproduced.
 * LOOKUP   min_off = linear[min(b1 >> 15, n_intv - 1)] of the name; every bin of the name whose range overlaps [b1, e1) contributes
 *          its chunks with end > min_off; sorted by begin; chunks that overlap (a foreign index) are merged, so that a line is never
 *          reported twice within one region.  A chunk of the index whose coffset is neither the start of a member of the file nor the
 *          file's length, or whose in-block offset exceeds that member's ISIZE: MKT_E_FORMAT "the index does not belong to this file".
 * LINES    in every chunk each line that starts in [beg, end) is a candidate (it ends at its newline or at the chunk's end).  One that
 *          starts with '#' is skipped.  A record with fewer than five columns (an empty line too), with a pos1 or pos2 that is empty,
 *          holds another byte than a digit, has more than ten digits or exceeds 2^31 - 1, or of more than 2^24 - 2 bytes never matches
 *          and is counted in info.unparsed (pairix reads such a field with strtol and may answer the line).  The others match when
 *          columns 2 and 4 equal A and B, max(pos1 - 1, 0) < e1, b1 < max(pos1, 1), and the same for pos2 against [b2, e2).
 * ANSWER   the matching lines, each with a '\n' behind it (the file's last line too where it has none), in the order of the regions,
 *          then of the sub-queries a star expands to, then of the file.  A line that two regions match stands twice.
 * SAFETY   the members of the plan are inflated into a compact buffer in which members adjacent in the file are adjacent, so that a
 *          line that straddles a member edge is contiguous; a member that is refused ends the query in MKT_E_FORMAT with reason and
 *          offset as run does.  Every read of the text lies inside a chunk, every write inside the counted size of the answer.
 *
 *   mkt_bgzf_add           compressed bytes, any chunking; copied before the call returns; forgets the text of an earlier run and the
 *                          answer of an earlier query, keeps a loaded index
 *   mkt_bgzf_run           opts NULL = the defaults; info may be NULL; repeatable.  On refusal MKT_E_FORMAT: the first refused member's
 *                          reason and file offset in mkt_bgzf_error ("... block at N: sentence [key]") and in info.reason / info.bad_offset
 *   mkt_bgzf_fetch_text    bytes [off, off + n) of the text (MKT_E_STATE unless the last run succeeded)
 *   mkt_bgzf_device_text   the text on the device, valid until the next add / run / destroy: what mkt_matrix_add_device,
 *                          mkt_paircmp_add_device and mkt_sorter_add_device take.  64 zero bytes stand behind it.
 *   mkt_bgzf_load_index    the bytes of a .px2 (BGZF itself: inflated by the same kernel, every field walked on the host; names, bins,
 *                          chunks and linear indexes are kept).  The file that was added stays.
 *   mkt_bgzf_count         the line count of the loaded index: `pairix -n`
 *   mkt_bgzf_names         bytes [off, off + n) of the name table, every name with a NUL behind it, *total its length: `pairix -l`
 *   mkt_bgzf_query         n regions (n = 0: an empty answer); opts NULL = no autoflip; info may be NULL.  MKT_E_STATE without a file or
 *                          without an index, MKT_E_ARG for a refused region, MKT_E_FORMAT for a refused member (info.reason,
 *                          info.bad_offset) or an index of another file
 *   mkt_bgzf_fetch_query   bytes [off, off + n) of the concatenated answer of the last query (MKT_E_STATE unless it succeeded)
 *   mkt_bgzf_fetch_query_offsets / _counts   n + 1 offsets at which the lines of each region begin in the answer (the last: its length);
 *                          n line counts
 *   mkt_bgzf_query_device  the answer on the device (64 zero bytes behind it), valid until the next add / run / query / destroy
 *   mkt_bgzf_timing        ms from HIP events.  Of the last run: table upload, inflate, CRC.  Of the last query: [3] plan upload, inflate
 *                          and CRC of the selected members; [4] line index, filter, scan and gather */
typedef struct mkt_bgzf mkt_bgzf;
typedef struct mkt_bgzf_opts {
    uint32_t reserved[8];                 /* 0 */
} mkt_bgzf_opts;
typedef struct mkt_bgzf_info {
    uint64_t blocks;                      /* members, empty ones included */
    uint64_t gz_bytes, text_bytes;
    uint64_t stored, fixed, dynamic;      /* deflate blocks by type, over all members */
    uint32_t has_eof;                     /* 1: the file ends with the 28-byte EOF block */
    uint32_t reason;                      /* 0, or why the file is refused (the numbers of mkt_inflate.h; the key stands in the message) */
    uint64_t bad_offset;                  /* file offset of the refused member */
} mkt_bgzf_info;
int mkt_bgzf_create(int device, mkt_bgzf** out);
void mkt_bgzf_destroy(mkt_bgzf* r);
const char* mkt_bgzf_error(const mkt_bgzf* r);
int mkt_bgzf_add(mkt_bgzf* r, const char* bytes, size_t n);
void mkt_bgzf_opts_default(mkt_bgzf_opts* o);
int mkt_bgzf_run(mkt_bgzf* r, const mkt_bgzf_opts* opts, mkt_bgzf_info* info);
int mkt_bgzf_fetch_text(mkt_bgzf* r, uint64_t off, char* out, size_t n);
int mkt_bgzf_device_text(mkt_bgzf* r, const void** d_ptr, uint64_t* n);
int mkt_bgzf_load_index(mkt_bgzf* r, const char* px2_bytes, size_t n);
int mkt_bgzf_count(mkt_bgzf* r, uint64_t* n_lines);
int mkt_bgzf_timing(const mkt_bgzf* r, double ms[5]);
typedef struct mkt_bgzf_query_opts {
    uint32_t autoflip;                    /* 1: `pairix -a` */
    uint32_t reserved[7];                 /* 0 */
} mkt_bgzf_query_opts;
typedef struct mkt_bgzf_query_info {
    uint64_t regions, subqueries, chunks;       /* sub-queries after the expansion of stars and flips; chunks scanned (merged ones count once) */
    uint64_t blocks_inflated, bytes_inflated;   /* members of the plan and their ISIZE; 0 when the resident text was used */
    uint64_t candidate_lines, lines, answer_bytes, unparsed;
    uint32_t reason;                      /* 0, or why a member is refused (as in mkt_bgzf_info) */
    uint32_t pad;
    uint64_t bad_offset;                  /* file offset of the refused member */
} mkt_bgzf_query_info;
int mkt_bgzf_query(mkt_bgzf* r, const char* const* regions, uint32_t n, const mkt_bgzf_query_opts* opts, mkt_bgzf_query_info* info);
int mkt_bgzf_fetch_query(mkt_bgzf* r, uint64_t off, char* out, size_t n);
int mkt_bgzf_fetch_query_offsets(mkt_bgzf* r, uint64_t* out);
int mkt_bgzf_fetch_query_counts(mkt_bgzf* r, uint64_t* out);
int mkt_bgzf_query_device(mkt_bgzf* r, const void** d_ptr, uint64_t* n);
int mkt_bgzf_names(mkt_bgzf* r, uint64_t off, char* out, size_t n, uint64_t* total);
/* forgets the file, the text, a loaded index and the last answer: the reader is as it was created, so that one reader inflates a large
 * file in batches of whole members (bin/bam2sam) */
int mkt_bgzf_clear(mkt_bgzf* r);

/* ---- reading BAM: the inflated stream of a BAM (SAMv1 4.2) decoded to SAM text on the GPU, the driver's `samtools view` ----
 * The text is what samtools 1.17 `view` prints for the records and `view -H` for the header, byte for byte, for every stream inside the
 * definition; tests/bamtextdef.py states it in Python, tests/golden/bamtext_golden.json records what samtools printed.  The input is
 * the INFLATED stream: mkt_bgzf_device_text hands it out, or the caller uploads it.  Independent of mkt_bgzf and of sam2bam.
 *
 * HEADER   magic BAM\1, l_text, text, n_ref, then l_name, name (with its NUL), l_ref per reference: walked on the host.  The header text
 *          as `view -H` prints it is the stored l_text bytes, NULs at their end included; where the text in front of those NULs is not
 *          empty and lacks its last newline, a '\n' stands in place of the first of them (behind the text where there is none).
 * LINE     per record, tab-separated, '\n' at the end: QNAME (the bytes before the first NUL), FLAG, RNAME (`*` for refID -1), pos + 1,
 *          MAPQ, CIGAR (MIDNSHP=X; `*` without operations), RNEXT (`*` for next_refID -1, `=` where it equals refID, else the name),
 *          next_pos + 1, TLEN, SEQ (=ACMGRSVTWYHKDBN; `*` for l_seq 0), QUAL (+ 33; `*` for l_seq 0 or a first byte 0xFF), then the tags
 *          in stored order: c C s S i I print as i; A, Z, H as stored; B as B:t,v,v,...; f and B:f as "%g" of the float (formatted on
 *          the host: the values are gathered in record order, their strings uploaded; no round trip for a stream without floats).
 * REFUSED  never trusted, never a fault; MKT_E_FORMAT with info.reason (key in brackets in mkt_bamtext_error), info.bad_record (the
 *          ordinal of the record in the whole stream, from 0) and info.bad_offset (its offset in the inflated stream):
 *          1 bad_magic; 2 bad_header (a negative l_text, n_ref or l_name, a name without its NUL); 3 no_sq_lines (n_ref > 0 and a text
 *          without an @SQ line: samtools makes lines up); 4 block_size_small (< 32); 5 block_size_large (> max_record); 6 past_end
 *          (32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq exceeds block_size); 7 ref_id (refID or next_refID below -1 or not
 *          below n_ref); 8 read_name (l_read_name 0, or a last byte that is not NUL); 9 cigar_op (a code above 8); 10 tag_overrun (the
 *          tags do not end exactly at the record's end); 11 tag_type (outside AcCsSiIfZHB); 12 b_subtype (outside cCsSiIf);
 *          13 z_unterminated; 14 cg_tag (a CG:B:I tag: the convention for more than 65535 operations, which samtools rewrites);
 *          15 truncated (finish with a partial record held); 16 header_truncated (finish before the header was complete, an n_ref
 *          that passes the data included); 17 cigar_seq_length (a mapped record whose CIGAR takes another number of bases than a
 *          non-zero l_seq: samtools ends with an error there); 18 header_nul (a NUL inside the header text, in front of its last byte that is not NUL:
 *          samtools cuts and mends such a text).  After a refusal the reader has forgotten the stream and takes a new one.
 * PIECES   the stream is added in any chunking.  A run decodes every complete record held and keeps what is no complete record (at
 *          most max_record + 4 bytes, or a header that is not complete yet) in front of the next piece; the texts of the runs, one
 *          behind the other, are the text of the whole.  finish refuses a tail that is not empty.
 * INDEX    records chain through block_size.  The record region of a run is cut into segments of segment_bytes; a workgroup per segment
 *          takes the lowest offset at which the fixed fields of four chained records are plausible and walks the chain from there;
 *          the segments are then put in order, and one whose guess is not where the segment before it ended is walked again from the
 *          true start (info.repairs).  The text never depends on a guess, only the time does.
 * SAFETY   every read lies inside a complete record (block_size is checked against the data held before anything else is read, every
 *          variable part against block_size), every write inside the line whose length the same routines measured from the same bytes.
 * LIMITS   max_record at most 16 MiB; the stream held, the record arrays and the text of one run are resident (feed pieces).
 *
 *   mkt_bamtext_add / _add_device   bytes of the inflated stream (host / device memory), copied before the call returns
 *   mkt_bamtext_run        decodes what is held; opts NULL = the defaults; info may be NULL.  The text of the run replaces the last one's.
 *   mkt_bamtext_finish     the end of the stream: MKT_E_FORMAT (truncated / header_truncated) unless nothing is held; a new stream may follow
 *   mkt_bamtext_fetch_header   bytes [off, off + n) of the header text as `view -H` prints it, *total its length (MKT_E_STATE before a run
 *                          reached the end of the header)
 *   mkt_bamtext_fetch_ref  reference k: name (cap bytes of room, NUL included) and length; *n_ref their number (name and length may be NULL)
 *   mkt_bamtext_fetch_text / _device_text   the text of the last run (64 zero bytes behind it on the device; valid until the next run)
 *   mkt_bamtext_timing     ms of the last run from HIP events: header, index guess, resolve + scan + fill, length, scan, emit */
typedef struct mkt_bamtext mkt_bamtext;
typedef struct mkt_bamtext_opts {
    uint32_t segment_bytes;               /* 0 = 256 KiB; a power of two >= 256 */
    uint32_t max_record;                  /* 0 = 16 MiB (the most); the largest block_size accepted */
    uint32_t reserved[6];                 /* 0 */
} mkt_bamtext_opts;
typedef struct mkt_bamtext_info {
    uint64_t records, text_bytes;         /* of this run */
    uint64_t segments, repairs;
    uint64_t float_records;               /* records that hold at least one float (an f tag, an element of a B:f array) */
    uint64_t carry_bytes;                 /* held for the next run */
    uint32_t reason;                      /* 0, or why the stream is refused (the numbers above) */
    uint32_t header_done;                 /* 1: the header is complete */
    uint64_t bad_record, bad_offset;
} mkt_bamtext_info;
int mkt_bamtext_create(int device, mkt_bamtext** out);
void mkt_bamtext_destroy(mkt_bamtext* r);
const char* mkt_bamtext_error(const mkt_bamtext* r);
int mkt_bamtext_add(mkt_bamtext* r, const char* bytes, size_t n);
int mkt_bamtext_add_device(mkt_bamtext* r, const void* d_bytes, uint64_t n);
void mkt_bamtext_opts_default(mkt_bamtext_opts* o);
int mkt_bamtext_run(mkt_bamtext* r, const mkt_bamtext_opts* opts, mkt_bamtext_info* info);
int mkt_bamtext_finish(mkt_bamtext* r, mkt_bamtext_info* info);
int mkt_bamtext_fetch_header(mkt_bamtext* r, uint64_t off, char* out, size_t n, uint64_t* total);
int mkt_bamtext_fetch_ref(mkt_bamtext* r, uint32_t k, char* name, size_t cap, int32_t* length, uint32_t* n_ref);
int mkt_bamtext_fetch_text(mkt_bamtext* r, uint64_t off, char* out, size_t n);
int mkt_bamtext_device_text(mkt_bamtext* r, const void** d_ptr, uint64_t* n);
int mkt_bamtext_timing(const mkt_bamtext* r, double ms[6]);

/* ---- pair statistics: distance by orientation, P(s), chromosome pairs of a .pairs text (what `pairtools stats` / `scaling` give) ----
 * One streaming pass; integers only on the device, so every number is the same on every call.  tests/pairstatdef.py states the
 * definition in Python; the host half (csrc/mkt_pairstat.h) needs no GPU.
 *
 * INPUT    .pairs text: readID chr1 pos1 chr2 pos2 strand1 strand2 [...], tab-separated, one pair per line.  A line that starts with
 *          '#' is skipped and counted in header_lines.  A chrom.sizes table is required: the grammar and the name lookup of
 *          mkt_matrix_create (name<TAB>length lines, names of 1 .. 63 bytes, lengths below 2^32, no name twice).
 * REFUSED  a data line with fewer than five columns (an empty line included) or a position that is empty or no plain decimal:
 *          mkt_pairstat_run fails with MKT_E_FORMAT and a message that names the smallest such line (1-based, all lines counted).
 * CLASSES  every data line counts in `total`; a position above 2^40 counts as 2^40.  A side whose name is not in the table, or whose position is 0 or past the chromosome's
 *          length, makes the pair `skipped` and it counts nowhere else.  counted = total - skipped; a counted pair is `cis` when both
 *          sides name one chromosome, else `trans`.  For a cis pair d = |pos2 - pos1|: cis_ge[k] counts d >= 1000, 2000, 4000, 10000,
 *          20000, 40000 (cis_1kb+ ... cis_40kb+).  A counted pair with fewer than seven columns, or whose strand fields are not
 *          exactly one byte '+' or '-', counts in everything but dist_freq, and in no_strand.
 * REFERENCE  cis0 (d < 1000), cis1K (1000 .. 9999), cis10K (>= 10000) and ref_trans are the reference's log counters cis0, cis1K, cis10K
 *          and trans: like the reference they take EVERY data line, skipped or not, and know no table: a line is cis when its two name
 *          fields are the same bytes.  (Names of more than 63 bytes, which no table can hold, occur in the reference's own test inputs.)
 *          Without skipped pairs they equal cis - cis_1kb+, cis_1kb+ - cis_10kb+, cis_10kb+ and trans.
 * CHROM    chrom_freq[i][j]: counted pairs per ordered (chr1 index, chr2 index) as written on the line, no flipping; dense n x n.
 * DIST     dist_freq[74][4]: cis pairs with strands by distance bin and orientation in the order ++ +- -+ --.  The 74 edges are 0 and
 *          round(10^(k/8)) for k = 0 .. 72 (0 1 1 2 2 3 4 6 7 10 ... 749894209 1000000000; kPsEdges in csrc/mkt_pairstat.h); the bin of
 *          d is (number of edges <= d) - 1, so [1,1) and [2,2) stay empty and bin 73 is 1000000000+.  The repeated edges are kept so
 *          that the keys line up with `pairtools stats`.
 * P(s)     area[k] = sum over chromosomes of sum_{d = lo}^{min(hi, L) - 1} (L - d) for bin [lo, hi) (hi = 2^32 for bin 73), exact in
 *          128 bits, converted to double once (round to nearest even); P[k] = double(sum_o dist_freq[k][o]) / area[k], 0.0 where the
 *          area is 0.  No logarithm and no slope.
 * CONVERGENCE  T_k = sum_o c[k][o]; bin k is thick when T_k >= min_count; a thick bin is balanced when for every o
 *          |4 c[k][o] - T_k| * 1000 <= 4 T_k tol_permille.  K is the smallest k such that bin k is thick and balanced and every thick
 *          bin behind it is balanced; convergence_dist = edge[K], or -1 when there is none.
 * TEXT     which 0, PREFIX.pairs.stat: key<TAB>value lines: total, skipped, counted, cis, trans, no_strand, header_lines, cis_1kb+ ...
 *          cis_40kb+, reference/trans, reference/cis10K, reference/cis1K, reference/cis0; summary/frac_cis, summary/frac_cis_1kb+ ... summary/frac_cis_40kb+, summary/frac_trans
 *          (double(x) / double(counted), 0 for counted 0, printed "%.17g" as PREFIX.<r>.expected.tsv prints a double),
 *          summary/convergence_dist; chrom_freq/A/B for the non-zero cells in table order; dist_freq/lo-hi/oo for all 74 x 4 (the last
 *          bin is written 1000000000+).  which 1, PREFIX.scaling.tsv: the header line lo hi area ++ +- -+ -- total P, then one row per
 *          bin (area as the exact integer, P as "%.17g").
 * STREAM   add / add_device take pieces cut anywhere, any number of times; the whole lines of a piece are counted and dropped, the
 *          partial last line is carried, run closes the carry.  Nothing is resident but one piece and the counters.  More may be added
 *          after a run; the next run reports everything seen so far.
 * LIMITS   at most 2048 names in the table (the dense chrom_freq is 32 MB there): mkt_pairstat_create refuses more with MKT_E_RANGE
 *          and a message that says so.  Compressed input is BGZF only (mkt_bgzf_*).  No slope, no pair types, no per-chromosome P(s).
 *
 *   mkt_pairstat_create        the table as bytes; mkt_pairstat_error(NULL) has the message of a failed create
 *   mkt_pairstat_add / _add_device   host / device bytes, copied (counted) before the call returns
 *   mkt_pairstat_add_keys      the reported pairs of a context created with MKT_EXT_KEYS, as mkt_matrix_add_keys takes them: drop_last,
 *                              and skip_flags (one byte per reported pair, non-zero = leave out; NULL = none) with n_flags >= the pairs
 *   mkt_pairstat_opts_default  tol_permille 50, min_count 1000
 *   mkt_pairstat_run           opts NULL = the defaults; info may be NULL.  MKT_E_FORMAT for a refused line, MKT_E_ARG for a non-zero
 *                              reserved word
 *   mkt_pairstat_fetch_dist    the 74 x 4 counts (MKT_E_STATE before a run that succeeded, as every fetch)
 *   mkt_pairstat_fetch_chrom   rows [first_row, first_row + n_rows) of chrom_freq, n_chrom values each
 *   mkt_pairstat_fetch_scaling edges (75 values: the 74 edges and 2^32), area and P (74 each); any pointer may be NULL
 *   mkt_pairstat_text          the text `which` into out (cap bytes, no NUL is added); returns its length, which may exceed cap (then
 *                              nothing is written), or a negative MKT_E_* code
 *   mkt_pairstat_timing        ms from HIP events, summed over every piece since create: line index, kernels, and both with the copies */
#define MKT_PAIRSTAT_BINS 74
#define MKT_PAIRSTAT_MAX_CHROM 2048
typedef struct mkt_pairstat mkt_pairstat;
typedef struct mkt_pairstat_opts {
    uint32_t tol_permille;                /* 50 */
    uint32_t reserved0;                   /* 0 */
    uint64_t min_count;                   /* 1000 */
    uint32_t reserved[4];                 /* 0 */
} mkt_pairstat_opts;
typedef struct mkt_pairstat_info {
    uint64_t total, skipped, counted, cis, trans, no_strand, header_lines;
    uint64_t cis_ge[6];                   /* d >= 1000, 2000, 4000, 10000, 20000, 40000 */
    uint64_t cis0, cis1K, cis10K, ref_trans;      /* the reference's classes: every data line, by name bytes and distance alone */
    int64_t convergence_dist;             /* -1: none */
    uint32_t n_chrom, reserved;
} mkt_pairstat_info;
int mkt_pairstat_create(int device, const char* chromsizes, size_t len, mkt_pairstat** out);
void mkt_pairstat_destroy(mkt_pairstat* ps);
const char* mkt_pairstat_error(const mkt_pairstat* ps);
int mkt_pairstat_add(mkt_pairstat* ps, const char* bytes, size_t n);
int mkt_pairstat_add_device(mkt_pairstat* ps, const void* d_bytes, size_t n);
int mkt_pairstat_add_keys(mkt_pairstat* ps, mkt_ctx* ctx, int drop_last, const uint8_t* skip_flags, size_t n_flags);
void mkt_pairstat_opts_default(mkt_pairstat_opts* o);
int mkt_pairstat_run(mkt_pairstat* ps, const mkt_pairstat_opts* opts, mkt_pairstat_info* info);
int mkt_pairstat_fetch_dist(mkt_pairstat* ps, uint64_t* out);
int mkt_pairstat_fetch_chrom(mkt_pairstat* ps, uint32_t first_row, uint32_t n_rows, uint64_t* out);
int mkt_pairstat_fetch_scaling(mkt_pairstat* ps, uint64_t* edges, double* area, double* p);
long mkt_pairstat_text(mkt_pairstat* ps, int which, char* out, size_t cap);
int mkt_pairstat_timing(const mkt_pairstat* ps, double* index_ms, double* kernel_ms, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* MKT_H */
