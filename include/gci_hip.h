/*
 * gci_hip.h -- C ABI of libgci_hip.so: the MI355X (gfx950) implementation of GCI's
 * alignment-filter -> per-base-depth -> issue-scan hot path.
 *
 * The reference (yeeus/GCI, a single pure-Python file) has no FFI; the seams below are the
 * function seams of its hot path, one export per seam so each is parity-testable against
 * the matching reference function (citations are into /root/reference/GCI.py):
 *
 *   gci_bam_filter      read_sam                      GCI.py:146-169  (+ fan-out 257-270)
 *   gci_name_join       filter(), cross-file join     GCI.py:272-301  (+ dict "last wins" 166, 269)
 *   gci_depth_build     filter(), slice += 1          GCI.py:201-208, 302-306
 *   gci_gap_mask        merge_gaps_depths             GCI.py:315-329
 *   gci_max2            merge_two_type_depth          GCI.py:350
 *   gci_issue_scan*     collapse_depth_range          GCI.py:356-390
 *   gci_depth_text_*    write_depth (text body)       GCI.py:110-117
 *   gci_depth_sum       np.mean numerator             GCI.py:862-868
 *   gci_range_sums      sliding_window_average_depth  GCI.py:660-705 (window sums)
 *   gci_depth_classes   analyze_depth_regions         utility/depth_plotter_v2.py (zero / low runs, non-zero statistics)
 *   gci_fasta_n_scan    get_Ns_ref                    GCI.py:27-35
 *   gci_depth_runs_*, gci_bedgraph_*   depth_to_bedgraph.py: a track as bedGraph lines (no counterpart in the reference)
 *   gci_depth_hist      depth_dist.py: the depth histogram, sum, min, max and count of windows (no counterpart in the reference)
 *   gci_bam_cover_*, gci_track_add     bam_depth.py: the unfiltered per-base depth of BAM files, `samtools depth -a` (no counterpart in the reference)
 *   gci_bam_fate, gci_bam_cover_size_sel   filter_depth.py: which test of read_sam drops a record (GCI.py:152-168), and the depth of every such class
 *   gci_name_join_fate, gci_fate_refine    filter_depth.py --join: what the cross-file join (GCI.py:272-301) does with every record, and why
 *   gci_bam_reads_size, gci_bam_reads_write   filter_reads.py: the records over a set of regions as rows of text, each with its class (no counterpart in the reference)
 *   gci_bam_sweep                          filter_sweep.py: the distribution of MAPQ, clip and identity over the primary records, and what every value of each threshold would keep (no counterpart in the reference)
 *   gci_paf_filter_device   filter(), PAF path        GCI.py:211-254  (+ helpers 49-61, 64-96)
 *
 * Conventions
 *   - every export returns int: GCI_OK (0) or a negative gci_status; nothing throws, exits,
 *     prints or touches files;
 *   - the caller owns every buffer (torch / hipMalloc / gci_malloc); the library owns only
 *     the scratch inside its gci_ctx;
 *   - pointers named d_* are DEVICE pointers, h_* are HOST pointers;
 *   - all work is enqueued on the ctx stream and is asynchronous unless stated; gci_sync()
 *     waits for it.  A ctx is not thread-safe; distinct ctxs are independent;
 *   - plain C structs with fixed layout, little endian.
 *
 * Track layout ("depth track"): one int32 per base, all selected contigs in ONE buffer.
 * Contig c starts at element gci_layout_offsets()[c], a multiple of GCI_TILE (4096 elements,
 * 16 KiB), so tiles never straddle contigs and every vector access is 16-byte aligned.
 * Elements between the end of a contig and the next multiple of GCI_TILE are padding (always 0).
 */
#ifndef GCI_HIP_H
#define GCI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCI_ABI_VERSION 1
#define GCI_TILE 4096          /* elements per tile of a depth track */
#define GCI_MAX_JOIN_FILES 16

typedef enum gci_status {
    GCI_OK = 0,
    GCI_E_INVALID = -1,        /* bad argument */
    GCI_E_HIP = -2,            /* a HIP runtime call failed: see gci_last_error() */
    GCI_E_NO_NM = -3,          /* a record that reaches GCI.py:163 has no NM tag (reference: KeyError) */
    GCI_E_ZERO_DIV = -4,       /* zero denominator at GCI.py:165 / 292 (reference: ZeroDivisionError) */
    GCI_E_BAD_NM_TYPE = -5,    /* NM tag present but not an integer type */
    GCI_E_NO_END = -6,         /* reference_end would be None (n_cigar_op == 0) */
    GCI_E_MALFORMED = -7,      /* record runs past the end of the stream */
    GCI_E_CAPACITY = -8,       /* output buffer too small: grow and call again */
    GCI_E_NOMEM = -9,
    GCI_E_NO_LAYOUT = -10      /* gci_layout_set() has not been called */
} gci_status;

/* Compact alignment record: what read_sam keeps per record (GCI.py:166-168), 32 bytes. */
typedef struct gci_rec {
    uint64_t name_hash;        /* gci_name_hash() of the query name */
    int32_t contig;            /* index among the SELECTED contigs (not the BAM refID), -1 if none */
    int32_t start;             /* reference_start */
    int32_t end;               /* reference_end */
    int32_t qlen;              /* query_length */
    uint32_t rec_idx;          /* rec_idx_base + index of the record in the K1 call (informational) */
    uint8_t mapq;
    uint8_t flags;             /* GCI_REC_PASS | GCI_REC_HQ */
    uint16_t name_len;         /* bytes, without NUL */
} gci_rec;
#define GCI_REC_PASS 1u        /* record reaches GCI.py:166 */
#define GCI_REC_HQ 2u          /* ... and mapq >= mq_cutoff (GCI.py:167) */
#define GCI_REC_NAME16 4u      /* where its query name lies (gci_join_file): at an address = 0 or 4 (mod 16), followed by zero
                                * bytes up to the next 16-byte boundary -- names inside record pages (gci_bam_filter_pages) and
                                * routed name slots (gci_route_records).  The join then compares two such names as whole 16-byte
                                * pieces (three loads per name instead of a dozen) */

/* Interval on a selected contig, 16 bytes. */
typedef struct gci_ivl {
    int32_t contig;
    int32_t start;
    int32_t end;
    int32_t pad;
} gci_ivl;

/* One input of the join: compact records + where the query-name bytes of the record at POSITION i of d_recs
 * live:  d_name_base + d_name_off[i] + name_delta  (BAM: base = the inflated stream, off = record offsets,
 * delta = 36;  packed names / PAF: base = a names blob, off = blob offsets, delta = 0).  Records must be in file
 * order: among records of one file with the same name the LAST position wins (dict semantics, GCI.py:166, 269). */
typedef struct gci_join_file {
    const gci_rec* d_recs;
    uint32_t n_recs;
    uint32_t name_delta;
    const uint8_t* d_name_base;
    const uint64_t* d_name_off;
} gci_join_file;

/* Scan window over a track, in flat element coordinates of the track buffer. */
typedef struct gci_window {
    int64_t begin;
    int64_t end;
} gci_window;

typedef struct gci_ctx gci_ctx;

/* ---- context ------------------------------------------------------------------------------ */
int gci_abi_version(void);
/* own_stream == 0: enqueue on `stream`, a hipStream_t of the caller (e.g. torch's current stream;
 * NULL is the device's default stream).  own_stream != 0: `stream` is ignored and the ctx creates
 * (and later destroys) a non-blocking stream of its own.
 * Environment, read here: GCI_FORCE_DENSE=1 makes the depth build take its dense (difference array in LDS) path for
 * every tile instead of only for tiles with many events -- same results, for testing and A/B timing.  GCI_PAGES_GRID=<n>
 * lets gci_bam_pages_write launch at most n workgroups per kernel (each then writes many pages, whatever the input's size:
 * testing). */
int gci_ctx_create(int device, void* stream, int own_stream, gci_ctx** out);
int gci_ctx_destroy(gci_ctx* ctx);
int gci_sync(gci_ctx* ctx);
const char* gci_strerror(int status);
const char* gci_last_error(gci_ctx* ctx);
/* Convenience for hosts without a device allocator of their own (cgo, JNI ...). */
int gci_malloc(gci_ctx* ctx, size_t bytes, void** d_out);
int gci_free(gci_ctx* ctx, void* d_ptr);
int gci_memcpy_h2d(gci_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);   /* synchronous */
int gci_memcpy_d2h(gci_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);   /* synchronous */
int gci_memset(gci_ctx* ctx, void* d_dst, int byte, size_t bytes);                /* async */

/* ---- device memory, streams and events for a host without a tensor library (k_hbm.hip; round 6) -------------------------------
 * What the single-GPU command line holds its HBM buffers with (gci_amd/hbm.py: a caching allocator, stream-ordered like the
 * one it replaces, over gci_dev_malloc) -- `import torch` costs half a second of a 4 s run and is needed only for
 * torch.distributed (--gpus N).  Not tied to a context: `device` is the HIP device index, `stream` / `event` are hipStream_t /
 * hipEvent_t handles (a stream made here can be handed to gci_ctx_create with own_stream = 0).  Every call returns a gci_status;
 * gci_dev_last_error() is the calling thread's last HIP message.  gci_dev_malloc returns GCI_E_NOMEM when the device is full
 * (the caller frees what it caches and tries again).
 * gci_dev_memcpy_async: kind 1 = host -> device, 2 = device -> host, 3 = device -> device.
 * The three element-wise helpers are what the host side does to buffers it cannot touch: out[i] = in[i] + delta (name offsets
 * of the runs of a file put behind one another), recs[i].flags &= mask (GCI_REC_NAME16 dropped when names are packed), and the
 * exclusive prefix sum of the .depth.gz member sizes (uint32 in, uint64 out, n + 1 entries; one workgroup). */
const char* gci_dev_last_error(void);
int gci_dev_count(int* n_out);
int gci_dev_malloc(int device, size_t bytes, void** d_out);
int gci_dev_free(int device, void* d_ptr);
/* Device memory of this library -- gci_dev_malloc, gci_malloc and every context's scratch -- comes from an ARENA (k_hbm.hip): small
 * and medium blocks are cut from slabs (256 MiB, then GCI_ARENA_SLAB_MB = 1024 each), a block of 64 MiB or more that nothing free
 * can hold is a driver allocation of its own, and whatever is given back coalesces and serves later requests -- the memory of one
 * phase of a run becomes the next phase's without the driver being asked again.  That matters because a driver allocation costs by
 * the GB on this chip (the kernel driver clears VRAM it does not know to be clean: 35 - 45 ms per GB measured).  Slabs stay until
 * the process ends; GCI_ARENA=0 turns the arena off.
 * gci_dev_reserve: slabs for at least `bytes` in all, now (for a host that wants that cost in a place of its choosing).
 * gci_dev_arena_info: bytes in slabs, bytes handed out, number of slabs. */
int gci_dev_reserve(int device, uint64_t bytes, uint64_t* reserved_out);
int gci_dev_arena_info(int device, uint64_t* reserved, uint64_t* in_use, uint32_t* n_slabs);
int gci_dev_mem_info(int device, uint64_t* free_bytes, uint64_t* total_bytes);
int gci_dev_sync(int device);
int gci_dev_host_alloc(int device, size_t bytes, void** h_out);      /* pinned */
int gci_dev_host_free(int device, void* h_ptr);
int gci_dev_stream_create(int device, void** out);                   /* non-blocking */
int gci_dev_stream_destroy(int device, void* stream);
int gci_dev_stream_sync(int device, void* stream);
int gci_dev_event_create(int device, int timing, void** out);
int gci_dev_event_destroy(int device, void* event);
int gci_dev_event_record(int device, void* event, void* stream);
int gci_dev_event_sync(int device, void* event);
int gci_dev_event_elapsed_ms(int device, void* event_a, void* event_b, double* ms);
int gci_dev_stream_wait_event(int device, void* stream, void* event);
int gci_dev_memcpy_async(int device, void* dst, const void* src, size_t bytes, int kind, void* stream);
int gci_dev_memset_async(int device, void* d_dst, int byte, size_t bytes, void* stream);
int gci_dev_i64_add(int device, const int64_t* d_in, uint64_t n, int64_t delta, int64_t* d_out, void* stream);
int gci_dev_rec_flags_and(int device, gci_rec* d_recs, uint64_t n, uint32_t mask, void* stream);
int gci_dev_u32_scan_u64(int device, const uint32_t* d_in, uint32_t n, uint64_t* d_out, void* stream);

/* ---- optional per-kernel timing with HIP events on the ctx stream ------------------------------
 * gci_profile_enable(mask): bit k enables an event pair around every launch of kernel id k.
 * gci_profile_read(): synchronises, folds finished event pairs in and returns the accumulated
 * milliseconds / launch count of one kernel id (reset != 0 clears that id afterwards). */
enum {
    GCI_PROF_BAM_FILTER = 0, GCI_PROF_JOIN_INSERT, GCI_PROF_JOIN_FOLD, GCI_PROF_DEPTH_DIFF, GCI_PROF_SCAN_TILES,
    GCI_PROF_DEPTH_SCAN, GCI_PROF_GAP_MASK, GCI_PROF_MAX2, GCI_PROF_ISSUE_SCAN, GCI_PROF_TEXT_COUNT,
    GCI_PROF_TEXT_WRITE, GCI_PROF_DEPTH_SUM, GCI_PROF_MEMSET, GCI_PROF_TILE_PASS1, GCI_PROF_TILE_DENSE, GCI_PROF_PARTITION,
    GCI_PROF_JOIN_PART, GCI_PROF_PAGES_SIZE, GCI_PROF_PAGES_WRITE, GCI_PROF_COUNT
};
int gci_profile_enable(gci_ctx* ctx, int mask);
int gci_profile_read(gci_ctx* ctx, int kernel_id, double* total_ms, uint64_t* launches, int reset);
const char* gci_profile_name(int kernel_id);

/* ---- layout (GCI.py:201-208: contig table of the first BAM, optionally restricted by --chrs) */
int gci_layout_set(gci_ctx* ctx, int32_t n_contigs, const int64_t* h_lengths);
int64_t gci_layout_total(gci_ctx* ctx);                    /* elements of one track buffer */
int gci_layout_offsets(gci_ctx* ctx, int64_t* h_offsets);  /* n_contigs entries */

/* ---- R1: record filter ---------------------------------------------------------------------
 * d_bam: inflated BAM stream; d_rec_off[i]: byte offset of record i's block_size word;
 * d_ref_sel[refID]: index among the selected contigs or -1.  Writes one gci_rec per input
 * record (flags == 0 for filtered records); out[i].rec_idx = rec_idx_base + i (a rank that
 * decodes a slice of a file passes the slice's first record index).  *d_status (uint64, device) receives
 * min over failing records of (rec_idx << 8 | -status), or UINT64_MAX if none failed;
 * decode with gci_decode_status(). */
int gci_bam_filter(gci_ctx* ctx, const uint8_t* d_bam, uint64_t n_bytes, const uint64_t* d_rec_off,
                   uint32_t n_rec, const int32_t* d_ref_sel, int32_t n_ref, int map_qual, int mq_cutoff,
                   double clip_percent, double iden_percent, uint32_t rec_idx_base, gci_rec* d_out,
                   uint64_t* d_status);
/* ---- R1 over RECORD PAGES (round 3): the layout the record filter is fastest on --------------------------------
 * read_sam (GCI.py:146-169) looks at ~400 of a HiFi record's 27 000 bytes.  gci_bam_pages_size / _write copy exactly
 * those bytes -- once, on the device, as the last step of the ingestion that walks the inflated stream anyway -- into
 * fixed-size pages in which every record and every CIGAR is 16-byte aligned and nothing needs an offset table:
 *
 *   buffer = [page 0] ... [page n_pages - 1] [blob] [16 zero bytes]
 *   page   = u32 n_recs | u32 first_rec | u32 used_bytes | u32 magic "GCP1" | u16 dir[n_recs] (record start / 16) | records
 *   record = the BAM record without SEQ / QUAL, its fixed 36 bytes kept except: block_size -> size of the record in the
 *            page (a multiple of 16, <= GCI_PAGE_MAX_REC); bin -> kind; next_refID -> aux_len; next_pos, tlen -> blob
 *            offset (u64, from the buffer start).  read_name at +36, zero padded so that the CIGAR starts at
 *            align16(36 + l_read_name); the CIGAR zero padded to 16 bytes; the aux bytes behind it.
 *            kind 1: the CIGAR words are in the blob (a record that does not fit: ONT), 16 bytes with the first
 *            operation stand in for them; kind 2: core only, the record's bytes (heads form) are in the blob (CG:B,I
 *            long-CIGAR records, kilobytes of tags); kind 4: a record the stream filter reports GCI_E_MALFORMED for.
 *   Record i goes to page floor(S_i / (page_bytes - GCI_PAGE_MAX_REC - 48)), S = exclusive scan of (size + 2).
 *
 * gci_bam_pages_size: d_stream / d_rec_off as for gci_bam_filter (has_seq != 0), or a HEADS STREAM (has_seq == 0: gci_bam_heads
 *   below -- the BAM header followed by every record without its SEQ and QUAL bytes, block_size shortened accordingly, l_seq
 *   unchanged: the bytes read_sam never looks at, GCI.py:146-169, are 98 % of a HiFi record);
 *   h_out[0] = n_pages, h_out[1] = bytes of the buffer to allocate, h_out[2] = offset of the blob.  Synchronises.
 * gci_bam_pages_write: fills d_out (cap >= h_out[1]) for the input the size call measured.
 * gci_bam_filter_pages: the filter over such a buffer -- same records, same status word as gci_bam_filter over the
 *   stream the pages were made from; d_name_off (nullable, n_rec entries) receives where every record's query name lies
 *   in the buffer (gci_join_file: d_name_base = d_pages, d_name_off, name_delta = 0). */
#define GCI_PAGE_MAX_REC 1024
#define GCI_PAGE_MAX_BYTES 32768
#define GCI_PAGE_BYTES_DEFAULT 24576
int gci_bam_pages_size(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec,
                       int has_seq, uint32_t page_bytes, uint64_t* h_out);
int gci_bam_pages_write(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec,
                        int has_seq, uint8_t* d_out, uint64_t cap);
int gci_bam_filter_pages(gci_ctx* ctx, const uint8_t* d_pages, uint64_t total_bytes, uint32_t page_bytes, uint32_t n_pages,
                         uint32_t n_rec, const int32_t* d_ref_sel, int32_t n_ref, int map_qual, int mq_cutoff,
                         double clip_percent, double iden_percent, uint32_t rec_idx_base, gci_rec* d_out,
                         uint64_t* d_name_off, uint64_t* d_status);
int gci_decode_status(uint64_t status_word, uint32_t* rec_idx);   /* -> gci_status */
/* The name hash K1 uses, for hosts that build gci_rec themselves (PAF path). */
uint64_t gci_name_hash(const uint8_t* h_name, uint32_t len);
/* Pack the query names of `n` records into a dense blob (multi-GPU exchange):
 * d_out_off[i] = byte offset of name i (exclusive scan of name_len), d_out_off[n] = total. */
int gci_pack_names(gci_ctx* ctx, const gci_join_file* h_file, uint8_t* d_out_names, uint64_t cap,
                   uint64_t* d_out_off);

/* ---- bam_depth.py: the reference bases every record covers, `samtools depth -a` without its base-quality options (k_cover.hip) ----
 * The same input as gci_bam_filter: the inflated stream and the record offsets (has_seq != 0), or a heads stream (has_seq == 0).
 * Needs gci_layout_set (the selected contigs, in the order d_ref_sel numbers them).
 *   skipped    a record with flag & excl_flags != 0, mapq < min_mapq, refID < 0 or >= n_ref, pos < 0 or d_ref_sel[refID] < 0
 *   covers     M, = and X cover their reference bases; D only with count_del != 0; N never; I, S, H and P consume no reference;
 *              operations of length 0 cover nothing.  A <l_seq>S<n>N placeholder with a CG:B,I (or B,i) tag stands for the tag's
 *              operations (the rule of gci_bam_filter); without the tag it covers nothing
 *   malformed  a record that runs past the end of the stream or contradicts its block_size (as gci_bam_filter finds it, skipped or
 *              not), and operation codes 9 - 15 in a record that is not skipped: GCI_E_MALFORMED in *d_status (the smallest such
 *              record index << 8 | -status, UINT64_MAX if none; decode with gci_decode_status)
 * gci_bam_cover_size: *h_n_ivl = the number of intervals the write call will emit; *d_status is complete after it.  Synchronises.
 *   The scratch of this call stays in the context for the write call.
 * gci_bam_cover_write: the intervals of the input the size call in front of it on this context measured (same d_stream, d_rec_off
 *   and n_rec: else GCI_E_INVALID) to d_out[0 .. *h_n_ivl), in no particular order; cap < *h_n_ivl: GCI_E_CAPACITY, nothing is
 *   written.  `end` is the LAST covered base (inclusive), so that gci_depth_build with flank 0 -- [start : end + 1] -- adds exactly
 *   the covered bases; positions are summed in 64 bits and clamped to the contig's length before they become int32 (what lies beyond
 *   the contig's end is dropped by the build's slice).  One interval per maximal run of covering operations inside a chunk of
 *   GCI_COVER_CHUNK_OPS operations: the unit of work is a chunk (one wave), never a record.
 * gci_track_add: d_acc[i] += d_add[i] over the layout (depths of several files, or of one file built in parts).  Both are whole
 *   tracks of gci_layout_total() elements, 16-byte aligned (any allocation is): an unaligned pointer is GCI_E_INVALID. */
#define GCI_COVER_CHUNK_OPS 2048
int gci_bam_cover_size(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                       const int32_t* d_ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq, int count_del, uint64_t* h_n_ivl,
                       uint64_t* d_status);
int gci_bam_cover_write(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                        gci_ivl* d_out, uint64_t cap, uint64_t* d_status);
int gci_track_add(gci_ctx* ctx, int32_t* d_acc, const int32_t* d_add);

/* ---- filter_depth.py: what becomes of every record in the record filter, and the depth of each class (k_fate.hip, k_cover.hip) ----
 * gci_bam_fate: the same input as gci_bam_filter (has_seq as for gci_bam_cover_size).  d_class[i] = the class of record i, named
 * after the FIRST test of read_sam (GCI.py:152-168) the record fails, in the reference's order:
 *   GCI_FATE_NONE           flag & 0x4, refID < 0 or >= n_ref, pos < 0 or d_ref_sel[refID] < 0: the skip rule of gci_bam_cover_size with
 *                           excl_flags = 0x4 -- a record the reference's fetch never yields
 *   GCI_FATE_SECONDARY      flag & 0x100
 *   GCI_FATE_SUPPLEMENTARY  flag & 0x800 (and not 0x100)
 *   GCI_FATE_MAPQ           mapq < map_qual
 *   GCI_FATE_CLIP           not S / (M + I + S) <= clip_percent           (M: the bases under M, = and X together)
 *   GCI_FATE_IDENTITY       not (M - mm) / (M + I + D) >= iden_percent    (mm = NM - (I + D))
 *   GCI_FATE_KEPT           reaches GCI.py:166: exactly the records gci_bam_filter marks GCI_REC_PASS
 *   GCI_FATE_ERROR          a record *d_status reports: one that runs past the end of the stream or contradicts its block_size, or one
 *                           the reference would have raised on
 * The last three use the IEEE f64 quotients, the first-NM rule and the CG:B,I restore of gci_bam_filter, and *d_status is the word
 * gci_bam_filter (rec_idx_base 0) gives for the same input and thresholds whenever no reported record has pos < 0: no NM
 * (GCI_E_NO_NM), NM of a non-integer type, M + I + S == 0, the clip test, M + I + D == 0, the identity test, in this order.  A record of
 * the first four classes is settled by its core fields: no tag is looked for, nothing is divided, its CIGAR is not read.
 * h_counts[c]: the records of class c (GCI_FATE_CLASSES entries, host).  Needs no layout.  Synchronises.
 * gci_bam_cover_size_sel: gci_bam_cover_size over the records whose class is in the mask -- a record is also skipped when bit
 *   d_class[i] of class_mask is clear (d_class == NULL: no record is; that is gci_bam_cover_size).  gci_bam_cover_write follows it
 *   unchanged.  A record that is not selected makes no chunk: walking class after class reads every CIGAR once in total. */
#define GCI_FATE_NONE 0
#define GCI_FATE_SECONDARY 1
#define GCI_FATE_SUPPLEMENTARY 2
#define GCI_FATE_MAPQ 3
#define GCI_FATE_CLIP 4
#define GCI_FATE_IDENTITY 5
#define GCI_FATE_KEPT 6
#define GCI_FATE_ERROR 7
#define GCI_FATE_CLASSES 8
int gci_bam_fate(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                 const int32_t* d_ref_sel, int32_t n_ref, int map_qual, double clip_percent, double iden_percent, uint8_t* d_class,
                 uint64_t* h_counts, uint64_t* d_status);
int gci_bam_cover_size_sel(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                           const int32_t* d_ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq, int count_del, const uint8_t* d_class,
                           uint32_t class_mask, uint64_t* h_n_ivl, uint64_t* d_status);

/* ---- R5: cross-file join --------------------------------------------------------------------
 * h_files in reference order (PAF files, then BAM files, each in command-line order).
 * One file: the dict semantics of GCI.py:166/269 only (a repeated name keeps its LAST record).
 * d_contig_map (nullable): remaps rec.contig -> output contig, entries < 0 drop the interval
 * (multi-GPU: keep only the contigs this rank owns).  Output order is unspecified.
 * *d_n_out may exceed cap: then nothing beyond cap was written, grow and retry. */
int gci_name_join(gci_ctx* ctx, const gci_join_file* h_files, int n_files, double ovlp_percent,
                  const int32_t* d_contig_map, gci_ivl* d_out, uint32_t cap, uint32_t* d_n_out,
                  uint64_t* d_status);
/* Which implementation gci_name_join / gci_name_join_count use: 0 = by size (an open-addressing table in HBM below 2^20
 * records, the radix-partitioned join with per-bucket tables in LDS from there up), 1 = always the table, 2 = always
 * partitioned.  Same results either way.  The partitioned join reports GCI_E_CAPACITY (record 0) in *d_status for inputs its
 * 32-byte entries cannot hold (a bucket with more distinct names than its table has slots -- forged hashes only --, a name of
 * 4 KiB and more, name bytes beyond 64 GiB from d_name_base): the caller then sets mode 1 and joins again. */
int gci_join_mode(gci_ctx* ctx, int mode);
/* The same join, fused with the first pass of the depth build: the kernel that emits an interval also counts it into
 * the per-tile tables of the layout (flank = the build's --flank-len), so a gci_depth_build_begin over exactly this
 * output with opts.counted = 1 skips that pass (one dependent launch and one read of the intervals less).  Needs
 * gci_layout_set; if *d_n_out exceeds cap, call it again with more room before building.  From 2^20 records up the
 * build buckets its events by radix partition and counts on the way (GCI_EVENTS=atomic|radix overrides): the call is then
 * the plain join, and opts.counted = 1 still says "these are the intervals of that join". */
int gci_name_join_count(gci_ctx* ctx, const gci_join_file* h_files, int n_files, double ovlp_percent,
                        const int32_t* d_contig_map, gci_ivl* d_out, uint32_t cap, uint32_t* d_n_out,
                        uint64_t* d_status, int flank);

/* ---- filter_depth.py --join: what the cross-file join does with every record, and why (k_join.hip, k_fate.hip) ----
 * gci_name_join_fate: the inputs of gci_name_join (h_files in the reference's order) -> one byte per record, h_d_fate[f][i] for
 * the record at POSITION i of file f's d_recs (h_d_fate: n_files device pointers on the host, h_d_fate[f] of n_recs bytes).
 * For a read name q: present[f] = q has a GCI_REC_PASS record in file f; the file's WINNER for q is the PASS record that is
 * last in (contig index, position) -- what the reference's dict keeps (GCI.py:166, 269); hq = any PASS record of q in any file
 * carries GCI_REC_HQ; comm = q is present in every file.  One file: the verdict of every name is `joined`.  Several files
 * (GCI.py:277-299): have = present[0] and (hq or comm), why = unpaired; then for the files 1 .. n - 1 in order that hold q:
 *   have:             the winner lies on another contig than the interval so far  -> have = false, why = contig
 *                     else ovlp / qlen < ovlp_percent (ovlp = length of the intersection, qlen = THIS file's winner's;
 *                       IEEE f64 quotient)                                          -> have = false, why = overlap
 *                     else the interval narrows to the intersection
 *   not have, and hq: have = true, the interval is this winner's (a name a test took out comes back)
 * and the verdict is `joined` if have holds at the end, else why.  qlen == 0 where the quotient is asked for: GCI_E_ZERO_DIV
 * with the winner's rec_idx in *d_status (the smallest such word, as gci_name_join reports it), the name's fold ends there and
 * its verdict is `overlap`.  `unpaired` thus names reads below mq_cutoff everywhere that some file has no passing record of.
 *   GCI_FATE_SHADOWED   a PASS record that is not its file's winner for its name (the dict overwrite)
 *   GCI_FATE_UNPAIRED / _CONTIG / _OVERLAP / _JOINED   a winner: the verdict of its name
 *   0                   a record without GCI_REC_PASS
 * The names whose verdict is `joined` are exactly the intervals gci_name_join emits (without a contig map); `joined` is the set
 * of reads GCI.py counts, not its depth.  h_counts[f * GCI_JOIN_FATE_CLASSES + c]: the records of file f with byte c (host).
 * ALWAYS the open-addressing table in HBM, whatever gci_join_mode says: the partitioned join keeps no way back from a name to
 * its records.  That table takes about 5 G records/s at genome scale (k_join.hip); this export has been measured only on 0.66 M
 * records in two files, at 1.6 times gci_name_join on the same table.  The
 * join tables are left as gci_name_join expects them.  Needs no layout.  Synchronises.
 * gci_fate_refine: d_class[i] == GCI_FATE_KEPT becomes d_join_fate[i] (gci_bam_fate's classes of a piece of a file, and the
 * slice of that file's join bytes that begins at the piece's first record).  A `kept` record whose join byte is not one of the
 * five above, or a join byte other than 0 on a record that is not `kept` -- the two passes disagree about which records pass
 * -- is GCI_E_INVALID with the record's index in *d_status, and that class byte stays.  Does not synchronise. */
#define GCI_FATE_SHADOWED 8
#define GCI_FATE_UNPAIRED 9
#define GCI_FATE_CONTIG 10
#define GCI_FATE_OVERLAP 11
#define GCI_FATE_JOINED 12
#define GCI_JOIN_FATE_CLASSES 16       /* entries of a row of gci_name_join_fate's counts */
int gci_name_join_fate(gci_ctx* ctx, const gci_join_file* h_files, int n_files, double ovlp_percent, uint8_t* const* h_d_fate,
                       uint64_t* h_counts, uint64_t* d_status);
int gci_fate_refine(gci_ctx* ctx, uint8_t* d_class, const uint8_t* d_join_fate, uint32_t n_rec, uint64_t* d_status);

/* ---- filter_reads.py: the records of chosen classes over a set of regions, one row of text each (k_reads.hip) ----
 * The same input as gci_bam_fate, d_class = its output (after gci_fate_refine where there is a join).  Needs gci_layout_set: the
 * selected contigs, n_sel of them, in the order d_ref_sel numbers them.  A record is SELECTED when bit d_class[i] of class_mask is
 * set and -- with windows -- its reference span overlaps one of its contig's windows.  Bits of class_mask for GCI_FATE_NONE,
 * GCI_FATE_ERROR or a class that does not exist: GCI_E_INVALID.  A record whose class bit is clear is not read beyond its class
 * byte, so a malformed record (class GCI_FATE_ERROR) is never touched.
 *   windows    d_win: the windows of all selected contigs in CONTIG coordinates [begin, end), contig after contig, per contig
 *              sorted, disjoint and not abutting; d_contig_win0[c] .. d_contig_win0[c + 1] (n_sel + 1 entries, device) are contig c's.
 *              d_contig_win0 == NULL: no window test.  A record with reference span R at pos overlaps [B, E) when pos < E and
 *              pos + max(R, 1) > B: a record that consumes no reference still sits on one base.
 *   CIGAR      the record's own, or the CG:B,I (B,i) array behind a <l_seq>S<n>N placeholder (the rule of gci_bam_filter).  M is the
 *              bases under M, = and X together, I, D, S and N the bases under those; R = M + D + N.  Totals are summed in 64 bits.
 *   row        file_no name contig start end strand flag mapq M I D S NM clip identity class, tab-separated, '\n' at the end:
 *              name = the bytes of read_name in front of its first NUL; contig = h_contig_name_len[c] (<= 65535) bytes at
 *              d_contig_names + h_contig_name_off[c]; start = pos; end = pos + R (not clamped); strand = '-' with flag 0x10, else '+';
 *              NM = the first NM tag as a signed decimal, '.' without one or with one of a non-integer type; clip = dec6(S, M + I + S),
 *              identity = dec6(M + I + D - NM, M + I + D), each '.' where its denominator is 0, identity also where NM is '.';
 *              dec6(n, d) = '-' if n < 0, |n| / d, '.', and the six digits of ((|n| % d) * 10^6) / d -- truncated, exact;
 *              class = the name of d_class[i] (none secondary supplementary mapq clip identity kept error shadowed unpaired contig
 *              overlap joined).  The class column is authoritative; the two decimals are for the eye.
 *   *d_status  (smallest record index << 8 | -status, UINT64_MAX if none) for records whose class bit is set: GCI_E_MALFORMED for one
 *              that runs past the end of the stream or contradicts its block_size (no row), and for operation codes 9 - 15 in a
 *              selected record (they add to no total; the row is listed); GCI_E_INVALID for one d_class cannot belong to -- refID outside 0 .. n_ref - 1,
 *              pos < 0, d_ref_sel[refID] outside 0 .. n_sel - 1 (no row).
 * gci_bam_reads_size: *h_n_rows = the selected records, *h_n_bytes = the bytes of their rows; *d_status is complete.  Synchronises.
 *   The scratch of this call stays in the context for the write call.
 * gci_bam_reads_write: the rows of the input the size call in front of it on this context measured (same d_stream, n_bytes,
 *   d_rec_off, n_rec and name lengths: else GCI_E_INVALID) to d_out[0 .. *h_n_bytes), in record order.  cap < *h_n_bytes:
 *   GCI_E_CAPACITY, nothing is written.  Does not synchronise. */
int gci_bam_reads_size(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                       const int32_t* d_ref_sel, int32_t n_ref, const uint8_t* d_class, uint32_t class_mask, const gci_window* d_win,
                       const uint32_t* d_contig_win0, const uint32_t* h_contig_name_len, uint32_t file_no, uint64_t* h_n_rows,
                       uint64_t* h_n_bytes, uint64_t* d_status);
int gci_bam_reads_write(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec,
                        const uint8_t* d_contig_names, const uint64_t* h_contig_name_off, const uint32_t* h_contig_name_len, uint8_t* d_out,
                        uint64_t cap);

/* ---- filter_sweep.py: how the record filter's three thresholds cut a BAM stream (k_sweep.hip) ----
 * The same input as gci_bam_fate, plus the windows of gci_bam_reads_size.  Every PRIMARY record is counted once in each of three
 * tables, by its MAPQ, its clip quotient and its identity quotient, so that what each threshold TAKEN ALONE would keep can be read
 * off for every value of it.  A record is primary when gci_bam_fate would not call it none, secondary or supplementary: flag & 0x904
 * clear, refID in 0 .. n_ref - 1, pos >= 0, d_ref_sel[refID] >= 0.  MAPQ settles nothing here: the first NM tag and the CIGAR are read
 * for every primary record (the record's own, or the CG:B,I / B,i array behind a <l_seq>S<n>N placeholder: the rule of gci_bam_filter).
 *   windows    as for gci_bam_reads_size (d_contig_win0 == NULL: no window test).  A primary record counts only if it overlaps a
 *              window of its contig: pos < E and pos + max(R, 1) > B, R the bases under M, D, N, = and X.  With windows the call needs
 *              gci_layout_set (the selected contigs, n_sel of them, index d_contig_win0); a record whose d_ref_sel[refID] >= n_sel has
 *              no window.  Without windows no layout is needed.
 *   totals     S, M (the bases under M, = and X together), I, D, N: summed in 64 bits, every one below 2^57.  NM: the first NM tag.
 *   weights    every row carries `records` (1 per record) and `bases` (M per record).
 *   digits     K in 1 .. 3 (else GCI_E_INVALID), B = 10^K = GCI_SWEEP_BINS(K).
 *   mapq       row = the MAPQ byte.
 *   clip       S / (M + I + S), ROUNDED UP to K digits: row b in 0 .. B holds the quotients in ((b - 1) / B, b / B], so that
 *              "clip <= b / B" is "row <= b"; `undefined` when the denominator is 0.
 *   identity   (M + I + D - NM) / (M + I + D), TRUNCATED to K digits: row b in 0 .. B holds [b / B, (b + 1) / B), so that
 *              "identity >= b / B" is "row >= b"; `<0` for a negative numerator, `>1` for one beyond the denominator (a negative NM);
 *              `undefined` without an NM tag, with one of a non-integer type, or with a zero denominator.
 *              The K digits come from long division in 64-bit integers (a remainder times ten fits); "rounded up" is the truncation
 *              plus one when a remainder is left.  No floating point takes part in the binning.
 *   flags      at the call's thresholds, each on its own (no short circuit): pm = mapq >= map_qual; pc = the filter's clip test,
 *              pi = its identity test (the IEEE f64 quotients of gci_bam_filter); an undefined quantity fails its test.
 *   h_table    host, GCI_SWEEP_ROWS(K) rows of GCI_SWEEP_COLS uint64 -- records, bases, records_others, bases_others -- where the
 *              `_others` columns count the row's records that pass the OTHER TWO tests.  Rows: 256 of mapq; clip 0 .. B, undefined;
 *              identity <0, 0 .. B, >1, undefined (the macros below).
 *   *d_status  (smallest record index << 8 | -status, UINT64_MAX if none): GCI_E_MALFORMED for a record that runs past the end of the
 *              stream or contradicts its block_size (not counted), and for operation codes 9 - 15 in a counted record (they add to no
 *              total; the record is counted).  Nothing else: a record GCI.py would raise on (no NM, a zero denominator) is counted on
 *              its `undefined` row.
 * Synchronises.  GCI_SWEEP_GRID=<n> in the environment (read by gci_ctx_create) caps the workgroups of the binning kernel: testing. */
#define GCI_SWEEP_COLS 4
#define GCI_SWEEP_BINS(digits) ((digits) == 1 ? 10 : (digits) == 2 ? 100 : 1000)
#define GCI_SWEEP_MAPQ(q) (q)                                                     /* q in 0 .. 255 */
#define GCI_SWEEP_CLIP(digits, b) (256 + (b))                                     /* b in 0 .. B */
#define GCI_SWEEP_CLIP_UNDEF(digits) (256 + GCI_SWEEP_BINS(digits) + 1)
#define GCI_SWEEP_IDEN_BELOW(digits) (256 + GCI_SWEEP_BINS(digits) + 2)           /* <0 */
#define GCI_SWEEP_IDEN(digits, b) (256 + GCI_SWEEP_BINS(digits) + 3 + (b))        /* b in 0 .. B */
#define GCI_SWEEP_IDEN_ABOVE(digits) (256 + 2 * GCI_SWEEP_BINS(digits) + 4)       /* >1 */
#define GCI_SWEEP_IDEN_UNDEF(digits) (256 + 2 * GCI_SWEEP_BINS(digits) + 5)
#define GCI_SWEEP_ROWS(digits) (256 + 2 * GCI_SWEEP_BINS(digits) + 6)
int gci_bam_sweep(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                  const int32_t* d_ref_sel, int32_t n_ref, const gci_window* d_win, const uint32_t* d_contig_win0, int map_qual,
                  double clip_percent, double iden_percent, int digits, uint64_t* h_table, uint64_t* d_status);

/* ---- clip_sites.py: where alignments break off, base by base (k_clips.hip) -------------------------------------------------------------
 * gci_bam_clip_size / _write: the same input as gci_bam_cover_size (the inflated stream plus record offsets, or a heads stream with
 * has_seq = 0); they need gci_layout_set.  Per record:
 *   skipped    exactly the skip rule of gci_bam_cover_size with the same excl_flags (0x704 by default: supplementary alignments count) and
 *              min_mapq; its CIGAR is not read.  A record whose R (below) is 0 is skipped as well.
 *   operations the record's own, or the CG:B,I / B,i array behind a <l_seq>S<n>N placeholder (the rule of gci_bam_filter: the first
 *              operation is S of length l_seq, the FIRST CG tag counts).  Such a first operation without a usable tag: R counts as 0, the
 *              record is skipped.
 *   R          the bases under M, =, X, D and N, summed in 64 bits.
 *   lead       len(op[0]) if op[0] is S or H, plus len(op[1]) if op[0] and op[1] are both S or H; only the first two operations are looked
 *              at.  trail: the same over op[n - 1], op[n - 2].  H counts like S (minimap2 writes supplementary alignments with hard
 *              clips); with R > 0 no operation counts on both sides.
 *   events     a LEFT event at pos if lead >= min_clip, a RIGHT event at pos + R - 1 if trail >= min_clip.  The site is computed in 64
 *              bits (pos + R may exceed int32); one at or beyond the contig's length is not emitted and not counted.  min_clip < 1:
 *              GCI_E_INVALID.
 *   *d_status  as gci_bam_cover_size reports it (smallest record index << 8 | -status, UINT64_MAX if none): GCI_E_MALFORMED for a
 *              record that runs past the end of the stream or contradicts its block_size, and for operation codes 9 - 15 in a record
 *              that is not skipped (they add nothing to R).
 *   h_counts   host, 3 entries: the records counted (not skipped), the left events, the right events.  The size call synchronises.
 * gci_bam_clip_write emits gci_ivl{contig, site, site, 0}: the left events to d_out[0 .. n_left), the right events to d_out[n_left ..
 * n_left + n_right), each in RECORD ORDER (ranks from an exclusive scan; no atomics: the output is deterministic).  cap < n_left +
 * n_right: GCI_E_CAPACITY, nothing is written.  The size call's scratch stays in the context for it; another stream, offsets or n_rec
 * than the size call in front of it on this context measured: GCI_E_INVALID.  gci_depth_build with flank 0 over either half gives that
 * side's track: per base the number of events there.
 *
 * gci_clip_sites_size / _write: the elements of two such tracks where left >= min_reads or right >= min_reads, in ascending flat order.
 *   input      whole tracks of gci_layout_total() elements, 16-byte aligned (else GCI_E_INVALID); d_depth == NULL: the depth column is 0.
 *   windows    [begin, end) in flat track elements, clamped to the track, sorted and disjoint (else GCI_E_INVALID), as gci_depth_hist
 *              takes them; n_windows == 0: every contig of the layout.  Only elements inside a window are looked at.
 *   a site     contig and pos from the layout's contig offsets, left, right and depth the three tracks' values there.  Elements of the
 *              padding between contigs are never sites.  min_reads < 1: GCI_E_INVALID.
 *   write      the sites of the size call in front of it on this context (same tracks, min_reads and n_windows, nothing between the two
 *              that sets windows: else GCI_E_INVALID) to d_out[0 .. *h_n_sites).  cap too small: GCI_E_CAPACITY, nothing is written.
 * The size pass reads the left and right tracks once, 16 bytes a lane, and leaves one count per 4096-element tile of the windows; the
 * counts are scanned; the write pass looks only at tiles with a count and stores by rank inside the tile.  No global atomics. */
typedef struct gci_clip_site {
    int32_t contig;
    int32_t pos;
    int32_t left;
    int32_t right;
    int32_t depth;
    int32_t pad;
} gci_clip_site;
int gci_bam_clip_size(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                      const int32_t* d_ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq, int min_clip, uint64_t* h_counts,
                      uint64_t* d_status);
int gci_bam_clip_write(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                       gci_ivl* d_out, uint64_t cap, uint64_t* d_status);
int gci_clip_sites_size(gci_ctx* ctx, const int32_t* d_left, const int32_t* d_right, const int32_t* d_depth, int32_t min_reads,
                        const gci_window* h_windows, uint32_t n_windows, uint64_t* h_n_sites);
int gci_clip_sites_write(gci_ctx* ctx, const int32_t* d_left, const int32_t* d_right, const int32_t* d_depth, int32_t min_reads,
                         const gci_window* h_windows, uint32_t n_windows, gci_clip_site* d_out, uint64_t cap);

/* ---- indel_sites.py: long insertions and deletions in reads, base by base (k_indels.hip) ------------------------------------------------
 * gci_bam_indel_size / _write: the same input as gci_bam_cover_size (the inflated stream plus record offsets, or a heads stream with
 * has_seq = 0); they need gci_layout_set.  Per record:
 *   counted    exactly when gci_bam_cover_size does not skip it with the same excl_flags (0x704 by default: supplementary alignments
 *              count) and min_mapq: flag, MAPQ, refID, pos and d_ref_sel are the whole skip rule.  A skipped record's CIGAR is not read.
 *   operations the record's own, or the first CG:B,I / B,i array behind a <l_seq>S<n>N placeholder, by the rule of gci_bam_cover_size.
 *              A placeholder without a usable tag stays as it is: it holds no I or D and emits nothing.
 *   at         of an operation: pos plus the lengths of all M, =, X, D and N operations in front of it in the record, in 64 bits.
 *   L          the contig's length as the layout has it, capped at 0x7FFFFFFE (as the cover pass caps it); a d_ref_sel beyond the
 *              layout: 0.
 *   deletion   a D operation of length >= min_len with at < L: the interval [at, min(at + len, L) - 1], both ends inclusive.  One with
 *              at >= L is not emitted and not counted.
 *   insertion  an I operation of length >= min_len: its site is the reference base in front of the inserted bases (VCF's anchor), at - 1
 *              if at > 0, else 0.  A site at or beyond L is not emitted and not counted.
 *   otherwise  operations are never merged (5D5D is two deletions of 5); N consumes reference and is no event; P, S, H and operations
 *              of length zero move nothing.  min_len < 1: GCI_E_INVALID.
 *   *d_status  as gci_bam_cover_size reports it (smallest record index << 8 | -status, UINT64_MAX if none): GCI_E_MALFORMED for a
 *              record that runs past the end of the stream or contradicts its block_size, and for operation codes 9 - 15 in a counted
 *              record (they move nothing).
 *   h_counts   host, 3 entries: the records counted, the deletions, the insertions.  The size call synchronises.
 * gci_bam_indel_write emits gci_ivl{contig, start, end, 0}: the deletions to d_out[0 .. n_del), the insertions (start == end == site)
 * to d_out[n_del .. n_del + n_ins), each half in (record, operation) order; the ranks come from exclusive scans, no atomics: two runs
 * give the same bytes.  cap < n_del + n_ins: GCI_E_CAPACITY, nothing is written.  The size call's scratch stays in the context for it;
 * another stream, n_bytes, offsets or n_rec than the size call in front of it on this context measured: GCI_E_INVALID.
 * gci_depth_build with flank 0 over the first half gives the del track (per base the counted records that delete it with one long
 * D), over the second half the ins track (per base the long insertions anchored there).  The depth of gci_bam_cover_size without
 * count_del does not count a read over the bases it deletes: the reads that span a deleted base are depth + del.
 *
 * gci_indel_sites_size / _write: the runs of hot elements of two such tracks.
 *   input      whole tracks of gci_layout_total() elements, 16-byte aligned (else GCI_E_INVALID); d_depth == NULL: the depth column is 0.
 *   windows    as gci_clip_sites_size takes them: [begin, end) in flat track elements, clamped, sorted and disjoint (else
 *              GCI_E_INVALID); n_windows == 0: every contig of the layout.
 *   hot        an element with del >= min_reads or ins >= min_reads that lies inside a window and inside its contig (never in the
 *              padding between contigs).  min_reads < 1: GCI_E_INVALID.
 *   a site     a maximal run of consecutive hot elements of one contig inside one window (two touching windows cut a run in two):
 *              contig, start and end (exclusive) as positions on the contig, and the maximum over the run of the del track, the ins
 *              track and the depth track.  Sites come in ascending flat order.
 *   write      the sites of the size call in front of it on this context (same tracks, min_reads and n_windows, nothing between the two
 *              that sets windows: else GCI_E_INVALID) to d_out[0 .. *h_n_sites).  cap too small: GCI_E_CAPACITY, nothing is written.
 * The size pass reads the del and ins tracks once, 16 bytes a lane, marks the run starts and leaves one count per 4096-element tile of
 * the windows; the counts are scanned; the write pass stores the starts of the tiles that hold one by rank, and a wave per site walks
 * the run to its end and takes the three maxima -- the depth track is read only there.  No global atomics. */
typedef struct gci_indel_site {
    int32_t contig;
    int32_t start;
    int32_t end;
    int32_t del;
    int32_t ins;
    int32_t depth;
} gci_indel_site;
int gci_bam_indel_size(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                       const int32_t* d_ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq, int min_len, uint64_t* h_counts,
                       uint64_t* d_status);
int gci_bam_indel_write(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                        gci_ivl* d_out, uint64_t cap, uint64_t* d_status);
int gci_indel_sites_size(gci_ctx* ctx, const int32_t* d_del, const int32_t* d_ins, const int32_t* d_depth, int32_t min_reads,
                         const gci_window* h_windows, uint32_t n_windows, uint64_t* h_n_sites);
int gci_indel_sites_write(gci_ctx* ctx, const int32_t* d_del, const int32_t* d_ins, const int32_t* d_depth, int32_t min_reads,
                          const gci_window* h_windows, uint32_t n_windows, gci_indel_site* d_out, uint64_t cap);

/* ---- mismatch_sites.py: bases where the reads carry another base than the assembly (k_mismatch.hip) -----------------------------------------
 * gci_fasta_codes: the assembly as one code byte per base, indexed as the tracks are (contig offset + position).  Needs gci_layout_set.
 *   input      d_text, n_bytes, d_body, n_records as gci_fasta_n_scan takes them (d_text 16-byte aligned, else GCI_E_INVALID), and
 *              d_tile_kept0 = the exclusive scan of that call's d_tile_kept with the total behind it (tiles + 1 entries of uint64:
 *              gci_dev_u32_scan_u64).  A sequence byte is gci_fasta_n_scan's: inside a record's body, not a line end, '\r' or blank.
 *   d_dst[r]   int64: the flat element of d_codes where the first base of record r goes, -1 to leave the record out.  Base k of the
 *              record goes to d_dst[r] + k; elements at or beyond gci_layout_total() are not written.  The caller has checked that
 *              the record is as long as its contig: the call writes as many elements as the record has bases.
 *   the code   of a byte: BAM's 4-bit encoding "=ACMGRSVTWYHKDBN" of the letter, case-insensitive: A = 1, C = 2, G = 4, T = 8, U / u
 *              as T, the other IUPAC letters their BAM codes (N = 15); any other byte is 15.
 *   d_codes    uint8, gci_layout_total() elements; every base is stored exactly once (its rank is the scanned tile count plus its
 *              rank inside the 4096-byte tile); elements no base goes to keep what they held.  Asynchronous on the context's stream.
 *
 * gci_bam_mismatch_size / _write: the input of gci_bam_indel_size plus d_codes; has_seq must be 1 (else GCI_E_INVALID).  Per record:
 *   counted    exactly when gci_bam_cover_size does not skip it with the same excl_flags (0x704 by default) and min_mapq.
 *   operations the record's own, or the first CG:B,I / B,i array behind a <l_seq>S<n>N placeholder (the rule of gci_bam_indel_size).  SEQ
 *              always lies behind the in-record CIGAR words, also in the CG case.
 *   positions  the query position q starts at 0 and advances under M, =, X, I and S; the reference position p starts at pos and
 *              advances under M, =, X, D and N, in 64 bits.  Under M, = and X query base q faces reference base p if p < L (the
 *              contig's length, clamped as for gci_bam_indel_size; a d_ref_sel beyond the layout: 0).  The letter of the operation
 *              does not matter: the bases decide.
 *   codes      the read's is the SEQ nibble (the high nibble of byte q / 2 is the even q), the reference's is d_codes[offset + p].
 *   compared   a facing pair whose two codes are each one of 1, 2, 4, 8.  A read nibble 0 ('='), N or another ambiguity code on
 *              either side is never compared.
 *   mismatch   a compared pair whose codes differ: one event gci_ivl{contig, p, p, 0}.
 *   l_seq      == 0 (SEQ '*'): counted, nothing compared, no status.  l_seq > 0 and S + M + I over all operations != l_seq:
 *              GCI_E_MALFORMED for that record, nothing of it is compared, no event, and no byte behind its SEQ is read.
 *   *d_status  as gci_bam_indel_size reports it (smallest record index << 8 | -status): records out of bounds, operation codes 9 - 15
 *              in a counted record (they move nothing), and the l_seq rule above.
 *   h_counts   host, 3 entries: the records counted, the mismatch events, the pairs compared.  The size call synchronises.
 * gci_bam_mismatch_write emits the events to d_out[0 .. h_counts[1]) in (record, reference position) order; ranks come from exclusive
 * scans, ballots and popcounts, no atomics: two runs give the same bytes.  cap < h_counts[1]: GCI_E_CAPACITY, nothing is written.
 * Another stream, n_bytes, offsets, n_rec or d_codes than the size call in front of it on this context measured: GCI_E_INVALID.
 * gci_depth_build with flank 0 over the events gives the mismatch track: per base the counted records that carry another base there.
 * Every mismatch lies on a base gci_bam_cover_size covers for the same record, so mismatch[b] <= depth[b] for the depth of the same
 * options without count_del.
 *
 * gci_mismatch_sites_size / _write: the runs of hot elements of such a track against the depth track.
 *   input      whole tracks of gci_layout_total() elements, 16-byte aligned (else GCI_E_INVALID); both are needed.
 *   windows    as gci_indel_sites_size takes them.
 *   hot        an element inside a window and inside its contig with mismatch >= min_reads and
 *              mismatch * 1000000 >= frac_ppm * depth in 64-bit integers.  min_reads < 1, frac_ppm outside 0 .. 1000000: GCI_E_INVALID.
 *   a site     a maximal run of consecutive hot elements of one contig inside one window, with the run rules of gci_indel_sites_size:
 *              contig, start and end (exclusive) on the contig, mismatch = the maximum of the mismatch track over the run, depth =
 *              the depth at the FIRST base of the run that reaches that maximum.  Sites come in ascending flat order.
 *   write      the sites of the size call in front of it on this context (same tracks, min_reads, frac_ppm and n_windows, nothing
 *              between the two that sets windows: else GCI_E_INVALID).  cap too small: GCI_E_CAPACITY, nothing is written.
 * Both passes read both tracks, 16 bytes a lane; run starts are counted per tile, scanned and stored by rank; a wave per site walks
 * the run.  No global atomics. */
typedef struct gci_mismatch_site {
    int32_t contig;
    int32_t start;
    int32_t end;
    int32_t mismatch;
    int32_t depth;
} gci_mismatch_site;
int gci_fasta_codes(gci_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, const int64_t* d_body, uint32_t n_records, const int64_t* d_dst,
                    const uint64_t* d_tile_kept0, uint8_t* d_codes);
int gci_bam_mismatch_size(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                          const int32_t* d_ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq, const uint8_t* d_codes, uint64_t* h_counts,
                          uint64_t* d_status);
int gci_bam_mismatch_write(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                           const uint8_t* d_codes, gci_ivl* d_out, uint64_t cap, uint64_t* d_status);
int gci_mismatch_sites_size(gci_ctx* ctx, const int32_t* d_mismatch, const int32_t* d_depth, int32_t min_reads, int32_t frac_ppm,
                            const gci_window* h_windows, uint32_t n_windows, uint64_t* h_n_sites);
int gci_mismatch_sites_write(gci_ctx* ctx, const int32_t* d_mismatch, const int32_t* d_depth, int32_t min_reads, int32_t frac_ppm,
                             const gci_window* h_windows, uint32_t n_windows, gci_mismatch_site* d_out, uint64_t cap);

/* ---- allele_sites.py: WHICH base the reads carry where they disagree with the assembly (k_mismatch.hip) ----------------------------------
 * gci_bam_allele_size / _write: the input of gci_bam_mismatch_size / _write, and its rules word for word -- which records count, which
 * pairs are compared, the contig's end, l_seq, what is malformed and the status word.  The one difference: a mismatch is an event of the
 * CLASS of the read's base, A, C, G or T (the SEQ nibble 1, 2, 4 or 8).
 *   h_counts   host, 6 entries: the records counted; the events whose read base is A; C; G; T; the pairs compared.  Entries 1 - 4 add up
 *              to gci_bam_mismatch_size's h_counts[1] for the same input, entries 0 and 5 are its h_counts[0] and [2].  The size call
 *              synchronises.
 *   write      d_out[0 .. nA + nC + nG + nT): the A list, then the C list, then G, then T (as gci_bam_indel_write lays out "deletions,
 *              then insertions"), every event gci_ivl{contig, p, p, 0}, inside a list in (record, reference position) order.  The ranks
 *              come from exclusive scans and wave scans, no atomics: two runs give the same bytes.  cap below the total:
 *              GCI_E_CAPACITY, nothing is written.  Another stream, n_bytes, offsets, n_rec or d_codes than gci_bam_allele_size measured
 *              last on this context: GCI_E_INVALID.  The pair keeps a memo of its own: a gci_bam_mismatch_size call between the two
 *              changes nothing.
 * gci_depth_build with flank 0 over list X gives track X: per base the counted records that carry X there where the assembly holds
 * another of A, C, G, T.  The four tracks add up to the mismatch track of gci_bam_mismatch_write.
 *
 * gci_allele_sites_size / _write: the SINGLE elements where one allele is hot -- not runs: two adjacent hot bases are two sites.
 *   input      the four allele tracks and the depth track, whole tracks of gci_layout_total() elements, 16-byte aligned (else
 *              GCI_E_INVALID), and d_codes, the gci_fasta_codes array; all six are needed.
 *   windows    as gci_indel_sites_size takes them.
 *   best       the largest of the four tracks at the element; alt is the first of A, C, G, T that reaches it: a tie goes to the earlier
 *              letter.
 *   hot        an element inside a window and inside its contig with best >= min_reads and best * 1000000 >= frac_ppm * depth in 64-bit
 *              integers.  min_reads < 1, frac_ppm outside 0 .. 1000000: GCI_E_INVALID.  The test is PER ALLELE: two alleles at 30 % of
 *              the depth each make gci_mismatch_sites_size hot at 500000 ppm (their sum is 60 %) and this lister cold.  That is meant:
 *              a site names one replacement base.  d_codes is no part of the test.
 *   a site     contig, pos (0-based on the contig); ref = d_codes[element] as it is (15, 0 and every other value are passed through);
 *              alt = 1, 2, 4 or 8; n = the A, C, G, T tracks at the element; depth.  Sites come in ascending flat order.
 *   write      the sites of the size call in front of it on this context (same six arrays, min_reads, frac_ppm and n_windows, nothing
 *              between the two that sets windows: else GCI_E_INVALID).  cap too small: GCI_E_CAPACITY, nothing is written.
 * The size pass reads the five tracks once, 16 bytes a lane and track (20 bytes a base); the write pass leaves a tile whose count is 0
 * at once and reads the code array only for the sites it stores.  No global atomics. */
typedef struct gci_allele_site {
    int32_t contig;
    int32_t pos;
    int32_t ref;
    int32_t alt;
    int32_t n[4];
    int32_t depth;
} gci_allele_site;
int gci_bam_allele_size(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                        const int32_t* d_ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq, const uint8_t* d_codes, uint64_t* h_counts,
                        uint64_t* d_status);
int gci_bam_allele_write(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                         const uint8_t* d_codes, gci_ivl* d_out, uint64_t cap, uint64_t* d_status);
int gci_allele_sites_size(gci_ctx* ctx, const int32_t* d_a, const int32_t* d_c, const int32_t* d_g, const int32_t* d_t, const int32_t* d_depth,
                          const uint8_t* d_codes, int32_t min_reads, int32_t frac_ppm, const gci_window* h_windows, uint32_t n_windows,
                          uint64_t* h_n_sites);
int gci_allele_sites_write(gci_ctx* ctx, const int32_t* d_a, const int32_t* d_c, const int32_t* d_g, const int32_t* d_t, const int32_t* d_depth,
                           const uint8_t* d_codes, int32_t min_reads, int32_t frac_ppm, const gci_window* h_windows, uint32_t n_windows,
                           gci_allele_site* d_out, uint64_t cap);

/* Cross-rank name check for contig-sharded runs (exact).  gci_hash_bucket sorts the 64-bit name hashes of the
 * passing records into n_parts buckets by (hash >> 33) % n_parts; a bucket is part_cap + 1 uint64 words:
 * [0] = number of hashes the sender had for it (> part_cap: overflow), [1..] = the hashes.  After ONE all-to-all of
 * the buckets, gci_hash_conflicts ADDS to *d_n_conflicts the number of hashes that arrived from more than one
 * source bucket (+1 per overflowing bucket).  Zero on every rank => no query name is shared between ranks, so
 * each rank's local join equals the global one.
 * d_next_out (may be NULL): a second bucket array the caller alternates with d_out.  When given, the call zeroes ITS
 * count words for the next call and relies on d_out's count words being zero already (zero-filled at allocation, then
 * kept so by this rule) -- no clearing launch per call.  NULL: d_out's count words are cleared by the call itself. */
int gci_hash_bucket(gci_ctx* ctx, const gci_rec* d_recs, uint32_t n, uint32_t n_parts, uint32_t part_cap,
                    uint64_t* d_out, uint64_t* d_next_out);
int gci_hash_conflicts(gci_ctx* ctx, const uint64_t* d_buckets, uint32_t n_parts, uint32_t part_cap,
                       uint32_t* d_n_conflicts);

/* ---- multi-GPU: the name-hash-sharded join ---------------------------------------------------------
 * Contigs are sharded over the ranks, the join (GCI.py:272-301) is by read name and independent per name: every passing
 * record goes to rank (name_hash >> 33) % n_parts, each rank joins the names it owns (gci_name_join over what arrived),
 * the surviving intervals go to the rank that owns their contig.  These calls fill / finish the fixed-shape buckets of the
 * three all-to-alls (the host side does the collectives: RCCL through torch.distributed, gci_amd/shard.py):
 *   gci_route_records   one file's records -> n_parts buckets of (cap + 1) gci_rec slots (slot 0: header, name_hash = number
 *                       of records routed to the part, flags = 0; then the records in FILE ORDER -- the routing is stable)
 *                       and n_parts * cap name slots of name_slot bytes (a multiple of 16, at least the longest name; zero padded)
 *   gci_route_seal_records   on the receiving side: slots beyond a bucket's count get flags = 0, so the whole receive buffer
 *                       is one gci_rec array in file order (source rank after source rank) for gci_name_join; the name of
 *                       slot d * (cap + 1) + 1 + k is at (d * cap + k) * name_slot of the received names
 *   gci_route_intervals intervals (contig = index among ALL selected contigs) -> buckets by d_owner[contig] (< 0: dropped);
 *                       slot 0 of a bucket = {contig = -1, start = count}
 *   gci_route_seal_intervals  receiving side: contig -> d_cmap[contig] (the rank's track layout), -1 beyond the count: the
 *                       buffer of n_parts * (cap + 1) intervals goes to gci_depth_build_* as it is
 * A count beyond cap or a name longer than name_slot sets *d_status to GCI_E_CAPACITY (grow the buckets).  With cap = 0 there
 * are no name slots and d_out_names may be NULL (gci_route_records, gci_route_hits): the headers still get the true counts. */
int gci_route_records(gci_ctx* ctx, const gci_join_file* h_file, uint32_t n_parts, uint32_t cap, gci_rec* d_out_recs,
                      uint8_t* d_out_names, uint32_t name_slot, uint64_t* d_status);
int gci_route_seal_records(gci_ctx* ctx, gci_rec* d_recs, uint32_t n_parts, uint32_t cap, uint64_t* d_status);
int gci_route_intervals(gci_ctx* ctx, const gci_ivl* d_ivl, const uint32_t* d_n, uint32_t max_n, const int32_t* d_owner,
                        int32_t n_contigs, uint32_t n_parts, uint32_t cap, gci_ivl* d_out, uint64_t* d_status);
int gci_route_seal_intervals(gci_ctx* ctx, gci_ivl* d_ivl, uint32_t n_parts, uint32_t cap, const int32_t* d_cmap,
                             int32_t n_contigs, uint64_t* d_status);

/* ---- R6: depth build ------------------------------------------------------------------------
 * depth[c][start+flank : end-flank+1] += 1 with Python/NumPy slice semantics, for n intervals
 * (n read from *d_n if d_n != NULL, clamped to max_n).  Overwrites the whole track. */
int gci_depth_build(gci_ctx* ctx, const gci_ivl* d_ivl, const uint32_t* d_n, uint32_t max_n, int flank,
                    int32_t* d_depth);

/* Fused form of the depth build (same result as gci_depth_build) that also delivers, from the
 * same pass and without re-reading the track from HBM, the things the reference computes from the
 * freshly built depths: the decimal text of write_depth (GCI.py:115-117), the per-contig sums behind
 * np.mean (GCI.py:862-868) and -- valid only when no gap mask will follow -- the run boundaries of
 * collapse_depth_range (GCI.py:369-390; same key format as gci_issue_scan).
 *   begin : buckets the intervals per tile, computes the requested by-products.  After it (and a
 *           sync) d_contig_text_off[n_contigs] tells the caller how large the text buffer must be.
 *   finish: writes the track and, if d_text != NULL, the text (requires want_text at begin). */
typedef struct gci_build_opts {
    int flank;                    /* --flank-len of the depth build */
    int want_text;                /* compute text offsets in begin so that finish can render text */
    uint64_t* d_contig_text_off;  /* n_contigs + 1 entries; required if want_text */
    int64_t* d_sums;              /* n_contigs entries or NULL */
    uint32_t* d_n_keys;           /* NULL: no fused issue scan */
    uint64_t* d_keys;
    uint32_t key_cap;
    int issue_flank;
    double lo, hi;
    int counted;                  /* 1: the intervals are exactly what the last gci_name_join_count emitted (same flank):
                                     the per-tile counting pass has been done there */
    int want_runs;                /* 1: finish also keeps, in the context, the constant-depth runs of every 4096-base tile as it
                                     wrote them; a gci_depth_deflate_size / _write pair over the SAME d_depth, announced by
                                     gci_depth_deflate_from_build(), then takes the runs from there instead of reading
                                     the track (members that start on a tile boundary: every contig does), once.  gci_gap_mask / gci_max2 / gci_two_type_tail, a new build and
                                     gci_layout_set drop the lists; a caller that writes the track by other means
                                     between the build and the deflate calls must not set this.  (Occupies what was
                                     padding: sizeof(gci_build_opts) is unchanged.) */
} gci_build_opts;
int gci_depth_build_begin(gci_ctx* ctx, const gci_ivl* d_ivl, const uint32_t* d_n, uint32_t max_n,
                          const gci_build_opts* h_opts);
int gci_depth_build_finish(gci_ctx* ctx, int32_t* d_depth, uint8_t* d_text, uint64_t text_cap);

/* ---- R8 / R9 -------------------------------------------------------------------------------- */
int gci_gap_mask(gci_ctx* ctx, int32_t* d_depth, const gci_ivl* d_gaps, uint32_t n_gaps);
int gci_max2(gci_ctx* ctx, const int32_t* d_a, const int32_t* d_b, int32_t* d_out);

/* The tail of a two-read-type run in one pass over the two tracks (GCI.py:1014-1024): N-run masks of both (GCI.py:324-328; h_gaps
 * in contig coordinates with Python's slice rules, HOST memory), their per-base maximum (GCI.py:350) into d_out, and the
 * issue-run boundary keys of all three tracks (GCI.py:369-390): d_keys = 3 x cap keys, d_n_keys = 3 counters -- per track the
 * keys gci_issue_scan(track, lo, hi, flank) gives.  d_a / d_b are masked in place.  d_sums (nullable): 3 x n_contigs sums of depth
 * (the masked a, the masked b, the maximum: what gci_depth_sum gives for each -- the numerator of np.mean, GCI.py:862-868).
 * 12 bytes per base instead of the 24 of gci_gap_mask x 2 + gci_max2 + gci_issue_scan x 3 (+ 12 for three gci_depth_sum). */
int gci_two_type_tail(gci_ctx* ctx, int32_t* d_a, int32_t* d_b, int32_t* d_out, const gci_ivl* h_gaps, uint32_t n_gaps,
                      double lo, double hi, int flank, uint64_t* d_keys, uint32_t cap, uint32_t* d_n_keys, int64_t* d_sums);

/* ---- R10: issue scan ------------------------------------------------------------------------
 * Finds every maximal run of `lo < depth <= hi` inside each window.  Emits unordered 64-bit
 * keys  (window << 33) | (rel << 1) | is_end,  rel = run start - window.begin for a start key,
 * run end (exclusive) - window.begin for an end key; sorted ascending they read
 * start,end,start,end... per window.  The reference's `i > flank_len` drop rule and
 * coordinate shifts are applied by the host.  gci_issue_scan uses one window per contig:
 * [flank, L - flank). */
int gci_issue_scan(gci_ctx* ctx, const int32_t* d_depth, double lo, double hi, int flank,
                   uint64_t* d_keys, uint32_t cap, uint32_t* d_n_keys);
int gci_issue_scan_windows(gci_ctx* ctx, const int32_t* d_depth, const gci_window* h_windows,
                           uint32_t n_windows, double lo, double hi, uint64_t* d_keys, uint32_t cap,
                           uint32_t* d_n_keys);

/* depth_plotter_v2.py, DataProcessor.analyze_depth_regions + the non-zero statistics of plot_single_sequence, in ONE read of
 * the windows: class 0 = (d == 0), class 1 = (0 < d < low_below).  d_keys: 2 x cap keys, d_n_keys: 2 counters, per class the keys
 * gci_issue_scan_windows would give for that predicate (same key format, same closing rule at the window end).
 * d_stats: n_windows x 2 int64, zeroed by the call: the sum of the depths > 0 and the number of bases with depth > 0. */
int gci_depth_classes(gci_ctx* ctx, const int32_t* d_depth, const gci_window* h_windows, uint32_t n_windows, int32_t low_below,
                      uint64_t* d_keys, uint32_t cap, uint32_t* d_n_keys, int64_t* d_stats);

/* ---- depth_to_bedgraph.py: the constant-depth runs of a set of windows, in order, and their bedGraph text (k_bedgraph.hip) ------
 * Element p of window [B, E) starts a run iff p == B or depth[p] != depth[p - 1]: a run never crosses a window's edge.  Windows are
 * clamped to the track as gci_issue_scan_windows clamps them; a window of more than 2^32 - 1 elements is GCI_E_INVALID.
 *   gci_depth_runs_count  d_win_run0[w] = index of window w's first run among the runs of all windows (window after window,
 *                         ascending inside a window), d_win_run0[n_windows] = the total.  Synchronises.
 *   gci_depth_runs_write  the runs of the windows of the count call in front of it on this context (same track, nothing between
 *                         the two that sets windows: else GCI_E_INVALID) to d_runs[0 .. total): start relative to the window's
 *                         beginning, and the depth.  cap < total: GCI_E_CAPACITY, nothing is written.
 * The text: per run one line  name '\t' start '\t' end '\t' depth '\n'  with start = h_coord0[w] + run start, end = h_coord0[w] +
 * the next run's start (the window's length behind its last run), both decimal without sign (h_coord0 >= 0), the depth a signed
 * decimal, the name h_name_len[w] (<= 65535) bytes at d_names + h_name_off[w].  A block of GCI_BG_RUNS_PER_BLOCK consecutive runs
 * is one workgroup's.
 *   gci_bedgraph_size     d_win_byte0[w] = byte offset of window w's first line, d_win_byte0[n_windows] = total bytes.  Synchronises.
 *   gci_bedgraph_write    the text of the size call in front of it on this context (same d_runs, d_win_run0 and n_windows: else
 *                         GCI_E_INVALID) to d_out[0 .. total).  cap < total: GCI_E_CAPACITY, nothing is written. */
#define GCI_BG_RUNS_PER_BLOCK 256
typedef struct gci_depth_run {
    uint32_t start;
    int32_t depth;
} gci_depth_run;
int gci_depth_runs_count(gci_ctx* ctx, const int32_t* d_depth, const gci_window* h_windows, uint32_t n_windows, uint64_t* d_win_run0);
int gci_depth_runs_write(gci_ctx* ctx, const int32_t* d_depth, gci_depth_run* d_runs, uint64_t cap);
int gci_bedgraph_size(gci_ctx* ctx, const gci_depth_run* d_runs, const uint64_t* d_win_run0, const gci_window* h_windows,
                      uint32_t n_windows, const int64_t* h_coord0, const uint32_t* h_name_len, uint64_t* d_win_byte0);
int gci_bedgraph_write(gci_ctx* ctx, const gci_depth_run* d_runs, const uint64_t* d_win_run0, const gci_window* h_windows,
                       uint32_t n_windows, const int64_t* h_coord0, const uint8_t* d_names, const uint64_t* h_name_off,
                       const uint32_t* h_name_len, uint8_t* d_out, uint64_t cap);

/* ---- depth_dist.py: the depth histogram and the sum / min / max / count of a set of windows, in one read (k_hist.hip) -------------
 * Windows are [begin, end) in track elements, clamped to the track as gci_issue_scan_windows clamps them; they may overlap, repeat,
 * share a tile or be empty.
 *   d_stats  n_windows x 4 int64, initialised by the call: the sum of the depths, the minimum, the maximum and the number of
 *            elements of the clamped window; an empty window gives 0, INT32_MAX, INT32_MIN, 0.
 *   d_hist   n_windows x (n_bins + 2) uint64, zeroed by the call: column b < n_bins counts the elements with depth == b, column
 *            n_bins ("over") those with depth >= n_bins, column n_bins + 1 ("under") those with depth < 0: every element of a window
 *            lands in exactly one column.
 * n_bins == 0 is a statistics-only pass: d_hist holds over / under only and may be NULL (nothing is counted then).  n_bins >
 * GCI_HIST_MAX_BINS, a NULL d_hist with n_bins > 0 and windows, a NULL d_stats with windows: GCI_E_INVALID; a refused call writes
 * nothing.  All results are integers and exact.  A workgroup accumulates GCI_HIST_CHUNK_TILES consecutive 4096-element tiles of ONE
 * window in LDS before it adds its non-zero bins to d_hist. */
#define GCI_HIST_MAX_BINS 65536
#define GCI_HIST_CHUNK_TILES 64
int gci_depth_hist(gci_ctx* ctx, const int32_t* d_depth, const gci_window* h_windows, uint32_t n_windows, uint32_t n_bins,
                   uint64_t* d_hist, int64_t* d_stats);

/* ---- R7: depth text -------------------------------------------------------------------------
 * size: d_contig_off[c] = byte offset of contig c's lines in the text, d_contig_off[n_contigs] =
 * total bytes (no '>' lines: the host writes those).  write: fills d_out (cap >= total). */
int gci_depth_text_size(gci_ctx* ctx, const int32_t* d_depth, uint64_t* d_contig_off);
int gci_depth_text_write(gci_ctx* ctx, const int32_t* d_depth, uint8_t* d_out, uint64_t cap);

/* ---- R7 / N2: the depth text as gzip members, written by the GPU ------------------------------------------------
 * write_depth (GCI.py:99-143) sends f'{depth}\n' per base through gzip; these two calls emit the same payload as
 * DEFLATE without ever materialising the text: per constant-depth run the line's literals + length/distance pairs
 * (distance = line length) in the fixed Huffman code, one block per 4096-base tile closed by an empty stored block,
 * 64 tiles (one wave) = one gzip member with its CRC-32 and ISIZE (CRC of the virtual text by GF(2) polynomial
 * arithmetic over the runs).  Any int32 track (fresh, gap-masked, two-type) with depths >= 0.
 * A member m covers d_member_n[m] <= 64 * 4096 consecutive bases starting at element d_member_elem[m] (a multiple
 * of 4; the caller cuts members so that none spans two contigs and writes the '>contig' lines as members of its own).
 *   size:  d_tile_bytes[64 m + t], d_member_bytes[m] (header and trailer included), d_member_crc[m], d_member_isize[m]
 *   write: d_member_out[m] = byte offset of member m in d_out (exclusive scan of d_member_bytes by the caller). */
/* The run lists a build kept (gci_build_opts.want_runs) are used by the NEXT size / write pair only when the caller says so, here:
 * "d_depth is the track that build wrote, and nothing -- no call of this library through any context, no other code -- has
 * written it since".  The library cannot see writes that go around this context (another context's gci_gap_mask, the caller's
 * own kernels, an allocator handing the address to a new buffer), so a pointer match alone is never taken as that statement.
 * Returns GCI_E_INVALID when this context holds no lists for d_depth; the pair that follows consumes the lists (one shot). */
int gci_depth_deflate_from_build(gci_ctx* ctx, const int32_t* d_depth);
int gci_depth_deflate_size(gci_ctx* ctx, const int32_t* d_depth, const uint64_t* d_member_elem, const uint32_t* d_member_n,
                           uint32_t n_members, uint32_t* d_tile_bytes, uint32_t* d_member_bytes, uint32_t* d_member_crc,
                           uint32_t* d_member_isize);
int gci_depth_deflate_write(gci_ctx* ctx, const int32_t* d_depth, const uint64_t* d_member_elem, const uint32_t* d_member_n,
                            uint32_t n_members, const uint32_t* d_tile_bytes, const uint32_t* d_member_crc,
                            const uint32_t* d_member_isize, const uint64_t* d_member_out, uint8_t* d_out, uint64_t cap);

/* ---- R15 ------------------------------------------------------------------------------------ */
int gci_depth_sum(gci_ctx* ctx, const int32_t* d_depth, int64_t* d_sums /* n_contigs */);

/* ---- N3: window sums for the `-p` numeric front-end (sliding_window_average_depth, GCI.py:660-705) ----------
 * d_ranges holds n_ranges pairs (begin, end) of TRACK element indices (contig offset + position); d_sums[r] = sum of
 * the depths in [begin, end).  The caller derives the ranges from the zero-depth runs (gci_issue_scan_windows with
 * lo = -1, hi = 0) and the window size: the reference restarts its window at every zero-depth base. */
int gci_range_sums(gci_ctx* ctx, const int32_t* d_depth, const int64_t* d_ranges, uint64_t n_ranges, int64_t* d_sums);

/* ---- N4 (first half): N runs of the assembly, get_Ns_ref (GCI.py:27-35) ------------------------------------------
 * d_text: the FASTA file's bytes.  d_body: n_records pairs (begin, end) of byte offsets, the body of every record
 * (behind its title line, up to the next '>' line), sorted.  Output: d_tile_kept[k] = bytes of the 4096-byte tile k
 * that count as sequence (not a line end, '\r' or blank, not in a title line), and keys = (byte offset << 1) | e for
 * every base where a run of N / n begins (e = 0) or that follows the last base of a run (e = 1); *d_n_keys may exceed
 * cap (nothing is written beyond it: call again with more room).  A run that reaches the end of a record has no end
 * key.  The host turns byte offsets into sequence coordinates with the prefix sum of d_tile_kept. */
int gci_fasta_n_scan(gci_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, const int64_t* d_body, uint32_t n_records,
                     uint32_t* d_tile_kept, uint64_t* d_keys, uint32_t cap, uint32_t* d_n_keys);

/* ---- depth text -> track: the parse of utility/GCI_score.py:11-39 (k_depth_parse.hip; tiles, ranks: gci_text_tiles.hpp) --
 * d_text: inflated `.depth.gz` text, ('>' name '\n' (decimal '\n')^L)*.  Tiles of 4096 bytes; a line belongs to the tile that
 * holds its first byte (offset 0 and every byte behind a '\n'; a last line without '\n' counts).  Two passes, no chain between
 * workgroups:
 *   gci_depth_text_index  d_tile_lines[k] = line starts in tile k; keys = (byte offset << 12) | rank of the line within its tile
 *                         for every line whose first byte is '>' (*d_n_hdr may exceed cap: nothing is written beyond it, call
 *                         again with more room); *d_bad = smallest byte offset of a data line outside [0-9]{1,10} followed by
 *                         '\n' or the end of the text, or with a value above INT32_MAX -- UINT64_MAX if none.
 *   gci_depth_text_parse  d_tile_line0 = exclusive scan of d_tile_lines (gci_dev_u32_scan_u64); d_segs = n_segs triples of int64
 *                         (first data line index, data lines, track element of the first or -1 = skip), sorted by first line;
 *                         every data line g of segment s goes to d_track[base + g - first] (element indices >= track_n are not
 *                         written).  Only for text that gci_depth_text_index found valid. */
int gci_depth_text_index(gci_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, uint32_t* d_tile_lines, uint64_t* d_hdr_keys,
                         uint32_t cap, uint32_t* d_n_hdr, uint64_t* d_bad);
int gci_depth_text_parse(gci_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, const uint64_t* d_tile_line0, const int64_t* d_segs,
                         uint32_t n_segs, int32_t* d_track, uint64_t track_n);

/* ---- samtools depth text -> track: the line loop of utility/convert_samtools_depth.py:12-19 (k_sdepth.hip, gci_text_tiles.hpp) --
 * d_text: the text of `samtools depth -a`, (name '\t' position '\t' depth '\n')*, 16-byte aligned.  Tiles and line ownership as
 * above.  The strict grammar: name = 1 or more bytes 0x21 .. 0x7E; position = [0-9]{1,10}; depth = 0 or [1-9][0-9]{0,9} with a
 * value <= INT32_MAX; the line closed by '\n' or the end of the text and, its '\n' included, at most 255 bytes long.
 *   gci_sdepth_index  d_tile_lines[k] = line starts in tile k; keys = (byte offset << 12) | rank of the line within its tile for
 *                     every line whose name (the bytes in front of its first '\t' or '\n') differs from the name of the line in
 *                     front of it, or whose line in front is longer than the bound; the first line of the text is compared with
 *                     d_prev_name[0 .. prev_len) (prev_len = 0 at the start of a file, <= 255; a later chunk of a file gives
 *                     the name of the last line of the chunk in front).  *d_n_keys may exceed cap (nothing is written beyond
 *                     it: call again with more room); *d_bad = smallest byte offset of a line outside the grammar, UINT64_MAX
 *                     if none.
 *   gci_sdepth_parse  d_tile_line0 = exclusive scan of d_tile_lines (gci_dev_u32_scan_u64); line_base = lines of the file in front
 *                     of this text; d_segs = n_segs triples of int64 (first line index in the file, lines, track element of the
 *                     first or -1 = skip), sorted by first line; line g of segment s goes to d_track[base + g - first] (element
 *                     indices >= track_n are not written).  Only for text that gci_sdepth_index found valid. */
int gci_sdepth_index(gci_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, const uint8_t* d_prev_name, uint32_t prev_len,
                     uint32_t* d_tile_lines, uint64_t* d_keys, uint32_t cap, uint32_t* d_n_keys, uint64_t* d_bad);
int gci_sdepth_parse(gci_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, const uint64_t* d_tile_line0, uint64_t line_base,
                     const int64_t* d_segs, uint32_t n_segs, int32_t* d_track, uint64_t track_n);

/* ---- this library's own .depth.gz -> track, without inflating it (k_depth_gz.hip) ---------------------------------------------
 * The counterpart of gci_depth_deflate_*: the members those calls write are decoded straight back into (depth, count) runs, their
 * CRC-32 and ISIZE checked by the same GF(2) algebra, and the runs expanded into the int32 track.  No text exists anywhere.
 * The grammar a member must obey (anything else, however legal as gzip, is GCI_DGZ_FOREIGN and the caller's to inflate):
 *   header   the ten bytes 1f 8b 08 00 00 00 00 00 00 ff
 *   blocks   fixed-Huffman blocks (at most 65), a stored block only behind a fixed one, empty and never final; the final block fixed
 *   a block  literals spell one line [0-9]{1,10} '\n' (no leading zero, value <= INT32_MAX) of width w; matches follow with distance
 *            exactly w; their lengths add up to whole lines before the next literal or the end of the block; at most 262 144 lines
 *            per member
 *   trailer  CRC-32 and ISIZE behind the final block, byte aligned
 * d_raw: the bytes of the file (any alignment, no padding needed: nothing at or beyond d_raw + n_raw is read).
 *   gci_depth_gz_scan    one lane per candidate member start d_cand_pos[i] (every position of the ten-byte header in the file will
 *                        do: a false candidate inside another member's bits is refused or, rarely, accepted -- the caller follows
 *                        the chain of end offsets from byte 0 and never looks at it).  d_info[i]: status; for GCI_DGZ_OK the end
 *                        offset (behind ISIZE), lines, runs (one per literal line) and whether the trailer's CRC-32 / ISIZE equal
 *                        those of the text the runs stand for; all zero behind GCI_DGZ_FOREIGN.
 *   gci_depth_gz_runs    d_members[m]: pos, runs and lines as the scan reported them, run0 = exclusive scan of runs; writes member
 *                        m's runs to d_runs[run0 ...] and keeps, per 4096 lines of a member, where they begin in its runs.
 *   gci_depth_gz_expand  the same d_members (elem0 = track element of the member's first line), right behind gci_depth_gz_runs on
 *                        the same context: line k of member m to d_track[elem0 + k] (16-byte stores where elem0 is a multiple of
 *                        4); elements at or beyond track_n are not written. */
enum { GCI_DGZ_OK = 0, GCI_DGZ_FOREIGN = 1 };
#define GCI_DGZ_MAX_LINES 262144u
#define GCI_DGZ_MAX_BLOCKS 65u
typedef struct gci_dgz_info {
    uint64_t end;
    uint32_t status;
    uint32_t lines;
    uint32_t runs;
    uint32_t crc_ok;
    uint32_t isize_ok;
    uint32_t reserved;
} gci_dgz_info;
typedef struct gci_dgz_member {
    uint64_t pos;
    uint64_t run0;
    uint64_t elem0;
    uint32_t runs;
    uint32_t lines;
} gci_dgz_member;
typedef struct gci_dgz_run {
    int32_t depth;
    uint32_t count;
} gci_dgz_run;
int gci_depth_gz_scan(gci_ctx* ctx, const uint8_t* d_raw, uint64_t n_raw, const uint64_t* d_cand_pos, uint32_t n_cand,
                      gci_dgz_info* d_info);
int gci_depth_gz_runs(gci_ctx* ctx, const uint8_t* d_raw, uint64_t n_raw, const gci_dgz_member* d_members, uint32_t n_members,
                      gci_dgz_run* d_runs);
int gci_depth_gz_expand(gci_ctx* ctx, const gci_dgz_run* d_runs, const gci_dgz_member* d_members, uint32_t n_members,
                        int32_t* d_track, uint64_t track_n);

/* ---- host-side container helpers (no GPU work) ---------------------------------
 * The reference reaches BGZF / BAM through pysam/htslib (GCI.py:150-151) and writes gzip through Python's gzip
 * module (GCI.py:111).  All pointers are HOST pointers.
 *   gci_bgzf_scan            member count and total inflated size (sum of ISIZE) of a BGZF byte string
 *   gci_bgzf_inflate         inflate every member into h_out, members in parallel on `threads` host threads
 *   gci_bam_record_offsets   end of the BAM header and the byte offset of every record (the one serial step of
 *                            the decode); h_offs may be NULL to count only
 *   gci_gzip_members         gzip-frame text as independent members of `chunk` input bytes, compressed in
 *                            parallel (any multi-member gzip whose payload equals the text is a valid .depth.gz)
 *   gci_bgzf_blocks / gci_bam_chunk_offsets   the same for a host that streams a large file chunk by chunk: the
 *                            member table, and the record offsets of one chunk with the partial tail reported
 *   gci_bam_heads            BGZF file bytes -> heads stream + record offsets in one pipelined pass (replaces
 *                            pysam's AlignmentFile + fetch, GCI.py:150-151, for a host that feeds
 *                            gci_bam_pages_* with has_seq = 0): groups of `group_bytes` (0 = 16 MiB) of inflated members rotate
 *                            through three buffers -- worker threads inflate group g while the caller's thread walks
 *                            the block_size chain of group g-1 and the workers copy the heads of group g-2 -- so the
 *                            inflated stream (27 KB per HiFi record) never exists as a whole and only ~400 B per
 *                            record cross PCIe.  A record whose l_seq / name / CIGAR lengths contradict its
 *                            block_size is emitted as its 36 fixed bytes with l_seq = -1 (the filter reports
 *                            GCI_E_MALFORMED with its index, as on the full stream); block_size < 32, a bad
 *                            member or a truncated last record return GCI_E_MALFORMED here.
 *                            gci_bam_heads_stream / _offsets stay valid until gci_bam_heads_free. */
/*   gci_fasta_titles         byte offsets of every '>' that begins a line (one per record SeqIO.parse yields,
 *                            GCI.py:30 / :940), in file order; h_pos may be NULL with cap 0 to count only */
int gci_fasta_titles(const uint8_t* h_text, uint64_t n, int threads, uint64_t* h_pos, uint64_t cap, uint64_t* n_pos);
typedef struct gci_heads gci_heads;
int gci_bam_heads(const uint8_t* h_raw, uint64_t n_raw, int threads, uint64_t group_bytes, int check_crc, gci_heads** out);
uint64_t gci_bam_heads_bytes(const gci_heads* h);          /* length of the heads stream */
uint64_t gci_bam_heads_count(const gci_heads* h);          /* records */
uint64_t gci_bam_heads_first(const gci_heads* h);          /* length of the BAM header = offset of record 0 */
const uint8_t* gci_bam_heads_stream(const gci_heads* h);
const uint64_t* gci_bam_heads_offsets(const gci_heads* h); /* offset of every record's block_size word */
int gci_bam_heads_free(gci_heads* h);
int gci_bgzf_scan(const uint8_t* h_raw, uint64_t n_raw, uint64_t* n_blocks, uint64_t* inflated_bytes);
int gci_bgzf_blocks(const uint8_t* h_raw, uint64_t n_raw, uint64_t* h_pos, uint64_t* h_isize, uint64_t cap,
                    uint64_t* n_blocks);
/* The member table in ONE pass by `threads` host threads (the chain of BSIZE fields is walked range by range and stitched: a
 * page fault per member is what the walk costs, 0.65 s for 64.5 GB on one thread): a handle; _export fills count + 1 offsets
 * (the last = n_raw) and count ISIZEs. */
typedef struct gci_bgzf_table gci_bgzf_table;
int gci_bgzf_table_build(const uint8_t* h_raw, uint64_t n_raw, int threads, gci_bgzf_table** out);
/* Only the members that start in front of byte `limit` (the table's byte length = the end of the last of them): the first run of
 * a large file can be on its way to the device while the table of the rest is made. */
int gci_bgzf_table_build_prefix(const uint8_t* h_raw, uint64_t n_raw, uint64_t limit, int threads, gci_bgzf_table** out);
/* The same table read with pread() through a descriptor of the file (n_raw = its size) instead of a mapping of it: one system
 * call per member and no page-table entry -- on a freshly mapped 77 GB file the page faults of the walk are 1.4 s on 16 threads,
 * in the address space the threads that stage the file's bytes fault in as well. */
int gci_bgzf_table_build_fd(int fd, uint64_t n_raw, int threads, gci_bgzf_table** out);
uint64_t gci_bgzf_table_count(const gci_bgzf_table* t);
int gci_bgzf_table_export(const gci_bgzf_table* t, uint64_t* h_pos, uint64_t* h_isize);
int gci_bgzf_table_free(gci_bgzf_table* t);
int gci_bam_chunk_offsets(const uint8_t* h_buf, uint64_t n, uint64_t start, uint64_t* h_offs, uint64_t cap,
                          uint64_t* n_rec, uint64_t* consumed);
int gci_bgzf_inflate(const uint8_t* h_raw, uint64_t n_raw, uint8_t* h_out, uint64_t cap, int threads, int check_crc);
int gci_bam_record_offsets(const uint8_t* h_stream, uint64_t n, uint64_t* h_offs, uint64_t cap, uint64_t* n_rec,
                           uint64_t* first_record);
uint64_t gci_gzip_bound(uint64_t n, uint64_t chunk);
int gci_gzip_members(const uint8_t* h_text, uint64_t n, uint64_t chunk, int level, int threads, uint8_t* h_out,
                     uint64_t cap, uint64_t* n_out);
/* A generic multi-member gzip file (a `.depth.gz` of this project or of the reference: members without BSIZE, so not BGZF)
 * inflated on `threads` host threads.  Candidate member starts (1f 8b 08 + a flag byte without reserved bits) are inflated
 * speculatively side by side; the members accepted are the chain that starts at offset 0, each ending where the next begins
 * (NUL padding between members and at the end is skipped, as Python's gzip reader does), CRC-32 and ISIZE checked by zlib.
 * A chain that does not close falls back to ONE serial pass.  GCI_E_MALFORMED: the file is not a valid gzip stream (the caller
 * reproduces the reference's exception).  The text stays with the handle: _export copies bytes [first, first + n) of it. */
typedef struct gci_gz gci_gz;
int gci_gz_inflate(const uint8_t* h_raw, uint64_t n_raw, int threads, gci_gz** out);
uint64_t gci_gz_bytes(const gci_gz* g);                    /* inflated length */
uint64_t gci_gz_members(const gci_gz* g);                  /* members of the chain */
int gci_gz_serial(const gci_gz* g);                        /* 1: the parallel chain did not close, the serial pass made the text */
int gci_gz_export(const gci_gz* g, uint64_t first, uint64_t n, uint8_t* h_out, int threads);
int gci_gz_free(gci_gz* g);

/* ---- N4 (second half, host): the PAF filter of filter(), GCI.py:211-254 --------------------------------------------
 * h_files[i] / n_bytes[i]: the bytes of PAF file i, in command-line order.  targets: the selected contigs (index =
 * gci_rec.contig).  On success *out holds, per file, one compact record + name for every query seen so far in first-
 * appearance order (the reference's block table is created once, outside its per-file loop); GCI_REC_HQ marks the
 * names of the reference's high_qual set as it stands after the last file.  GCI_E_MALFORMED / GCI_E_ZERO_DIV: a line
 * the reference would raise IndexError / ValueError / ZeroDivisionError on; *err_line = its 1-based number.
 * Lines are tokenised and filtered on `threads` host threads (byte ranges cut at line starts), queries are numbered in
 * first-appearance order by one pass over the surviving lines, and the per-query arithmetic runs in parallel again. */
typedef struct gci_paf gci_paf;
int gci_paf_filter(const uint8_t* const* h_files, const uint64_t* n_bytes, int n_files, const char* const* targets,
                   int n_targets, int map_qual, int mq_cutoff, double iden_percent, int threads /* 0 = automatic */,
                   gci_paf** out, uint64_t* err_line);
uint64_t gci_paf_count(const gci_paf* r, int file);
uint64_t gci_paf_name_bytes(const gci_paf* r, int file);
int gci_paf_export(const gci_paf* r, int file, gci_rec* h_recs, uint8_t* h_names, uint64_t* h_name_off /* count + 1 */);
int gci_paf_free(gci_paf* r);

/* ---- R3 / N4: the same PAF filter on the GPU (k_paf.hip) ----------------------------------------------------------------
 * d_text: the bytes of all PAF files back to back in ONE device buffer, h_file_end[i] = end offset of file i (host array).
 * Line starts, the tokeniser (str.strip + split, int() of the eight numeric columns, target lookup, identity and the
 * mapq / identity filter), the grouping of the surviving lines by query and the per-query scoring (GCI.py:241-254) all run
 * on the device; results and errors are those of gci_paf_filter (*err_line = 1-based line of the offending file, 0 for an
 * error raised while scoring).  The call synchronises.  Per file the handle holds one compact record per query seen so
 * far (order unspecified) and the byte offset of its name INSIDE d_text: join with d_name_base = d_text, name_delta = 0.
 * gci_paf_dev_export copies them into the caller's device buffers (gci_paf_dev_count entries each), on the ctx stream. */
typedef struct gci_paf_dev gci_paf_dev;
int gci_paf_filter_device(gci_ctx* ctx, const uint8_t* d_text, const uint64_t* h_file_end, int n_files, const char* const* targets,
                          int n_targets, int map_qual, int mq_cutoff, double iden_percent, gci_paf_dev** out, uint64_t* err_line);
uint64_t gci_paf_dev_count(const gci_paf_dev* r, int file);
int gci_paf_dev_export(const gci_paf_dev* r, int file, gci_rec* d_recs, uint64_t* d_name_off);
int gci_paf_dev_free(gci_paf_dev* r);

/* The same filter in two halves, for runs that shard a PAF file over the GPUs of a node by BYTE RANGE (each rank tokenises the
 * lines of its range; a query's lines may lie in several ranges, and GCI.py:241-254 scores a query over all of them -- in
 * file order, over all files so far -- so the hits travel to the rank that owns the query name before they are scored):
 *   gci_paf_hits_device   stage A: the lines of this rank's ranges (d_text: the ranges of the files back to back, cut at line
 *                         starts) that pass GCI.py:218-239, as gci_paf_hit in line order; errors as gci_paf_filter_device,
 *                         *err_line counted from the start of the range (sharded callers fall back to the whole files on
 *                         any error, where the reference's exception comes out exactly)
 *   gci_route_hits        hits -> n_parts buckets of (cap + 1) slots by (qhash >> 33) % n_parts, stable (slot 0: header,
 *                         qhash = count), query names into slots of name_slot bytes -- as gci_route_records
 *   gci_paf_score_device  stage B: the hits of the queries this rank owns, file after file (h_hits_upto), every file in line
 *                         order (source rank after source rank: the ranges ascend with the rank), qn_off relative to d_names
 *                         -> the handle of gci_paf_filter_device */
typedef struct gci_paf_hit {
    uint64_t qn_off;          /* where the query name lies (stage A: in d_text; stage B: in d_names) */
    uint64_t qhash;           /* gci_name_hash of the query name */
    int64_t qlen, qs, qe, ts, te;
    double identity;          /* nmatch / alnlen, IEEE f64 */
    uint32_t qn_len;
    int32_t t;                /* target: index among the selected contigs */
    uint32_t hq;              /* mapq >= mq_cutoff */
    uint32_t slot;            /* scratch of stage B */
} gci_paf_hit;
#define GCI_PAF_HIT_BYTES 80
typedef struct gci_paf_hits gci_paf_hits;
int gci_paf_hits_device(gci_ctx* ctx, const uint8_t* d_text, const uint64_t* h_file_end, int n_files, const char* const* targets,
                        int n_targets, int map_qual, int mq_cutoff, double iden_percent, gci_paf_hits** out, uint64_t* err_line);
uint64_t gci_paf_hits_count(const gci_paf_hits* r, int file);
int gci_paf_hits_export(const gci_paf_hits* r, int file, uint8_t* d_hits);
int gci_paf_hits_free(gci_paf_hits* r);
int gci_route_hits(gci_ctx* ctx, const uint8_t* d_hits, uint32_t n, const uint8_t* d_name_base, uint32_t n_parts, uint32_t cap,
                   uint8_t* d_out_hits, uint8_t* d_out_names, uint32_t name_slot, uint64_t* d_status);
int gci_paf_score_device(gci_ctx* ctx, const uint8_t* d_names, uint8_t* d_hits, const uint32_t* h_hits_upto, int n_files,
                         const char* const* targets, int n_targets, gci_paf_dev** out);
/* The PAF filter's pooled scratch (kept in the context between calls, up to 16 GB) given back to the driver: for a host whose other
 * stages allocate through an allocator of their own.  Synchronises when there is something to free. */
int gci_paf_pool_release(gci_ctx* ctx);
/* The tokeniser parses a workgroup's 256 lines from a copy in LDS, or -- when their stretch and its alignment slack exceed 49152
 * bytes -- walks them in global memory: the number of workgroups that did in the last gci_paf_filter_device /
 * gci_paf_hits_device of this context.  The two walks give the same hits; this tells them apart. */
uint64_t gci_paf_global_groups(const gci_ctx* ctx);

/* ---- the way of a memory-mapped input file to the device (staging.cpp) ---------------------------------------------------------
 * A ring of n_slots pinned host buffers of slot_bytes each, filled by `threads` host threads (parallel memcpy out of the page
 * cache) and emptied by DMA on the caller's stream.  gci_stage_send: h_src[0, n) -> d_dst[0, n) on `stream` (a hipStream_t);
 * returns when the last piece is enqueued -- its bytes are in a pinned slot by then, the caller may unmap the file.  forget != 0
 * drops the pages of h_src from the process's page table as they are read (madvise DONTNEED; the page cache keeps the data);
 * urgent == 0 lets urgent calls of other threads go first, piece by piece.  Calls from several threads take slots in turns. */
typedef struct gci_stage gci_stage;
int gci_stage_create(gci_ctx* ctx, uint64_t slot_bytes, int n_slots, int threads, gci_stage** out);
int gci_stage_send(gci_ctx* ctx, gci_stage* stage, const uint8_t* h_src, uint64_t n, uint8_t* d_dst, void* stream, int forget, int urgent);
/* ... from a file descriptor: bytes [offset, offset + n) by pread() straight into the pinned slots (no mapping, no page faults) */
int gci_stage_send_fd(gci_ctx* ctx, gci_stage* stage, int fd, uint64_t offset, uint64_t n, uint8_t* d_dst, void* stream, int urgent);
int gci_stage_free(gci_stage* stage);

/* ---- N1 on the GPU: BGZF inflate and the BAM record walk (k_inflate.hip, k_records.hip; replaces pysam / htslib at GCI.py:150-151) ---------
 * gci_bgzf_inflate_device: d_raw = the bytes of a BGZF file (or of a run of its members) on the device; d_member_pos[m] =
 * offset of member m in d_raw, n_members + 1 entries (the last = end of the run; gci_bgzf_blocks makes the table on the
 * host); d_out_off[m] = where member m's output goes in d_out (exclusive scan of the members' ISIZE, n_members + 1 entries).
 * A WAVE per member (k_inflate_wave.hip: the block's body cut into 64 pieces decoded side by side from guessed bit offsets and
 * stitched where neighbouring decoders fall into step, the symbols as a stream in scratch memory of the context, the copies
 * resolved by pointer jumping over the member's output in LDS); the members that do not stitch -- a few in a thousand -- and,
 * with GCI_INFLATE=lane in the environment, all of them by one LANE per member (k_inflate.hip: decode tables in LDS, the output
 * buffer is the window).  Every member's length and -- check_crc != 0, by a further kernel, one wave per member -- CRC-32 are
 * verified.  d_raw must be readable for 8 bytes past its last member (the decoders fetch whole aligned words).
 * *d_status: min over failing members of (member << 8 | -status), UINT64_MAX if none (decode with gci_decode_status).
 * gci_bgzf_inflate_streams(ctx, 2): every other batch of members runs on a second stream of the context's own.  For a host
 * whose HIP runtime has hardware queues to spare: the queues are shared by all streams of a process, and a copy stream that
 * shares one with the inflate waits for it (uploads at 26 instead of 58 GB/s); only the host knows how many queues its runtime
 * was given: the default is 1.
 * GCI_INFLATE_STREAMS=1|2 in the environment overrides (measurements).
 * gci_bgzf_inflate_last_stats (synchronises): how the members of the context's LAST gci_bgzf_inflate_device call fared with the
 * wave decoder -- h_counts[0] decoded, [1] header not taken, [2] no meeting point, [3] end-of-block codes on wrong paths,
 * [4] undecodable / copies, [5] length, [6] lanes, [7] not tried (GCI_INFLATE=lane); [1 .. 6] went to the lane decoder.
 *
 * gci_bam_record_offsets_device: the byte offset of every record of an inflated BAM stream on the device, without the serial
 * block_size chain: candidate record starts by a strict format test on every byte position, successor lookup, reachability
 * from `first_record` (= end of the BAM header) by pointer doubling.  d_result (device, 3 x uint64): [0] records found (may
 * exceed cap: nothing is written beyond it), [1] bytes consumed (n_bytes, or the offset of a partial last record when the
 * stream is a chunk), [2] != 0: the chain broke at offset [1] (a record the strict test rejects: take the host walk).
 * The call synchronises. */
int gci_bgzf_inflate_device(gci_ctx* ctx, const uint8_t* d_raw, const uint64_t* d_member_pos, const uint64_t* d_out_off,
                            uint32_t n_members, uint8_t* d_out, uint64_t out_cap, int check_crc, uint64_t* d_status);
int gci_bgzf_inflate_streams(gci_ctx* ctx, int n);
int gci_bgzf_inflate_last_stats(gci_ctx* ctx, uint32_t h_counts[32]);
/* Members the device decodes at a time (a launch takes a whole number of such rounds: size runs of a large file accordingly); 0 = unknown. */
uint32_t gci_bgzf_inflate_round(gci_ctx* ctx);
int gci_bam_record_offsets_device(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, uint64_t first_record, int32_t n_ref,
                                  uint64_t* d_offs, uint64_t cap, uint64_t* d_result);

#ifdef __cplusplus
}
#endif
#endif /* GCI_HIP_H */
