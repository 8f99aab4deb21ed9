// gci_cover_chunks.hpp -- the CIGAR of a BAM stream as CHUNKS of at most GCI_COVER_CHUNK_OPS operations, one wave each: what the
// kernels that walk whole CIGARs share (k_cover.hip: the covered bases; k_fate.hip: the base totals of the record filter's two
// quotients; k_clips.hip, k_indels.hip, k_mismatch.hip: the events of a record or of a walk), with cv_parse_counted as the one record
// parse of k_cover.hip and those three, and RecFrame as the head of their per-record scratch.  A lane per
// record says where the record's operations lie and how many chunks they make (CoverRec), an exclusive scan of the chunk counts
// numbers the chunks, and a wave finds its record (cv_rec_of_chunk), its piece of the operation array (cv_chunk_of) and its
// operation words, 64 a round (cv_op_word).
//
// CIGAR words lie at any byte phase of the stream: a lane loads the naturally aligned dword its operation begins in, takes the next
// one from its neighbour lane and re-aligns the two in registers (v_alignbyte), as k_cigar_chunks and pg_src_dword do.
#pragma once
#include "gci_ctx.hpp"

#define CV_OPS GCI_COVER_CHUNK_OPS
static_assert(CV_OPS % 64 == 0, "a chunk is whole rounds of one operation per lane");

struct CoverRec {
    uint64_t ops_off;              // byte offset of the first operation word in the stream
    uint32_t n_ops;
    int32_t contig;                // index among the selected contigs (the record is not skipped when it has chunks)
    int32_t pos;
    uint32_t pad;
};

__device__ __forceinline__ void cv_report(unsigned long long* status, uint32_t rec, int code)
{
    atomicMin(status, ((unsigned long long)rec << 8) | (unsigned long long)(uint8_t)(-code));
}

__device__ __forceinline__ uint32_t cv_rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ uint32_t cv_rd32(const uint8_t* p) { return cv_rd16(p) | (cv_rd16(p + 2) << 16); }

// size of an aux value of type t at p; -1: malformed / past the end of the record (as the record filter walks them)
__device__ __forceinline__ int64_t cv_aux_size(const uint8_t* p, const uint8_t* end, uint8_t t)
{
    switch (t) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    case 'Z': case 'H': {
        const uint8_t* q = p;
        while (q < end && *q) q++;
        return q < end ? (q - p) + 1 : -1;
    }
    case 'B': {
        if (p + 5 > end) return -1;
        const uint8_t sub = p[0];
        const int64_t n = cv_rd32(p + 1);
        const int64_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : -1;
        return es < 0 ? -1 : 5 + n * es;
    }
    default: return -1;
    }
}

// where a record's SEQ lies: behind its in-record CIGAR words, also when the operations come from a CG array (k_mismatch.hip)
struct CvSeq {
    uint64_t seq_off;
    uint32_t l_seq;
    uint32_t pad;
};

// One lane per record, what k_cover_parse, k_clip_parse, k_indel_parse and k_mm_parse share: bounds, core fields, the skip rule of
// gci_bam_cover_size, where the
// operations lie (own CIGAR or the first CG:B,I / B,i array behind a <l_seq>S<n>N placeholder) and how many chunks they make.
// contig >= 0: the record is counted, with or without operations.  A record out of bounds is reported and makes no chunk.
__device__ __forceinline__ CoverRec cv_parse_counted(const uint8_t* __restrict__ bam, uint64_t n_bytes, uint64_t off, uint32_t i, int has_seq,
                                                     const int32_t* __restrict__ ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq,
                                                     unsigned long long* __restrict__ status, uint32_t& chunks, CvSeq& sq)
{
    CoverRec r;
    r.ops_off = 0; r.n_ops = 0; r.contig = -1; r.pos = 0; r.pad = 0;
    sq.seq_off = 0; sq.l_seq = 0; sq.pad = 0;
    chunks = 0;
    if (off > n_bytes || n_bytes - off < 36) {
        cv_report(status, i, GCI_E_MALFORMED);
    } else {
        const uint8_t* p = bam + off;
        const int32_t block_size = (int32_t)cv_rd32(p), ref_id = (int32_t)cv_rd32(p + 4), pos = (int32_t)cv_rd32(p + 8);
        const uint32_t l_read_name = p[12];
        const int mapq = p[13];
        const uint32_t n_cigar = cv_rd16(p + 16), flag = cv_rd16(p + 18);
        const int32_t l_seq = (int32_t)cv_rd32(p + 20);
        const uint64_t rec_end = off + 4 + (uint64_t)(uint32_t)block_size;
        const uint64_t cig_off = off + 36 + l_read_name;
        const uint64_t aux_off = cig_off + 4ull * n_cigar + (has_seq ? (((uint64_t)(uint32_t)l_seq + 1) >> 1) + (uint64_t)(uint32_t)l_seq : 0ull);
        if (block_size < 32 || rec_end > n_bytes || l_seq < 0 || aux_off > rec_end) {
            cv_report(status, i, GCI_E_MALFORMED);
        } else if (!(flag & excl_flags) && mapq >= min_mapq && ref_id >= 0 && ref_id < n_ref && pos >= 0 && ref_sel[ref_id] >= 0) {
            r.contig = ref_sel[ref_id];                // (>= 0: the record is counted, with or without operations)
            r.pos = pos;
            r.ops_off = cig_off;
            r.n_ops = n_cigar;
            sq.seq_off = cig_off + 4ull * n_cigar;     // (with has_seq its (l_seq + 1) / 2 bytes end at or before aux_off <= rec_end)
            sq.l_seq = (uint32_t)l_seq;
            // a CIGAR of more than 65535 operations lies in CG:B,I (or B,i) behind the placeholder <l_seq>S<n>N: the rule of
            // formats/bam.py::decode_record and the record filter (the FIRST CG tag counts, bam_aux_get); without a usable one the
            // placeholder's own S and N stay
            if (n_cigar > 0) {
                const uint32_t op0 = cv_rd32(bam + cig_off);
                if ((op0 & 0xFu) == 4u && (op0 >> 4) == (uint32_t)l_seq) {
                    const uint8_t* end = bam + rec_end;
                    for (const uint8_t* q = bam + aux_off; q + 3 <= end;) {
                        const int64_t sz = cv_aux_size(q + 3, end, q[2]);
                        if (sz < 0 || q + 3 + sz > end) break;
                        if (q[0] == 'C' && q[1] == 'G') {
                            if (q[2] == 'B' && (q[3] == 'I' || q[3] == 'i')) {
                                const uint32_t cg_len = cv_rd32(q + 4);
                                if (cg_len >= n_cigar && cg_len < (1u << 29)) { r.ops_off = (uint64_t)(q + 8 - bam); r.n_ops = cg_len; }
                            }
                            break;
                        }
                        q += 3 + sz;
                    }
                }
            }
            chunks = (r.n_ops + CV_OPS - 1) / CV_OPS;    // (every operation word lies inside the record: aux_off <= rec_end, q + 3 + sz <= end)
        }
    }
    return r;
}

// The head of the per-record scratch of k_clips.hip, k_indels.hip and k_mismatch.hip, carved out of a DevBuf of rec_frame_bytes(n_rec)
// + whatever the tool appends at `tail` (8-byte aligned).
struct RecFrame {
    unsigned long long* status;
    unsigned long long* chunk0;          // n_rec + 1: exclusive scan of the chunk counts
    unsigned long long* cnt0;            // n_rec + 1: exclusive scan of `counted`
    CoverRec* recs;
    unsigned long long* blk;
    uint32_t* nch;
    uint32_t* counted;
    uint8_t* tail;
};

static inline size_t rec_frame_bytes(uint32_t n_rec)
{
    const size_t n = n_rec;
    return 16 + 2 * 8 * (n + 1) + sizeof(CoverRec) * n + 8 * (scan_blocks(n) + 2) + 2 * 4 * n;
}

static inline RecFrame rec_frame(const DevBuf& buf, uint32_t n_rec)
{
    const size_t n = n_rec;
    RecFrame s;
    uint8_t* p = (uint8_t*)buf.p;
    s.status = (unsigned long long*)p; p += 16;
    s.chunk0 = (unsigned long long*)p; p += 8 * (n + 1);
    s.cnt0 = (unsigned long long*)p; p += 8 * (n + 1);
    s.recs = (CoverRec*)p; p += sizeof(CoverRec) * n;
    s.blk = (unsigned long long*)p; p += 8 * (scan_blocks(n) + 2);
    s.nch = (uint32_t*)p; p += 4 * n;
    s.counted = (uint32_t*)p; p += 4 * n;
    s.tail = p;
    return s;
}

// what opens a *_size call over records: the scratch, and the status word at "nothing to report"
static inline int rec_frame_open(gci_ctx* ctx, DevBuf& buf, size_t tail_bytes, uint32_t n_rec, RecFrame& F)
{
    GCI_TRY(gci_ensure(ctx, buf, rec_frame_bytes(n_rec) + tail_bytes));
    F = rec_frame(buf, n_rec);
    HIPCHK(hipMemsetAsync(F.status, 0xFF, 8, ctx->stream));
    return GCI_OK;
}

// ... and what follows its parse: the chunks numbered, their count on the host (n_rec > 0)
static inline int rec_frame_chunks(gci_ctx* ctx, const RecFrame& F, uint32_t n_rec, unsigned long long& n_chunks)
{
    GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, F.nch, F.chunk0, F.blk, (int64_t)n_rec, true)));
    HIPCHK(hipMemcpyAsync(&n_chunks, F.chunk0 + n_rec, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return n_chunks > 0x7FFFFFFFull ? GCI_E_INVALID : GCI_OK;                // (2^42 operations in one call)
}

// the record of chunk c: the largest i with chunk0[i] <= c (records without chunks share their value with the record behind them)
__device__ __forceinline__ uint32_t cv_rec_of_chunk(const unsigned long long* __restrict__ chunk0, uint32_t n_rec, unsigned long long c)
{
    uint32_t lo = 0, hi = n_rec;                       // chunk0[lo] <= c < chunk0[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (chunk0[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

// the dword at byte offset o of the stream (bam + o is 4-byte aligned); bytes at or beyond n_bytes read as zero and are not touched
__device__ __forceinline__ uint32_t cv_dword(const uint8_t* __restrict__ bam, uint64_t n_bytes, uint64_t o)
{
    if (o + 4 <= n_bytes) return *reinterpret_cast<const uint32_t*>(bam + o);
    uint32_t w = 0;
    for (int k = 0; k < 4; k++) if (o + k < n_bytes) w |= (uint32_t)bam[o + k] << (8 * k);
    return w;
}

struct CvChunk {
    uint64_t first;                // byte offset of the aligned dword the chunk's first operation begins in
    uint32_t b;                    // ... and the byte phase of the operation words inside their dwords
    uint32_t n;                    // operations of the chunk
};

__device__ __forceinline__ CvChunk cv_chunk_of(const uint8_t* __restrict__ bam, const CoverRec& r, uint32_t ci)
{
    CvChunk c;
    const uint64_t at = r.ops_off + 4ull * (uint64_t)ci * CV_OPS;
    c.b = (uint32_t)(((uintptr_t)bam + at) & 3u);
    c.first = at - c.b;                                // (at >= 36)
    const uint64_t left = (uint64_t)r.n_ops - (uint64_t)ci * CV_OPS;
    c.n = (uint32_t)(left < CV_OPS ? left : CV_OPS);
    return c;
}

// operation word k = 64 * round + lane of the chunk (0 for a lane beyond the chunk's operations); every lane of the wave calls it
__device__ __forceinline__ uint32_t cv_op_word(const uint8_t* __restrict__ bam, uint64_t n_bytes, const CvChunk& c, uint32_t k, int lane)
{
    const bool valid = k < c.n;
    const uint64_t o = c.first + 4ull * k;
    const uint32_t w0 = valid ? cv_dword(bam, n_bytes, o) : 0u;
    if (c.b == 0) return w0;                           // (uniform)
    uint32_t w1 = (uint32_t)__shfl((int)w0, (lane + 1) & 63, 64);
    if (valid && (lane == 63 || k + 1 >= c.n)) w1 = cv_dword(bam, n_bytes, o + 4);     // nobody holds the dword that completes this word
    return __builtin_amdgcn_alignbyte(w1, w0, c.b);
}
