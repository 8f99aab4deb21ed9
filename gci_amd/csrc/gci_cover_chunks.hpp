// gci_cover_chunks.hpp -- the CIGAR of a BAM stream as CHUNKS of at most GCI_COVER_CHUNK_OPS operations, one wave each: what the
// kernels that walk whole CIGARs share (k_cover.hip: the covered bases; k_fate.hip: the base totals of the record filter's two
// quotients).  A lane per record says where the record's operations lie and how many chunks they make (CoverRec), an exclusive scan
// of the chunk counts numbers the chunks, and a wave finds its record (cv_rec_of_chunk), its piece of the operation array
// (cv_chunk_of) and its operation words, 64 a round (cv_op_word).
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
