// k_clips.hip -- clip_sites.py: where alignments break off.  gci_bam_clip_size / _write turn every counted record of a BAM stream into
// at most two EVENTS -- its alignment begins (left) or ends (right) at a reference base with a clip of at least min_clip bases beyond
// it --, as intervals of one base for the depth build; gci_clip_sites_size / _write list the elements of the two built tracks that
// reach min_reads (include/gci_hip.h states both).
//
// The record side.  Input as for gci_bam_cover_size; the CIGAR work is k_reads.hip's: a CHUNK of at most GCI_COVER_CHUNK_OPS operations
// is a wave's, never a record's (gci_cover_chunks.hpp, gci_cigar_sums.hpp).
//   k_clip_parse    one lane per record: cv_parse_counted (bounds, core fields, the skip rule, where the operations lie -- own CIGAR
//                   or CG array -- and how many chunks they make), this file's rule for a placeholder without its array, and the at
//                   most four END operations, read here, directly: lead and trail
//   k_cigar_sums    one wave per chunk: the bases under M / = / X, D and N (R is their sum), codes 9 - 15; no atomics
//   k_clip_decide   one lane per record: adds its chunks' sums, decides the two events and where the right one lies
//   k_clip_write    one lane per record: its events to the rank an exclusive scan gave them -- left and right ranks packed into one
//                   64-bit word, so one scan serves both -- : record order, no atomics
// with the project's exclusive scan between them (chunks per record; events and counted records per record).
//
// The track side.  gci_site_tiles.hpp's lister over the left and right tracks: the hot ELEMENTS (HotEither, RUNS = false), counted by
// k_sites_count and written by k_sites_write; the depth track is read by ClipEmit only, where there is a site.
#include "gci_cigar_sums.hpp"
#include "gci_site_tiles.hpp"

struct ClipScratch : RecFrame {          // carved out of ctx->clip_rec: the frame, and behind it
    unsigned long long* ev;              // the events of a record: 1 = left, 1 << 32 = right
    unsigned long long* ev0;             // n_rec + 1: its exclusive scan -- left rank in the low word, right rank in the high one
    uint2* ends;                         // lead, trail
    int32_t* rsite;                      // where the right event lies
};

static inline size_t cl_tail_bytes(uint32_t n_rec) { return 8 * ((size_t)n_rec + 1) + (8 + 8 + 4) * (size_t)n_rec; }

static inline ClipScratch cl_scratch(const RecFrame& F, uint32_t n_rec)
{
    const size_t n = n_rec;
    ClipScratch s;
    static_cast<RecFrame&>(s) = F;
    uint8_t* p = F.tail;
    s.ev0 = (unsigned long long*)p; p += 8 * (n + 1);
    s.ev = (unsigned long long*)p; p += 8 * n;
    s.ends = (uint2*)p; p += 8 * n;
    s.rsite = (int32_t*)p;
    return s;
}

// ---- step 1: one lane per record ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool cl_is_clip(uint32_t w) { const uint32_t op = w & 0xFu; return op == 4u || op == 5u; }     // S, H

__global__ __launch_bounds__(BLOCK) void k_clip_parse(const uint8_t* __restrict__ bam, uint64_t n_bytes, const uint64_t* __restrict__ rec_off,
                                                      uint32_t n_rec, int has_seq, const int32_t* __restrict__ ref_sel, int32_t n_ref,
                                                      uint32_t excl_flags, int min_mapq, CoverRec* __restrict__ recs, uint32_t* __restrict__ nch,
                                                      uint2* __restrict__ ends, unsigned long long* __restrict__ status)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_rec) return;
    CvSeq sq;
    uint32_t chunks, lead = 0, trail = 0;
    CoverRec r = cv_parse_counted(bam, n_bytes, rec_off[i], i, has_seq, ref_sel, n_ref, excl_flags, min_mapq, status, chunks, sq);
    if (r.n_ops > 0) {
        const uint8_t* ops = bam + r.ops_off;          // (every operation word lies inside the record: cv_parse_counted)
        const uint32_t a0 = cv_rd32(ops), z0 = cv_rd32(ops + 4ull * (r.n_ops - 1));
        // This file's rule, NOT cover's and indels' (tests/clips_ref.py states it): <l_seq>S in front of the record's OWN operations
        // -- a placeholder without a usable CG array; with one the operations lie behind SEQ -- is no clip of l_seq bases.  The record
        // has no operations, R counts as 0 and it is not counted.
        if (r.ops_off + 4ull * r.n_ops == sq.seq_off && (a0 & 0xFu) == 4u && (a0 >> 4) == sq.l_seq) {
            r.n_ops = 0;
            chunks = 0;
        } else {
            if (cl_is_clip(a0)) {
                lead = a0 >> 4;
                if (r.n_ops > 1) { const uint32_t a1 = cv_rd32(ops + 4); if (cl_is_clip(a1)) lead += a1 >> 4; }
            }
            if (cl_is_clip(z0)) {
                trail = z0 >> 4;
                if (r.n_ops > 1) { const uint32_t z1 = cv_rd32(ops + 4ull * (r.n_ops - 2)); if (cl_is_clip(z1)) trail += z1 >> 4; }
            }
        }
    }
    recs[i] = r;
    nch[i] = chunks;
    ends[i] = make_uint2(lead, trail);
}

// ---- step 3: one lane per record ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_clip_decide(uint32_t n_rec, const CoverRec* __restrict__ recs, const unsigned long long* __restrict__ chunk0,
                                                       const CigarSums* __restrict__ sums, const uint2* __restrict__ ends,
                                                       const int64_t* __restrict__ contig_len, int32_t n_contigs, uint32_t min_clip,
                                                       unsigned long long* __restrict__ ev, uint32_t* __restrict__ counted,
                                                       int32_t* __restrict__ rsite, unsigned long long* __restrict__ status)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_rec) return;
    const CoverRec r = recs[i];
    unsigned long long e = 0;
    uint32_t c = 0;
    int32_t site = 0;
    if (r.contig >= 0) {
        unsigned long long R = 0, bad = 0;
        for (unsigned long long ch = chunk0[i], last = chunk0[i + 1]; ch < last; ch++) {
            const CigarSums s = sums[ch];
            R += s.M + s.D + s.N;                      // (every total is below 2^57)
            bad |= s.bad;
        }
        if (R > 0) {
            c = 1;
            if (bad) cv_report(status, i, GCI_E_MALFORMED);
            // a d_ref_sel beyond the layout: no site of that contig is inside it
            int64_t L = r.contig < n_contigs ? contig_len[r.contig] : 0;
            L = L < 0 ? 0 : L > 0x7FFFFFFFll ? 0x7FFFFFFFll : L;
            const uint2 lt = ends[i];
            const unsigned long long right = (unsigned long long)(uint32_t)r.pos + R - 1ull;      // 64 bits: pos + R may exceed int32
            if (lt.x >= min_clip && (int64_t)r.pos < L) e |= 1ull;
            if (lt.y >= min_clip && right < (unsigned long long)L) { e |= 1ull << 32; site = (int32_t)right; }
        }
    }
    ev[i] = e;
    counted[i] = c;
    rsite[i] = site;
}

// ---- step 4: one lane per record ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_clip_write(uint32_t n_rec, const CoverRec* __restrict__ recs, const unsigned long long* __restrict__ ev,
                                                      const unsigned long long* __restrict__ ev0, const int32_t* __restrict__ rsite,
                                                      unsigned long long n_left, unsigned long long total, gci_ivl* __restrict__ out)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_rec) return;
    const unsigned long long e = ev[i];
    if (!e) return;
    const unsigned long long rank = ev0[i];
    const CoverRec r = recs[i];
    gci_ivl v;
    v.contig = r.contig; v.pad = 0;
    if (e & 1ull) {
        const unsigned long long slot = rank & 0xFFFFFFFFull;
        v.start = v.end = r.pos;
        if (slot < n_left) out[slot] = v;
    }
    if (e >> 32) {
        const unsigned long long slot = n_left + (rank >> 32);
        v.start = v.end = rsite[i];
        if (slot < total) out[slot] = v;
    }
}

// ---- exports: the record side -----------------------------------------------------------------------------------------------------
extern "C" int gci_bam_clip_size(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                                 const int32_t* d_ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq, int min_clip, uint64_t* h_counts,
                                 uint64_t* d_status)
{
    if (!ctx || !h_counts || !d_status || n_ref < 0 || min_clip < 1 || (n_rec && (!d_stream || !d_rec_off || !d_ref_sel))) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    ctx->clip_valid = false;
    h_counts[0] = h_counts[1] = h_counts[2] = 0;
    RecFrame F;
    GCI_TRY(rec_frame_open(ctx, ctx->clip_rec, cl_tail_bytes(n_rec), n_rec, F));
    const ClipScratch R = cl_scratch(F, n_rec);
    unsigned long long n_chunks = 0, n_ev = 0, n_counted = 0;
    if (n_rec) {
        const uint32_t groups = (n_rec + BLOCK - 1) / BLOCK;
        hipLaunchKernelGGL(k_clip_parse, dim3(groups), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, d_rec_off, n_rec, has_seq, d_ref_sel, n_ref,
                           excl_flags, min_mapq, R.recs, R.nch, R.ends, R.status);
        LAUNCHCHK("k_clip_parse");
        GCI_TRY(rec_frame_chunks(ctx, R, n_rec, n_chunks));
        CigarSums* sums = nullptr;
        if (n_chunks) {
            GCI_TRY(gci_ensure(ctx, ctx->clip_chunk, sizeof(CigarSums) * (size_t)n_chunks));
            sums = (CigarSums*)ctx->clip_chunk.p;
            hipLaunchKernelGGL(k_cigar_sums, cigar_sums_grid(n_chunks), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, R.recs, R.chunk0, n_rec, n_chunks,
                               sums);
            LAUNCHCHK("k_cigar_sums");
        }
        hipLaunchKernelGGL(k_clip_decide, dim3(groups), dim3(BLOCK), 0, ctx->stream, n_rec, R.recs, R.chunk0, sums, R.ends, (const int64_t*)ctx->d_len.p,
                           ctx->n_contigs, (uint32_t)min_clip, R.ev, R.counted, R.rsite, R.status);
        LAUNCHCHK("k_clip_decide");
        GCI_TRY((device_exclusive_scan<unsigned long long, unsigned long long>(ctx, R.ev, R.ev0, R.blk, (int64_t)n_rec, true)));
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, R.counted, R.cnt0, R.blk, (int64_t)n_rec, true)));
        HIPCHK(hipMemcpyAsync(&n_ev, R.ev0 + n_rec, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(&n_counted, R.cnt0 + n_rec, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipMemcpyAsync(d_status, R.status, 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->clip_valid = true;
    ctx->clip_n_rec = n_rec; ctx->clip_n_left = n_ev & 0xFFFFFFFFull; ctx->clip_n_right = n_ev >> 32;
    ctx->clip_stream = d_stream; ctx->clip_off = d_rec_off;
    h_counts[0] = n_counted; h_counts[1] = ctx->clip_n_left; h_counts[2] = ctx->clip_n_right;
    return GCI_OK;
}

extern "C" int gci_bam_clip_write(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                                  gci_ivl* d_out, uint64_t cap, uint64_t* d_status)
{
    (void)n_bytes; (void)has_seq;                                            // (the parse of the size call has used them)
    if (!ctx || !d_status || (n_rec && (!d_stream || !d_rec_off))) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    // not the input gci_bam_clip_size measured last on this context
    if (!ctx->clip_valid || n_rec != ctx->clip_n_rec || d_stream != ctx->clip_stream || d_rec_off != ctx->clip_off) return GCI_E_INVALID;
    const unsigned long long total = ctx->clip_n_left + ctx->clip_n_right;
    if (total && !d_out) return GCI_E_INVALID;
    if (cap < total) return GCI_E_CAPACITY;
    const ClipScratch R = cl_scratch(rec_frame(ctx->clip_rec, n_rec), n_rec);
    if (n_rec && total) {
        hipLaunchKernelGGL(k_clip_write, dim3((n_rec + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, ctx->stream, n_rec, R.recs, R.ev, R.ev0, R.rsite,
                           (unsigned long long)ctx->clip_n_left, total, d_out);
        LAUNCHCHK("k_clip_write");
    }
    HIPCHK(hipMemcpyAsync(d_status, R.status, 8, hipMemcpyDeviceToDevice, ctx->stream));
    return GCI_OK;
}

// ---- the track side ---------------------------------------------------------------------------------------------------------------
struct ClipEmit {
    static constexpr int LISTER = 1;
    static constexpr bool RUNS = false;
    const int32_t* left;
    const int32_t* right;
    const int32_t* depth;
    gci_clip_site* out;
    __device__ __forceinline__ void operator()(unsigned long long slot, const SiteTile& x, int64_t q) const
    {
        gci_clip_site s;
        s.contig = x.contig; s.pos = (int32_t)(q - x.contig_off);
        s.left = left[q]; s.right = right[q]; s.depth = depth ? depth[q] : 0; s.pad = 0;
        out[slot] = s;
    }
};

static inline SiteMemo cl_site_ask(const int32_t* d_left, const int32_t* d_right, const int32_t* d_depth, int32_t min_reads, uint32_t n_windows)
{
    SiteMemo m;
    m.track[0] = d_left; m.track[1] = d_right; m.track[2] = d_depth; m.min_reads = min_reads; m.n_windows = n_windows;
    return m;
}

extern "C" int gci_clip_sites_size(gci_ctx* ctx, const int32_t* d_left, const int32_t* d_right, const int32_t* d_depth, int32_t min_reads,
                                   const gci_window* h_windows, uint32_t n_windows, uint64_t* h_n_sites)
{
    if (!ctx || !d_left || !d_right || !h_n_sites || min_reads < 1 || (n_windows && !h_windows)) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    if ((((uintptr_t)d_left) | ((uintptr_t)d_right) | ((uintptr_t)d_depth)) & 15u) return GCI_E_INVALID;      // whole tracks, as allocated
    return site_size<ClipEmit>(ctx, HotEither{d_left, d_right, min_reads}, cl_site_ask(d_left, d_right, d_depth, min_reads, n_windows),
                                       h_windows, h_n_sites, "k_sites_count (clips)");
}

extern "C" int gci_clip_sites_write(gci_ctx* ctx, const int32_t* d_left, const int32_t* d_right, const int32_t* d_depth, int32_t min_reads,
                                    const gci_window* h_windows, uint32_t n_windows, gci_clip_site* d_out, uint64_t cap)
{
    if (!ctx || !d_left || !d_right || min_reads < 1 || (n_windows && !h_windows)) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    return site_write(ctx, HotEither{d_left, d_right, min_reads}, cl_site_ask(d_left, d_right, d_depth, min_reads, n_windows),
                                        ClipEmit{d_left, d_right, d_depth, d_out}, d_out, cap, "k_sites_write (clips)");
}
