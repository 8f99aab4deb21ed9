// k_cover.hip -- the reference bases the records of a BAM stream cover: `samtools depth -a` without its base-quality options, as
// intervals for the depth build (gci_bam_cover_size / _write), and the element-wise sum of two tracks (gci_track_add).
//
// gci_bam_cover_size_sel is the size call over the records of chosen classes only (gci_bam_fate's class bytes: k_fate.hip).
//
// Input as for gci_bam_filter: the inflated stream (or a heads stream) and the record offsets.  The unit of work is a CHUNK of at
// most GCI_COVER_CHUNK_OPS CIGAR operations, never a record: an ONT record holds 10^3 - 10^5 operations.  Three steps:
//   k_cover_parse   one lane per record: cv_parse_counted -- bounds, the skip decision (flag, MAPQ, refID, pos, contig), where the
//                   operations lie (the record's own CIGAR, or the CG:B,I array behind a <l_seq>S<n>N placeholder) and how many
//                   chunks they make --, then the class mask
//   k_cover_count   one wave per chunk: the chunk's reference length, its intervals, operation codes 9 - 15
//   k_cover_write   one wave per chunk: the same walk with positions (reference lengths scanned across the lanes, 64 operations a
//                   round), one interval per maximal run of covering operations inside the chunk
// with exclusive scans between them (chunks per record; reference length and intervals per chunk).  An operation covers when it is
// M, = or X (D too with count_del) and longer than zero; D (without count_del) and N of non-zero length end a run; I, S, H, P,
// zero-length operations and the codes 9 - 15 leave a run as it is.
//
// The chunk helpers (where a chunk lies, its operation words at any byte phase) are gci_cover_chunks.hpp, shared with k_fate.hip.
#include "gci_cover_chunks.hpp"

struct CoverRecScratch {           // carved out of ctx->cover_rec
    unsigned long long* status;
    unsigned long long* chunk0;    // n_rec + 1: exclusive scan of the chunk counts
    CoverRec* recs;
    unsigned long long* blk;
    uint32_t* nch;
};

struct CoverChunkScratch {         // carved out of ctx->cover_chunk
    unsigned long long* ref;       // reference length of a chunk
    unsigned long long* ref0;      // n_chunks + 1: its exclusive scan
    unsigned long long* ivl0;      // n_chunks + 1: exclusive scan of the interval counts
    unsigned long long* blk;
    uint32_t* cnt;
};

static inline size_t cv_rec_bytes(uint32_t n_rec)
{
    return 16 + 8 * ((size_t)n_rec + 1) + sizeof(CoverRec) * (size_t)n_rec + 8 * (scan_blocks(n_rec) + 2) + 4 * (size_t)n_rec;
}

static inline CoverRecScratch cv_rec_scratch(gci_ctx* ctx, uint32_t n_rec)
{
    CoverRecScratch s;
    uint8_t* p = (uint8_t*)ctx->cover_rec.p;
    s.status = (unsigned long long*)p; p += 16;
    s.chunk0 = (unsigned long long*)p; p += 8 * ((size_t)n_rec + 1);
    s.recs = (CoverRec*)p; p += sizeof(CoverRec) * (size_t)n_rec;
    s.blk = (unsigned long long*)p; p += 8 * (scan_blocks(n_rec) + 2);
    s.nch = (uint32_t*)p;
    return s;
}

static inline size_t cv_chunk_bytes(uint64_t n)
{
    return 8 * (size_t)n + 2 * 8 * ((size_t)n + 1) + 8 * (scan_blocks(n) + 2) + 4 * (size_t)n;
}

static inline CoverChunkScratch cv_chunk_scratch(gci_ctx* ctx, uint64_t n)
{
    CoverChunkScratch s;
    uint8_t* p = (uint8_t*)ctx->cover_chunk.p;
    s.ref = (unsigned long long*)p; p += 8 * (size_t)n;
    s.ref0 = (unsigned long long*)p; p += 8 * ((size_t)n + 1);
    s.ivl0 = (unsigned long long*)p; p += 8 * ((size_t)n + 1);
    s.blk = (unsigned long long*)p; p += 8 * (scan_blocks(n) + 2);
    s.cnt = (uint32_t*)p;
    return s;
}

// ---- step 1: one lane per record ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_cover_parse(const uint8_t* __restrict__ bam, uint64_t n_bytes, const uint64_t* __restrict__ rec_off,
                                                       uint32_t n_rec, int has_seq, const int32_t* __restrict__ ref_sel, int32_t n_ref,
                                                       uint32_t excl_flags, int min_mapq, const uint8_t* __restrict__ cls, uint32_t class_mask,
                                                       CoverRec* __restrict__ recs, uint32_t* __restrict__ nch,
                                                       unsigned long long* __restrict__ status)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_rec) return;
    CvSeq q;
    uint32_t chunks;
    CoverRec r = cv_parse_counted(bam, n_bytes, rec_off[i], i, has_seq, ref_sel, n_ref, excl_flags, min_mapq, status, chunks, q);
    // gci_bam_cover_size_sel: only the classes of the mask -- a record of another class is a skipped one (what it has to report as
    // malformed it has reported)
    if (r.contig >= 0 && cls && !(cls[i] < 32u && ((class_mask >> cls[i]) & 1u))) {
        r.ops_off = 0; r.n_ops = 0; r.contig = -1; r.pos = 0;
        chunks = 0;
    }
    recs[i] = r;
    nch[i] = chunks;
}

// ---- the walk of one chunk, shared by the two passes ------------------------------------------------------------------------------

struct CvClass { bool cov, brk, bad; uint32_t ref_len; };

__device__ __forceinline__ CvClass cv_classify(uint32_t v, bool valid, int count_del)
{
    CvClass x;
    const uint32_t op = v & 0xFu, len = v >> 4;
    const bool consumes = valid && ((0x18Du >> op) & 1u);                       // M D N = X
    const bool covering = ((0x181u >> op) & 1u) || (count_del && op == 2u);      // M = X (, D)
    x.bad = valid && op >= 9u;
    x.ref_len = consumes ? len : 0u;
    x.cov = consumes && covering && len > 0u;
    x.brk = consumes && !covering && len > 0u;
    return x;
}

__device__ __forceinline__ int cv_top(unsigned long long m) { return 63 - __builtin_clzll(m); }     // m != 0
// the lanes above lane t (t = 63: none)
__device__ __forceinline__ unsigned long long cv_above(int t) { return t >= 63 ? 0ull : ~((2ull << t) - 1ull); }

// ---- step 2: one wave per chunk ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_cover_count(const uint8_t* __restrict__ bam, uint64_t n_bytes, const CoverRec* __restrict__ recs,
                                                       const unsigned long long* __restrict__ chunk0, uint32_t n_rec, unsigned long long n_chunks,
                                                       int count_del, unsigned long long* __restrict__ chunk_ref, uint32_t* __restrict__ chunk_cnt,
                                                       unsigned long long* __restrict__ status)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long ch = (unsigned long long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (ch >= n_chunks) return;                        // (the whole wave)
    const uint32_t rec = cv_rec_of_chunk(chunk0, n_rec, ch);
    const CoverRec r = recs[rec];
    const CvChunk c = cv_chunk_of(bam, r, (uint32_t)(ch - chunk0[rec]));
    unsigned long long ref = 0;
    uint32_t cnt = 0;
    bool open = false, bad = false;
    for (uint32_t k0 = 0; k0 < c.n; k0 += 64) {
        const uint32_t k = k0 + lane;
        const CvClass x = cv_classify(cv_op_word(bam, n_bytes, c, k, lane), k < c.n, count_del);
        bad |= x.bad;
        ref += x.ref_len;
        const unsigned long long covm = __ballot(x.cov), brkm = __ballot(x.brk), all = covm | brkm;
        const unsigned long long below = all & lanes_below(lane);
        const bool prev_cov = below ? ((covm >> cv_top(below)) & 1ull) != 0 : open;
        cnt += (uint32_t)__builtin_popcountll(__ballot(x.brk && prev_cov));       // a run ends where D / N follows a covering operation
        if (all) open = ((covm >> cv_top(all)) & 1ull) != 0;
    }
    cnt += open ? 1u : 0u;                                                        // ... and at the end of the chunk
    ref = wave_sum<unsigned long long>(ref);
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0) {
        chunk_ref[ch] = ref;
        chunk_cnt[ch] = cnt;
        if (any_bad) cv_report(status, rec, GCI_E_MALFORMED);
    }
}

// ---- step 3: one wave per chunk ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ gci_ivl cv_ivl(int32_t contig, unsigned long long a, unsigned long long b_excl, unsigned long long lim)
{
    gci_ivl v;                                         // [a, b_excl) with a < b_excl, clamped to the contig: the build's slice drops the rest
    v.contig = contig;
    v.start = (int32_t)(a < lim ? a : lim);
    v.end = (int32_t)(b_excl - 1 < lim ? b_excl - 1 : lim);
    v.pad = 0;
    return v;
}

__global__ __launch_bounds__(BLOCK) void k_cover_write(const uint8_t* __restrict__ bam, uint64_t n_bytes, const CoverRec* __restrict__ recs,
                                                       const unsigned long long* __restrict__ chunk0, uint32_t n_rec, unsigned long long n_chunks,
                                                       int count_del, const unsigned long long* __restrict__ chunk_ref0,
                                                       const unsigned long long* __restrict__ chunk_ivl0, const int64_t* __restrict__ contig_len,
                                                       int32_t n_contigs, gci_ivl* __restrict__ out, unsigned long long cap)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long ch = (unsigned long long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (ch >= n_chunks) return;
    const uint32_t rec = cv_rec_of_chunk(chunk0, n_rec, ch);
    const CoverRec r = recs[rec];
    const unsigned long long ch_first = chunk0[rec];
    const CvChunk c = cv_chunk_of(bam, r, (uint32_t)(ch - ch_first));
    // positions in 64 bits: a forged record's reference lengths may sum past 2^31; clamped to the contig before they become int32
    unsigned long long at = (unsigned long long)(uint32_t)r.pos + (chunk_ref0[ch] - chunk_ref0[ch_first]);
    const int64_t L = r.contig < n_contigs ? contig_len[r.contig] : 0;       // (a d_ref_sel beyond the layout: the build drops the contig)
    const unsigned long long lim = (unsigned long long)(L < 0x7FFFFFFEll ? (L < 0 ? 0 : L) : 0x7FFFFFFEll);
    unsigned long long o = chunk_ivl0[ch];             // where the chunk's next interval goes
    bool open = false;
    unsigned long long open_start = 0;
    for (uint32_t k0 = 0; k0 < c.n; k0 += 64) {
        const uint32_t k = k0 + lane;
        const CvClass x = cv_classify(cv_op_word(bam, n_bytes, c, k, lane), k < c.n, count_del);
        const unsigned long long inc = wave_inclusive<unsigned long long>((unsigned long long)x.ref_len, lane);
        const unsigned long long mine = at + inc - x.ref_len;                    // where this lane's operation begins on the reference
        const unsigned long long covm = __ballot(x.cov), brkm = __ballot(x.brk), all = covm | brkm;
        const unsigned long long lowm = lanes_below(lane), below = all & lowm;
        const bool prev_cov = below ? ((covm >> cv_top(below)) & 1ull) != 0 : open;
        const bool close = x.brk && prev_cov;
        const unsigned long long closem = __ballot(close);
        // the run this lane closes began behind the last D / N in front of it -- or, with none in this round, where the open run did
        const unsigned long long brk_below = brkm & lowm;
        const unsigned long long cand = covm & lowm & (brk_below ? cv_above(cv_top(brk_below)) : ~0ull);
        const unsigned long long from_lane = __shfl(mine, cand ? __builtin_ctzll(cand) : 0, 64);
        if (close) {
            const unsigned long long a = (!brk_below && open) ? open_start : from_lane;
            const unsigned long long slot = o + (unsigned long long)__builtin_popcountll(closem & lowm);
            if (slot < cap) out[slot] = cv_ivl(r.contig, a, mine, lim);
        }
        o += (unsigned long long)__builtin_popcountll(closem);
        // what the round leaves open
        if (all) {
            if ((covm >> cv_top(all)) & 1ull) {
                const unsigned long long tail = covm & (brkm ? cv_above(cv_top(brkm)) : ~0ull);
                const unsigned long long s = __shfl(mine, __builtin_ctzll(tail), 64);
                if (brkm || !open) open_start = s;
                open = true;
            } else open = false;
        }
        at += __shfl(inc, 63, 64);
    }
    if (open && lane == 0 && o < cap) out[o] = cv_ivl(r.contig, open_start, at, lim);
}

// ---- exports ----------------------------------------------------------------------------------------------------------------------
extern "C" int gci_bam_cover_size_sel(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                                      const int32_t* d_ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq, int count_del,
                                      const uint8_t* d_class, uint32_t class_mask, uint64_t* h_n_ivl, uint64_t* d_status)
{
    if (!ctx || !h_n_ivl || !d_status || n_ref < 0 || (n_rec && (!d_stream || !d_rec_off || !d_ref_sel))) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    ctx->cover_valid = false;
    *h_n_ivl = 0;
    GCI_TRY(gci_ensure(ctx, ctx->cover_rec, cv_rec_bytes(n_rec)));
    const CoverRecScratch R = cv_rec_scratch(ctx, n_rec);
    HIPCHK(hipMemsetAsync(R.status, 0xFF, 8, ctx->stream));
    unsigned long long n_chunks = 0, n_ivl = 0;
    if (n_rec) {
        hipLaunchKernelGGL(k_cover_parse, dim3((n_rec + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, d_rec_off, n_rec, has_seq,
                           d_ref_sel, n_ref, excl_flags, min_mapq, d_class, class_mask, R.recs, R.nch, R.status);
        LAUNCHCHK("k_cover_parse");
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, R.nch, R.chunk0, R.blk, (int64_t)n_rec, true)));
        HIPCHK(hipMemcpyAsync(&n_chunks, R.chunk0 + n_rec, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    if (n_chunks > 0x7FFFFFFFull) return GCI_E_INVALID;                      // (2^42 operations in one call)
    if (n_chunks) {
        GCI_TRY(gci_ensure(ctx, ctx->cover_chunk, cv_chunk_bytes(n_chunks)));
        const CoverChunkScratch C = cv_chunk_scratch(ctx, n_chunks);
        hipLaunchKernelGGL(k_cover_count, wave_grid(n_chunks), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes,
                           R.recs, R.chunk0, n_rec, n_chunks, count_del, C.ref, C.cnt, R.status);
        LAUNCHCHK("k_cover_count");
        GCI_TRY((device_exclusive_scan<unsigned long long, unsigned long long>(ctx, C.ref, C.ref0, C.blk, (int64_t)n_chunks, true)));
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, C.cnt, C.ivl0, C.blk, (int64_t)n_chunks, true)));
        HIPCHK(hipMemcpyAsync(&n_ivl, C.ivl0 + n_chunks, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipMemcpyAsync(d_status, R.status, 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->cover_valid = true;
    ctx->cover_n_rec = n_rec; ctx->cover_n_chunks = n_chunks; ctx->cover_n_ivl = n_ivl; ctx->cover_count_del = count_del;
    ctx->cover_stream = d_stream; ctx->cover_off = d_rec_off;
    *h_n_ivl = n_ivl;
    return GCI_OK;
}

extern "C" int gci_bam_cover_size(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                                  const int32_t* d_ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq, int count_del, uint64_t* h_n_ivl,
                                  uint64_t* d_status)
{
    return gci_bam_cover_size_sel(ctx, d_stream, n_bytes, d_rec_off, n_rec, has_seq, d_ref_sel, n_ref, excl_flags, min_mapq, count_del, nullptr, 0,
                                  h_n_ivl, d_status);
}

extern "C" int gci_bam_cover_write(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                                   gci_ivl* d_out, uint64_t cap, uint64_t* d_status)
{
    (void)has_seq;                                                           // (the parse of the size call has used it)
    if (!ctx || !d_status || (n_rec && (!d_stream || !d_rec_off))) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    // not the input gci_bam_cover_size measured last on this context
    if (!ctx->cover_valid || n_rec != ctx->cover_n_rec || d_stream != ctx->cover_stream || d_rec_off != ctx->cover_off) return GCI_E_INVALID;
    if (ctx->cover_n_ivl && !d_out) return GCI_E_INVALID;
    if (cap < ctx->cover_n_ivl) return GCI_E_CAPACITY;
    const CoverRecScratch R = cv_rec_scratch(ctx, n_rec);
    const unsigned long long n_chunks = ctx->cover_n_chunks;
    if (n_chunks && ctx->cover_n_ivl) {
        const CoverChunkScratch C = cv_chunk_scratch(ctx, n_chunks);
        hipLaunchKernelGGL(k_cover_write, wave_grid(n_chunks), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes,
                           R.recs, R.chunk0, n_rec, n_chunks, ctx->cover_count_del, C.ref0, C.ivl0, (const int64_t*)ctx->d_len.p, ctx->n_contigs, d_out,
                           (unsigned long long)ctx->cover_n_ivl);
        LAUNCHCHK("k_cover_write");
    }
    HIPCHK(hipMemcpyAsync(d_status, R.status, 8, hipMemcpyDeviceToDevice, ctx->stream));
    return GCI_OK;
}

// ---- acc += add over the layout ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_track_add(int4* __restrict__ acc, const int4* __restrict__ add, int64_t n4)
{
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n4; i += (int64_t)gridDim.x * BLOCK) {
        int4 x = acc[i];
        const int4 y = add[i];
        x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
        acc[i] = x;
    }
}

extern "C" int gci_track_add(gci_ctx* ctx, int32_t* d_acc, const int32_t* d_add)
{
    if (!ctx || !d_acc || !d_add) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    if ((((uintptr_t)d_acc) | ((uintptr_t)d_add)) & 15u) return GCI_E_INVALID;      // whole tracks, as allocated: 16-byte vector accesses
    ctx->build_runs_track = nullptr; ctx->build_runs_armed = false;          // (a track is written: the build's run lists are stale)
    const int64_t n4 = ctx->total / 4;
    if (n4 == 0) return GCI_OK;
    const int64_t want = (n4 + BLOCK * 4 - 1) / (BLOCK * 4);
    const uint32_t grid = (uint32_t)(want < 1 ? 1 : want > 16384 ? 16384 : want);
    hipLaunchKernelGGL(k_track_add, dim3(grid), dim3(BLOCK), 0, ctx->stream, (int4*)d_acc, (const int4*)d_add, n4);
    LAUNCHCHK("k_track_add");
    return GCI_OK;
}
