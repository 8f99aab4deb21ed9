// k_clips.hip -- clip_sites.py: where alignments break off.  gci_bam_clip_size / _write turn every counted record of a BAM stream into
// at most two EVENTS -- its alignment begins (left) or ends (right) at a reference base with a clip of at least min_clip bases beyond
// it --, as intervals of one base for the depth build; gci_clip_sites_size / _write list the elements of the two built tracks that
// reach min_reads (include/gci_hip.h states both).
//
// The record side.  Input as for gci_bam_cover_size; the CIGAR work is k_reads.hip's: a CHUNK of at most GCI_COVER_CHUNK_OPS operations
// is a wave's, never a record's (gci_cover_chunks.hpp, gci_cigar_sums.hpp).
//   k_clip_parse    one lane per record: bounds, core fields, the skip rule, where the operations lie (own CIGAR or CG array) and how
//                   many chunks they make; the at most four END operations are read here, directly: lead and trail
//   k_cigar_sums    one wave per chunk: the bases under M / = / X, D and N (R is their sum), codes 9 - 15; no atomics
//   k_clip_decide   one lane per record: adds its chunks' sums, decides the two events and where the right one lies
//   k_clip_write    one lane per record: its events to the rank an exclusive scan gave them -- left and right ranks packed into one
//                   64-bit word, so one scan serves both -- : record order, no atomics
// with the project's exclusive scan between them (chunks per record; events and counted records per record).
//
// The track side.  K8's windows and tiling (gci_set_windows, 4096-element tiles, int4 loads, elements outside [begin, end) or in the
// padding behind a contig masked off).
//   k_clip_sites_count   one workgroup per window tile: the left and right tracks, 16 bytes a lane, one count per tile
//   k_clip_sites_write   one workgroup per window tile, gone at once when the tile's count is 0 (nearly every tile of a genome): a
//                        thread takes 16 consecutive elements, a workgroup scan ranks them, the depth track is read here only
#include "gci_cigar_sums.hpp"

struct ClipScratch {                     // carved out of ctx->clip_rec
    unsigned long long* status;
    unsigned long long* chunk0;          // n_rec + 1: exclusive scan of the chunk counts
    unsigned long long* ev;              // the events of a record: 1 = left, 1 << 32 = right
    unsigned long long* ev0;             // n_rec + 1: its exclusive scan -- left rank in the low word, right rank in the high one
    unsigned long long* cnt0;            // n_rec + 1: exclusive scan of `counted`
    CoverRec* recs;
    unsigned long long* blk;
    uint2* ends;                         // lead, trail
    int32_t* rsite;                      // where the right event lies
    uint32_t* nch;
    uint32_t* counted;
};

static inline size_t cl_blocks(uint64_t n) { return (size_t)((n + TILE - 1) / TILE); }

static inline size_t cl_rec_bytes(uint32_t n_rec)
{
    const size_t n = n_rec;
    return 16 + 3 * 8 * (n + 1) + 8 * n + sizeof(CoverRec) * n + 8 * (cl_blocks(n) + 2) + 8 * n + 3 * 4 * n;
}

static inline ClipScratch cl_scratch(gci_ctx* ctx, uint32_t n_rec)
{
    const size_t n = n_rec;
    ClipScratch s;
    uint8_t* p = (uint8_t*)ctx->clip_rec.p;
    s.status = (unsigned long long*)p; p += 16;
    s.chunk0 = (unsigned long long*)p; p += 8 * (n + 1);
    s.ev0 = (unsigned long long*)p; p += 8 * (n + 1);
    s.cnt0 = (unsigned long long*)p; p += 8 * (n + 1);
    s.ev = (unsigned long long*)p; p += 8 * n;
    s.recs = (CoverRec*)p; p += sizeof(CoverRec) * n;
    s.blk = (unsigned long long*)p; p += 8 * (cl_blocks(n) + 2);
    s.ends = (uint2*)p; p += 8 * n;
    s.rsite = (int32_t*)p; p += 4 * n;
    s.nch = (uint32_t*)p; p += 4 * n;
    s.counted = (uint32_t*)p;
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
    CoverRec r;
    r.ops_off = 0; r.n_ops = 0; r.contig = -1; r.pos = 0; r.pad = 0;
    uint32_t chunks = 0, lead = 0, trail = 0;
    const uint64_t off = rec_off[i];
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
        } else if (!(flag & excl_flags) && mapq >= min_mapq && ref_id >= 0 && ref_id < n_ref && pos >= 0 && ref_sel[ref_id] >= 0 && n_cigar > 0) {
            uint64_t ops_off = cig_off;
            uint32_t n_ops = n_cigar;
            // <l_seq>S in front: the operations are the first CG:B,I (or B,i) array, as k_cover_parse walks to it -- or, without a usable
            // one, nothing: R counts as 0 and the record is skipped
            const uint32_t op0 = cv_rd32(bam + cig_off);
            if ((op0 & 0xFu) == 4u && (op0 >> 4) == (uint32_t)l_seq) {
                n_ops = 0;
                const uint8_t* end = bam + rec_end;
                for (const uint8_t* q = bam + aux_off; q + 3 <= end;) {
                    const int64_t sz = cv_aux_size(q + 3, end, q[2]);
                    if (sz < 0 || q + 3 + sz > end) break;
                    if (q[0] == 'C' && q[1] == 'G') {
                        if (q[2] == 'B' && (q[3] == 'I' || q[3] == 'i')) {
                            const uint32_t cg_len = cv_rd32(q + 4);
                            if (cg_len >= n_cigar && cg_len < (1u << 29)) { ops_off = (uint64_t)(q + 8 - bam); n_ops = cg_len; }
                        }
                        break;
                    }
                    q += 3 + sz;
                }
            }
            if (n_ops > 0) {                           // (every operation word lies inside the record: aux_off <= rec_end, q + 3 + sz <= end)
                r.contig = ref_sel[ref_id]; r.pos = pos; r.ops_off = ops_off; r.n_ops = n_ops;
                chunks = (n_ops + CV_OPS - 1) / CV_OPS;
                const uint8_t* ops = bam + ops_off;
                const uint32_t a0 = cv_rd32(ops), z0 = cv_rd32(ops + 4ull * (n_ops - 1));
                if (cl_is_clip(a0)) {
                    lead = a0 >> 4;
                    if (n_ops > 1) { const uint32_t a1 = cv_rd32(ops + 4); if (cl_is_clip(a1)) lead += a1 >> 4; }
                }
                if (cl_is_clip(z0)) {
                    trail = z0 >> 4;
                    if (n_ops > 1) { const uint32_t z1 = cv_rd32(ops + 4ull * (n_ops - 2)); if (cl_is_clip(z1)) trail += z1 >> 4; }
                }
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
    GCI_TRY(gci_ensure(ctx, ctx->clip_rec, cl_rec_bytes(n_rec)));
    const ClipScratch R = cl_scratch(ctx, n_rec);
    HIPCHK(hipMemsetAsync(R.status, 0xFF, 8, ctx->stream));
    unsigned long long n_chunks = 0, n_ev = 0, n_counted = 0;
    if (n_rec) {
        const uint32_t groups = (n_rec + BLOCK - 1) / BLOCK;
        hipLaunchKernelGGL(k_clip_parse, dim3(groups), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, d_rec_off, n_rec, has_seq, d_ref_sel, n_ref,
                           excl_flags, min_mapq, R.recs, R.nch, R.ends, R.status);
        LAUNCHCHK("k_clip_parse");
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, R.nch, R.chunk0, R.blk, (int64_t)n_rec, true)));
        HIPCHK(hipMemcpyAsync(&n_chunks, R.chunk0 + n_rec, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (n_chunks > 0x7FFFFFFFull) return GCI_E_INVALID;                  // (2^42 operations in one call)
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
    const ClipScratch R = cl_scratch(ctx, n_rec);
    if (n_rec && total) {
        hipLaunchKernelGGL(k_clip_write, dim3((n_rec + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, ctx->stream, n_rec, R.recs, R.ev, R.ev0, R.rsite,
                           (unsigned long long)ctx->clip_n_left, total, d_out);
        LAUNCHCHK("k_clip_write");
    }
    HIPCHK(hipMemcpyAsync(d_status, R.status, 8, hipMemcpyDeviceToDevice, ctx->stream));
    return GCI_OK;
}

// ---- the track side ---------------------------------------------------------------------------------------------------------------
struct ClipTile {
    int64_t p0;                          // the tile's first element (a multiple of TILE)
    int64_t lo, hi;                      // the elements of it that are inside the window AND inside their contig
    int64_t contig_off;
    int32_t contig;
};

__device__ __forceinline__ ClipTile clip_tile_of(const gci_window* __restrict__ win, const int64_t* __restrict__ win_tile_first, int32_t n_win,
                                                 int64_t wt, const int64_t* __restrict__ off, const int64_t* __restrict__ len,
                                                 const int64_t* __restrict__ tile_first, int32_t n_contigs)
{
    ClipTile x;
    const int32_t w = contig_of_tile(win_tile_first, n_win, wt);
    const gci_window W = win[w];
    x.p0 = (W.begin / TILE + (wt - win_tile_first[w])) * TILE;
    x.contig = contig_of_tile(tile_first, n_contigs, x.p0 / TILE);
    x.contig_off = off[x.contig];
    x.lo = max(x.p0, W.begin);
    x.hi = min(min(x.p0 + TILE, W.end), x.contig_off + len[x.contig]);
    return x;
}

__global__ __launch_bounds__(BLOCK) void k_clip_sites_count(const int32_t* __restrict__ left, const int32_t* __restrict__ right,
                                                            const gci_window* __restrict__ win, const int64_t* __restrict__ win_tile_first,
                                                            int32_t n_win, const int64_t* __restrict__ off, const int64_t* __restrict__ len,
                                                            const int64_t* __restrict__ tile_first, int32_t n_contigs, int32_t min_reads,
                                                            uint32_t* __restrict__ tile_cnt)
{
    __shared__ uint32_t part[BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const ClipTile x = clip_tile_of(win, win_tile_first, n_win, blockIdx.x, off, len, tile_first, n_contigs);
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t p = x.p0 + (int64_t)(j * BLOCK + t) * 4;
        const int4 a = *reinterpret_cast<const int4*>(left + p), b = *reinterpret_cast<const int4*>(right + p);
        const int32_t l[4] = {a.x, a.y, a.z, a.w}, r[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int k = 0; k < 4; k++) n += (p + k >= x.lo && p + k < x.hi && (l[k] >= min_reads || r[k] >= min_reads)) ? 1u : 0u;
    }
    n = wave_sum<uint32_t>(n);
    if (lane == 0) part[wave] = n;
    __syncthreads();
    if (t == 0) {
        uint32_t all = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; w++) all += part[w];
        tile_cnt[blockIdx.x] = all;
    }
}

__global__ __launch_bounds__(BLOCK) void k_clip_sites_write(const int32_t* __restrict__ left, const int32_t* __restrict__ right,
                                                            const int32_t* __restrict__ depth, const gci_window* __restrict__ win,
                                                            const int64_t* __restrict__ win_tile_first, int32_t n_win,
                                                            const int64_t* __restrict__ off, const int64_t* __restrict__ len,
                                                            const int64_t* __restrict__ tile_first, int32_t n_contigs, int32_t min_reads,
                                                            const uint32_t* __restrict__ tile_cnt, const unsigned long long* __restrict__ tile_off,
                                                            gci_clip_site* __restrict__ out, unsigned long long total)
{
    __shared__ uint32_t wtot[BLOCK / 64];
    if (tile_cnt[blockIdx.x] == 0) return;             // (the whole workgroup)
    const int t = threadIdx.x;
    const ClipTile x = clip_tile_of(win, win_tile_first, n_win, blockIdx.x, off, len, tile_first, n_contigs);
    const int64_t p = x.p0 + (int64_t)t * 16;          // a thread's 16 consecutive elements: ascending order is thread order
    uint32_t flags = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int4 a = *reinterpret_cast<const int4*>(left + p + 4 * j), b = *reinterpret_cast<const int4*>(right + p + 4 * j);
        const int32_t l[4] = {a.x, a.y, a.z, a.w}, r[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t q = p + 4 * j + k;
            flags |= (q >= x.lo && q < x.hi && (l[k] >= min_reads || r[k] >= min_reads)) ? (1u << (4 * j + k)) : 0u;
        }
    }
    uint32_t all;
    const uint32_t pre = block_exclusive<uint32_t, BLOCK / 64>((uint32_t)__builtin_popcount(flags), wtot, all);
    unsigned long long slot = tile_off[blockIdx.x] + pre;
    while (flags) {                                    // (few: a genome has thousands of sites)
        const int k = __builtin_ctz(flags);
        flags &= flags - 1u;
        gci_clip_site s;
        s.contig = x.contig; s.pos = (int32_t)(p + k - x.contig_off);
        s.left = left[p + k]; s.right = right[p + k]; s.depth = depth ? depth[p + k] : 0; s.pad = 0;
        if (slot < total) out[slot] = s;
        slot++;
    }
}

struct ClipTileScratch { uint32_t* cnt; unsigned long long* off; unsigned long long* blk; };

static inline ClipTileScratch cl_tile_scratch(gci_ctx* ctx, int64_t tiles)
{
    ClipTileScratch s;
    uint8_t* p = (uint8_t*)ctx->clip_tiles.p;
    s.off = (unsigned long long*)p; p += 8 * ((size_t)tiles + 1);
    s.blk = (unsigned long long*)p; p += 8 * (cl_blocks((uint64_t)tiles) + 2);
    s.cnt = (uint32_t*)p;
    return s;
}

extern "C" int gci_clip_sites_size(gci_ctx* ctx, const int32_t* d_left, const int32_t* d_right, const int32_t* d_depth, int32_t min_reads,
                                   const gci_window* h_windows, uint32_t n_windows, uint64_t* h_n_sites)
{
    if (!ctx || !d_left || !d_right || !h_n_sites || min_reads < 1 || (n_windows && !h_windows)) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    if ((((uintptr_t)d_left) | ((uintptr_t)d_right) | ((uintptr_t)d_depth)) & 15u) return GCI_E_INVALID;      // whole tracks, as allocated
    if (n_windows >= (1u << 31)) return GCI_E_INVALID;
    std::vector<gci_window> ws;
    if (!gci_site_windows(ctx, h_windows, n_windows, ws)) return GCI_E_INVALID;
    ctx->clip_sites_epoch = 0;
    *h_n_sites = 0;
    GCI_TRY(gci_set_windows(ctx, ws.data(), (uint32_t)ws.size()));
    ctx->win_flank = INT32_MIN;
    const int64_t tiles = ctx->win_tiles;
    if (tiles > 0x7FFFFFFFll) return GCI_E_INVALID;
    unsigned long long total = 0;
    if (tiles) {
        GCI_TRY(gci_ensure(ctx, ctx->clip_tiles, 8 * ((size_t)tiles + 1) + 8 * (cl_blocks((uint64_t)tiles) + 2) + 4 * (size_t)tiles));
        const ClipTileScratch T = cl_tile_scratch(ctx, tiles);
        hipLaunchKernelGGL(k_clip_sites_count, dim3((uint32_t)tiles), dim3(BLOCK), 0, ctx->stream, d_left, d_right, (const gci_window*)ctx->win.p,
                           (const int64_t*)ctx->win_tile_first.p, (int32_t)ctx->win_n, (const int64_t*)ctx->d_off.p, (const int64_t*)ctx->d_len.p,
                           (const int64_t*)ctx->d_tile_first.p, ctx->n_contigs, min_reads, T.cnt);
        LAUNCHCHK("k_clip_sites_count");
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, T.cnt, T.off, T.blk, tiles, true)));
        HIPCHK(hipMemcpyAsync(&total, T.off + tiles, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    ctx->clip_sites_epoch = ctx->win_epoch; ctx->clip_sites_total = total;
    ctx->clip_sites_left = d_left; ctx->clip_sites_right = d_right; ctx->clip_sites_depth = d_depth;
    ctx->clip_sites_min_reads = min_reads; ctx->clip_sites_windows = n_windows;
    *h_n_sites = total;
    return GCI_OK;
}

extern "C" int gci_clip_sites_write(gci_ctx* ctx, const int32_t* d_left, const int32_t* d_right, const int32_t* d_depth, int32_t min_reads,
                                    const gci_window* h_windows, uint32_t n_windows, gci_clip_site* d_out, uint64_t cap)
{
    if (!ctx || !d_left || !d_right || min_reads < 1 || (n_windows && !h_windows)) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    // not what gci_clip_sites_size measured last on this context, or its windows are no longer the context's
    if (!ctx->clip_sites_epoch || ctx->clip_sites_epoch != ctx->win_epoch || d_left != ctx->clip_sites_left || d_right != ctx->clip_sites_right ||
        d_depth != ctx->clip_sites_depth || min_reads != ctx->clip_sites_min_reads || n_windows != ctx->clip_sites_windows)
        return GCI_E_INVALID;
    const unsigned long long total = ctx->clip_sites_total;
    if (total && !d_out) return GCI_E_INVALID;
    if (cap < total) return GCI_E_CAPACITY;
    const int64_t tiles = ctx->win_tiles;
    if (!tiles || !total) return GCI_OK;
    const ClipTileScratch T = cl_tile_scratch(ctx, tiles);
    hipLaunchKernelGGL(k_clip_sites_write, dim3((uint32_t)tiles), dim3(BLOCK), 0, ctx->stream, d_left, d_right, d_depth, (const gci_window*)ctx->win.p,
                       (const int64_t*)ctx->win_tile_first.p, (int32_t)ctx->win_n, (const int64_t*)ctx->d_off.p, (const int64_t*)ctx->d_len.p,
                       (const int64_t*)ctx->d_tile_first.p, ctx->n_contigs, min_reads, T.cnt, T.off, d_out, total);
    LAUNCHCHK("k_clip_sites_write");
    return GCI_OK;
}
