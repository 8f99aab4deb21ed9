// k_indels.hip -- indel_sites.py: long insertions and deletions in reads.  gci_bam_indel_size / _write turn every D and I operation of at
// least min_len bases in a counted record of a BAM stream into an EVENT -- the deleted reference bases as one interval, the base in
// front of the inserted bases as an interval of one base -- for the depth build; gci_indel_sites_size / _write list the RUNS of the
// two built tracks that reach min_reads (include/gci_hip.h states both).
//
// The record side.  Input as for gci_bam_cover_size; a CHUNK of at most GCI_COVER_CHUNK_OPS operations is a wave's, never a record's
// (gci_cover_chunks.hpp, gci_cigar_sums.hpp).
//   k_indel_parse   one lane per record: bounds, core fields, the skip rule, where the operations lie (own CIGAR or CG array) and how
//                   many chunks they make
//   k_cigar_sums    one wave per chunk: the bases under M / = / X, D and N, codes 9 - 15; no atomics
//   k_indel_ref     one lane per chunk: its reference length M + D + N -- scanned, it is the carry that places an operation of chunk k
//   k_indel_count   one wave per chunk, 64 operations a round: a scan of the reference lengths across the lanes gives every
//                   operation its position, a ballot the chunk's deletions and insertions that lie inside the contig
//   k_indel_finish  one lane per record: ORs its chunks' `bad` into the status word, says whether the record is counted
//   k_indel_write   one wave per chunk: the same walk; a lane's slot is its chunk's offset + the events of earlier rounds + the events
//                   of the lanes below it
// with the project's exclusive scan between them (chunks per record; reference length, deletions and insertions per chunk; counted
// records).  The only global atomic is the status word's atomicMin.
//
// The track side.  K8's windows and tiling (gci_set_windows, 4096-element tiles, int4 loads), as k_clips.hip.
//   k_indel_sites_count   one workgroup per window tile: the del and ins tracks, 16 bytes a lane; a RUN START is a hot element whose
//                         predecessor is not hot, or outside the window, or outside the contig; one count per tile
//   k_indel_sites_write   one workgroup per window tile, gone at once when the tile's count is 0: a thread takes 16 consecutive
//                         elements, a workgroup scan ranks the starts
//   k_indel_site_finish   one wave per site: walks forward from the start, 64 elements a round, to the first element that is not hot
//                         or the end of the window or contig; the maxima of the three tracks; the depth track is read here only
#include "gci_cigar_sums.hpp"
#include "gci_site_tiles.hpp"

struct IndelRecScratch {                 // carved out of ctx->indel_rec
    unsigned long long* status;
    unsigned long long* chunk0;          // n_rec + 1: exclusive scan of the chunk counts
    unsigned long long* cnt0;            // n_rec + 1: exclusive scan of `counted`
    CoverRec* recs;
    unsigned long long* blk;
    uint32_t* nch;
    uint32_t* counted;
};

struct IndelChunkScratch {               // carved out of ctx->indel_chunk
    CigarSums* sums;
    unsigned long long* ref;             // reference length of a chunk
    unsigned long long* ref0;            // n_chunks + 1: its exclusive scan
    unsigned long long* del0;            // n_chunks + 1: exclusive scan of the deletions
    unsigned long long* ins0;            // n_chunks + 1: ... of the insertions
    unsigned long long* blk;
    uint32_t* n_del;
    uint32_t* n_ins;
};

static inline size_t in_blocks(uint64_t n) { return (size_t)((n + TILE - 1) / TILE); }

static inline size_t in_rec_bytes(uint32_t n_rec)
{
    const size_t n = n_rec;
    return 16 + 2 * 8 * (n + 1) + sizeof(CoverRec) * n + 8 * (in_blocks(n) + 2) + 2 * 4 * n;
}

static inline IndelRecScratch in_rec_scratch(gci_ctx* ctx, uint32_t n_rec)
{
    const size_t n = n_rec;
    IndelRecScratch s;
    uint8_t* p = (uint8_t*)ctx->indel_rec.p;
    s.status = (unsigned long long*)p; p += 16;
    s.chunk0 = (unsigned long long*)p; p += 8 * (n + 1);
    s.cnt0 = (unsigned long long*)p; p += 8 * (n + 1);
    s.recs = (CoverRec*)p; p += sizeof(CoverRec) * n;
    s.blk = (unsigned long long*)p; p += 8 * (in_blocks(n) + 2);
    s.nch = (uint32_t*)p; p += 4 * n;
    s.counted = (uint32_t*)p;
    return s;
}

static inline size_t in_chunk_bytes(uint64_t n_chunks)
{
    const size_t n = (size_t)n_chunks;
    return sizeof(CigarSums) * n + 8 * n + 3 * 8 * (n + 1) + 8 * (in_blocks(n) + 2) + 2 * 4 * n;
}

static inline IndelChunkScratch in_chunk_scratch(gci_ctx* ctx, uint64_t n_chunks)
{
    const size_t n = (size_t)n_chunks;
    IndelChunkScratch s;
    uint8_t* p = (uint8_t*)ctx->indel_chunk.p;
    s.sums = (CigarSums*)p; p += sizeof(CigarSums) * n;
    s.ref = (unsigned long long*)p; p += 8 * n;
    s.ref0 = (unsigned long long*)p; p += 8 * (n + 1);
    s.del0 = (unsigned long long*)p; p += 8 * (n + 1);
    s.ins0 = (unsigned long long*)p; p += 8 * (n + 1);
    s.blk = (unsigned long long*)p; p += 8 * (in_blocks(n) + 2);
    s.n_del = (uint32_t*)p; p += 4 * n;
    s.n_ins = (uint32_t*)p;
    return s;
}

// ---- step 1: one lane per record ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_indel_parse(const uint8_t* __restrict__ bam, uint64_t n_bytes, const uint64_t* __restrict__ rec_off,
                                                       uint32_t n_rec, int has_seq, const int32_t* __restrict__ ref_sel, int32_t n_ref,
                                                       uint32_t excl_flags, int min_mapq, CoverRec* __restrict__ recs, uint32_t* __restrict__ nch,
                                                       unsigned long long* __restrict__ status)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_rec) return;
    CvSeq q;
    uint32_t chunks;
    const CoverRec r = cv_parse_counted(bam, n_bytes, rec_off[i], i, has_seq, ref_sel, n_ref, excl_flags, min_mapq, status, chunks, q);
    recs[i] = r;
    nch[i] = chunks;
}

// ---- step 2b: one lane per chunk --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_indel_ref(const CigarSums* __restrict__ sums, unsigned long long n_chunks,
                                                     unsigned long long* __restrict__ chunk_ref)
{
    const unsigned long long ch = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (ch >= n_chunks) return;
    const CigarSums s = sums[ch];
    chunk_ref[ch] = s.M + s.D + s.N;                   // (every total is below 2^57)
}

// ---- steps 3 and 4: one wave per chunk, the walk both share ----------------------------------------------------------------------
__device__ __forceinline__ unsigned long long in_below(int lane) { return (1ull << lane) - 1ull; }

template <bool WRITE>
__device__ __forceinline__ void indel_walk(const uint8_t* __restrict__ bam, uint64_t n_bytes, const CoverRec* __restrict__ recs,
                                           const unsigned long long* __restrict__ chunk0, uint32_t n_rec, unsigned long long n_chunks,
                                           const unsigned long long* __restrict__ chunk_ref0, const int64_t* __restrict__ contig_len,
                                           int32_t n_contigs, uint32_t min_len, uint32_t* __restrict__ chunk_del, uint32_t* __restrict__ chunk_ins,
                                           const unsigned long long* __restrict__ chunk_del0, const unsigned long long* __restrict__ chunk_ins0,
                                           unsigned long long n_del, unsigned long long total, gci_ivl* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long ch = (unsigned long long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (ch >= n_chunks) return;                        // (the whole wave)
    const uint32_t rec = cv_rec_of_chunk(chunk0, n_rec, ch);
    const CoverRec r = recs[rec];
    const unsigned long long ch_first = chunk0[rec];
    const CvChunk c = cv_chunk_of(bam, r, (uint32_t)(ch - ch_first));
    // positions in 64 bits: pos + the reference lengths in front may pass 2^31; compared with L before they become int32
    unsigned long long at = (unsigned long long)(uint32_t)r.pos + (chunk_ref0[ch] - chunk_ref0[ch_first]);
    const int64_t len = r.contig < n_contigs ? contig_len[r.contig] : 0;     // (a d_ref_sel beyond the layout: no base of it is inside)
    const unsigned long long L = (unsigned long long)(len < 0x7FFFFFFEll ? (len < 0 ? 0 : len) : 0x7FFFFFFEll);
    unsigned long long o_del = 0, o_ins = 0;           // where the chunk's next deletion / insertion goes
    if (WRITE) { o_del = chunk_del0[ch]; o_ins = n_del + chunk_ins0[ch]; }
    uint32_t dels = 0, inss = 0;
    for (uint32_t k0 = 0; k0 < c.n; k0 += 64) {
        const uint32_t k = k0 + lane;
        const bool valid = k < c.n;
        const uint32_t v = cv_op_word(bam, n_bytes, c, k, lane);
        const uint32_t op = v & 0xFu, n = v >> 4;
        const unsigned long long ref_len = (valid && ((0x18Du >> op) & 1u)) ? n : 0u;        // M D N = X
        const unsigned long long inc = wave_inclusive<unsigned long long>(ref_len, lane);
        const unsigned long long mine = at + inc - ref_len;                      // where this lane's operation begins on the reference
        const unsigned long long site = mine > 0 ? mine - 1 : 0;                 // the base in front of an insertion
        const bool is_del = valid && op == 2u && n >= min_len && mine < L;
        const bool is_ins = valid && op == 1u && n >= min_len && site < L;
        const unsigned long long delm = __ballot(is_del), insm = __ballot(is_ins);
        if (WRITE) {
            gci_ivl e;
            e.contig = r.contig; e.pad = 0;
            if (is_del) {
                const unsigned long long last = mine + n < L ? mine + n : L;     // (exclusive; n >= 1)
                const unsigned long long slot = o_del + (unsigned long long)__builtin_popcountll(delm & in_below(lane));
                e.start = (int32_t)mine; e.end = (int32_t)(last - 1);
                if (slot < n_del) out[slot] = e;
            }
            if (is_ins) {
                const unsigned long long slot = o_ins + (unsigned long long)__builtin_popcountll(insm & in_below(lane));
                e.start = e.end = (int32_t)site;
                if (slot < total) out[slot] = e;
            }
            o_del += (unsigned long long)__builtin_popcountll(delm);
            o_ins += (unsigned long long)__builtin_popcountll(insm);
        } else {
            dels += (uint32_t)__builtin_popcountll(delm);
            inss += (uint32_t)__builtin_popcountll(insm);
        }
        at += __shfl(inc, 63, 64);
    }
    if (!WRITE && lane == 0) { chunk_del[ch] = dels; chunk_ins[ch] = inss; }
}

__global__ __launch_bounds__(BLOCK) void k_indel_count(const uint8_t* __restrict__ bam, uint64_t n_bytes, const CoverRec* __restrict__ recs,
                                                       const unsigned long long* __restrict__ chunk0, uint32_t n_rec, unsigned long long n_chunks,
                                                       const unsigned long long* __restrict__ chunk_ref0, const int64_t* __restrict__ contig_len,
                                                       int32_t n_contigs, uint32_t min_len, uint32_t* __restrict__ chunk_del,
                                                       uint32_t* __restrict__ chunk_ins)
{
    indel_walk<false>(bam, n_bytes, recs, chunk0, n_rec, n_chunks, chunk_ref0, contig_len, n_contigs, min_len, chunk_del, chunk_ins, nullptr, nullptr,
                      0, 0, nullptr);
}

__global__ __launch_bounds__(BLOCK) void k_indel_write(const uint8_t* __restrict__ bam, uint64_t n_bytes, const CoverRec* __restrict__ recs,
                                                       const unsigned long long* __restrict__ chunk0, uint32_t n_rec, unsigned long long n_chunks,
                                                       const unsigned long long* __restrict__ chunk_ref0, const int64_t* __restrict__ contig_len,
                                                       int32_t n_contigs, uint32_t min_len, const unsigned long long* __restrict__ chunk_del0,
                                                       const unsigned long long* __restrict__ chunk_ins0, unsigned long long n_del,
                                                       unsigned long long total, gci_ivl* __restrict__ out)
{
    indel_walk<true>(bam, n_bytes, recs, chunk0, n_rec, n_chunks, chunk_ref0, contig_len, n_contigs, min_len, nullptr, nullptr, chunk_del0, chunk_ins0,
                     n_del, total, out);
}

// ---- step 5: one lane per record ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_indel_finish(uint32_t n_rec, const CoverRec* __restrict__ recs, const unsigned long long* __restrict__ chunk0,
                                                        const CigarSums* __restrict__ sums, uint32_t* __restrict__ counted,
                                                        unsigned long long* __restrict__ status)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_rec) return;
    uint32_t c = 0;
    if (recs[i].contig >= 0) {
        c = 1;
        unsigned long long bad = 0;
        for (unsigned long long ch = chunk0[i], last = chunk0[i + 1]; ch < last; ch++) bad |= sums[ch].bad;
        if (bad) cv_report(status, i, GCI_E_MALFORMED);
    }
    counted[i] = c;
}

// ---- exports: the record side -----------------------------------------------------------------------------------------------------
static inline dim3 in_wave_grid(unsigned long long n_chunks) { return dim3((uint32_t)((n_chunks + BLOCK / 64 - 1) / (BLOCK / 64))); }

extern "C" int gci_bam_indel_size(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                                  const int32_t* d_ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq, int min_len, uint64_t* h_counts,
                                  uint64_t* d_status)
{
    if (!ctx || !h_counts || !d_status || n_ref < 0 || min_len < 1 || (n_rec && (!d_stream || !d_rec_off || !d_ref_sel))) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    ctx->indel_valid = false;
    h_counts[0] = h_counts[1] = h_counts[2] = 0;
    GCI_TRY(gci_ensure(ctx, ctx->indel_rec, in_rec_bytes(n_rec)));
    const IndelRecScratch R = in_rec_scratch(ctx, n_rec);
    HIPCHK(hipMemsetAsync(R.status, 0xFF, 8, ctx->stream));
    unsigned long long n_chunks = 0, n_del = 0, n_ins = 0, n_counted = 0;
    if (n_rec) {
        const uint32_t groups = (n_rec + BLOCK - 1) / BLOCK;
        hipLaunchKernelGGL(k_indel_parse, dim3(groups), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, d_rec_off, n_rec, has_seq, d_ref_sel, n_ref,
                           excl_flags, min_mapq, R.recs, R.nch, R.status);
        LAUNCHCHK("k_indel_parse");
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, R.nch, R.chunk0, R.blk, (int64_t)n_rec, true)));
        HIPCHK(hipMemcpyAsync(&n_chunks, R.chunk0 + n_rec, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (n_chunks > 0x7FFFFFFFull) return GCI_E_INVALID;                  // (2^42 operations in one call)
        const CigarSums* sums = nullptr;
        if (n_chunks) {
            GCI_TRY(gci_ensure(ctx, ctx->indel_chunk, in_chunk_bytes(n_chunks)));
            const IndelChunkScratch C = in_chunk_scratch(ctx, n_chunks);
            sums = C.sums;
            hipLaunchKernelGGL(k_cigar_sums, cigar_sums_grid(n_chunks), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, R.recs, R.chunk0, n_rec, n_chunks,
                               C.sums);
            LAUNCHCHK("k_cigar_sums");
            hipLaunchKernelGGL(k_indel_ref, dim3((uint32_t)((n_chunks + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, ctx->stream, C.sums, n_chunks, C.ref);
            LAUNCHCHK("k_indel_ref");
            GCI_TRY((device_exclusive_scan<unsigned long long, unsigned long long>(ctx, C.ref, C.ref0, C.blk, (int64_t)n_chunks, true)));
            hipLaunchKernelGGL(k_indel_count, in_wave_grid(n_chunks), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, R.recs, R.chunk0, n_rec, n_chunks,
                               C.ref0, (const int64_t*)ctx->d_len.p, ctx->n_contigs, (uint32_t)min_len, C.n_del, C.n_ins);
            LAUNCHCHK("k_indel_count");
            GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, C.n_del, C.del0, C.blk, (int64_t)n_chunks, true)));
            GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, C.n_ins, C.ins0, C.blk, (int64_t)n_chunks, true)));
            HIPCHK(hipMemcpyAsync(&n_del, C.del0 + n_chunks, 8, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(&n_ins, C.ins0 + n_chunks, 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        hipLaunchKernelGGL(k_indel_finish, dim3(groups), dim3(BLOCK), 0, ctx->stream, n_rec, R.recs, R.chunk0, sums, R.counted, R.status);
        LAUNCHCHK("k_indel_finish");
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, R.counted, R.cnt0, R.blk, (int64_t)n_rec, true)));
        HIPCHK(hipMemcpyAsync(&n_counted, R.cnt0 + n_rec, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipMemcpyAsync(d_status, R.status, 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->indel_valid = true;
    ctx->indel_n_rec = n_rec; ctx->indel_n_bytes = n_bytes; ctx->indel_n_chunks = n_chunks; ctx->indel_min_len = min_len;
    ctx->indel_n_del = n_del; ctx->indel_n_ins = n_ins;
    ctx->indel_stream = d_stream; ctx->indel_off = d_rec_off;
    h_counts[0] = n_counted; h_counts[1] = n_del; h_counts[2] = n_ins;
    return GCI_OK;
}

extern "C" int gci_bam_indel_write(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                                   gci_ivl* d_out, uint64_t cap, uint64_t* d_status)
{
    (void)has_seq;                                                           // (the parse of the size call has used it)
    if (!ctx || !d_status || (n_rec && (!d_stream || !d_rec_off))) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    // not the input gci_bam_indel_size measured last on this context
    if (!ctx->indel_valid || n_rec != ctx->indel_n_rec || n_bytes != ctx->indel_n_bytes || d_stream != ctx->indel_stream || d_rec_off != ctx->indel_off)
        return GCI_E_INVALID;
    const unsigned long long total = ctx->indel_n_del + ctx->indel_n_ins;
    if (total && !d_out) return GCI_E_INVALID;
    if (cap < total) return GCI_E_CAPACITY;
    const IndelRecScratch R = in_rec_scratch(ctx, n_rec);
    const unsigned long long n_chunks = ctx->indel_n_chunks;
    if (n_chunks && total) {
        const IndelChunkScratch C = in_chunk_scratch(ctx, n_chunks);
        hipLaunchKernelGGL(k_indel_write, in_wave_grid(n_chunks), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, R.recs, R.chunk0, n_rec, n_chunks,
                           C.ref0, (const int64_t*)ctx->d_len.p, ctx->n_contigs, (uint32_t)ctx->indel_min_len, C.del0, C.ins0,
                           (unsigned long long)ctx->indel_n_del, total, d_out);
        LAUNCHCHK("k_indel_write");
    }
    HIPCHK(hipMemcpyAsync(d_status, R.status, 8, hipMemcpyDeviceToDevice, ctx->stream));
    return GCI_OK;
}

// ---- the track side ---------------------------------------------------------------------------------------------------------------
// whether the element in front of q is hot AND of the same window and contig -- for the first element of a wave's stretch, which no
// neighbour lane holds; q - 1 may lie in the tile in front
__device__ __forceinline__ bool indel_prev_hot(const int32_t* __restrict__ del, const int32_t* __restrict__ ins, const SiteTile& x, int64_t q,
                                               int32_t min_reads)
{
    if (q - 1 < x.run_lo || q - 1 >= x.run_hi) return false;
    return del[q - 1] >= min_reads || ins[q - 1] >= min_reads;
}

__global__ __launch_bounds__(BLOCK) void k_indel_sites_count(const int32_t* __restrict__ del, const int32_t* __restrict__ ins,
                                                             const gci_window* __restrict__ win, const int64_t* __restrict__ win_tile_first,
                                                             int32_t n_win, const int64_t* __restrict__ off, const int64_t* __restrict__ len,
                                                             const int64_t* __restrict__ tile_first, int32_t n_contigs, int32_t min_reads,
                                                             uint32_t* __restrict__ tile_cnt)
{
    __shared__ uint32_t part[BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const SiteTile x = site_tile_of(win, win_tile_first, n_win, blockIdx.x, off, len, tile_first, n_contigs);
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t p = x.p0 + (int64_t)(j * BLOCK + t) * 4;
        const int4 a = *reinterpret_cast<const int4*>(del + p), b = *reinterpret_cast<const int4*>(ins + p);
        const int32_t d[4] = {a.x, a.y, a.z, a.w}, s[4] = {b.x, b.y, b.z, b.w};
        uint32_t hot = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) hot |= (p + k >= x.lo && p + k < x.hi && (d[k] >= min_reads || s[k] >= min_reads)) ? (1u << k) : 0u;
        // the element in front of the lane's four: the lane below holds it, but for the wave's first lane
        uint32_t prev = (uint32_t)__shfl_up((int)(hot >> 3), 1, 64);
        if (lane == 0) prev = indel_prev_hot(del, ins, x, p, min_reads) ? 1u : 0u;
        n += (uint32_t)__builtin_popcount(hot & ~((hot << 1) | prev) & 0xFu);
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

__global__ __launch_bounds__(BLOCK) void k_indel_sites_write(const int32_t* __restrict__ del, const int32_t* __restrict__ ins,
                                                             const gci_window* __restrict__ win, const int64_t* __restrict__ win_tile_first,
                                                             int32_t n_win, const int64_t* __restrict__ off, const int64_t* __restrict__ len,
                                                             const int64_t* __restrict__ tile_first, int32_t n_contigs, int32_t min_reads,
                                                             const uint32_t* __restrict__ tile_cnt, const unsigned long long* __restrict__ tile_off,
                                                             gci_indel_site* __restrict__ out, unsigned long long total)
{
    __shared__ uint32_t wtot[BLOCK / 64];
    if (tile_cnt[blockIdx.x] == 0) return;             // (the whole workgroup)
    const int t = threadIdx.x, lane = t & 63;
    const SiteTile x = site_tile_of(win, win_tile_first, n_win, blockIdx.x, off, len, tile_first, n_contigs);
    const int64_t p = x.p0 + (int64_t)t * 16;          // a thread's 16 consecutive elements: ascending order is thread order
    uint32_t hot = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int4 a = *reinterpret_cast<const int4*>(del + p + 4 * j), b = *reinterpret_cast<const int4*>(ins + p + 4 * j);
        const int32_t d[4] = {a.x, a.y, a.z, a.w}, s[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t q = p + 4 * j + k;
            hot |= (q >= x.lo && q < x.hi && (d[k] >= min_reads || s[k] >= min_reads)) ? (1u << (4 * j + k)) : 0u;
        }
    }
    uint32_t prev = (uint32_t)__shfl_up((int)(hot >> 15), 1, 64);
    if (lane == 0) prev = indel_prev_hot(del, ins, x, p, min_reads) ? 1u : 0u;
    uint32_t starts = hot & ~((hot << 1) | prev) & 0xFFFFu;
    uint32_t all;
    const uint32_t pre = block_exclusive<uint32_t, BLOCK / 64>((uint32_t)__builtin_popcount(starts), wtot, all);
    unsigned long long slot = tile_off[blockIdx.x] + pre;
    while (starts) {                                   // (few: a genome has thousands of sites)
        const int k = __builtin_ctz(starts);
        starts &= starts - 1u;
        gci_indel_site s;
        s.contig = x.contig; s.start = (int32_t)(p + k - x.contig_off);
        s.end = (int32_t)(x.run_hi - x.contig_off);    // where the run ends at the latest: k_indel_site_finish walks up to it
        s.del = 0; s.ins = 0; s.depth = 0;
        if (slot < total) out[slot] = s;
        slot++;
    }
}

__device__ __forceinline__ int32_t in_wave_max(int32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}

__global__ __launch_bounds__(BLOCK) void k_indel_site_finish(const int32_t* __restrict__ del, const int32_t* __restrict__ ins,
                                                             const int32_t* __restrict__ depth, const int64_t* __restrict__ off, int32_t min_reads,
                                                             gci_indel_site* __restrict__ out, unsigned long long total)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long i = (unsigned long long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= total) return;                            // (the whole wave)
    const gci_indel_site s = out[i];
    const int64_t base = off[s.contig], lim = base + s.end;
    int64_t q = base + s.start;                        // (hot, and below lim)
    int32_t md = INT32_MIN, mi = INT32_MIN, mx = INT32_MIN;
    for (;;) {
        const int64_t e = q + lane;
        const bool in = e < lim;
        const int32_t d = in ? del[e] : 0, n = in ? ins[e] : 0;
        const unsigned long long cold = ~__ballot(in && (d >= min_reads || n >= min_reads));
        const int first = cold ? __builtin_ctzll(cold) : 64;                    // the run's elements of this round: the lanes below `first`
        if (lane < first) {
            md = max(md, d); mi = max(mi, n);
            if (depth) mx = max(mx, depth[e]);
        }
        q += first;
        if (first < 64) break;
    }
    md = in_wave_max(md); mi = in_wave_max(mi); mx = depth ? in_wave_max(mx) : 0;
    if (lane == 0) {
        gci_indel_site r = s;
        r.end = (int32_t)(q - base); r.del = md; r.ins = mi; r.depth = mx;
        out[i] = r;
    }
}

struct IndelTileScratch { uint32_t* cnt; unsigned long long* off; unsigned long long* blk; };

static inline IndelTileScratch in_tile_scratch(gci_ctx* ctx, int64_t tiles)
{
    IndelTileScratch s;
    uint8_t* p = (uint8_t*)ctx->indel_tiles.p;
    s.off = (unsigned long long*)p; p += 8 * ((size_t)tiles + 1);
    s.blk = (unsigned long long*)p; p += 8 * (in_blocks((uint64_t)tiles) + 2);
    s.cnt = (uint32_t*)p;
    return s;
}

extern "C" int gci_indel_sites_size(gci_ctx* ctx, const int32_t* d_del, const int32_t* d_ins, const int32_t* d_depth, int32_t min_reads,
                                    const gci_window* h_windows, uint32_t n_windows, uint64_t* h_n_sites)
{
    if (!ctx || !d_del || !d_ins || !h_n_sites || min_reads < 1 || (n_windows && !h_windows)) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    if ((((uintptr_t)d_del) | ((uintptr_t)d_ins) | ((uintptr_t)d_depth)) & 15u) return GCI_E_INVALID;         // whole tracks, as allocated
    if (n_windows >= (1u << 31)) return GCI_E_INVALID;
    std::vector<gci_window> ws;
    if (!gci_site_windows(ctx, h_windows, n_windows, ws)) return GCI_E_INVALID;
    ctx->indel_sites_epoch = 0;
    *h_n_sites = 0;
    GCI_TRY(gci_set_windows(ctx, ws.data(), (uint32_t)ws.size()));
    ctx->win_flank = INT32_MIN;
    const int64_t tiles = ctx->win_tiles;
    if (tiles > 0x7FFFFFFFll) return GCI_E_INVALID;
    unsigned long long total = 0;
    if (tiles) {
        GCI_TRY(gci_ensure(ctx, ctx->indel_tiles, 8 * ((size_t)tiles + 1) + 8 * (in_blocks((uint64_t)tiles) + 2) + 4 * (size_t)tiles));
        const IndelTileScratch T = in_tile_scratch(ctx, tiles);
        hipLaunchKernelGGL(k_indel_sites_count, dim3((uint32_t)tiles), dim3(BLOCK), 0, ctx->stream, d_del, d_ins, (const gci_window*)ctx->win.p,
                           (const int64_t*)ctx->win_tile_first.p, (int32_t)ctx->win_n, (const int64_t*)ctx->d_off.p, (const int64_t*)ctx->d_len.p,
                           (const int64_t*)ctx->d_tile_first.p, ctx->n_contigs, min_reads, T.cnt);
        LAUNCHCHK("k_indel_sites_count");
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, T.cnt, T.off, T.blk, tiles, true)));
        HIPCHK(hipMemcpyAsync(&total, T.off + tiles, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    ctx->indel_sites_epoch = ctx->win_epoch; ctx->indel_sites_total = total;
    ctx->indel_sites_del = d_del; ctx->indel_sites_ins = d_ins; ctx->indel_sites_depth = d_depth;
    ctx->indel_sites_min_reads = min_reads; ctx->indel_sites_windows = n_windows;
    *h_n_sites = total;
    return GCI_OK;
}

extern "C" int gci_indel_sites_write(gci_ctx* ctx, const int32_t* d_del, const int32_t* d_ins, const int32_t* d_depth, int32_t min_reads,
                                     const gci_window* h_windows, uint32_t n_windows, gci_indel_site* d_out, uint64_t cap)
{
    if (!ctx || !d_del || !d_ins || min_reads < 1 || (n_windows && !h_windows)) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    // not what gci_indel_sites_size measured last on this context, or its windows are no longer the context's
    if (!ctx->indel_sites_epoch || ctx->indel_sites_epoch != ctx->win_epoch || d_del != ctx->indel_sites_del || d_ins != ctx->indel_sites_ins ||
        d_depth != ctx->indel_sites_depth || min_reads != ctx->indel_sites_min_reads || n_windows != ctx->indel_sites_windows)
        return GCI_E_INVALID;
    const unsigned long long total = ctx->indel_sites_total;
    if (total && !d_out) return GCI_E_INVALID;
    if (cap < total) return GCI_E_CAPACITY;
    const int64_t tiles = ctx->win_tiles;
    if (!tiles || !total) return GCI_OK;
    const IndelTileScratch T = in_tile_scratch(ctx, tiles);
    hipLaunchKernelGGL(k_indel_sites_write, dim3((uint32_t)tiles), dim3(BLOCK), 0, ctx->stream, d_del, d_ins, (const gci_window*)ctx->win.p,
                       (const int64_t*)ctx->win_tile_first.p, (int32_t)ctx->win_n, (const int64_t*)ctx->d_off.p, (const int64_t*)ctx->d_len.p,
                       (const int64_t*)ctx->d_tile_first.p, ctx->n_contigs, min_reads, T.cnt, T.off, d_out, total);
    LAUNCHCHK("k_indel_sites_write");
    hipLaunchKernelGGL(k_indel_site_finish, in_wave_grid(total), dim3(BLOCK), 0, ctx->stream, d_del, d_ins, d_depth, (const int64_t*)ctx->d_off.p,
                       min_reads, d_out, total);
    LAUNCHCHK("k_indel_site_finish");
    return GCI_OK;
}
