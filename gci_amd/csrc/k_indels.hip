// k_indels.hip -- indel_sites.py: long insertions and deletions in reads.  gci_bam_indel_size / _write turn every D and I operation of at
// least min_len bases in a counted record of a BAM stream into an EVENT -- the deleted reference bases as one interval, the base in
// front of the inserted bases as an interval of one base -- for the depth build; gci_indel_sites_size / _write list the RUNS of the
// two built tracks that reach min_reads (include/gci_hip.h states both).
//
// The record side.  Input as for gci_bam_cover_size; a CHUNK of at most GCI_COVER_CHUNK_OPS operations is a wave's, never a record's
// (gci_cover_chunks.hpp, gci_cigar_sums.hpp).
//   k_indel_parse   one lane per record: cv_parse_counted -- bounds, core fields, the skip rule, where the operations lie (own CIGAR or
//                   CG array) and how many chunks they make
//   k_cigar_sums    one wave per chunk: the bases under M / = / X, D and N, codes 9 - 15; no atomics
//   k_chunk_lens    one lane per chunk: its reference length M + D + N -- scanned, it is the carry that places an operation of chunk k
//   k_indel_count   one wave per chunk, 64 operations a round: a scan of the reference lengths across the lanes gives every
//                   operation its position, a ballot the chunk's deletions and insertions that lie inside the contig
//   k_rec_finish    one lane per record: ORs its chunks' `bad` into the status word, says whether the record is counted
//   k_indel_write   one wave per chunk: the same walk; a lane's slot is its chunk's offset + the events of earlier rounds + the events
//                   of the lanes below it
// with the project's exclusive scan between them (chunks per record; reference length, deletions and insertions per chunk; counted
// records).  The only global atomic is the status word's atomicMin.
//
// The track side.  gci_site_tiles.hpp's lister over the del and ins tracks: the RUNS of hot elements (HotEither, RUNS = true) --
// k_sites_count, k_sites_write with IndelEmit, then k_site_runs_finish with IndelMax: the maxima of the three tracks over a run; the
// depth track is read there only.
#include "gci_cigar_sums.hpp"
#include "gci_site_tiles.hpp"

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

static inline size_t in_chunk_bytes(uint64_t n_chunks)
{
    const size_t n = (size_t)n_chunks;
    return sizeof(CigarSums) * n + 8 * n + 3 * 8 * (n + 1) + 8 * (scan_blocks(n) + 2) + 2 * 4 * n;
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
    s.blk = (unsigned long long*)p; p += 8 * (scan_blocks(n) + 2);
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

// ---- steps 3 and 4: one wave per chunk, the walk both share ----------------------------------------------------------------------
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
                const unsigned long long slot = o_del + (unsigned long long)__builtin_popcountll(delm & lanes_below(lane));
                e.start = (int32_t)mine; e.end = (int32_t)(last - 1);
                if (slot < n_del) out[slot] = e;
            }
            if (is_ins) {
                const unsigned long long slot = o_ins + (unsigned long long)__builtin_popcountll(insm & lanes_below(lane));
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

// ---- exports: the record side -----------------------------------------------------------------------------------------------------
extern "C" int gci_bam_indel_size(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                                  const int32_t* d_ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq, int min_len, uint64_t* h_counts,
                                  uint64_t* d_status)
{
    if (!ctx || !h_counts || !d_status || n_ref < 0 || min_len < 1 || (n_rec && (!d_stream || !d_rec_off || !d_ref_sel))) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    ctx->indel_valid = false;
    h_counts[0] = h_counts[1] = h_counts[2] = 0;
    RecFrame R;
    GCI_TRY(rec_frame_open(ctx, ctx->indel_rec, 0, n_rec, R));
    unsigned long long n_chunks = 0, n_del = 0, n_ins = 0, n_counted = 0;
    if (n_rec) {
        const uint32_t groups = (n_rec + BLOCK - 1) / BLOCK;
        hipLaunchKernelGGL(k_indel_parse, dim3(groups), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, d_rec_off, n_rec, has_seq, d_ref_sel, n_ref,
                           excl_flags, min_mapq, R.recs, R.nch, R.status);
        LAUNCHCHK("k_indel_parse");
        GCI_TRY(rec_frame_chunks(ctx, R, n_rec, n_chunks));
        const CigarSums* sums = nullptr;
        if (n_chunks) {
            GCI_TRY(gci_ensure(ctx, ctx->indel_chunk, in_chunk_bytes(n_chunks)));
            const IndelChunkScratch C = in_chunk_scratch(ctx, n_chunks);
            sums = C.sums;
            hipLaunchKernelGGL(k_cigar_sums, cigar_sums_grid(n_chunks), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, R.recs, R.chunk0, n_rec, n_chunks,
                               C.sums);
            LAUNCHCHK("k_cigar_sums");
            launch_chunk_lens(ctx, C.sums, n_chunks, C.ref, nullptr);
            LAUNCHCHK("k_chunk_lens");
            GCI_TRY((device_exclusive_scan<unsigned long long, unsigned long long>(ctx, C.ref, C.ref0, C.blk, (int64_t)n_chunks, true)));
            hipLaunchKernelGGL(k_indel_count, wave_grid(n_chunks), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, R.recs, R.chunk0, n_rec, n_chunks,
                               C.ref0, (const int64_t*)ctx->d_len.p, ctx->n_contigs, (uint32_t)min_len, C.n_del, C.n_ins);
            LAUNCHCHK("k_indel_count");
            GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, C.n_del, C.del0, C.blk, (int64_t)n_chunks, true)));
            GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, C.n_ins, C.ins0, C.blk, (int64_t)n_chunks, true)));
            HIPCHK(hipMemcpyAsync(&n_del, C.del0 + n_chunks, 8, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(&n_ins, C.ins0 + n_chunks, 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        launch_rec_finish(ctx, n_rec, R.recs, R.chunk0, sums, nullptr, nullptr, R.counted, R.status);
        LAUNCHCHK("k_rec_finish");
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
    const RecFrame R = rec_frame(ctx->indel_rec, n_rec);
    const unsigned long long n_chunks = ctx->indel_n_chunks;
    if (n_chunks && total) {
        const IndelChunkScratch C = in_chunk_scratch(ctx, n_chunks);
        hipLaunchKernelGGL(k_indel_write, wave_grid(n_chunks), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, R.recs, R.chunk0, n_rec, n_chunks,
                           C.ref0, (const int64_t*)ctx->d_len.p, ctx->n_contigs, (uint32_t)ctx->indel_min_len, C.del0, C.ins0,
                           (unsigned long long)ctx->indel_n_del, total, d_out);
        LAUNCHCHK("k_indel_write");
    }
    HIPCHK(hipMemcpyAsync(d_status, R.status, 8, hipMemcpyDeviceToDevice, ctx->stream));
    return GCI_OK;
}

// ---- the track side ---------------------------------------------------------------------------------------------------------------
struct IndelEmit {
    static constexpr int LISTER = 2;
    static constexpr bool RUNS = true;
    gci_indel_site* out;
    __device__ __forceinline__ void operator()(unsigned long long slot, const SiteTile& x, int64_t q) const
    {
        gci_indel_site s;
        s.contig = x.contig; s.start = (int32_t)(q - x.contig_off);
        s.end = (int32_t)(x.run_hi - x.contig_off);    // where the run ends at the latest: k_site_runs_finish walks up to it
        s.del = 0; s.ins = 0; s.depth = 0;
        out[slot] = s;
    }
};

struct IndelMax {                        // of a run: the maxima of the three tracks (no depth track: 0)
    const int32_t* depth;
    struct Acc { int32_t d, i, x; };
    __device__ __forceinline__ Acc init() const { return Acc{INT32_MIN, INT32_MIN, INT32_MIN}; }
    __device__ __forceinline__ void take(Acc& a, int2 v, int64_t e, int64_t) const
    {
        a.d = max(a.d, v.x); a.i = max(a.i, v.y);
        if (depth) a.x = max(a.x, depth[e]);
    }
    __device__ __forceinline__ void wave(Acc& a) const { a.d = wave_max(a.d); a.i = wave_max(a.i); a.x = depth ? wave_max(a.x) : 0; }
    __device__ __forceinline__ void store(gci_indel_site& s, const Acc& a, int64_t) const { s.del = a.d; s.ins = a.i; s.depth = a.x; }
};

static inline SiteMemo in_site_ask(const int32_t* d_del, const int32_t* d_ins, const int32_t* d_depth, int32_t min_reads, uint32_t n_windows)
{
    SiteMemo m;
    m.track[0] = d_del; m.track[1] = d_ins; m.track[2] = d_depth; m.min_reads = min_reads; m.n_windows = n_windows;
    return m;
}

extern "C" int gci_indel_sites_size(gci_ctx* ctx, const int32_t* d_del, const int32_t* d_ins, const int32_t* d_depth, int32_t min_reads,
                                    const gci_window* h_windows, uint32_t n_windows, uint64_t* h_n_sites)
{
    if (!ctx || !d_del || !d_ins || !h_n_sites || min_reads < 1 || (n_windows && !h_windows)) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    if ((((uintptr_t)d_del) | ((uintptr_t)d_ins) | ((uintptr_t)d_depth)) & 15u) return GCI_E_INVALID;         // whole tracks, as allocated
    return site_size<IndelEmit>(ctx, HotEither{d_del, d_ins, min_reads}, in_site_ask(d_del, d_ins, d_depth, min_reads, n_windows), h_windows,
                                      h_n_sites, "k_sites_count (indels)");
}

extern "C" int gci_indel_sites_write(gci_ctx* ctx, const int32_t* d_del, const int32_t* d_ins, const int32_t* d_depth, int32_t min_reads,
                                     const gci_window* h_windows, uint32_t n_windows, gci_indel_site* d_out, uint64_t cap)
{
    if (!ctx || !d_del || !d_ins || min_reads < 1 || (n_windows && !h_windows)) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    const HotEither hot{d_del, d_ins, min_reads};
    GCI_TRY((site_write(ctx, hot, in_site_ask(d_del, d_ins, d_depth, min_reads, n_windows), IndelEmit{d_out}, d_out, cap,
                                         "k_sites_write (indels)")));
    const unsigned long long total = ctx->site_memo.total;
    if (!total) return GCI_OK;
    hipLaunchKernelGGL((k_site_runs_finish<HotEither, IndelMax, gci_indel_site>), wave_grid(total), dim3(BLOCK), 0, ctx->stream, hot,
                       IndelMax{d_depth}, (const int64_t*)ctx->d_off.p, d_out, total);
    LAUNCHCHK("k_site_runs_finish (indels)");
    return GCI_OK;
}
