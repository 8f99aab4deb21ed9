// k_fate.hip -- what becomes of every record of a BAM stream in the record filter, and why: gci_bam_fate gives each record the class
// named after the FIRST test of read_sam (the reference's GCI.py:152-168) it fails, in the reference's order -- none (never seen by
// the reference: unmapped, no or unselected contig, pos < 0), secondary, supplementary, mapq, clip, identity -- or `kept`.  The
// decisions are those of gci_bam_filter (k_filter.hip): the same first-NM and CG:B,I rules, the same quotients (ratio_cmp), the same
// status word.
//
// Input as for gci_bam_filter: the inflated stream (or a heads stream) and the record offsets.  The shape is k_cover.hip's: the unit
// of the CIGAR work is a CHUNK of at most GCI_COVER_CHUNK_OPS operations, never a record.  Three steps:
//   k_fate_parse    one lane per record: bounds, the classes the core fields settle (none, secondary, supplementary, mapq), and for
//                   the others the first NM tag, where the operations lie (own CIGAR or CG array) and how many chunks they make;
//                   a settled record makes no chunk, looks for no tag
//   k_fate_sum      one wave per chunk: the bases under S, M / = / X, I and D, summed over the wave; no atomics
//   k_fate_decide   one lane per record: adds the record's chunk sums, runs the two ratio tests in the order of decide4 (k_filter.hip),
//                   writes the class byte; the records per class go through an LDS histogram per workgroup, flushed once
// with an exclusive scan of the chunk counts between the first two.  gci_fate_refine (filter_depth.py --join) then moves every `kept`
// byte to the class the cross-file join gave the record (k_join.hip: gci_name_join_fate), one lane per record.
#include "gci_cover_chunks.hpp"
#include "gci_ratio.hpp"

#define FATE_PENDING 0xFFu                 // a class byte between k_fate_parse and k_fate_decide: the CIGAR decides
#define FATE_NM_NONE INT64_MAX             // no NM tag
#define FATE_NM_BAD INT64_MIN              // an NM tag of a non-integer type

struct FateRecScratch {                    // carved out of ctx->fate_rec
    unsigned long long* status;
    unsigned long long* counts;            // GCI_FATE_CLASSES
    unsigned long long* chunk0;            // n_rec + 1: exclusive scan of the chunk counts
    long long* nm;
    CoverRec* recs;
    unsigned long long* blk;
    uint32_t* nch;
};

static inline size_t ft_blocks(uint64_t n) { return (size_t)((n + TILE - 1) / TILE); }

static inline size_t ft_rec_bytes(uint32_t n_rec)
{
    return 16 + 8 * GCI_FATE_CLASSES + 8 * ((size_t)n_rec + 1) + 8 * (size_t)n_rec + sizeof(CoverRec) * (size_t)n_rec + 8 * (ft_blocks(n_rec) + 2) +
           4 * (size_t)n_rec;
}

static inline FateRecScratch ft_rec_scratch(gci_ctx* ctx, uint32_t n_rec)
{
    FateRecScratch s;
    uint8_t* p = (uint8_t*)ctx->fate_rec.p;
    s.status = (unsigned long long*)p; p += 16;
    s.counts = (unsigned long long*)p; p += 8 * GCI_FATE_CLASSES;
    s.chunk0 = (unsigned long long*)p; p += 8 * ((size_t)n_rec + 1);
    s.nm = (long long*)p; p += 8 * (size_t)n_rec;
    s.recs = (CoverRec*)p; p += sizeof(CoverRec) * (size_t)n_rec;
    s.blk = (unsigned long long*)p; p += 8 * (ft_blocks(n_rec) + 2);
    s.nch = (uint32_t*)p;
    return s;
}

struct FateSums { unsigned long long S, M, I, D; };     // bases of a chunk under S, M / = / X, I, D

// ---- step 1: one lane per record ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_fate_parse(const uint8_t* __restrict__ bam, uint64_t n_bytes, const uint64_t* __restrict__ rec_off,
                                                      uint32_t n_rec, int has_seq, const int32_t* __restrict__ ref_sel, int32_t n_ref, int map_qual,
                                                      CoverRec* __restrict__ recs, uint32_t* __restrict__ nch, long long* __restrict__ nm_out,
                                                      uint8_t* __restrict__ cls, unsigned long long* __restrict__ status)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_rec) return;
    CoverRec r;
    r.ops_off = 0; r.n_ops = 0; r.contig = -1; r.pos = 0; r.pad = 0;
    uint32_t chunks = 0;
    long long nm = FATE_NM_NONE;
    uint8_t c = GCI_FATE_ERROR;
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
        } else if ((flag & 0x4u) || ref_id < 0 || ref_id >= n_ref || pos < 0 || ref_sel[ref_id] < 0) {
            c = GCI_FATE_NONE;
        } else if (flag & 0x100u) {
            c = GCI_FATE_SECONDARY;                                              // GCI.py:156, test by test
        } else if (flag & 0x800u) {
            c = GCI_FATE_SUPPLEMENTARY;
        } else if (mapq < map_qual) {
            c = GCI_FATE_MAPQ;
        } else {
            c = FATE_PENDING;
            r.contig = ref_sel[ref_id];
            r.pos = pos;
            r.ops_off = cig_off;
            r.n_ops = n_cigar;
            // the first NM and -- behind the placeholder <l_seq>S<n>N of a CIGAR of more than 65535 operations -- the first CG tag
            // (bam_aux_get), walked as the record filter walks them
            bool want_cg = false;
            if (n_cigar > 0) {
                const uint32_t op0 = cv_rd32(bam + cig_off);
                want_cg = (op0 & 0xFu) == 4u && (op0 >> 4) == (uint32_t)l_seq;
            }
            bool have_nm = false;
            const uint8_t* end = bam + rec_end;
            for (const uint8_t* q = bam + aux_off; q + 3 <= end && (!have_nm || want_cg);) {
                const int64_t sz = cv_aux_size(q + 3, end, q[2]);
                if (sz < 0 || q + 3 + sz > end) break;
                if (q[0] == 'N' && q[1] == 'M' && !have_nm) {
                    have_nm = true;
                    const uint8_t* t = q + 2;                                    // the type byte, the value behind it
                    switch (t[0]) {
                    case 'c': nm = (int8_t)t[1]; break;
                    case 'C': nm = t[1]; break;
                    case 's': nm = (int16_t)cv_rd16(t + 1); break;
                    case 'S': nm = cv_rd16(t + 1); break;
                    case 'i': nm = (int32_t)cv_rd32(t + 1); break;
                    case 'I': nm = cv_rd32(t + 1); break;
                    default: nm = FATE_NM_BAD; break;
                    }
                } else if (q[0] == 'C' && q[1] == 'G' && want_cg) {
                    want_cg = false;
                    if (q[2] == 'B' && (q[3] == 'I' || q[3] == 'i')) {
                        const uint32_t cg_len = cv_rd32(q + 4);
                        if (cg_len >= n_cigar && cg_len < (1u << 29)) { r.ops_off = (uint64_t)(q + 8 - bam); r.n_ops = cg_len; }
                    }
                }
                q += 3 + sz;
            }
            chunks = (r.n_ops + CV_OPS - 1) / CV_OPS;
        }
    }
    recs[i] = r;
    nch[i] = chunks;
    nm_out[i] = nm;
    cls[i] = c;
}

// ---- step 2: one wave per chunk ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_fate_sum(const uint8_t* __restrict__ bam, uint64_t n_bytes, const CoverRec* __restrict__ recs,
                                                    const unsigned long long* __restrict__ chunk0, uint32_t n_rec, unsigned long long n_chunks,
                                                    FateSums* __restrict__ sums)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long ch = (unsigned long long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (ch >= n_chunks) return;                        // (the whole wave)
    const uint32_t rec = cv_rec_of_chunk(chunk0, n_rec, ch);
    const CoverRec r = recs[rec];
    const CvChunk c = cv_chunk_of(bam, r, (uint32_t)(ch - chunk0[rec]));
    unsigned long long s = 0, m = 0, ins = 0, del = 0;
    for (uint32_t k0 = 0; k0 < c.n; k0 += 64) {
        const uint32_t k = k0 + lane;
        const uint32_t v = cv_op_word(bam, n_bytes, c, k, lane);
        const uint32_t op = v & 0xFu, len = k < c.n ? v >> 4 : 0u;
        s += op == 4u ? len : 0u;
        m += ((0x181u >> op) & 1u) ? len : 0u;                                   // M = X
        ins += op == 1u ? len : 0u;
        del += op == 2u ? len : 0u;
    }
    FateSums t;
    t.S = wave_sum<unsigned long long>(s);
    t.M = wave_sum<unsigned long long>(m);
    t.I = wave_sum<unsigned long long>(ins);
    t.D = wave_sum<unsigned long long>(del);
    if (lane == 0) sums[ch] = t;
}

// ---- step 3: one lane per record ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_fate_decide(uint32_t n_rec, const unsigned long long* __restrict__ chunk0, const FateSums* __restrict__ sums,
                                                       const long long* __restrict__ nm_in, double clip_percent, double iden_percent,
                                                       uint8_t* __restrict__ cls, unsigned long long* __restrict__ counts,
                                                       unsigned long long* __restrict__ status)
{
    __shared__ uint32_t hist[GCI_FATE_CLASSES];
    if (threadIdx.x < GCI_FATE_CLASSES) hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n_rec) {
        uint32_t c = cls[i];
        if (c == FATE_PENDING) {
            long long S = 0, M = 0, I = 0, D = 0;
            for (unsigned long long ch = chunk0[i], e = chunk0[i + 1]; ch < e; ch++) {
                const FateSums t = sums[ch];
                S += (long long)t.S; M += (long long)t.M; I += (long long)t.I; D += (long long)t.D;
            }
            const long long nm = nm_in[i], den1 = M + I + S, den2 = M + I + D;
            int st = GCI_OK;
            // the order of decide4 (k_filter.hip); Python's `and` short-circuits: the identity division only runs when the clip test passed
            if (nm == FATE_NM_NONE) st = GCI_E_NO_NM;
            else if (nm == FATE_NM_BAD) st = GCI_E_BAD_NM_TYPE;
            else if (den1 == 0) st = GCI_E_ZERO_DIV;
            else if (!ratio_cmp(S, den1, clip_percent, true)) c = GCI_FATE_CLIP;
            else if (den2 == 0) st = GCI_E_ZERO_DIV;
            else if (!ratio_cmp(den2 - nm, den2, iden_percent, false)) c = GCI_FATE_IDENTITY;
            else c = GCI_FATE_KEPT;
            if (st != GCI_OK) { c = GCI_FATE_ERROR; cv_report(status, i, st); }
            cls[i] = (uint8_t)c;
        }
        atomicAdd(&hist[c & (GCI_FATE_CLASSES - 1)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < GCI_FATE_CLASSES && hist[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)hist[threadIdx.x]);
}

// ---- gci_fate_refine: a `kept` record takes the class the cross-file join gave it (gci_name_join_fate) -------------------------------
__global__ __launch_bounds__(BLOCK) void k_fate_refine(uint8_t* __restrict__ cls, const uint8_t* __restrict__ join_fate, uint32_t n_rec,
                                                       unsigned long long* __restrict__ status)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_rec) return;
    const uint32_t c = cls[i], j = join_fate[i];
    if (c == GCI_FATE_KEPT) {
        if (j >= GCI_FATE_SHADOWED && j <= GCI_FATE_JOINED) cls[i] = (uint8_t)j;
        else cv_report(status, i, GCI_E_INVALID);                                // the join saw no passing record here: the two passes disagree
    } else if (j != 0) cv_report(status, i, GCI_E_INVALID);                      // ... or a passing one where the classes see none
}

extern "C" int gci_fate_refine(gci_ctx* ctx, uint8_t* d_class, const uint8_t* d_join_fate, uint32_t n_rec, uint64_t* d_status)
{
    if (!ctx || !d_status || (n_rec && (!d_class || !d_join_fate))) return GCI_E_INVALID;
    HIPCHK(hipMemsetAsync(d_status, 0xFF, 8, ctx->stream));
    if (n_rec) {
        hipLaunchKernelGGL(k_fate_refine, dim3((n_rec + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, ctx->stream, d_class, d_join_fate, n_rec,
                           (unsigned long long*)d_status);
        LAUNCHCHK("k_fate_refine");
    }
    return GCI_OK;
}

// ---- export -------------------------------------------------------------------------------------------------------------------------
extern "C" int gci_bam_fate(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                            const int32_t* d_ref_sel, int32_t n_ref, int map_qual, double clip_percent, double iden_percent, uint8_t* d_class,
                            uint64_t* h_counts, uint64_t* d_status)
{
    if (!ctx || !h_counts || !d_status || n_ref < 0 || (n_rec && (!d_stream || !d_rec_off || !d_ref_sel || !d_class))) return GCI_E_INVALID;
    for (int k = 0; k < GCI_FATE_CLASSES; k++) h_counts[k] = 0;
    GCI_TRY(gci_ensure(ctx, ctx->fate_rec, ft_rec_bytes(n_rec)));
    const FateRecScratch R = ft_rec_scratch(ctx, n_rec);
    HIPCHK(hipMemsetAsync(R.status, 0xFF, 8, ctx->stream));
    HIPCHK(hipMemsetAsync(R.counts, 0, 8 * GCI_FATE_CLASSES, ctx->stream));
    if (n_rec) {
        const dim3 rec_grid((n_rec + BLOCK - 1) / BLOCK);
        unsigned long long n_chunks = 0;
        hipLaunchKernelGGL(k_fate_parse, rec_grid, dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, d_rec_off, n_rec, has_seq, d_ref_sel, n_ref, map_qual,
                           R.recs, R.nch, R.nm, d_class, R.status);
        LAUNCHCHK("k_fate_parse");
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, R.nch, R.chunk0, R.blk, (int64_t)n_rec, true)));
        HIPCHK(hipMemcpyAsync(&n_chunks, R.chunk0 + n_rec, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (n_chunks > 0x7FFFFFFFull) return GCI_E_INVALID;                  // (2^42 operations in one call)
        FateSums* sums = nullptr;
        if (n_chunks) {
            GCI_TRY(gci_ensure(ctx, ctx->fate_chunk, sizeof(FateSums) * (size_t)n_chunks));
            sums = (FateSums*)ctx->fate_chunk.p;
            hipLaunchKernelGGL(k_fate_sum, dim3((uint32_t)((n_chunks + BLOCK / 64 - 1) / (BLOCK / 64))), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes,
                               R.recs, R.chunk0, n_rec, n_chunks, sums);
            LAUNCHCHK("k_fate_sum");
        }
        hipLaunchKernelGGL(k_fate_decide, rec_grid, dim3(BLOCK), 0, ctx->stream, n_rec, R.chunk0, sums, R.nm, clip_percent, iden_percent, d_class,
                           R.counts, R.status);
        LAUNCHCHK("k_fate_decide");
    }
    HIPCHK(hipMemcpyAsync(h_counts, R.counts, 8 * GCI_FATE_CLASSES, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_status, R.status, 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GCI_OK;
}
