// k_sweep.hip -- filter_sweep.py: how the record filter's three thresholds cut a BAM stream.  gci_bam_sweep counts every PRIMARY record
// (one gci_bam_fate would call mapq, clip, identity or kept) once in each of three tables -- by its MAPQ, by its clip quotient rounded
// up to K digits, by its identity quotient truncated to K digits --, with two weights (records, the bases under M / = / X) and, beside
// both, the part of them that passes the OTHER TWO tests at the call's thresholds (include/gci_hip.h states the rows and the columns).
//
// Input as for gci_bam_fate, windows as for gci_bam_reads_size.  The CIGAR work is k_reads.hip's: a CHUNK of at most
// GCI_COVER_CHUNK_OPS operations is a wave's, never a record's (gci_cover_chunks.hpp, gci_cigar_sums.hpp).
//   k_sweep_parse   one lane per record: bounds, core fields, the primary test, the contig's first window that ends behind pos -- none:
//                   not counted, no chunk --, the first NM tag, where the operations lie (own CIGAR or CG array) and how many chunks
//                   they make.  MAPQ settles nothing: every primary record's CIGAR is read
//   k_cigar_sums    one wave per chunk: the bases under S, M / = / X, I, D and N, summed over the wave; no atomics
//   k_sweep_bin     persistent workgroups, a grid-stride loop over blocks of 256 records: a lane adds its record's chunk sums, tests the
//                   one window, computes the three rows (long division in 64-bit integers) and the three pass flags (ratio_cmp, the
//                   filter's own comparison) and adds the record into the workgroup's LDS histogram -- 32-bit record counters, 64-bit
//                   base counters, 24 bytes a row, 54 KB at K = 3: two workgroups a CU --, one LDS atomic per lane and counter.  At the
//                   end of its loop a workgroup adds its non-zero entries to the table in memory, 64-bit atomics, once
// with an exclusive scan of the chunk counts between the first two.
#include "gci_cigar_sums.hpp"
#include "gci_ratio.hpp"

#define SW_NM_NONE INT64_MAX             // no NM tag, or one of a non-integer type: the identity is undefined
#define SW_NO_WINDOWS INT64_MIN          // SweepScratch.win_b without a window test

struct SweepScratch {                    // carved out of ctx->sweep_rec
    unsigned long long* status;
    unsigned long long* table;           // GCI_SWEEP_ROWS(3) * GCI_SWEEP_COLS
    unsigned long long* chunk0;          // n_rec + 1: exclusive scan of the chunk counts
    long long* nm;
    long long* win_b;                    // the beginning of the window to test against
    CoverRec* recs;                      // (contig >= 0: a primary record with a window behind its pos; pad = its MAPQ)
    unsigned long long* blk;
    uint32_t* nch;
};

static inline size_t sw_blocks(uint64_t n) { return (size_t)((n + TILE - 1) / TILE); }
static inline size_t sw_table_bytes() { return 8 * (size_t)GCI_SWEEP_COLS * GCI_SWEEP_ROWS(3); }

static inline size_t sw_rec_bytes(uint32_t n_rec)
{
    const size_t n = n_rec;
    return 16 + sw_table_bytes() + 8 * (n + 1) + 8 * n + 8 * n + sizeof(CoverRec) * n + 8 * (sw_blocks(n) + 2) + 4 * n;
}

static inline SweepScratch sw_scratch(gci_ctx* ctx, uint32_t n_rec)
{
    const size_t n = n_rec;
    SweepScratch s;
    uint8_t* p = (uint8_t*)ctx->sweep_rec.p;
    s.status = (unsigned long long*)p; p += 16;
    s.table = (unsigned long long*)p; p += sw_table_bytes();
    s.chunk0 = (unsigned long long*)p; p += 8 * (n + 1);
    s.nm = (long long*)p; p += 8 * n;
    s.win_b = (long long*)p; p += 8 * n;
    s.recs = (CoverRec*)p; p += sizeof(CoverRec) * n;
    s.blk = (unsigned long long*)p; p += 8 * (sw_blocks(n) + 2);
    s.nch = (uint32_t*)p;
    return s;
}

// ---- step 1: one lane per record ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_sweep_parse(const uint8_t* __restrict__ bam, uint64_t n_bytes, const uint64_t* __restrict__ rec_off,
                                                       uint32_t n_rec, int has_seq, const int32_t* __restrict__ ref_sel, int32_t n_ref, int32_t n_sel,
                                                       const gci_window* __restrict__ win, const uint32_t* __restrict__ contig_win0,
                                                       CoverRec* __restrict__ recs, uint32_t* __restrict__ nch, long long* __restrict__ nm_out,
                                                       long long* __restrict__ win_b_out, unsigned long long* __restrict__ status)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_rec) return;
    CoverRec r;
    r.ops_off = 0; r.n_ops = 0; r.contig = -1; r.pos = 0; r.pad = 0;
    uint32_t chunks = 0;
    long long nm = SW_NM_NONE, win_b = SW_NO_WINDOWS;
    const uint64_t off = rec_off[i];
    if (off > n_bytes || n_bytes - off < 36) {
        cv_report(status, i, GCI_E_MALFORMED);
    } else {
        const uint8_t* p = bam + off;
        const int32_t block_size = (int32_t)cv_rd32(p), ref_id = (int32_t)cv_rd32(p + 4), pos = (int32_t)cv_rd32(p + 8);
        const uint32_t l_read_name = p[12];
        const uint32_t n_cigar = cv_rd16(p + 16), flag = cv_rd16(p + 18);
        const int32_t l_seq = (int32_t)cv_rd32(p + 20);
        const uint64_t rec_end = off + 4 + (uint64_t)(uint32_t)block_size;
        const uint64_t cig_off = off + 36 + l_read_name;
        const uint64_t aux_off = cig_off + 4ull * n_cigar + (has_seq ? (((uint64_t)(uint32_t)l_seq + 1) >> 1) + (uint64_t)(uint32_t)l_seq : 0ull);
        int32_t sel = -1;
        if (block_size < 32 || rec_end > n_bytes || l_seq < 0 || aux_off > rec_end) {
            cv_report(status, i, GCI_E_MALFORMED);
        } else if (!(flag & 0x904u) && ref_id >= 0 && ref_id < n_ref && pos >= 0 && (sel = ref_sel[ref_id]) >= 0) {       // primary
            bool candidate = true;
            if (contig_win0) {                                                   // the contig's first window that ends behind pos
                candidate = sel < n_sel;
                if (candidate) {
                    uint32_t lo = contig_win0[sel];
                    const uint32_t last = contig_win0[sel + 1];
                    for (uint32_t hi = last; lo < hi;) {
                        const uint32_t mid = lo + ((hi - lo) >> 1);
                        if (win[mid].end > (int64_t)pos) hi = mid; else lo = mid + 1;
                    }
                    candidate = lo < last;
                    if (candidate) win_b = win[lo].begin;
                }
            }
            if (candidate) {
                r.contig = sel; r.pos = pos; r.pad = p[13];
                r.ops_off = cig_off; r.n_ops = n_cigar;
                // the first NM and -- behind the placeholder <l_seq>S<n>N -- the first CG tag, as k_fate_parse walks them
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
                        const uint8_t* t = q + 2;
                        switch (t[0]) {
                        case 'c': nm = (int8_t)t[1]; break;
                        case 'C': nm = t[1]; break;
                        case 's': nm = (int16_t)cv_rd16(t + 1); break;
                        case 'S': nm = cv_rd16(t + 1); break;
                        case 'i': nm = (int32_t)cv_rd32(t + 1); break;
                        case 'I': nm = cv_rd32(t + 1); break;
                        default: break;
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
    }
    recs[i] = r;
    nch[i] = chunks;
    nm_out[i] = nm;
    win_b_out[i] = win_b;
}

// ---- step 3: the rows of a record, and the workgroup's histogram ------------------------------------------------------------------
// K digits of n / d (0 <= n <= d, d > 0) by long division: floor(n * 10^K / d); `rest`: a remainder is left.  Every total is below
// 2^57, so a remainder times ten fits 64 bits (as dec6, gci_ctx.hpp).
__device__ __forceinline__ uint32_t sw_digits(unsigned long long n, unsigned long long d, int digits, bool& rest)
{
    uint32_t q = (uint32_t)(n / d);
    unsigned long long r = n % d;
    for (int k = 0; k < digits; k++) { r *= 10ull; q = q * 10u + (uint32_t)(r / d); r %= d; }
    rest = r != 0;
    return q;
}

struct SweepLds {                        // the histogram of a workgroup: per row and per column pair (all, others)
    unsigned long long* bases;           // [rows][2]
    uint32_t* records;                   // [rows][2]
};

// a record into row `row` of the histogram, `oth`: also into the row's _others columns; one LDS atomic per lane and counter.  (Combining
// the lanes of a wave that hold the same row first -- a ballot loop, the wave's sums per distinct row, four atomics a round -- was
// built and measured: slower on the input it was meant for)
__device__ __forceinline__ void sw_add(const SweepLds& h, uint32_t row, bool oth, unsigned long long bases)
{
    atomicAdd(&h.records[2 * row], 1u);
    if (bases) atomicAdd(&h.bases[2 * row], bases);
    if (oth) {
        atomicAdd(&h.records[2 * row + 1], 1u);
        if (bases) atomicAdd(&h.bases[2 * row + 1], bases);
    }
}

__global__ __launch_bounds__(BLOCK) void k_sweep_bin(uint32_t n_rec, const CoverRec* __restrict__ recs, const unsigned long long* __restrict__ chunk0,
                                                     const CigarSums* __restrict__ sums, const long long* __restrict__ nm_in,
                                                     const long long* __restrict__ win_b_in, int map_qual, double clip_percent, double iden_percent,
                                                     int digits, unsigned long long* __restrict__ table, unsigned long long* __restrict__ status)
{
    extern __shared__ unsigned long long sw_lds[];                               // 24 bytes a row: bases [rows][2], then records [rows][2]
    const uint32_t rows = (uint32_t)GCI_SWEEP_ROWS(digits);
    SweepLds h;
    h.bases = sw_lds;
    h.records = (uint32_t*)(sw_lds + 2 * rows);
    const int t = threadIdx.x;
    for (uint32_t k = t; k < 2 * rows; k += BLOCK) { h.bases[k] = 0ull; h.records[k] = 0u; }
    __syncthreads();
    const uint32_t n_groups = (n_rec + BLOCK - 1) / BLOCK;
    for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const uint32_t i = g * BLOCK + t;
        bool counted = false, pm = false, pc = false, pi = false;
        uint32_t row_c = 0, row_i = 0, mapq = 0;
        unsigned long long M = 0;
        if (i < n_rec) {
            const CoverRec r = recs[i];
            if (r.contig >= 0) {
                unsigned long long S = 0, I = 0, D = 0, N = 0, bad = 0;
                for (unsigned long long ch = chunk0[i], e = chunk0[i + 1]; ch < e; ch++) {
                    const CigarSums s = sums[ch];
                    S += s.S; M += s.M; I += s.I; D += s.D; N += s.N; bad |= s.bad;
                }
                const unsigned long long R = M + D + N;                          // (every total is below 2^57)
                const long long reach = (long long)((unsigned long long)(uint32_t)r.pos + (R ? R : 1ull)), win_b = win_b_in[i];
                counted = win_b == SW_NO_WINDOWS || reach > win_b;
                if (counted) {
                    if (bad) cv_report(status, i, GCI_E_MALFORMED);               // (the codes add to no total; the record is counted)
                    mapq = r.pad;
                    pm = (int)mapq >= map_qual;
                    const unsigned long long den1 = M + I + S, den2 = M + I + D;
                    const long long nm = nm_in[i];
                    bool rest;
                    if (den1 == 0) row_c = (uint32_t)GCI_SWEEP_CLIP_UNDEF(digits);
                    else {
                        const uint32_t q = sw_digits(S, den1, digits, rest);
                        row_c = (uint32_t)GCI_SWEEP_CLIP(digits, q + (rest ? 1u : 0u));       // rounded up: (b - 1) / B < S / den1 <= b / B
                        pc = ratio_cmp((int64_t)S, (int64_t)den1, clip_percent, true);
                    }
                    if (nm == SW_NM_NONE || den2 == 0) row_i = (uint32_t)GCI_SWEEP_IDEN_UNDEF(digits);
                    else {
                        const long long num = (long long)den2 - nm;
                        if (num < 0) row_i = (uint32_t)GCI_SWEEP_IDEN_BELOW(digits);
                        else if ((unsigned long long)num > den2) row_i = (uint32_t)GCI_SWEEP_IDEN_ABOVE(digits);
                        else row_i = (uint32_t)GCI_SWEEP_IDEN(digits, sw_digits((unsigned long long)num, den2, digits, rest));   // truncated
                        pi = ratio_cmp((int64_t)num, (int64_t)den2, iden_percent, false);
                    }
                }
            }
        }
        if (counted) {
            sw_add(h, (uint32_t)GCI_SWEEP_MAPQ(mapq), pc && pi, M);
            sw_add(h, row_c, pm && pi, M);
            sw_add(h, row_i, pm && pc, M);
        }
    }
    __syncthreads();
    for (uint32_t k = t; k < 2 * rows; k += BLOCK) {                             // entry k: row k / 2, the `all` (0) or the `others` (1) pair of columns
        const uint32_t n = h.records[k];
        if (n) {
            unsigned long long* cell = table + (size_t)(k >> 1) * GCI_SWEEP_COLS + 2 * (k & 1u);
            atomicAdd(cell, (unsigned long long)n);
            if (h.bases[k]) atomicAdd(cell + 1, h.bases[k]);
        }
    }
}

// ---- export -------------------------------------------------------------------------------------------------------------------------
extern "C" int gci_bam_sweep(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                             const int32_t* d_ref_sel, int32_t n_ref, const gci_window* d_win, const uint32_t* d_contig_win0, int map_qual,
                             double clip_percent, double iden_percent, int digits, uint64_t* h_table, uint64_t* d_status)
{
    if (!ctx || !h_table || !d_status || n_ref < 0 || (n_rec && (!d_stream || !d_rec_off || !d_ref_sel))) return GCI_E_INVALID;
    if (digits < 1 || digits > 3 || (d_contig_win0 && !d_win)) return GCI_E_INVALID;
    if (d_contig_win0 && !ctx->n_contigs) return GCI_E_NO_LAYOUT;
    const int32_t n_sel = ctx->n_contigs;
    const size_t table_bytes = 8 * (size_t)GCI_SWEEP_COLS * GCI_SWEEP_ROWS(digits);
    GCI_TRY(gci_ensure(ctx, ctx->sweep_rec, sw_rec_bytes(n_rec)));
    const SweepScratch R = sw_scratch(ctx, n_rec);
    HIPCHK(hipMemsetAsync(R.status, 0xFF, 8, ctx->stream));
    HIPCHK(hipMemsetAsync(R.table, 0, table_bytes, ctx->stream));
    if (n_rec) {
        const uint32_t groups = (n_rec + BLOCK - 1) / BLOCK;
        unsigned long long n_chunks = 0;
        hipLaunchKernelGGL(k_sweep_parse, dim3(groups), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, d_rec_off, n_rec, has_seq, d_ref_sel, n_ref, n_sel,
                           d_win, d_contig_win0, R.recs, R.nch, R.nm, R.win_b, R.status);
        LAUNCHCHK("k_sweep_parse");
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, R.nch, R.chunk0, R.blk, (int64_t)n_rec, true)));
        HIPCHK(hipMemcpyAsync(&n_chunks, R.chunk0 + n_rec, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (n_chunks > 0x7FFFFFFFull) return GCI_E_INVALID;                  // (2^42 operations in one call)
        CigarSums* sums = nullptr;
        if (n_chunks) {
            GCI_TRY(gci_ensure(ctx, ctx->sweep_chunk, sizeof(CigarSums) * (size_t)n_chunks));
            sums = (CigarSums*)ctx->sweep_chunk.p;
            hipLaunchKernelGGL(k_cigar_sums, cigar_sums_grid(n_chunks), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, R.recs, R.chunk0, n_rec, n_chunks,
                               sums);
            LAUNCHCHK("k_cigar_sums");
        }
        // as many workgroups as the device holds at a time, two a CU (the histogram of K = 3 takes 54 KB of a CU's 160 KB; fewer
        // workgroups: fewer flushes); GCI_SWEEP_GRID caps them, so that a test's few records go round the loop more than once
        if (!ctx->pg_cus) {
            int cus = 0;
            HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
            ctx->pg_cus = cus > 0 ? (uint32_t)cus : 256u;
        }
        uint32_t grid = 2 * ctx->pg_cus;
        if (grid > groups) grid = groups;
        if (ctx->sweep_grid_cap && grid > ctx->sweep_grid_cap) grid = ctx->sweep_grid_cap;
        const size_t lds = 24 * (size_t)GCI_SWEEP_ROWS(digits);
        hipLaunchKernelGGL(k_sweep_bin, dim3(grid), dim3(BLOCK), lds, ctx->stream, n_rec, R.recs, R.chunk0, sums, R.nm, R.win_b, map_qual, clip_percent,
                           iden_percent, digits, R.table, R.status);
        LAUNCHCHK("k_sweep_bin");
    }
    HIPCHK(hipMemcpyAsync(h_table, R.table, table_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_status, R.status, 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GCI_OK;
}
