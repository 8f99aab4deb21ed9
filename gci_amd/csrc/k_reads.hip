// k_reads.hip -- filter_reads.py: the records of chosen classes (gci_bam_fate's bytes) whose reference span overlaps a set of windows,
// IN RECORD ORDER, one row of text each: gci_bam_reads_size / _write (include/gci_hip.h states the row).
//
// Input as for gci_bam_fate.  The CIGAR work is k_fate.hip's: a CHUNK of at most GCI_COVER_CHUNK_OPS operations is a wave's, never a
// record's (gci_cover_chunks.hpp).  The text is k_bedgraph.hip's scheme: count, scan, ranked stores, rows rendered in LDS.
//   k_reads_parse    one lane per record whose class bit is set (the others are not read beyond their class byte): bounds, core fields,
//                    the contig's first window that ends behind pos -- none: no row, no chunk --, the first NM tag, where the operations
//                    lie (own CIGAR or CG array) and how many chunks they make
//   k_cigar_sums     one wave per chunk: the bases under S, M / = / X, I, D and N, summed over the wave; whether it holds a code 9 - 15;
//                    no atomics (gci_cigar_sums.hpp, shared with k_sweep.hip)
//   k_reads_measure  one lane per record: adds the chunk sums, span and overlap (the windows of a contig are sorted and disjoint, so the
//                    one k_reads_parse found is the only one to ask), the row's length, GCI_E_MALFORMED for codes 9 - 15 in a row;
//                    rows and bytes per workgroup
//   k_reads_text     a workgroup takes its own 256 records again, ranks the rows (block_exclusive), renders each at its offset into an LDS
//                    stage and copies the stage out with 16-byte stores (text_copy_out); a workgroup whose rows do not fit the stage
//                    (read names of 254 bytes, contig names of any length) renders them straight into memory
// with exclusive scans between them (chunks per record; bytes and rows per workgroup, 64 bits).  What a row holds besides the two names
// lives in the context between the two calls (ReadsRow): the write pass reads no record again but its name.
#include "gci_cigar_sums.hpp"

#define RD_STAGE 49152                   // LDS bytes of staging: 16 for the alignment shift + the rows of a workgroup (~120 bytes each for HiFi names)
#define RD_CONTIG_NAME_MAX 65535u
#define RD_NM_NONE INT64_MAX             // no NM tag, or one of a non-integer type: '.'
#define RD_NO_WINDOWS INT64_MIN          // ReadsRow.win_b without a window test
#define RD_CLASS_MASK 0x1F7Eu            // the classes a caller may ask for: all but none (0) and error (7)

struct ReadsRow {                        // what a row holds besides the two names
    unsigned long long M, I, D, S, end;
    long long nm;
    long long win_b;                     // between k_reads_parse and k_reads_measure: the beginning of the window to test against
    unsigned long long name_at;          // byte offset of the read name in the stream
    uint32_t len;                        // bytes of the row; 0: the record is not selected
    uint16_t flag;
    uint8_t mapq, name_len;
};

struct ReadsScratch {                    // carved out of ctx->reads_rec
    unsigned long long* status;
    unsigned long long* chunk0;          // n_rec + 1: exclusive scan of the chunk counts
    ReadsRow* rows;
    CoverRec* recs;                      // (pad = the class byte)
    unsigned long long* blk;             // block totals of the chunk scan
    unsigned long long* byte0;           // n_blocks + 1: exclusive scan of the workgroups' row bytes
    unsigned long long* row0;            // n_blocks + 1: ... of their rows
    unsigned long long* blk2;
    uint32_t* nch;
    uint32_t* blk_bytes;
    uint32_t* blk_rows;
};

static inline size_t rd_scan_blocks(uint64_t n) { return (size_t)((n + TILE - 1) / TILE); }
static inline size_t rd_groups(uint32_t n_rec) { return ((size_t)n_rec + BLOCK - 1) / BLOCK; }

static inline size_t rd_rec_bytes(uint32_t n_rec)
{
    const size_t n = n_rec, g = rd_groups(n_rec);
    return 16 + 8 * (n + 1) + sizeof(ReadsRow) * n + sizeof(CoverRec) * n + 8 * (rd_scan_blocks(n) + 2) + 2 * 8 * (g + 1) + 8 * (rd_scan_blocks(g) + 2) +
           4 * n + 2 * 4 * g;
}

static inline ReadsScratch rd_scratch(gci_ctx* ctx, uint32_t n_rec)
{
    const size_t n = n_rec, g = rd_groups(n_rec);
    ReadsScratch s;
    uint8_t* p = (uint8_t*)ctx->reads_rec.p;
    s.status = (unsigned long long*)p; p += 16;
    s.chunk0 = (unsigned long long*)p; p += 8 * (n + 1);
    s.rows = (ReadsRow*)p; p += sizeof(ReadsRow) * n;
    s.recs = (CoverRec*)p; p += sizeof(CoverRec) * n;
    s.blk = (unsigned long long*)p; p += 8 * (rd_scan_blocks(n) + 2);
    s.byte0 = (unsigned long long*)p; p += 8 * (g + 1);
    s.row0 = (unsigned long long*)p; p += 8 * (g + 1);
    s.blk2 = (unsigned long long*)p; p += 8 * (rd_scan_blocks(g) + 2);
    s.nch = (uint32_t*)p; p += 4 * n;
    s.blk_bytes = (uint32_t*)p; p += 4 * g;
    s.blk_rows = (uint32_t*)p;
    return s;
}

// ---- step 1: one lane per record ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_reads_parse(const uint8_t* __restrict__ bam, uint64_t n_bytes, const uint64_t* __restrict__ rec_off,
                                                       uint32_t n_rec, int has_seq, const int32_t* __restrict__ ref_sel, int32_t n_ref, int32_t n_sel,
                                                       const uint8_t* __restrict__ cls, uint32_t class_mask, const gci_window* __restrict__ win,
                                                       const uint32_t* __restrict__ contig_win0, CoverRec* __restrict__ recs,
                                                       uint32_t* __restrict__ nch, ReadsRow* __restrict__ rows, unsigned long long* __restrict__ status)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_rec) return;
    CoverRec r;
    r.ops_off = 0; r.n_ops = 0; r.contig = -1; r.pos = 0; r.pad = 0;
    ReadsRow w;
    w.M = w.I = w.D = w.S = w.end = 0; w.nm = RD_NM_NONE; w.win_b = RD_NO_WINDOWS; w.name_at = 0; w.len = 0; w.flag = 0; w.mapq = 0; w.name_len = 0;
    uint32_t chunks = 0;
    const uint32_t c = cls[i];
    if (c < 32u && ((class_mask >> c) & 1u)) {
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
            } else if (ref_id < 0 || ref_id >= n_ref || pos < 0 || (sel = ref_sel[ref_id]) < 0 || sel >= n_sel) {
                cv_report(status, i, GCI_E_INVALID);                             // the class bytes of another input: such a record is `none`
            } else {
                bool candidate = true;
                if (contig_win0) {                                               // the contig's first window that ends behind pos
                    uint32_t lo = contig_win0[sel];
                    const uint32_t last = contig_win0[sel + 1];
                    for (uint32_t hi = last; lo < hi;) {
                        const uint32_t mid = lo + ((hi - lo) >> 1);
                        if (win[mid].end > (int64_t)pos) hi = mid; else lo = mid + 1;
                    }
                    candidate = lo < last;
                    if (candidate) w.win_b = win[lo].begin;
                }
                if (candidate) {
                    r.contig = sel; r.pos = pos; r.pad = c;
                    r.ops_off = cig_off; r.n_ops = n_cigar;
                    w.flag = (uint16_t)flag; w.mapq = p[13];
                    w.name_at = off + 36;
                    uint32_t nl = 0;
                    while (nl < l_read_name && p[36 + nl]) nl++;
                    w.name_len = (uint8_t)nl;
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
                            case 'c': w.nm = (int8_t)t[1]; break;
                            case 'C': w.nm = t[1]; break;
                            case 's': w.nm = (int16_t)cv_rd16(t + 1); break;
                            case 'S': w.nm = cv_rd16(t + 1); break;
                            case 'i': w.nm = (int32_t)cv_rd32(t + 1); break;
                            case 'I': w.nm = cv_rd32(t + 1); break;
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
    }
    recs[i] = r;
    nch[i] = chunks;
    rows[i] = w;
}

// ---- a row, written once for the pass that measures it and the pass that renders it ---------------------------------------------------
__device__ static const char RD_CLASS_NAME[13][14] = {"none", "secondary", "supplementary", "mapq", "clip", "identity", "kept", "error",
                                                      "shadowed", "unpaired", "contig", "overlap", "joined"};

struct RdCount {                         // the length of what is emitted
    static constexpr bool counts = true;
    uint32_t n = 0;
    __device__ __forceinline__ void ch(uint8_t) { n++; }
    __device__ __forceinline__ void span(const uint8_t*, uint32_t len) { n += len; }
    __device__ __forceinline__ void dec(uint64_t v) { n += ndigits64(v); }
};

struct RdPut {                           // ... and its bytes at p (LDS or global memory)
    static constexpr bool counts = false;
    uint8_t* p;
    __device__ __forceinline__ void ch(uint8_t c) { *p++ = c; }
    __device__ __forceinline__ void span(const uint8_t* s, uint32_t len) { for (uint32_t k = 0; k < len; k++) p[k] = s[k]; p += len; }
    __device__ __forceinline__ void dec(uint64_t v) { const uint32_t w = ndigits64(v); put_dec64(p, v, w); p += w; }
};

template <typename E>
__device__ __forceinline__ void rd_signed(E& e, long long v)
{
    if (v < 0) e.ch('-');
    e.dec(v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v);
}

// dec6(n, d), d > 0: '-' if n < 0, |n| / d, '.', six digits of the remainder by long division (r < d < 2^59: r * 10 fits 64 bits)
template <typename E>
__device__ __forceinline__ void rd_dec6(E& e, long long n, unsigned long long d)
{
    if (n < 0) e.ch('-');
    const unsigned long long a = n < 0 ? 0ull - (unsigned long long)n : (unsigned long long)n;
    e.dec(a / d);
    e.ch('.');
    if constexpr (E::counts) {
        e.n += 6;
    } else {
        unsigned long long r = a % d;
        for (int k = 0; k < 6; k++) { r *= 10ull; e.ch((uint8_t)('0' + r / d)); r %= d; }
    }
}

template <typename E>
__device__ __forceinline__ void rd_row(E& e, const ReadsRow& w, const CoverRec& r, uint32_t file_no, const uint8_t* name, const uint8_t* contig,
                                       uint32_t contig_len)
{
    e.dec(file_no); e.ch('\t');
    e.span(name, w.name_len); e.ch('\t');
    e.span(contig, contig_len); e.ch('\t');
    e.dec((uint64_t)(uint32_t)r.pos); e.ch('\t');
    e.dec(w.end); e.ch('\t');
    e.ch((w.flag & 0x10u) ? '-' : '+'); e.ch('\t');
    e.dec(w.flag); e.ch('\t');
    e.dec(w.mapq); e.ch('\t');
    e.dec(w.M); e.ch('\t');
    e.dec(w.I); e.ch('\t');
    e.dec(w.D); e.ch('\t');
    e.dec(w.S); e.ch('\t');
    if (w.nm == RD_NM_NONE) e.ch('.'); else rd_signed(e, w.nm);
    e.ch('\t');
    const unsigned long long den1 = w.M + w.I + w.S, den2 = w.M + w.I + w.D;
    if (den1 == 0) e.ch('.'); else rd_dec6(e, (long long)w.S, den1);
    e.ch('\t');
    if (den2 == 0 || w.nm == RD_NM_NONE) e.ch('.'); else rd_dec6(e, (long long)den2 - w.nm, den2);
    e.ch('\t');
    const char* cn = RD_CLASS_NAME[r.pad < 13u ? r.pad : 7u];
    for (uint32_t k = 0; cn[k]; k++) e.ch((uint8_t)cn[k]);
    e.ch('\n');
}

// ---- step 3: one lane per record ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_reads_measure(uint32_t n_rec, const CoverRec* __restrict__ recs, const unsigned long long* __restrict__ chunk0,
                                                         const CigarSums* __restrict__ sums, const uint32_t* __restrict__ contig_name_len,
                                                         uint32_t file_no, ReadsRow* __restrict__ rows, uint32_t* __restrict__ blk_bytes,
                                                         uint32_t* __restrict__ blk_rows, unsigned long long* __restrict__ status)
{
    __shared__ uint32_t part[2][BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t i = blockIdx.x * BLOCK + t;
    uint32_t len = 0;
    if (i < n_rec) {
        const CoverRec r = recs[i];
        if (r.contig >= 0) {
            ReadsRow w = rows[i];
            unsigned long long N = 0, bad = 0;
            for (unsigned long long ch = chunk0[i], e = chunk0[i + 1]; ch < e; ch++) {
                const CigarSums s = sums[ch];
                w.S += s.S; w.M += s.M; w.I += s.I; w.D += s.D; N += s.N; bad |= s.bad;
            }
            const unsigned long long R = w.M + w.D + N;                          // (every total is below 2^57)
            w.end = (unsigned long long)(uint32_t)r.pos + R;
            const long long reach = (long long)((unsigned long long)(uint32_t)r.pos + (R ? R : 1ull));
            if (w.win_b == RD_NO_WINDOWS || reach > w.win_b) {
                RdCount e;
                rd_row(e, w, r, file_no, nullptr, nullptr, contig_name_len[r.contig]);
                len = e.n;
                if (bad) cv_report(status, i, GCI_E_MALFORMED);                   // (the codes add to no total; the row is listed)
            }
            w.len = len;
            rows[i] = w;
        }
    }
    const uint32_t bytes = wave_sum<uint32_t>(len), n = wave_sum<uint32_t>(len ? 1u : 0u);
    if (lane == 0) { part[0][wave] = bytes; part[1][wave] = n; }
    __syncthreads();
    if (t == 0) {
        blk_bytes[blockIdx.x] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        blk_rows[blockIdx.x] = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    }
}

// ---- step 4: one workgroup per 256 records ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_reads_text(const uint8_t* __restrict__ bam, uint32_t n_rec, const CoverRec* __restrict__ recs,
                                                      const ReadsRow* __restrict__ rows, const uint8_t* __restrict__ contig_names,
                                                      const unsigned long long* __restrict__ contig_name_off,
                                                      const uint32_t* __restrict__ contig_name_len, uint32_t file_no,
                                                      const unsigned long long* __restrict__ byte0, uint8_t* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[RD_STAGE];
    __shared__ uint32_t wtot[BLOCK / 64];
    const int t = threadIdx.x;
    const uint32_t i = blockIdx.x * BLOCK + t;
    ReadsRow w;
    w.len = 0;
    if (i < n_rec) w = rows[i];
    uint32_t total;
    const uint32_t pre = block_exclusive<uint32_t, BLOCK / 64>(w.len, wtot, total);
    const unsigned long long dst = byte0[blockIdx.x];
    if ((unsigned long long)total != byte0[blockIdx.x + 1] - dst) return;         // not the rows the size pass measured: write nothing
    if (total == 0) return;
    const bool staged = total + 16u <= RD_STAGE;
    const uint32_t shift = (uint32_t)((uintptr_t)(out + dst) & 15u);
    if (w.len) {
        const CoverRec r = recs[i];
        RdPut e;
        e.p = staged ? stage + shift + pre : out + dst + pre;
        rd_row(e, w, r, file_no, bam + w.name_at, contig_names + contig_name_off[r.contig], contig_name_len[r.contig]);
    }
    if (staged) {
        __syncthreads();
        text_copy_out(out + dst, stage, shift, total, t);
    }
}

// ---- exports ----------------------------------------------------------------------------------------------------------------------
extern "C" int gci_bam_reads_size(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                                  const int32_t* d_ref_sel, int32_t n_ref, const uint8_t* d_class, uint32_t class_mask, const gci_window* d_win,
                                  const uint32_t* d_contig_win0, const uint32_t* h_contig_name_len, uint32_t file_no, uint64_t* h_n_rows,
                                  uint64_t* h_n_bytes, uint64_t* d_status)
{
    if (!ctx || !h_n_rows || !h_n_bytes || !d_status || n_ref < 0 || (n_rec && (!d_stream || !d_rec_off || !d_ref_sel || !d_class))) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    if ((class_mask & ~RD_CLASS_MASK) || !h_contig_name_len || (d_contig_win0 && !d_win)) return GCI_E_INVALID;
    const int32_t n_sel = ctx->n_contigs;
    for (int32_t c = 0; c < n_sel; c++) if (h_contig_name_len[c] > RD_CONTIG_NAME_MAX) return GCI_E_INVALID;
    ctx->reads_valid = false;
    *h_n_rows = 0; *h_n_bytes = 0;
    GCI_TRY(gci_ensure(ctx, ctx->reads_rec, rd_rec_bytes(n_rec)));
    GCI_TRY(gci_ensure(ctx, ctx->reads_names, (size_t)n_sel * 12));
    const ReadsScratch R = rd_scratch(ctx, n_rec);
    uint32_t* d_name_len = (uint32_t*)((uint8_t*)ctx->reads_names.p + (size_t)n_sel * 8);
    GCI_TRY(gci_upload_small(ctx, d_name_len, h_contig_name_len, (size_t)n_sel * 4));
    HIPCHK(hipMemsetAsync(R.status, 0xFF, 8, ctx->stream));
    unsigned long long n_chunks = 0, totals[2] = {0, 0};
    if (n_rec) {
        const uint32_t groups = (uint32_t)rd_groups(n_rec);
        hipLaunchKernelGGL(k_reads_parse, dim3(groups), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, d_rec_off, n_rec, has_seq, d_ref_sel, n_ref, n_sel,
                           d_class, class_mask, d_win, d_contig_win0, R.recs, R.nch, R.rows, R.status);
        LAUNCHCHK("k_reads_parse");
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, R.nch, R.chunk0, R.blk, (int64_t)n_rec, true)));
        HIPCHK(hipMemcpyAsync(&n_chunks, R.chunk0 + n_rec, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (n_chunks > 0x7FFFFFFFull) return GCI_E_INVALID;                  // (2^42 operations in one call)
        CigarSums* sums = nullptr;
        if (n_chunks) {
            GCI_TRY(gci_ensure(ctx, ctx->reads_chunk, sizeof(CigarSums) * (size_t)n_chunks));
            sums = (CigarSums*)ctx->reads_chunk.p;
            hipLaunchKernelGGL(k_cigar_sums, cigar_sums_grid(n_chunks), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, R.recs, R.chunk0, n_rec, n_chunks,
                               sums);
            LAUNCHCHK("k_cigar_sums");
        }
        hipLaunchKernelGGL(k_reads_measure, dim3(groups), dim3(BLOCK), 0, ctx->stream, n_rec, R.recs, R.chunk0, sums, d_name_len, file_no, R.rows,
                           R.blk_bytes, R.blk_rows, R.status);
        LAUNCHCHK("k_reads_measure");
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, R.blk_bytes, R.byte0, R.blk2, (int64_t)groups, true)));
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, R.blk_rows, R.row0, R.blk2, (int64_t)groups, true)));
        HIPCHK(hipMemcpyAsync(&totals[0], R.byte0 + groups, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(&totals[1], R.row0 + groups, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipMemcpyAsync(d_status, R.status, 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->reads_valid = true;
    ctx->reads_n_rec = n_rec; ctx->reads_n_bytes = n_bytes; ctx->reads_file_no = file_no;
    ctx->reads_stream = d_stream; ctx->reads_off = d_rec_off;
    ctx->reads_total = totals[0]; ctx->reads_rows = totals[1];
    ctx->reads_name_len.assign(h_contig_name_len, h_contig_name_len + n_sel);
    *h_n_bytes = totals[0];
    *h_n_rows = totals[1];
    return GCI_OK;
}

extern "C" int gci_bam_reads_write(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec,
                                   const uint8_t* d_contig_names, const uint64_t* h_contig_name_off, const uint32_t* h_contig_name_len, uint8_t* d_out,
                                   uint64_t cap)
{
    if (!ctx || !h_contig_name_off || !h_contig_name_len || (n_rec && (!d_stream || !d_rec_off))) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    // not the input gci_bam_reads_size measured last on this context
    if (!ctx->reads_valid || n_rec != ctx->reads_n_rec || n_bytes != ctx->reads_n_bytes || d_stream != ctx->reads_stream || d_rec_off != ctx->reads_off ||
        (size_t)ctx->n_contigs != ctx->reads_name_len.size())
        return GCI_E_INVALID;
    const int32_t n_sel = ctx->n_contigs;
    for (int32_t c = 0; c < n_sel; c++) {
        if (h_contig_name_len[c] != ctx->reads_name_len[(size_t)c] || (h_contig_name_len[c] && !d_contig_names)) return GCI_E_INVALID;
    }
    if (ctx->reads_total && !d_out) return GCI_E_INVALID;
    if (cap < ctx->reads_total) return GCI_E_CAPACITY;
    if (ctx->reads_total == 0) return GCI_OK;
    const ReadsScratch R = rd_scratch(ctx, n_rec);
    GCI_TRY(gci_upload_small(ctx, ctx->reads_names.p, h_contig_name_off, (size_t)n_sel * 8));
    const uint32_t* d_name_len = (const uint32_t*)((const uint8_t*)ctx->reads_names.p + (size_t)n_sel * 8);
    hipLaunchKernelGGL(k_reads_text, dim3((uint32_t)rd_groups(n_rec)), dim3(BLOCK), 0, ctx->stream, d_stream, n_rec, R.recs, R.rows, d_contig_names,
                       (const unsigned long long*)ctx->reads_names.p, d_name_len, ctx->reads_file_no, R.byte0, d_out);
    LAUNCHCHK("k_reads_text");
    return GCI_OK;
}
