// k_pages.hip -- N1, last step of the ingestion: the records of an inflated BAM stream (or of a heads stream) laid out
// as RECORD PAGES, the input format of the paged record filter (k_filter_pages.hip, gci_bam_filter_pages).
//
// Why a format of our own.  read_sam (/root/reference/GCI.py:146-169) never looks at SEQ / QUAL -- 98 % of a HiFi
// record -- and what it does look at sits at byte-granular offsets inside a stream whose records are found through an
// offset table: the filter over that stream (k_filter.hip) spends its time on three dependent round trips to memory
// (offset -> head -> CIGAR tail / aux) and on re-aligning every dword in registers.  Here the bytes the filter reads are
// copied ONCE, while the inflated stream is walked anyway, into fixed-size pages:
//
//   buffer = [page 0] ... [page n_pages - 1] [blob] [16 zero bytes]
//   page (page_bytes, a multiple of 4096):
//     +0  u32 n_recs | u32 first_rec (index of its first record in the call) | u32 used_bytes | u32 magic "GCP1"
//     +16 u16 dir[n_recs]: start of record j / 16;  records from 16 + align16(2 n_recs) on, each 16-byte aligned
//   record (size a multiple of 16, at most GCI_PAGE_MAX_REC = 1024 bytes):
//     +0  u32 size                       (BAM: block_size)
//     +4  refID, pos, l_read_name, mapq  (as in BAM)
//     +14 u16 kind                       (BAM: bin)       1 = CIGAR in the blob, 2 = whole record in the blob, 4 = malformed
//     +16 n_cigar_op, flag, l_seq        (as in BAM)
//     +24 u32 aux_len                    (BAM: next_refID)
//     +28 u64 blob offset, from the buffer start   (BAM: next_pos, tlen)
//     +36 read_name, zero padded so that the CIGAR starts at align16(36 + l_read_name); the CIGAR zero padded to 16
//         bytes (a zero word is "0M": it adds nothing to any total); the aux bytes behind it; zero padded to 16.
//   A record that does not fit 1024 bytes keeps its CIGAR words in the blob (kind 1: ONT reads, 10^3 - 10^5 operations,
//   summed chunk by chunk by k_cigar_chunks anyway; 16 bytes with the first operation stand in for them); one that still does not fit (a CG:B,I tag, long Z tags) leaves its
//   48-byte core in the page and its bytes -- the heads form: the record without SEQ / QUAL -- in the blob (kind 2).
//   No record straddles a page, nothing in a page needs the offset table, every CIGAR is 16-byte aligned: the filter
//   loads a page with one round of coalesced 16-byte loads and parses it out of LDS.
//
// Page assignment without a serial packing pass: with cost_i = size_i + 2 (the directory entry) and S = exclusive scan
// of the costs, record i goes to page floor(S_i / Q), Q = page_bytes - 1024 - 48 -- whatever starts inside a quantum
// fits its page, because only the last record can reach beyond it, by less than 1026 bytes.
#include "gci_ctx.hpp"

#define PG_MAX_REC GCI_PAGE_MAX_REC
#define PG_MAGIC 0x31504347u
#define PG_EXT 1u
#define PG_OVERSIZE 2u
#define PG_MALFORMED 4u

__device__ __forceinline__ uint32_t a16(uint32_t x) { return (x + 15u) & ~15u; }

__device__ __forceinline__ uint32_t pg_rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ uint32_t pg_rd32(const uint8_t* p) { return pg_rd16(p) | (pg_rd16(p + 2) << 16); }

struct PgRec {
    uint32_t kind, size, blob;          // blob: bytes of the blob this record takes (a multiple of 16)
    uint32_t lrn, n_cig, aux_len;
    uint64_t aux_off;                   // in the source stream
    bool short_core;                    // fewer than 36 bytes of the record lie inside the stream
};

// What a record takes in the page format; the conditions under which the stream filter reports GCI_E_MALFORMED
// (k_filter.hip) make it a malformed stub here.
__device__ __forceinline__ PgRec pg_measure(const uint8_t* __restrict__ bam, uint64_t n_bytes, uint64_t off, bool has_seq)
{
    PgRec r;
    r.kind = PG_MALFORMED; r.size = 48; r.blob = 0; r.lrn = r.n_cig = r.aux_len = 0; r.aux_off = 0; r.short_core = false;
    if (off + 36 > n_bytes) { r.short_core = true; return r; }
    const uint8_t* p = bam + off;
    const int32_t block_size = (int32_t)pg_rd32(p);
    const uint32_t lrn = p[12], n_cig = pg_rd16(p + 16);
    const int32_t l_seq = (int32_t)pg_rd32(p + 20);
    const uint64_t rec_end = off + 4 + (uint64_t)(uint32_t)block_size;
    const uint64_t aux_off = off + 36 + lrn + 4ull * n_cig + (has_seq ? (((uint64_t)(uint32_t)l_seq + 1) >> 1) + (uint64_t)(uint32_t)l_seq : 0ull);
    if (block_size < 32 || rec_end > n_bytes || l_seq < 0 || aux_off > rec_end) return r;
    r.lrn = lrn; r.n_cig = n_cig; r.aux_off = aux_off;
    const uint64_t aux_len = rec_end - aux_off;
    const uint32_t cig_at = a16(36 + lrn);
    if (aux_len <= PG_MAX_REC && 4ull * n_cig <= PG_MAX_REC && a16(cig_at + a16(4 * n_cig) + (uint32_t)aux_len) <= PG_MAX_REC) {
        r.kind = 0; r.size = a16(cig_at + a16(4 * n_cig) + (uint32_t)aux_len); r.aux_len = (uint32_t)aux_len;
    } else if (aux_len <= PG_MAX_REC && a16(cig_at + 16 + (uint32_t)aux_len) <= PG_MAX_REC) {
        r.kind = PG_EXT; r.size = a16(cig_at + 16 + (uint32_t)aux_len); r.blob = a16(4 * n_cig); r.aux_len = (uint32_t)aux_len;
    } else {
        r.kind = PG_OVERSIZE; r.size = 48; r.aux_len = (uint32_t)aux_len;
        r.blob = (uint32_t)((36 + lrn + 4ull * n_cig + aux_len + 15ull) & ~15ull);
    }
    return r;
}

// The two levels of the size pass's sums (k_pg_measure, below)
struct PgSums { const uint32_t* S_loc; const unsigned long long* B_loc; const unsigned long long* blk; uint32_t nb; };   // blk: [0, nb) costs, [nb, 2 nb) blob
__device__ __forceinline__ unsigned long long pg_S(const PgSums& s, uint32_t i) { return s.S_loc[i] + s.blk[i / TILE]; }
__device__ __forceinline__ unsigned long long pg_B(const PgSums& s, uint32_t i) { return s.B_loc[i] + s.blk[s.nb + i / TILE]; }

// page_first[k] = first record whose cost offset is >= k * Q (k = n_pages: n_rec); page_off[k] = where that record starts in the
// stream (k = n_pages: n_bytes), which is all the page writer needs to ask for a page's bytes
__global__ __launch_bounds__(BLOCK) void k_pg_first(const PgSums S, uint32_t n_rec, uint32_t n_pages, uint32_t Q,
                                                    const uint64_t* __restrict__ rec_off, uint64_t n_bytes,
                                                    uint32_t* __restrict__ page_first, uint64_t* __restrict__ page_off)
{
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k > n_pages) return;
    if (k == n_pages) { page_first[k] = n_rec; page_off[k] = n_bytes; return; }
    const unsigned long long want = (unsigned long long)k * Q;
    uint32_t lo = 0, hi = n_rec;                                 // first i in [0, n_rec] with S[i] >= want
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (pg_S(S, mid) >= want) hi = mid; else lo = mid + 1; }
    page_first[k] = lo;
    page_off[k] = lo < n_rec ? rec_off[lo] : n_bytes;
}

// the naturally aligned dword at address q of the stream [bam, end); bytes past the end read as zero
__device__ __forceinline__ uint32_t pg_ldw(const uint8_t* q, const uint8_t* end)
{
    if (q + 4 <= end) return *reinterpret_cast<const uint32_t*>(q);
    uint32_t w = 0;
    for (int b = 0; b < 4; b++) if (q + b < end) w |= (uint32_t)q[b] << (8 * b);
    return w;
}

// dword d of the `len` bytes that start at stream offset `src` (any alignment); bytes beyond len read as zero.  Two naturally
// aligned loads re-aligned in registers (an unaligned vector load from global memory is ~100x slower on gfx950).
__device__ __forceinline__ uint32_t pg_src_dword(const uint8_t* __restrict__ bam, uint64_t n_bytes, uint64_t src, uint32_t len, uint32_t d)
{
    const uint8_t* p = bam + src + 4ull * d;
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
    const uint8_t* end = bam + n_bytes;
    const uint32_t lo = pg_ldw(p - sh, end);
    const uint32_t hi = sh ? pg_ldw(p - sh + 4, end) : 0u;
    uint32_t w = __builtin_amdgcn_alignbyte(hi, lo, sh);
    const uint32_t left = len - 4u * d;
    if (left < 4u) w &= (1u << (8u * left)) - 1u;
    return w;
}

struct PgArgs {
    const uint8_t* bam; uint64_t n_bytes; const uint64_t* rec_off; uint32_t n_rec; int has_seq;
    PgSums sums; const uint32_t* page_first; const uint64_t* page_off;
    uint32_t n_pages, page_bytes; uint64_t blob_off; uint8_t* out;
};

// What the copy phase needs of a record, left in LDS by the thread that measured it: where its three runs of bytes lie in the stream
// (name + CIGAR directly behind the core, aux behind SEQ / QUAL) and where they go in the page.
struct PgMeta {
    uint64_t off, aux_off;
    uint16_t n_cig, aux_len, at;       // (aux_len <= 1024 for the kinds that are copied, n_cig is 16 bits in BAM, at < page_bytes <= 32768)
    uint8_t lrn, kind;                 // kind | PG_IN_* : which of the runs lie in the window
};
#define PG_IN_NAME 0x10u
#define PG_IN_CIGAR 0x20u
#define PG_IN_AUX 0x40u
static_assert(sizeof(PgMeta) == 24, "PgMeta");
#define PG_META_MAX 128                // records measured at a time (a page of 24 KiB holds ~58 HiFi records; tiny records: several passes)

// What pg_measure() says of a record, from its 36 core bytes already in registers as nine dwords.
__device__ __forceinline__ PgRec pg_classify(const uint32_t core[9], uint64_t n_bytes, uint64_t off, bool has_seq)
{
    PgRec r;
    r.kind = PG_MALFORMED; r.size = 48; r.blob = 0; r.lrn = r.n_cig = r.aux_len = 0; r.aux_off = 0; r.short_core = false;
    const int32_t block_size = (int32_t)core[0];
    const uint32_t lrn = core[3] & 0xFFu, n_cig = core[4] & 0xFFFFu;
    const int32_t l_seq = (int32_t)core[5];
    const uint64_t rec_end = off + 4 + (uint64_t)(uint32_t)block_size;
    const uint64_t aux_off = off + 36 + lrn + 4ull * n_cig + (has_seq ? (((uint64_t)(uint32_t)l_seq + 1) >> 1) + (uint64_t)(uint32_t)l_seq : 0ull);
    if (block_size < 32 || rec_end > n_bytes || l_seq < 0 || aux_off > rec_end) return r;
    r.lrn = lrn; r.n_cig = n_cig; r.aux_off = aux_off;
    const uint64_t aux_len = rec_end - aux_off;
    const uint32_t cig_at = a16(36 + lrn);
    if (aux_len <= PG_MAX_REC && 4ull * n_cig <= PG_MAX_REC && a16(cig_at + a16(4 * n_cig) + (uint32_t)aux_len) <= PG_MAX_REC) {
        r.kind = 0; r.size = a16(cig_at + a16(4 * n_cig) + (uint32_t)aux_len); r.aux_len = (uint32_t)aux_len;
    } else if (aux_len <= PG_MAX_REC && a16(cig_at + 16 + (uint32_t)aux_len) <= PG_MAX_REC) {
        r.kind = PG_EXT; r.size = a16(cig_at + 16 + (uint32_t)aux_len); r.blob = a16(4 * n_cig); r.aux_len = (uint32_t)aux_len;
    } else {
        r.kind = PG_OVERSIZE; r.size = 48; r.aux_len = (uint32_t)aux_len;
        r.blob = (uint32_t)((36 + lrn + 4ull * n_cig + aux_len + 15ull) & ~15ull);
    }
    return r;
}

// The 36 core bytes of the record at stream offset off (off + 36 <= n_bytes) from naturally aligned dword loads (the byte loads of
// pg_measure() are a dozen memory instructions per record): 10 aligned dwords re-aligned in registers.
__device__ __forceinline__ void pg_core_gather(const uint8_t* __restrict__ bam, uint64_t n_bytes, uint64_t off, uint32_t core[9])
{
    const uint8_t* p = bam + off;
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
    const uint8_t* end = bam + n_bytes;
    uint32_t w[10];
#pragma unroll
    for (int d = 0; d < 10; d++) w[d] = (d < 9 || sh) ? pg_ldw(p - sh + 4 * d, end) : 0u;
#pragma unroll
    for (int d = 0; d < 9; d++) core[d] = __builtin_amdgcn_alignbyte(w[d + 1], w[d], sh);
}

// a dword at any byte address of LDS (gfx950 serves an unaligned ds_read_b32: tools/hwtests/lds_unaligned.hip)
__device__ __forceinline__ uint32_t pg_lds32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }

// The size pass: S = exclusive sums of the costs (size + 2), B = exclusive sums of the blob bytes, over all records and with the totals
// at index n_rec.  Kept in two levels, never added up in memory: k_pg_measure measures TILE records per workgroup and leaves the sums
// LOCAL to the workgroup (the cost sums fit 32 bits) and both totals of it, k_pg_blk_scan -- one workgroup -- turns the totals into what
// lies in front of every workgroup; pg_S / pg_B add the two.  (Before: the costs and blob bytes written out as arrays, a two-kernel
// scan over each, 64-bit sums read and written once more to add the block prefixes: 5 launches and ~0.5 GB of traffic per HiFi file.)
// grid: n_rec / TILE + 1 workgroups (index n_rec, the totals, is an entry like any other: a record that costs nothing)
__global__ __launch_bounds__(BLOCK) void k_pg_measure(const uint8_t* __restrict__ bam, uint64_t n_bytes, const uint64_t* __restrict__ rec_off,
                                                      uint32_t n_rec, int has_seq, uint32_t* __restrict__ S_loc,
                                                      unsigned long long* __restrict__ B_loc, unsigned long long* __restrict__ blk_tot, uint32_t nb)
{
    __shared__ uint16_t s_cost[TILE];                                       // (a cost is at most 1026)
    __shared__ uint32_t s_blob[TILE];
    __shared__ unsigned long long wtot[2][BLOCK / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t base0 = blockIdx.x * TILE;
    // a lane per record, neighbours in neighbouring lanes
    // (byte loads: pg_core_gather's ten aligned dwords were measured SLOWER here -- 0.181 against 0.155 ms per quarter genome for the size
    //  pass: every lane its own cache line, and the dozen byte loads of a lane hit that one line)
    for (uint32_t r = 0; r < TILE / BLOCK; r++) {
        const uint32_t e = r * BLOCK + t, i = base0 + e;
        uint32_t c = 0, b = 0;
        if (i < n_rec) {
            const PgRec rec = pg_measure(bam, n_bytes, rec_off[i], has_seq != 0);
            c = rec.size + 2u; b = rec.blob;
        }
        s_cost[e] = (uint16_t)c; s_blob[e] = b;
    }
    __syncthreads();
    // the exclusive sums inside the workgroup: TILE / BLOCK consecutive records per thread
    constexpr int PER = TILE / BLOCK;
    uint32_t c[PER], b[PER];
    uint32_t run_c = 0;
    unsigned long long run_b = 0;
#pragma unroll
    for (int i = 0; i < PER; i++) { c[i] = s_cost[t * PER + i]; b[i] = s_blob[t * PER + i]; run_c += c[i]; run_b += b[i]; }
    const uint32_t inc_c = wave_inclusive<uint32_t>(run_c, lane);
    const unsigned long long inc_b = wave_inclusive<unsigned long long>(run_b, lane);
    if (lane == 63) { wtot[0][wave] = inc_c; wtot[1][wave] = inc_b; }
    __syncthreads();
    uint32_t pre_c = inc_c - run_c, all_c = 0;
    unsigned long long pre_b = inc_b - run_b, all_b = 0;
#pragma unroll
    for (uint32_t w = 0; w < BLOCK / 64; w++) {
        if (w < wave) { pre_c += (uint32_t)wtot[0][w]; pre_b += wtot[1][w]; }
        all_c += (uint32_t)wtot[0][w]; all_b += wtot[1][w];
    }
    const uint32_t base = base0 + t * PER;
#pragma unroll
    for (int i = 0; i < PER; i++) {
        if (base + i <= n_rec) { S_loc[base + i] = pre_c; B_loc[base + i] = pre_b; }
        pre_c += c[i]; pre_b += b[i];
    }
    if (t == 0) { blk_tot[blockIdx.x] = all_c; blk_tot[nb + blockIdx.x] = all_b; }
}

// One workgroup: both rows of workgroup totals into exclusive sums, in place; then what the host reads back:
// tot[0] = S[n_rec - 1], tot[1] = S[n_rec], tot[2] = B[n_rec].
__global__ __launch_bounds__(BLOCK) void k_pg_blk_scan(unsigned long long* __restrict__ blk, uint32_t nb, const uint32_t* __restrict__ S_loc,
                                                       const unsigned long long* __restrict__ B_loc, uint32_t n_rec,
                                                       unsigned long long* __restrict__ tot)
{
    __shared__ unsigned long long wtot[2][BLOCK / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned long long carry_c = 0, carry_b = 0;
    for (uint32_t k0 = 0; k0 < nb; k0 += BLOCK) {
        const uint32_t k = k0 + t;
        const unsigned long long vc = k < nb ? blk[k] : 0ull, vb = k < nb ? blk[nb + k] : 0ull;
        const unsigned long long ic = wave_inclusive<unsigned long long>(vc, lane), ib = wave_inclusive<unsigned long long>(vb, lane);
        if (lane == 63) { wtot[0][wave] = ic; wtot[1][wave] = ib; }
        __syncthreads();
        unsigned long long pc = carry_c + ic - vc, pb = carry_b + ib - vb;
#pragma unroll
        for (uint32_t w = 0; w < BLOCK / 64; w++) {
            if (w < wave) { pc += wtot[0][w]; pb += wtot[1][w]; }
            carry_c += wtot[0][w]; carry_b += wtot[1][w];
        }
        if (k < nb) { blk[k] = pc; blk[nb + k] = pb; }
        __syncthreads();                                           // (wtot is written again; the sums are read below)
    }
    if (t == 0) {
        const PgSums s = {S_loc, B_loc, blk, nb};
        tot[0] = pg_S(s, n_rec - 1); tot[1] = pg_S(s, n_rec); tot[2] = pg_B(s, n_rec);
    }
}

// The window: the piece of the stream a workgroup staged in LDS with coalesced 16-byte loads (k_pg_write, below).
struct PgWin { const uint8_t* lds; const uint8_t* lo; const uint8_t* hi; };     // LDS copy of the stream addresses [lo, hi); lo 16-byte aligned

__device__ __forceinline__ bool pg_in_win(const PgWin& W, const uint8_t* p, uint32_t len) { return p >= W.lo && p + len <= W.hi; }

// Sixteen bytes of the run of `len` bytes at stream offset src, from byte roff of it on (a multiple of 4); bytes beyond the run are
// zero.  From the window, four ds_read_b32 at any byte alignment (up to 15 bytes behind the run are read and dropped: the window has
// that much slack), or gathered from memory: two naturally aligned dwords per dword, re-aligned in registers.
__device__ __forceinline__ uint4 pg_piece(const uint8_t* __restrict__ bam, uint64_t n_bytes, const PgWin& W, bool in_win, uint64_t src,
                                          uint32_t len, uint32_t roff)
{
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (roff >= len) return make_uint4(0, 0, 0, 0);
    if (in_win) {
        const uint8_t* q = W.lds + (uint32_t)(bam + src - W.lo) + roff;
        const uint32_t left = len - roff;
#pragma unroll
        for (int d = 0; d < 4; d++) {
            w[d] = pg_lds32(q + 4 * d);
            if (left < 4u * d + 4u) w[d] = left > 4u * d ? w[d] & ((1u << (8u * (left - 4u * d))) - 1u) : 0u;
        }
    } else {
#pragma unroll
        for (int d = 0; d < 4; d++) if (roff + 4u * d < len) w[d] = pg_src_dword(bam, n_bytes, src, len, roff / 4u + d);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

#ifndef PG_BLOCK
#define PG_BLOCK BLOCK                 // threads of a k_pg_write workgroup
#endif
// The window: in a heads stream the records of a page are one contiguous piece of the stream, never longer than the page (the page
// image of an inline record is not smaller than its source), so the workgroup copies that piece into LDS with one round of coalesced
// 16-byte loads and takes cores, names, CIGARs and aux blocks from there.  Its capacity is page_bytes / PG_WIN_DIV.  A page takes as
// many fills as it needs: each starts at its first record that is still to do and ends before the first record that starts behind
// what was loaded.
#ifndef PG_WIN_DIV
#define PG_WIN_DIV 1
#endif
#define PG_WIN_SLACK 16u               // readable bytes behind the window (the dropped tail of a run's last piece)
#define PG_WIN_REGS (8 / PG_WIN_DIV)   // 16-byte pieces of a window per thread
static_assert(GCI_PAGE_MAX_BYTES / PG_WIN_DIV <= PG_WIN_REGS * PG_BLOCK * 16, "a thread holds its share of a whole window in registers");
static inline __host__ __device__ uint32_t pg_win_cap(uint32_t page_bytes) { return (page_bytes / PG_WIN_DIV) & ~15u; }

// the window for records from stream offset off0 on, none of them expected behind span_end (<= n_bytes): empty when that lies below
// off0.  Whole 16-byte pieces that lie inside the stream only -- no load touches a byte outside [bam, end) -- so what a record has in
// the stream's first or last, partial, piece is not in the window and is gathered.
// whole_only: a span longer than the window gets none (the table says before any load that the page cannot be staged: a whole
// stream with SEQ / QUAL, ONT -- its records are gathered, and the window's bytes would have been loaded for nothing)
__device__ __forceinline__ PgWin pg_win_of(const uint8_t* lds, const uint8_t* bam, const uint8_t* end, uint64_t off0, uint64_t span_end, uint32_t cap,
                                           bool whole_only = false)
{
    PgWin W;
    W.lds = lds; W.lo = W.hi = bam;
    if (off0 < span_end) {
        const uint8_t* p0 = bam + off0;
        const uint8_t* lo = p0 - ((uintptr_t)p0 & 15u);            // (the ADDRESS rounded down: the stream pointer need not be aligned)
        if (lo < bam) lo += 16;
        const uint8_t* last = bam + span_end + 15;
        const uint8_t* hi = last - ((uintptr_t)last & 15u);
        if (hi > end) hi = end - ((uintptr_t)end & 15u);
        if (hi > lo && !(whole_only && (uint64_t)(hi - lo) > cap)) { W.lo = lo; W.hi = (uint64_t)(hi - lo) < cap ? hi : lo + cap; }
    }
    return W;
}
// a thread's pieces of the window: all of them requested before any is used ...
__device__ __forceinline__ void pg_win_load(const PgWin& W, uint32_t t, uint4 v[PG_WIN_REGS])
{
    const uint32_t pieces = (uint32_t)(W.hi - W.lo) / 16u;
#pragma unroll
    for (int u = 0; u < PG_WIN_REGS; u++) {
        const uint32_t i = u * PG_BLOCK + t;
        v[u] = i < pieces ? reinterpret_cast<const uint4*>(W.lo)[i] : make_uint4(0, 0, 0, 0);
    }
}
// ... and put into LDS
__device__ __forceinline__ void pg_win_store(uint8_t* win, const PgWin& W, uint32_t t, const uint4 v[PG_WIN_REGS])
{
    const uint32_t pieces = (uint32_t)(W.hi - W.lo) / 16u;
#pragma unroll
    for (int u = 0; u < PG_WIN_REGS; u++) {
        const uint32_t i = u * PG_BLOCK + t;
        if (i < pieces) reinterpret_cast<uint4*>(win)[i] = v[u];
    }
}

// What a workgroup must know of a page before it can ask for the page's bytes (k_pg_first left it in two tables).
struct PgPage { uint32_t first, cnt; uint64_t off0, span_end; };
__device__ __forceinline__ PgPage pg_page_of(const PgArgs& A, uint32_t k)
{
    PgPage p;
    p.first = A.page_first[k]; p.cnt = A.page_first[k + 1] - p.first;
    p.off0 = A.page_off[k];
    // the stream offset no record of this page is expected behind: it only bounds the window (the table need not be ascending)
    p.span_end = A.page_off[k + 1];
    if (p.span_end > A.n_bytes) p.span_end = A.n_bytes;
    return p;
}
// ... and of its records before it can measure them: offset and cost offset of record t of the page, the cost offsets of its first
// record and behind its last
struct PgMine { uint64_t off; unsigned long long S, S0, S_end; };
__device__ __forceinline__ PgMine pg_mine_of(const PgArgs& A, const PgPage& p, uint32_t t)
{
    PgMine m;
    m.off = 0; m.S = 0;
    if (t < p.cnt && t < PG_META_MAX) { m.off = A.rec_off[p.first + t]; m.S = pg_S(A.sums, p.first + t); }
    m.S0 = p.cnt ? pg_S(A.sums, p.first) : 0ull;
    m.S_end = p.cnt ? pg_S(A.sums, p.first + p.cnt) : 0ull;
    return m;
}

// A workgroup writes pages blockIdx.x, + gridDim.x, ... and is one page ahead with its loads: while it composes page k out of LDS, the
// window of page k + gridDim.x and that page's offsets are on their way into registers, and the two table entries of the page behind
// it are being fetched -- a page's three dependent trips to memory (page tables -> offsets and window -> bytes) are each one page old
// when their result is needed.
//
// There is no image of the page in LDS: the page is composed 16 bytes at a time, a thread per PIECE, and stored straight to memory.
// Everything in a record's image from byte 48 on is a 16-byte aligned copy of sixteen bytes of ONE of its runs (the CIGAR and the aux
// block start at multiples of 16, the name at 36), so a piece is: which record (a byte per piece, left by the thread that measured
// the record), which run, four dwords out of the window.  A record's first 48 bytes -- the patched core and the first twelve bytes of
// the name -- are put together by the thread that measures it.  (Composed dword by dword by eight lanes per record into an image in
// LDS, the kernel was bound by the instructions it issued: ~60 per dword.)
#ifndef PG_PERSIST
#define PG_PERSIST 1                   // 0: a workgroup per page, nothing fetched ahead
#endif
#ifndef PG_WAVES
#define PG_WAVES 4                     // waves per SIMD the registers are cut to: 4 workgroups per CU, what the LDS allows too (3 without: 146 VGPRs)
#endif
//
// With a list (`listed`, its length read here from *n_listed) the pages are the listed ones -- those the lean writer below left --
// instead of all of them.  Workgroup 0 also writes the 16 zero bytes behind the blob (`guard`).
__global__ __launch_bounds__(PG_BLOCK) __attribute__((amdgpu_waves_per_eu(PG_WAVES, PG_WAVES))) void k_pg_write(const PgArgs A, const uint32_t* __restrict__ n_listed,
                                                                                                                const uint32_t* __restrict__ listed, uint8_t* __restrict__ guard)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t win[];              // the window
    // which records of the page leave something in the blob (nearly none of a HiFi file): the pass over the blob below looks
    // at those only -- measuring every record again there, one after the other by the whole workgroup, was 60 dependent trips
    // to memory per page and most of this kernel's time
    __shared__ uint16_t s_blob_rec[GCI_PAGE_MAX_BYTES / 48];
    __shared__ uint32_t s_n_blob, s_take, s_sparse;
    __shared__ PgMeta s_meta[PG_META_MAX];
    __shared__ __attribute__((aligned(16))) uint32_t s_core[PG_META_MAX][12];           // a record's first 48 bytes in the page
    __shared__ uint8_t s_map[GCI_PAGE_MAX_BYTES / 16];                                  // piece of the page -> record of the fill
    __shared__ __attribute__((aligned(16))) uint8_t s_head[16 + ((2 * ((GCI_PAGE_MAX_BYTES - 16) / 50) + 15) & ~15)];   // header and directory
    const uint32_t t = threadIdx.x, G = gridDim.x;
    const uint32_t P = A.page_bytes;
    const uint32_t win_cap = pg_win_cap(P);
    const uint8_t* end = A.bam + A.n_bytes;
    const PgPage none = {0u, 0u, 0ull, 0ull};

    if (blockIdx.x == 0 && t < 16) guard[t] = 0;
    const uint32_t n_items = listed ? *n_listed : A.n_pages;
    uint32_t it = blockIdx.x;                                      // item `it` is page listed[it], or page `it`
    if (it >= n_items) return;
    uint32_t k = listed ? listed[it] : it;
    uint32_t k_after = it + G < n_items ? (listed ? listed[it + G] : it + G) : 0u;
    PgPage p_next = pg_page_of(A, k);
    PgPage p_after = it + G < n_items ? pg_page_of(A, k_after) : none;
    PgWin W_next = pg_win_of(win, A.bam, end, p_next.off0, p_next.span_end, win_cap, true);
    uint4 v[PG_WIN_REGS];
    pg_win_load(W_next, t, v);
    PgMine m_next = pg_mine_of(A, p_next, t);

    uint32_t k_next = 0u;
    for (; it < n_items; it += G, k = k_next) {
        const PgPage pg = p_next;
        const PgMine mine = m_next;
        const PgWin W0 = W_next;
        const uint32_t first = pg.first, cnt = pg.cnt;
        const unsigned long long S0 = mine.S0;
        const uint32_t rec0 = 16u + a16(2u * cnt);
        const uint32_t used = cnt ? rec0 + (uint32_t)(mine.S_end - S0) - 2u * cnt : 16u;
        uint4* const g = reinterpret_cast<uint4*>(A.out + (uint64_t)k * P);
        pg_win_store(win, W0, t, v);
        if (t < sizeof(s_head) / 16) reinterpret_cast<uint4*>(s_head)[t] = make_uint4(0, 0, 0, 0);
        if (t == 0) {
            s_n_blob = 0;
            uint32_t* h = reinterpret_cast<uint32_t*>(s_head);
            h[0] = cnt; h[1] = first; h[2] = used; h[3] = PG_MAGIC;
        }
        // ---- the loads of the pages behind this one
        p_next = p_after;
        if (it + G < n_items) {
            W_next = pg_win_of(win, A.bam, end, p_next.off0, p_next.span_end, win_cap, true);
            pg_win_load(W_next, t, v);
            m_next = pg_mine_of(A, p_next, t);
        }
        const bool two_on = (uint64_t)it + 2ull * G < n_items;
        k_next = k_after;
        k_after = two_on ? (listed ? listed[it + 2 * G] : it + 2 * G) : 0u;
        p_after = two_on ? pg_page_of(A, k_after) : none;

        if (cnt == 0) __syncthreads();
        for (uint32_t m0 = 0; m0 < cnt;) {
            const uint32_t mc = cnt - m0 < PG_META_MAX ? cnt - m0 : PG_META_MAX;
            // ---- the window of this fill: from the address of record m0 rounded down to 16 bytes.  The page's first fill came with
            // the page; a later one is loaded here and waited for.
            uint64_t off0 = pg.off0, off = mine.off;
            unsigned long long Si = mine.S;
            PgWin W = W0;
            if (m0) {
                off0 = A.rec_off[first + m0];
                W = pg_win_of(win, A.bam, end, off0, pg.span_end, win_cap);
                uint4 w[PG_WIN_REGS];
                pg_win_load(W, t, w);
                if (t < mc) { off = A.rec_off[first + m0 + t]; Si = pg_S(A.sums, first + m0 + t); }
                pg_win_store(win, W, t, w);
            }
            if (t == 0) { s_take = mc; s_sparse = 0u; }
            __syncthreads();
            // ---- phase A: one thread per record measures it (its core from the window, or 10 aligned dwords from memory), leaves
            // what the pieces need in LDS: the record's first 48 bytes, its directory entry, where its runs lie, its pieces in the map
            uint32_t my_blob = 0;
            if (t < mc) {
                const uint32_t j = m0 + t, i = first + j;
                uint32_t core[12];
                PgRec r;
                bool core_in = false;
                if (off + 36 > A.n_bytes) {
#pragma unroll
                    for (int d = 0; d < 9; d++) core[d] = 0u;
                    r.kind = PG_MALFORMED; r.size = 48; r.blob = 0; r.lrn = r.n_cig = r.aux_len = 0; r.aux_off = 0; r.short_core = true;
                    core_in = true;
                } else {
                    const uint8_t* p = A.bam + off;
                    core_in = pg_in_win(W, p, 36);
                    if (core_in) {
#pragma unroll
                        for (int d = 0; d < 9; d++) core[d] = pg_lds32(win + (uint32_t)(p - W.lo) + 4 * d);
                    } else {
                        pg_core_gather(A.bam, A.n_bytes, off, core);
                    }
                    r = pg_classify(core, A.n_bytes, off, A.has_seq != 0);
                }
                const bool copied = r.kind == 0 || r.kind == PG_EXT;
                const uint32_t cig_len = r.kind == 0 ? 4u * r.n_cig : r.n_cig ? 4u : 0u;    // kind 1: the first operation stays visible in the page
                uint32_t in = 0;
                if (copied) {
                    if (pg_in_win(W, A.bam + off + 36, r.lrn)) in |= PG_IN_NAME;
                    if (pg_in_win(W, A.bam + off + 36 + r.lrn, cig_len)) in |= PG_IN_CIGAR;
                    if (pg_in_win(W, A.bam + r.aux_off, r.aux_len)) in |= PG_IN_AUX;
                }
                // where the fill ends: a fill's first record that reaches out of its window says that the stream is not a run of
                // small records (ONT, SEQ / QUAL in between, a table out of order): the whole batch is then done from this one fill,
                // by the gather.  Otherwise the fill ends before the first record whose core lies behind the window.
                if (t == 0) { if (!core_in || (copied && in != (PG_IN_NAME | PG_IN_CIGAR | PG_IN_AUX))) s_sparse = 1u; }
                else if (off >= off0 && A.bam + off + 36 > W.hi) atomicMin(&s_take, t);
                const uint32_t at = rec0 + (uint32_t)(Si - S0) - 2u * j;
                const uint64_t blob_at = r.blob ? A.blob_off + pg_B(A.sums, i) : 0ull;
                my_blob = r.blob;
                *reinterpret_cast<uint16_t*>(s_head + 16 + 2 * j) = (uint16_t)(at >> 4);
                core[0] = r.size;
                core[3] = (core[3] & 0xFFFFu) | (r.kind << 16);
                core[6] = r.aux_len; core[7] = (uint32_t)blob_at; core[8] = (uint32_t)(blob_at >> 32);
                if (r.kind == PG_MALFORMED) core[6] = core[7] = core[8] = 0u;
                // the first twelve bytes of the name
                const uint4 nm = copied ? pg_piece(A.bam, A.n_bytes, W, (in & PG_IN_NAME) != 0, off + 36, r.lrn, 0) : make_uint4(0, 0, 0, 0);
                core[9] = nm.x; core[10] = nm.y; core[11] = nm.z;
#pragma unroll
                for (int d = 0; d < 12; d += 4) *reinterpret_cast<uint4*>(&s_core[t][d]) = make_uint4(core[d], core[d + 1], core[d + 2], core[d + 3]);
                for (uint32_t q = 0; q < r.size / 16u; q++) s_map[(at >> 4) + q] = (uint8_t)t;
                PgMeta mt;
                mt.off = off; mt.aux_off = r.aux_off; mt.lrn = (uint8_t)r.lrn; mt.n_cig = (uint16_t)r.n_cig;
                mt.aux_len = (uint16_t)(r.aux_len <= PG_MAX_REC ? r.aux_len : 0u);
                mt.at = (uint16_t)at; mt.kind = (uint8_t)(r.kind | in);
                s_meta[t] = mt;
            }
            __syncthreads();
            // (records from `take` on are measured again by the next fill)
            const uint32_t take = __builtin_amdgcn_readfirstlane(s_sparse ? mc : s_take);
            if (t < take && my_blob) s_blob_rec[atomicAdd(&s_n_blob, 1u)] = (uint16_t)(m0 + t);
            // ---- phase B: the pieces of the records of this fill, a thread per piece, straight to memory
            const uint32_t piece_lo = s_meta[0].at >> 4;
            const uint32_t piece_hi = m0 + take == cnt ? used >> 4 : take < mc ? s_meta[take].at >> 4
                                                                               : (rec0 + (uint32_t)(pg_S(A.sums, first + m0 + take) - S0) - 2u * (m0 + take)) >> 4;
            for (uint32_t piece = piece_lo + t; piece < piece_hi; piece += PG_BLOCK) {
                const uint32_t jj = s_map[piece];
                const PgMeta mt = s_meta[jj];
                const uint32_t q = 16u * piece - mt.at, kind = mt.kind & 0xFu;
                uint4 o;
                if (q < 48u) o = *reinterpret_cast<const uint4*>(&s_core[jj][q / 4u]);
                else {
                    const uint32_t c = a16(36u + mt.lrn), c2 = c + (kind == 0 ? a16(4u * mt.n_cig) : 16u);
                    if (q < c) o = pg_piece(A.bam, A.n_bytes, W, (mt.kind & PG_IN_NAME) != 0, mt.off + 36, mt.lrn, q - 36u);
                    else if (q < c2) o = pg_piece(A.bam, A.n_bytes, W, (mt.kind & PG_IN_CIGAR) != 0, mt.off + 36 + mt.lrn,
                                                  kind == 0 ? 4u * mt.n_cig : mt.n_cig ? 4u : 0u, q - c);
                    else o = pg_piece(A.bam, A.n_bytes, W, (mt.kind & PG_IN_AUX) != 0, mt.aux_off, mt.aux_len, q - c2);
                }
                g[piece] = o;
            }
            __syncthreads();                                       // (the tables and the window are reused by the next fill)
            m0 += take;
        }
        // ---- header and directory; zeros behind the last record
        for (uint32_t piece = t; piece < rec0 / 16u; piece += PG_BLOCK) g[piece] = reinterpret_cast<const uint4*>(s_head)[piece];
        for (uint32_t piece = (used >> 4) + t; piece < P / 16u; piece += PG_BLOCK) g[piece] = make_uint4(0, 0, 0, 0);
        // what the page leaves in the blob: CIGAR words (kind 1) or heads-form records (kind 2), record after record, all threads
        const uint32_t n_blob = s_n_blob;                            // (written before the last barrier)
        for (uint32_t b = 0; b < n_blob; b++) {
            const uint32_t i = first + s_blob_rec[b];
            const uint64_t off = A.rec_off[i];
            const PgRec r = pg_measure(A.bam, A.n_bytes, off, A.has_seq != 0);         // (uniform over the workgroup)
            if (!r.blob) continue;
            uint32_t* o = reinterpret_cast<uint32_t*>(A.out + A.blob_off + pg_B(A.sums, i));
            if (r.kind == PG_EXT) {
                for (uint32_t d = t; d < r.blob / 4; d += PG_BLOCK)
                    o[d] = d < r.n_cig ? pg_src_dword(A.bam, A.n_bytes, off + 36 + r.lrn, 4 * r.n_cig, d) : 0u;
            } else {
                // heads form: core (block_size shortened), name + CIGAR (contiguous in the stream), aux (behind SEQ / QUAL there)
                const uint32_t head = 36 + r.lrn + 4 * r.n_cig, total = head + r.aux_len;
                for (uint32_t d = t; d < r.blob / 4; d += PG_BLOCK) {
                    uint32_t w = 0;
                    const uint32_t b0 = 4 * d;
                    if (b0 + 4 <= head) w = pg_src_dword(A.bam, A.n_bytes, off, head, d);
                    else if (b0 >= head) { if (b0 < total) w = pg_src_dword(A.bam, A.n_bytes, r.aux_off + (b0 - head), total - b0, 0); }
                    else {                                             // the dword that holds the seam
                        for (uint32_t x0 = 0; x0 < 4 && b0 + x0 < total; x0++) {
                            const uint32_t x = b0 + x0;
                            w |= (uint32_t)(x < head ? A.bam[off + x] : A.bam[r.aux_off + (x - head)]) << (8 * x0);
                        }
                    }
                    if (d == 0) w = total - 4;
                    o[d] = w;
                }
            }
        }
        __syncthreads();                                           // (the next page's header, directory and list)
    }
}

// ---- the lean writer: pages staged whole -----------------------------------------------------------------------------------------
// Nearly every page of a heads stream is LEAN: its span, taken from the page table, is whole 16-byte pieces of the stream that
// fit the window; it has 1 .. PG_META_MAX records at ascending offsets; each measures as kind 0 and lies in the window.  k_pg_lean
// writes those and nothing else: no gather, no blob pass, no second fill -- its only global loads are the page tables, the
// offsets, the sums and the window.  A page it finds not lean it leaves alone and appends to a list (one atomic per such page);
// k_pg_write then runs over the list.  (K1's scheme: a lean path for nearly every record, the path that knows every case for the
// rest.)
//
// How it waits.  A page is NP * PG_BLOCK pieces of 16 bytes -- header, directory, records and zero tail alike -- and every thread
// stores exactly NP of them, unconditionally, after ALL loads of the iteration (the next page's window, its offsets and sums, the
// table entries of the page behind it) have been issued.  The memory counter retires in order, so the wait at the loop's top for
// those loads is "all but the last NP": the stores of the page just composed stay in flight, and nothing between the loads and
// the back edge waits for them.  That needs a store that is issued whether or not the page is written: the stores go through a
// buffer descriptor over the page whose size is 0 for a page that is not lean -- the hardware drops them.
struct PglWin { const uint8_t* lo; uint32_t pieces; };             // the window: `pieces` 16-byte pieces from lo on; 0: not staged
__device__ __forceinline__ PglWin pgl_win_of(const PgArgs& A, const PgPage& p, uint32_t cap)
{
    PglWin W;
    W.lo = A.bam; W.pieces = 0;
    if (p.cnt == 0 || p.cnt > PG_META_MAX || p.off0 >= p.span_end) return W;          // (span_end <= n_bytes: pg_page_of)
    const uint8_t* p0 = A.bam + p.off0;
    const uint8_t* lo = p0 - ((uintptr_t)p0 & 15u);                // (the ADDRESS rounded down: the stream pointer need not be aligned)
    const uint8_t* last = A.bam + p.span_end + 15;
    const uint8_t* hi = last - ((uintptr_t)last & 15u);
    if (lo < A.bam || hi > A.bam + A.n_bytes || (uint64_t)(hi - lo) > cap) return W;   // the stream's partial first and last piece: not here
    W.lo = lo; W.pieces = (uint32_t)(hi - lo) / 16u;
    return W;
}

// What the loads of an iteration bring, as loaded: any arithmetic on it would be a wait where it stands, so it is done at the loop's top.
// (z: a zero the compiler cannot see through, in a vector register.  With it the same-for-all-lanes loads below are vector loads
//  whose results stay where they land; without it the compiler moves each into a scalar register right behind the load -- a wait.)
struct PglTab { uint32_t first, first1; uint64_t off0, off1; };    // the table entries of pages k and k + 1
__device__ __forceinline__ uint32_t pgl_rfl(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint64_t pgl_rfl(uint64_t x) { return pgl_rfl((uint32_t)x) | ((uint64_t)pgl_rfl((uint32_t)(x >> 32)) << 32); }
__device__ __forceinline__ PglTab pgl_tab_of(const PgArgs& A, uint32_t k, uint32_t z)
{
    PglTab r;
    r.first = A.page_first[k + z]; r.first1 = A.page_first[k + 1 + z]; r.off0 = A.page_off[k + z]; r.off1 = A.page_off[k + 1 + z];
    return r;
}
__device__ __forceinline__ PgPage pgl_page_of(const PgArgs& A, const PglTab& r)   // = pg_page_of()
{
    PgPage p;
    p.first = pgl_rfl(r.first); p.cnt = pgl_rfl(r.first1) - p.first; p.off0 = pgl_rfl(r.off0); p.span_end = pgl_rfl(r.off1);
    if (p.span_end > A.n_bytes) p.span_end = A.n_bytes;
    return p;
}
// the two levels of a cost offset (pg_S() adds them), the low word of each: all that is asked of them here is the difference of two
// within a page (a loaded word nobody reads is a register the compiler reuses at once -- behind a wait for the load)
struct PglSum { uint32_t loc, blk; };
__device__ __forceinline__ PglSum pgl_sum_of(const PgSums& s, uint32_t i)
{
    PglSum r;
    r.loc = s.S_loc[i]; r.blk = reinterpret_cast<const uint32_t*>(s.blk)[2u * (i / TILE)];
    return r;
}
__device__ __forceinline__ uint32_t pgl_diff(const PglSum& a, const PglSum& b) { return (a.loc + a.blk) - (b.loc + b.blk); }
__device__ __forceinline__ PglSum pgl_rfl(const PglSum& a) { PglSum r; r.loc = pgl_rfl(a.loc); r.blk = pgl_rfl(a.blk); return r; }
struct PglMine { uint64_t off; PglSum S, S0, S_end; };             // = PgMine
__device__ __forceinline__ PglMine pgl_mine_of(const PgArgs& A, const PgPage& p, uint32_t t, uint32_t z)
{
    PglMine m;
    m.off = 0; m.S.loc = 0; m.S.blk = 0;
    if (t < p.cnt && t < PG_META_MAX) { m.off = A.rec_off[p.first + t]; m.S = pgl_sum_of(A.sums, p.first + t); }
    m.S0 = pgl_sum_of(A.sums, p.first + z);                        // (index n_rec is an entry like any other)
    m.S_end = pgl_sum_of(A.sums, p.first + p.cnt + z);
    return m;
}

typedef uint32_t pgl_u32x4 __attribute__((ext_vector_type(4)));
// The window is read once and the page written once, 5.6 GB per file that no cache holds: both non-temporal (1102 -> 1034 us per file,
// the loads 52 and the stores 19 of it on their own: profiles/pages_lean_variants.txt)
__device__ __forceinline__ uint4 pgl_load16(const uint4* p)
{
    const pgl_u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const pgl_u32x4*>(p));
    return make_uint4(x[0], x[1], x[2], x[3]);
}
#define PGL_STORE_NT 2                 // the cache policy word of the buffer store: "nt"

template <int NP>                      // pieces of a page per thread: page_bytes = NP * 16 * PG_BLOCK  (7, 8: the LDS holds three workgroups per CU)
__global__ __launch_bounds__(PG_BLOCK) __attribute__((amdgpu_waves_per_eu(NP > 6 ? 3 : PG_WAVES, NP > 6 ? 3 : PG_WAVES))) void k_pg_lean(const PgArgs A, uint32_t* __restrict__ n_listed,
                                                                                                               uint32_t* __restrict__ listed, uint32_t* __restrict__ n_listed_next)
{
    constexpr uint32_t P = NP * 16u * PG_BLOCK;
    constexpr uint32_t HEAD = P + PG_WIN_SLACK, HEAD_BYTES = 16u + 2u * PG_META_MAX, CORE = HEAD + HEAD_BYTES;
    // one array, so that a piece is "16 bytes at an offset": the window and its slack | header and directory | the records' first 48 bytes
    __shared__ __attribute__((aligned(16))) uint8_t lds[CORE + 48u * PG_META_MAX];
    __shared__ uint32_t s_desc[P / 16];                                             // piece of the page -> src | len << 16
    __shared__ __attribute__((aligned(16))) uint32_t s_mask[17][4];                 // the first `len` bytes of sixteen
    __shared__ uint32_t s_rel[PG_META_MAX];                                         // a record's offset in the window (beyond it: ~0)
    __shared__ uint32_t s_bad;
    const uint32_t t = threadIdx.x, G = gridDim.x;
    if (blockIdx.x == 0 && t == 0) *n_listed_next = 0u;            // nobody reads that counter during this call
    if (t < 17u) {
#pragma unroll
        for (int d = 0; d < 4; d++) s_mask[t][d] = t >= 4u * d + 4u ? ~0u : t > 4u * d ? (1u << (8u * (t - 4u * d))) - 1u : 0u;
    }

    uint32_t k = blockIdx.x;                                       // (< n_pages: the grid is no larger)
    const PglTab no_tab = {0u, 0u, 0ull, 0ull};
    uint32_t z;
    asm("v_mov_b32 %0, 0" : "=v"(z));
    PgPage p_next = pg_page_of(A, k);
    PglTab tab_after = k + G < A.n_pages ? pgl_tab_of(A, k + G, z) : no_tab;
    PglWin W_next = pgl_win_of(A, p_next, P);
    uint4 v[NP];
#pragma unroll
    for (int u = 0; u < NP; u++) {
        const uint32_t i = u * PG_BLOCK + t;
        v[u] = i < W_next.pieces ? pgl_load16(reinterpret_cast<const uint4*>(W_next.lo) + i) : make_uint4(0, 0, 0, 0);
    }
    PglMine m_next = pgl_mine_of(A, p_next, t, z);
    // (the loop is entered as it is re-entered: with nothing but a page's stores in flight -- here none -- so that the compiler's count
    //  of what the top may leave outstanding is the steady state's)
    __builtin_amdgcn_s_waitcnt(0x0F70);                            // vmcnt(0)

    for (; k < A.n_pages; k += G) {
        const PgPage pg = p_next;
        PglMine mine = m_next;
        mine.S0 = pgl_rfl(mine.S0); mine.S_end = pgl_rfl(mine.S_end);
        const PglWin W = W_next;
        const uint32_t cnt = pg.cnt;
        const uint32_t rec0 = 16u + a16(2u * cnt);
        uint32_t used = cnt ? rec0 + pgl_diff(mine.S_end, mine.S0) - 2u * cnt : 16u;
        if (used > P) used = P;
        // ---- the window into LDS; where each record lies in it; the header
#pragma unroll
        for (int u = 0; u < NP; u++) {
            const uint32_t i = u * PG_BLOCK + t;
            if (i < W.pieces) reinterpret_cast<uint4*>(lds)[i] = v[u];
        }
        const uint64_t rel64 = (uint64_t)(A.bam + mine.off - W.lo);                 // (wraps to something huge in front of the window)
        const uint32_t rel = rel64 < 16ull * W.pieces ? (uint32_t)rel64 : ~0u;
        if (t < PG_META_MAX) s_rel[t] = rel;
        if (t < HEAD_BYTES / 16u) reinterpret_cast<uint4*>(lds + HEAD)[t] = t ? make_uint4(0, 0, 0, 0) : make_uint4(cnt, pg.first, used, PG_MAGIC);
        if (t == 0) s_bad = W.pieces ? 0u : 1u;
        __syncthreads();
        // ---- every load of the iteration: the window of the next page, its offsets and sums, the table entries of the page behind it.
        // Nothing below uses what they bring before the loop's top.
        p_next = pgl_page_of(A, tab_after);
        if (k + G < A.n_pages) {
            W_next = pgl_win_of(A, p_next, P);
#pragma unroll
            for (int u = 0; u < NP; u++) {
                const uint32_t i = u * PG_BLOCK + t;
                v[u] = i < W_next.pieces ? pgl_load16(reinterpret_cast<const uint4*>(W_next.lo) + i) : make_uint4(0, 0, 0, 0);
            }
            m_next = pgl_mine_of(A, p_next, t, z);
        }
        tab_after = (uint64_t)k + 2ull * G < A.n_pages ? pgl_tab_of(A, k + 2 * G, z) : no_tab;
        // ---- phase A: a thread per record measures it out of the window and leaves what the pieces need
        if (W.pieces && t < cnt) {
            const uint32_t win_bytes = 16u * W.pieces;
            bool good = rel != ~0u && rel + 36u <= win_bytes && (t == 0 || s_rel[t - 1] < rel);
            if (good) {
                uint32_t core[12];
#pragma unroll
                for (int d = 0; d < 12; d++) core[d] = pg_lds32(lds + rel + 4 * d);          // (behind the record: the slack, or older bytes)
                const PgRec r = pg_classify(core, A.n_bytes, mine.off, false);
                const uint32_t at = rec0 + pgl_diff(mine.S, mine.S0) - 2u * t;
                const uint32_t src_len = 36u + r.lrn + 4u * r.n_cig + r.aux_len;             // the record in the stream: one run of bytes
                good = r.kind == 0 && rel + src_len <= win_bytes && (at & 15u) == 0 && at >= rec0 && at + r.size <= used;
                if (good) {
                    *reinterpret_cast<uint16_t*>(lds + HEAD + 16 + 2 * t) = (uint16_t)(at >> 4);
                    core[0] = r.size;
                    core[3] &= 0xFFFFu;                                                      // kind 0
                    core[6] = r.aux_len; core[7] = 0u; core[8] = 0u;
#pragma unroll
                    for (int d = 0; d < 3; d++)                                              // the first twelve bytes of the name
                        core[9 + d] = r.lrn >= 4u * d + 4u ? core[9 + d] : r.lrn > 4u * d ? core[9 + d] & ((1u << (8u * (r.lrn - 4u * d))) - 1u) : 0u;
#pragma unroll
                    for (int d = 0; d < 12; d += 4) *reinterpret_cast<uint4*>(lds + CORE + 48u * t + 4u * d) = make_uint4(core[d], core[d + 1], core[d + 2], core[d + 3]);
                    // its pieces: three out of the 48 bytes above, then the rest of the name, the CIGAR, the aux block
                    uint32_t* d = s_desc + (at >> 4);
                    const uint32_t name_end = 36u + r.lrn, cig = 4u * r.n_cig, c = a16(name_end);
                    d[0] = (CORE + 48u * t) | (16u << 16); d[1] = (CORE + 48u * t + 16u) | (16u << 16); d[2] = (CORE + 48u * t + 32u) | (16u << 16);
                    d += 3;
                    for (uint32_t b = 48u; b < c; b += 16u) *d++ = (rel + b) | ((name_end - b < 16u ? name_end - b : 16u) << 16);
                    for (uint32_t b = 0; b < cig; b += 16u) *d++ = (rel + name_end + b) | ((cig - b < 16u ? cig - b : 16u) << 16);
                    for (uint32_t b = 0; b < r.aux_len; b += 16u) *d++ = (rel + name_end + cig + b) | ((r.aux_len - b < 16u ? r.aux_len - b : 16u) << 16);
                }
            }
            if (!good) s_bad = 1u;
        }
        // ... and the pieces that belong to no record: header and directory, zeros behind the last record
#pragma unroll
        for (int u = 0; u < NP; u++) {
            const uint32_t piece = u * PG_BLOCK + t;
            if (piece < rec0 / 16u) s_desc[piece] = (HEAD + 16u * piece) | (16u << 16);
            else if (piece >= used / 16u) s_desc[piece] = 0u;
        }
        __syncthreads();
        // ---- phase B: the page, NP pieces per thread.  A piece is 16 bytes of `lds` from `src` on, of which the first `len` count.
        const bool lean = __builtin_amdgcn_readfirstlane(s_bad) == 0u;
        const __amdgpu_buffer_rsrc_t page = __builtin_amdgcn_make_buffer_rsrc(A.out + (uint64_t)k * P, 0, lean ? P : 0u, 0x00020000);
#pragma unroll
        for (int u = 0; u < NP; u++) {
            const uint32_t piece = u * PG_BLOCK + t;
            const uint32_t desc = lean ? s_desc[piece] : 0u;                                // (not lean: the table may hold anything)
            const uint32_t src = desc & 0xFFFFu;
            const uint4 m = *reinterpret_cast<const uint4*>(s_mask[desc >> 16 < 16u ? desc >> 16 : 16u]);
            pgl_u32x4 o;
            o[0] = pg_lds32(lds + src) & m.x; o[1] = pg_lds32(lds + src + 4) & m.y;
            o[2] = pg_lds32(lds + src + 8) & m.z; o[3] = pg_lds32(lds + src + 12) & m.w;
            __builtin_amdgcn_raw_buffer_store_b128(o, page, 16u * piece, 0, PGL_STORE_NT);
        }
        if (!lean && t == 0) listed[atomicAdd(n_listed, 1u)] = k;
        __syncthreads();                                           // (the window and the tables are written again)
    }
}

// The scratch of the size pass, all of it in pg_scan -- gci_bam_pages_write reads it in a later call, and the context's shared scan
// scratch does not last that long: three totals (what the host reads back) | B_loc (n_rec + 1, u64) | the two rows of workgroup
// totals (2 nb, u64) | S_loc (n_rec + 1, u32).
static inline PgSums pg_sums_of(gci_ctx* ctx, uint32_t n_rec)
{
    PgSums s;
    s.nb = n_rec / TILE + 1;
    s.B_loc = (const unsigned long long*)ctx->pg_scan.p + 3;
    s.blk = s.B_loc + (size_t)n_rec + 1;
    s.S_loc = (const uint32_t*)(s.blk + 2 * (size_t)s.nb);
    return s;
}
static inline int pg_sums_ensure(gci_ctx* ctx, uint32_t n_rec)
{
    return gci_ensure(ctx, ctx->pg_scan, (3 + 2 * ((size_t)n_rec / TILE + 1)) * 8 + ((size_t)n_rec + 1) * (8 + 4));
}

extern "C" int gci_bam_pages_size(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec,
                                  int has_seq, uint32_t page_bytes, uint64_t* h_out)
{
    if (!ctx || !h_out || (n_rec && (!d_stream || !d_rec_off))) return GCI_E_INVALID;
    if (page_bytes < 8192 || page_bytes > GCI_PAGE_MAX_BYTES || (page_bytes & 4095u)) return GCI_E_INVALID;
    h_out[0] = h_out[1] = h_out[2] = 0;
    ctx->pg_n_rec = n_rec; ctx->pg_page_bytes = page_bytes; ctx->pg_n_pages = 0; ctx->pg_blob_off = 0; ctx->pg_blob_bytes = 0;
    if (n_rec == 0) { h_out[1] = 16; return GCI_OK; }
    const uint32_t Q = page_bytes - PG_MAX_REC - 48;
    GCI_TRY(pg_sums_ensure(ctx, n_rec));
    const PgSums sums = pg_sums_of(ctx, n_rec);
    unsigned long long* tot = (unsigned long long*)ctx->pg_scan.p;
    {
        ProfScope _ps(ctx, GCI_PROF_PAGES_SIZE);
        hipLaunchKernelGGL(k_pg_measure, dim3(sums.nb), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, d_rec_off, n_rec, has_seq,
                           (uint32_t*)sums.S_loc, (unsigned long long*)sums.B_loc, (unsigned long long*)sums.blk, sums.nb);
        LAUNCHCHK("k_pg_measure");
        hipLaunchKernelGGL(k_pg_blk_scan, dim3(1), dim3(BLOCK), 0, ctx->stream, (unsigned long long*)sums.blk, sums.nb, sums.S_loc, sums.B_loc,
                           n_rec, tot);
        LAUNCHCHK("k_pg_blk_scan");
    }
    unsigned long long tail[3];
    HIPCHK(hipMemcpyAsync(tail, tot, 24, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const unsigned long long b_total = tail[2];
    const uint64_t n_pages = tail[0] / Q + 1;
    if (n_pages > 0xFFFFFFF0ull) return GCI_E_INVALID;
    GCI_TRY(gci_ensure(ctx, ctx->pg_first, (size_t)(n_pages + 1) * (8 + 4)));          // page_off (u64), then page_first (u32)
    uint64_t* page_off = (uint64_t*)ctx->pg_first.p;
    hipLaunchKernelGGL(k_pg_first, dim3((uint32_t)((n_pages + 1 + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, ctx->stream, sums, n_rec,
                       (uint32_t)n_pages, Q, d_rec_off, n_bytes, (uint32_t*)(page_off + n_pages + 1), page_off);
    LAUNCHCHK("k_pg_first");
    ctx->pg_n_pages = (uint32_t)n_pages;
    ctx->pg_blob_off = n_pages * page_bytes;
    ctx->pg_blob_bytes = b_total;
    h_out[0] = n_pages;
    h_out[1] = n_pages * page_bytes + b_total + 16;
    h_out[2] = ctx->pg_blob_off;
    return GCI_OK;
}

typedef void (*pg_lean_fn)(const PgArgs, uint32_t*, uint32_t*, uint32_t*);
static inline pg_lean_fn pg_lean_of(uint32_t page_bytes)           // (8192 .. GCI_PAGE_MAX_BYTES in steps of 4096: gci_bam_pages_size)
{
    static_assert(GCI_PAGE_MAX_BYTES == 8 * 16 * PG_BLOCK, "k_pg_lean is instantiated for 2 .. 8 pieces per thread");
    switch (page_bytes / (16u * PG_BLOCK)) {
    case 2: return k_pg_lean<2>;
    case 3: return k_pg_lean<3>;
    case 4: return k_pg_lean<4>;
    case 5: return k_pg_lean<5>;
    case 6: return k_pg_lean<6>;
    case 7: return k_pg_lean<7>;
    default: return k_pg_lean<8>;
    }
}

extern "C" int gci_bam_pages_write(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec,
                                   int has_seq, uint8_t* d_out, uint64_t cap)
{
    if (!ctx || !d_out || (n_rec && (!d_stream || !d_rec_off))) return GCI_E_INVALID;
    if (n_rec != ctx->pg_n_rec) return GCI_E_INVALID;                       // not the input gci_bam_pages_size measured
    if (n_rec == 0) { HIPCHK(hipMemsetAsync(d_out, 0, cap < 16 ? cap : 16, ctx->stream)); return GCI_OK; }
    // (size of the blob: read back by the size call; the caller allocated what that call said)
    PgArgs A;
    A.bam = d_stream; A.n_bytes = n_bytes; A.rec_off = d_rec_off; A.n_rec = n_rec; A.has_seq = has_seq;
    A.sums = pg_sums_of(ctx, n_rec); A.page_off = (const uint64_t*)ctx->pg_first.p; A.page_first = (const uint32_t*)(A.page_off + ctx->pg_n_pages + 1);
    A.n_pages = ctx->pg_n_pages; A.page_bytes = ctx->pg_page_bytes;
    A.blob_off = ctx->pg_blob_off; A.out = d_out;
    const uint64_t need = ctx->pg_blob_off + ctx->pg_blob_bytes + 16;        // = h_out[1] of the size call
    if (cap < need) return GCI_E_CAPACITY;
    // as many workgroups as the device holds at a time: each walks its share of the pages, one page ahead with its loads
    const uint32_t lds = pg_win_cap(ctx->pg_page_bytes) + PG_WIN_SLACK;
    if (!ctx->pg_cus) {
        int cus = 0;
        HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
        ctx->pg_cus = cus > 0 ? (uint32_t)cus : 256u;
    }
    if (ctx->pg_per_cu_page_bytes != ctx->pg_page_bytes) {                  // (the LDS a workgroup takes depends on the page size alone)
        int per_cu = 0;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pg_write, PG_BLOCK, lds));
        ctx->pg_per_cu = per_cu > 0 ? (uint32_t)per_cu : 1u;
        ctx->pg_per_cu_page_bytes = ctx->pg_page_bytes;
    }
    // (GCI_PAGES_GRID caps both grids: a test's few pages then go through the steady state of the loops)
    const auto grid_of = [&](uint32_t per_cu) {
        uint32_t g = ctx->pg_cus * per_cu;
        if (!PG_PERSIST || g > ctx->pg_n_pages) g = ctx->pg_n_pages;
        return ctx->pg_grid_cap && g > ctx->pg_grid_cap ? ctx->pg_grid_cap : g;
    };
    // the 16 zero bytes directly behind the blob (k_cigar_chunks fetches whole 16-byte pieces): k_pg_write's first workgroup writes them
    uint8_t* const guard = d_out + need - 16;
    ProfScope _ps(ctx, GCI_PROF_PAGES_WRITE);
    if (has_seq) {                                                          // SEQ / QUAL between a record's runs: no page is lean
        hipLaunchKernelGGL(k_pg_write, dim3(grid_of(ctx->pg_per_cu)), dim3(PG_BLOCK), lds, ctx->stream, A, (const uint32_t*)nullptr, (const uint32_t*)nullptr, guard);
        LAUNCHCHK("k_pg_write");
        return GCI_OK;
    }
    // the lean writer over all pages, k_pg_write over those it lists: two counters | the list.  The counters are used alternately --
    // the lean writer of one call zeroes the one of the next, so no memset is launched per call (as K1's counters, k_filter.hip)
    const size_t cap_before = ctx->pg_list.cap;
    GCI_TRY(gci_ensure(ctx, ctx->pg_list, 16 + 4 * (size_t)ctx->pg_n_pages));
    if (ctx->pg_list.cap != cap_before) { HIPCHK(hipMemsetAsync(ctx->pg_list.p, 0, 16, ctx->stream)); ctx->pg_parity = 0; }
    uint32_t* const counters = (uint32_t*)ctx->pg_list.p;
    uint32_t* const listed = counters + 4;
    const uint32_t par = ctx->pg_parity;
    const pg_lean_fn lean = pg_lean_of(ctx->pg_page_bytes);
    if (ctx->pg_lean_page_bytes != ctx->pg_page_bytes) {
        int per_cu = 0;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, lean, PG_BLOCK, 0));
        ctx->pg_lean_per_cu = per_cu > 0 ? (uint32_t)per_cu : 1u;
        ctx->pg_lean_page_bytes = ctx->pg_page_bytes;
    }
    ctx->pg_parity ^= 1u;
    hipLaunchKernelGGL(lean, dim3(grid_of(ctx->pg_lean_per_cu)), dim3(PG_BLOCK), 0, ctx->stream, A, counters + par, listed, counters + (par ^ 1u));
    LAUNCHCHK("k_pg_lean");
    hipLaunchKernelGGL(k_pg_write, dim3(grid_of(ctx->pg_per_cu)), dim3(PG_BLOCK), lds, ctx->stream, A, (const uint32_t*)(counters + par), (const uint32_t*)listed, guard);
    LAUNCHCHK("k_pg_write");
    return GCI_OK;
}
