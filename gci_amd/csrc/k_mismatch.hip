// k_mismatch.hip -- mismatch_sites.py: bases where the reads carry another base than the assembly.  gci_fasta_codes turns the FASTA
// bytes into one 4-bit code per base in the track layout; gci_bam_mismatch_size / _write walk every counted record's CIGAR with a
// reference AND a query position, compare the SEQ nibble with the assembly's code under M / = / X and turn every mismatch into an
// EVENT of one base for the depth build; gci_mismatch_sites_size / _write list the RUNS of bases where the built track is hot
// against the depth track (include/gci_hip.h states all three).  allele_sites.py is the same walk with the read's base kept:
// gci_bam_allele_size / _write rank the events by that base into four lists, gci_allele_sites_size / _write list the single bases
// where one allele's track is hot.
//
// The FASTA side.  Tiles of 4096 bytes, a lane 16 consecutive bytes (gci_text_tiles.hpp); a sequence byte is gci_fasta_n_scan's.
//   k_fasta_rec_rank  one lane per record: the sequence bytes of the file in front of its body -- the scanned count of its tile plus
//                     the sequence bytes of that tile in front of the body
//   k_fasta_codes     one workgroup per tile: a workgroup scan of the lanes' sequence bytes ranks every byte in the file, minus its
//                     record's rank that is its position, and d_dst[record] + position is the one byte it stores
//
// The record side.  Input and chunks as k_indels.hip (gci_cover_chunks.hpp, gci_cigar_sums.hpp).
//   k_mm_parse    one lane per record: cv_parse_counted, and where SEQ lies and how long it is
//   k_cigar_sums  one wave per chunk
//   k_chunk_lens  one lane per chunk: its reference length M + D + N and its query length S + M + I -- scanned, the two carries
//   k_mm_count    one wave per chunk, 64 operations a round: wave scans of the reference, query and match lengths place every
//                 operation on both axes; the round's MATCH BASES are then dealt to the lanes by base, MM_BASES consecutive ones a
//                 lane, 64 * MM_BASES a step, and a lane finds the operation of its first base by a search over the 64 scanned match
//                 lengths in LDS -- a record of 15-base operations fills the wave as one of 15,000-base operations does
//   k_rec_finish  one lane per record: codes 9 - 15 and S + M + I != l_seq into the status word, whether the record is counted
//   k_mm_write    the same walk; a lane's slot is its chunk's offset + the mismatches of earlier steps + those of the lanes below it
//                 (ballots and popcounts), so events come in (record, reference position) order
//   k_al_count    the walk with a count per class of the read's base (A, C, G, T): cnt[class * n_chunks + chunk], so ONE scan over the
//                 4 * n_chunks entries is the slot of every (class, chunk) in the concatenated output and the four list ends
//   k_al_write    the walk; a lane packs its four counts of a step into 4 x 16 bits of one word (a step holds at most 64 * MM_BASES
//                 events), one wave scan of the word ranks the lanes in all four classes; inside a lane base order decides
// A record whose S + M + I is not l_seq is never walked: no SEQ byte beyond (l_seq + 1) / 2 is ever read.  The only global atomic
// is the status word's atomicMin.
//
// The track side.  gci_site_tiles.hpp's lister, as k_indels.hip: the RUNS of hot elements, hot = mismatch >= min_reads and
// mismatch * 1000000 >= frac_ppm * depth in 64 bits (HotMismatch); the depth track is read in every pass.  A site keeps the largest
// mismatch count of its run and the depth at the FIRST base that reaches it (MmBest).  The allele lister lists single elements, as
// k_clips.hip's: hot = the largest of the four allele tracks passes the two tests (HotAllele), five tracks read in every pass; the
// code array is read by the Emit only, for the sites it stores.
#include "gci_cigar_sums.hpp"
#include "gci_site_tiles.hpp"
#include "gci_text_tiles.hpp"

#ifndef MM_BASES
#define MM_BASES 4                       // consecutive match bases a lane takes in one step (1, 4 and 8 measured)
#endif

// ---- the FASTA side ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool mm_fasta_dropped(uint8_t c) { return c == '\n' || c == '\r' || c == ' '; }

// BAM's 4-bit code ("=ACMGRSVTWYHKDBN") of a FASTA byte, case-insensitive; U is T; anything that is no IUPAC letter is 15
__device__ __forceinline__ uint8_t mm_fasta_code(uint8_t c)
{
    const uint32_t l = c | 0x20u;
    if (l < 'a' || l > 'z') return 15;
    const uint32_t k = c & 0x1Fu;                      // A = 1 .. Z = 26
    const unsigned long long tab = k < 16u ? 0xFF3FCFFB4FFD2E1Full : 0xFFFFFFAF978865FFull;
    return (uint8_t)((tab >> (4u * (k & 15u))) & 15u);
}

// the record whose body holds byte i, or -1 (a title line, in front of the first record): steps back from the candidate
__device__ __forceinline__ int64_t mm_record_of(const int64_t* __restrict__ body, int64_t cand, uint64_t i)
{
    while (cand >= 0 && (uint64_t)body[2 * cand] > i) cand--;
    if (cand < 0 || i >= (uint64_t)body[2 * cand + 1]) return -1;
    return cand;
}

__global__ __launch_bounds__(BLOCK) void k_fasta_rec_rank(const uint8_t* __restrict__ text, uint64_t n_bytes, const int64_t* __restrict__ body,
                                                          uint32_t n_records, const unsigned long long* __restrict__ tile_kept0,
                                                          unsigned long long* __restrict__ rec_rank)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n_records) return;
    uint64_t b = (uint64_t)(body[2 * r] < 0 ? 0 : body[2 * r]);
    if (b > n_bytes) b = n_bytes;
    const uint64_t tile0 = b / TEXT_TILE * TEXT_TILE;
    unsigned long long rank = tile_kept0[b / TEXT_TILE];                 // (tiles + 1 entries: b == n_bytes may be the end of the last tile)
    for (int64_t q = (int64_t)r - 1; q >= 0 && (uint64_t)body[2 * q + 1] > tile0; q--) {
        const uint64_t lo = (uint64_t)body[2 * q] > tile0 ? (uint64_t)body[2 * q] : tile0;
        const uint64_t hi = (uint64_t)body[2 * q + 1] < b ? (uint64_t)body[2 * q + 1] : b;
        for (uint64_t i = lo; i < hi; i++) rank += mm_fasta_dropped(text[i]) ? 0u : 1u;
    }
    rec_rank[r] = rank;
}

__global__ __launch_bounds__(TEXT_BLOCK) void k_fasta_codes(const uint8_t* __restrict__ text, uint64_t n_bytes, const int64_t* __restrict__ body,
                                                            uint32_t n_records, const int64_t* __restrict__ dst,
                                                            const unsigned long long* __restrict__ tile_kept0,
                                                            const unsigned long long* __restrict__ rec_rank, uint8_t* __restrict__ codes,
                                                            int64_t total)
{
    __shared__ uint32_t wtot[TEXT_BLOCK / 64];
    const int t = threadIdx.x;
    const uint64_t tile0 = (uint64_t)blockIdx.x * TEXT_TILE, at = tile0 + 16u * t;
    // the last record whose body begins at or before this lane's last byte (bodies are sorted and disjoint)
    uint32_t lo = 0, hi = n_records;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)body[2 * mid] < at + 16) lo = mid + 1; else hi = mid; }
    const int64_t cand = (int64_t)lo - 1;
    const uint4 v = load16(text, n_bytes, (int64_t)at);
    union { uint4 v; uint8_t b[16]; } u;
    u.v = v;
    uint32_t keep = 0;
    int64_t rec[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        rec[k] = at + k < n_bytes ? mm_record_of(body, cand, at + k) : -1;
        keep |= (rec[k] >= 0 && !mm_fasta_dropped(u.b[k])) ? (1u << k) : 0u;
    }
    uint32_t all;
    const uint32_t pre = block_exclusive<uint32_t, TEXT_BLOCK / 64>((uint32_t)__builtin_popcount(keep), wtot, all);
    unsigned long long g = tile_kept0[blockIdx.x] + pre;                 // the rank in the file of this lane's next sequence byte
#pragma unroll
    for (int k = 0; k < 16; k++) {
        if (!((keep >> k) & 1u)) continue;
        const int64_t d = dst[rec[k]];
        if (d >= 0) {
            const unsigned long long e = (unsigned long long)d + (g - rec_rank[rec[k]]);
            if (e < (unsigned long long)total) codes[e] = mm_fasta_code(u.b[k]);
        }
        g++;
    }
}

extern "C" int gci_fasta_codes(gci_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, const int64_t* d_body, uint32_t n_records, const int64_t* d_dst,
                               const uint64_t* d_tile_kept0, uint8_t* d_codes)
{
    if (!ctx || !d_codes || (n_bytes && (!d_text || !d_tile_kept0)) || (n_records && (!d_body || !d_dst))) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    if (((uintptr_t)d_text) & 15u) return GCI_E_INVALID;
    if (!n_bytes || !n_records) return GCI_OK;
    const int64_t tiles = text_tiles(n_bytes, false);
    if (tiles < 0) return GCI_E_INVALID;
    GCI_TRY(gci_ensure(ctx, ctx->mm_fasta, 8 * (size_t)n_records));
    unsigned long long* rank = (unsigned long long*)ctx->mm_fasta.p;
    hipLaunchKernelGGL(k_fasta_rec_rank, dim3((n_records + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, ctx->stream, d_text, n_bytes, d_body, n_records,
                       (const unsigned long long*)d_tile_kept0, rank);
    LAUNCHCHK("k_fasta_rec_rank");
    hipLaunchKernelGGL(k_fasta_codes, dim3((uint32_t)tiles), dim3(TEXT_BLOCK), 0, ctx->stream, d_text, n_bytes, d_body, n_records, d_dst,
                       (const unsigned long long*)d_tile_kept0, rank, d_codes, ctx->total);
    LAUNCHCHK("k_fasta_codes");
    return GCI_OK;
}

// ---- the record side ----------------------------------------------------------------------------------------------------------------
struct MmRecScratch : RecFrame {         // carved out of ctx->mm_rec: the frame, and behind it
    CvSeq* seqs;
};

static inline MmRecScratch mm_rec_scratch(const RecFrame& F)
{
    MmRecScratch s;
    static_cast<RecFrame&>(s) = F;
    s.seqs = (CvSeq*)F.tail;
    return s;
}

struct MmChunkScratch {                  // carved out of ctx->mm_chunk
    CigarSums* sums;
    unsigned long long* ref;             // reference length of a chunk
    unsigned long long* qry;             // query length of a chunk
    unsigned long long* cmp;             // pairs compared in a chunk
    unsigned long long* ref0;            // n_chunks + 1 each: the exclusive scans
    unsigned long long* qry0;
    unsigned long long* cmp0;
    unsigned long long* mm0;             // classes * n_chunks + 1
    unsigned long long* blk;
    uint32_t* n_mm;                      // mismatches of a chunk: [class * n_chunks + chunk]
};

// classes: 1 (gci_bam_mismatch_*: ctx->mm_chunk) or 4, the read's base A, C, G, T (gci_bam_allele_*: ctx->al_chunk)
static inline size_t mm_chunk_bytes(uint64_t n_chunks, int classes)
{
    const size_t n = (size_t)n_chunks, m = (size_t)classes * n;
    return sizeof(CigarSums) * n + 3 * 8 * n + 3 * 8 * (n + 1) + 8 * (m + 1) + 8 * (scan_blocks(m) + 2) + 4 * m;
}

static inline MmChunkScratch mm_chunk_scratch(const DevBuf& buf, uint64_t n_chunks, int classes)
{
    const size_t n = (size_t)n_chunks, m = (size_t)classes * n;
    MmChunkScratch s;
    uint8_t* p = (uint8_t*)buf.p;
    s.sums = (CigarSums*)p; p += sizeof(CigarSums) * n;
    s.ref = (unsigned long long*)p; p += 8 * n;
    s.qry = (unsigned long long*)p; p += 8 * n;
    s.cmp = (unsigned long long*)p; p += 8 * n;
    s.ref0 = (unsigned long long*)p; p += 8 * (n + 1);
    s.qry0 = (unsigned long long*)p; p += 8 * (n + 1);
    s.cmp0 = (unsigned long long*)p; p += 8 * (n + 1);
    s.mm0 = (unsigned long long*)p; p += 8 * (m + 1);
    s.blk = (unsigned long long*)p; p += 8 * (scan_blocks(m) + 2);
    s.n_mm = (uint32_t*)p;
    return s;
}

__global__ __launch_bounds__(BLOCK) void k_mm_parse(const uint8_t* __restrict__ bam, uint64_t n_bytes, const uint64_t* __restrict__ rec_off,
                                                    uint32_t n_rec, const int32_t* __restrict__ ref_sel, int32_t n_ref, uint32_t excl_flags,
                                                    int min_mapq, CoverRec* __restrict__ recs, CvSeq* __restrict__ seqs, uint32_t* __restrict__ nch,
                                                    unsigned long long* __restrict__ status)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_rec) return;
    CvSeq q;
    uint32_t chunks;
    const CoverRec r = cv_parse_counted(bam, n_bytes, rec_off[i], i, 1, ref_sel, n_ref, excl_flags, min_mapq, status, chunks, q);
    recs[i] = r;
    seqs[i] = q;
    nch[i] = chunks;
}

// LDS written by the lanes of ONE wave is read by its other lanes: no workgroup barrier (the waves of a workgroup walk chunks of
// different lengths), the wave's own LDS operations complete in order
__device__ __forceinline__ void mm_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct MmWalkArgs {
    const uint8_t* bam;
    uint64_t n_bytes;
    const CoverRec* recs;
    const CvSeq* seqs;
    const unsigned long long* chunk0;
    uint32_t n_rec;
    unsigned long long n_chunks;
    const unsigned long long* ref0;
    const unsigned long long* qry0;
    const int64_t* contig_len;
    const int64_t* contig_off;
    int32_t n_contigs;
    const uint8_t* codes;
};

// ALLELES: a mismatch is an event of the class of the read's base (A, C, G, T = 0 .. 3); chunk_mm and chunk_mm0 hold four entries a
// chunk, [class * n_chunks + chunk], and chunk_mm0 is the scan over all of them: the slot in the concatenated lists
template <bool WRITE, bool ALLELES>
__device__ __forceinline__ void mm_walk(const MmWalkArgs& A, uint32_t* __restrict__ chunk_mm, unsigned long long* __restrict__ chunk_cmp,
                                        const unsigned long long* __restrict__ chunk_mm0, unsigned long long total, gci_ivl* __restrict__ out)
{
    static_assert(MM_BASES <= 8, "a step's events of one class must fit 16 bits, a lane's bases and classes 8 and 16");
    constexpr int CLASSES = ALLELES ? 4 : 1;
    // of the round's 64 operations: the inclusive scan of the match lengths, and where each begins on the reference and in the read
    __shared__ unsigned long long s_inc[BLOCK / 64][64], s_ref[BLOCK / 64][64], s_qry[BLOCK / 64][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long ch = (unsigned long long)blockIdx.x * (BLOCK / 64) + w;
    if (ch >= A.n_chunks) return;                      // (the whole wave)
    const uint32_t rec = cv_rec_of_chunk(A.chunk0, A.n_rec, ch);
    const CoverRec r = A.recs[rec];
    const CvSeq sq = A.seqs[rec];
    const unsigned long long ch_first = A.chunk0[rec], ch_last = A.chunk0[rec + 1];
    uint32_t mms[CLASSES] = {0};                       // (constant indices only: registers)
    unsigned long long cmps = 0;
    // SEQ `*`, or a record whose operations do not add up to l_seq (k_rec_finish reports it): nothing is compared, no SEQ byte is read
    const bool walk = sq.l_seq != 0 && A.qry0[ch_last] - A.qry0[ch_first] == (unsigned long long)sq.l_seq;
    if (walk) {
        const CvChunk c = cv_chunk_of(A.bam, r, (uint32_t)(ch - ch_first));
        // positions in 64 bits: pos + the reference lengths in front may pass 2^31; compared with L before they index anything
        unsigned long long at = (unsigned long long)(uint32_t)r.pos + (A.ref0[ch] - A.ref0[ch_first]);
        unsigned long long qat = A.qry0[ch] - A.qry0[ch_first];
        const int64_t len = r.contig < A.n_contigs ? A.contig_len[r.contig] : 0;       // (a d_ref_sel beyond the layout: no base of it is inside)
        const unsigned long long L = (unsigned long long)(len < 0x7FFFFFFEll ? (len < 0 ? 0 : len) : 0x7FFFFFFEll);
        const uint8_t* __restrict__ ref = A.codes + (L ? A.contig_off[r.contig] : 0);
        const uint8_t* __restrict__ seq = A.bam + sq.seq_off;
        unsigned long long o_mm[CLASSES];                                               // where the chunk's next mismatch (of a class) goes
#pragma unroll
        for (int k = 0; k < CLASSES; k++) o_mm[k] = WRITE ? chunk_mm0[(unsigned long long)k * A.n_chunks + ch] : 0ull;
        for (uint32_t k0 = 0; k0 < c.n && at < L; k0 += 64) {                           // (behind the contig's end nothing is compared)
            const uint32_t k = k0 + lane;
            const bool valid = k < c.n;
            const uint32_t v = cv_op_word(A.bam, A.n_bytes, c, k, lane);
            const uint32_t op = v & 0xFu, n = v >> 4;
            const unsigned long long ref_len = (valid && ((0x18Du >> op) & 1u)) ? n : 0u;   // M D N = X
            const unsigned long long qry_len = (valid && ((0x193u >> op) & 1u)) ? n : 0u;   // M I S = X
            const unsigned long long m_len = (valid && ((0x181u >> op) & 1u)) ? n : 0u;     // M = X
            const unsigned long long inc_r = wave_inclusive<unsigned long long>(ref_len, lane);
            const unsigned long long inc_q = wave_inclusive<unsigned long long>(qry_len, lane);
            const unsigned long long inc_m = wave_inclusive<unsigned long long>(m_len, lane);
            mm_wave_sync();                            // (the reads of the round in front are done)
            s_inc[w][lane] = inc_m;
            s_ref[w][lane] = at + inc_r - ref_len;
            s_qry[w][lane] = qat + inc_q - qry_len;
            mm_wave_sync();
            const unsigned long long T = __shfl(inc_m, 63, 64);          // the round's match bases, dealt MM_BASES to a lane
            for (unsigned long long b0 = 0; b0 < T; b0 += 64 * MM_BASES) {
                const unsigned long long j0 = b0 + (unsigned long long)lane * MM_BASES;
                uint32_t o = 0;                        // the operation of base j0: the entries of s_inc at or below it
                if (j0 < T) {
#pragma unroll
                    for (uint32_t step = 32; step >= 1; step >>= 1) if (s_inc[w][o + step - 1] <= j0) o += step;
                }
                uint32_t cmp = 0, mis = 0, cls = 0;    // (cls: two bits a base, the class of its mismatch)
                unsigned long long p_first = ~0ull;
#pragma unroll
                for (int b = 0; b < MM_BASES; b++) {
                    const unsigned long long j = j0 + b;
                    if (j >= T) break;
                    while (s_inc[w][o] <= j) o++;      // (j < T = s_inc[63]: o stays below 64; operations without match bases are passed)
                    const unsigned long long in_op = j - (o ? s_inc[w][o - 1] : 0ull);
                    const unsigned long long p = s_ref[w][o] + in_op, q = s_qry[w][o] + in_op;
                    if (b == 0) p_first = p;
                    if (p < L && q < (unsigned long long)sq.l_seq) {
                        const uint32_t rc = ref[p], sb = seq[q >> 1];
                        const uint32_t nib = (q & 1ull) ? (sb & 15u) : (sb >> 4);             // the high nibble is the even q
                        const bool both = ((0x116u >> rc) & 1u) && ((0x116u >> nib) & 1u);    // both one of 1 2 4 8 (rc, nib < 16)
                        cmp |= both ? (1u << b) : 0u;
                        mis |= (both && rc != nib) ? (1u << b) : 0u;
                        if (ALLELES) cls |= (both && rc != nib) ? (((nib >> 1) - (nib >> 3)) << (2 * b)) : 0u;      // 1 2 4 8 -> 0 1 2 3
                    }
                }
                // ALLELES: the lane's events of the step per class, 16 bits each
                unsigned long long word = 0;
                if (ALLELES) {
#pragma unroll
                    for (int b = 0; b < MM_BASES; b++) word += ((mis >> b) & 1u) ? 1ull << (16u * ((cls >> (2 * b)) & 3u)) : 0ull;
                }
                if (WRITE) {
                    // base order is lane order, then the order inside the lane: the lanes below, then the lane's own lower bits
                    unsigned long long slot = o_mm[0], below = 0, all = 0;
                    if (ALLELES) {
                        const unsigned long long inc = wave_inclusive<unsigned long long>(word, lane);
                        below = inc - word;            // per class: the events of the lanes below, then of the lane's own lower bases too
                        all = __shfl(inc, 63, 64);     // ... and of the whole step
                    } else {
                        uint32_t step_total = 0;
#pragma unroll
                        for (int b = 0; b < MM_BASES; b++) {
                            const unsigned long long m = __ballot((mis >> b) & 1u);
                            slot += (unsigned long long)__builtin_popcountll(m & lanes_below(lane));
                            step_total += (uint32_t)__builtin_popcountll(m);
                        }
                        o_mm[0] += step_total;
                    }
                    uint32_t bits = mis;
                    while (bits) {
                        const int b = __builtin_ctz(bits);
                        bits &= bits - 1u;
                        const unsigned long long j = j0 + b;
                        uint32_t oo = 0;
#pragma unroll
                        for (uint32_t step = 32; step >= 1; step >>= 1) if (s_inc[w][oo + step - 1] <= j) oo += step;
                        const unsigned long long p = s_ref[w][oo] + (j - (oo ? s_inc[w][oo - 1] : 0ull));
                        gci_ivl e;
                        e.contig = r.contig; e.start = (int32_t)p; e.end = (int32_t)p; e.pad = 0;
                        if (ALLELES) {
                            const uint32_t k = (cls >> (2 * b)) & 3u;
                            // (selects, not an index: o_mm stays in registers)
                            const unsigned long long o_k = k == 0 ? o_mm[0] : k == 1 ? o_mm[CLASSES > 1 ? 1 : 0] : k == 2 ? o_mm[CLASSES > 2 ? 2 : 0]
                                                                                                                        : o_mm[CLASSES > 3 ? 3 : 0];
                            slot = o_k + ((below >> (16u * k)) & 0xFFFFull);
                            below += 1ull << (16u * k);
                        }
                        if (slot < total) out[slot] = e;
                        slot++;
                    }
                    if (ALLELES) {
#pragma unroll
                        for (int k = 0; k < CLASSES; k++) o_mm[k] += (all >> (16 * k)) & 0xFFFFull;
                    }
                } else {
                    if (ALLELES) {
#pragma unroll
                        for (int k = 0; k < CLASSES; k++) mms[k] += (uint32_t)(word >> (16 * k)) & 0xFFFFu;
                    } else {
                        mms[0] += (uint32_t)__builtin_popcount(mis);
                    }
                    cmps += (unsigned long long)__builtin_popcount(cmp);
                }
                if (__shfl(p_first, 0, 64) >= L) break;                  // (positions ascend with the base index: the rest is outside)
            }
            at += __shfl(inc_r, 63, 64);
            qat += __shfl(inc_q, 63, 64);
        }
    }
    if (!WRITE) {
#pragma unroll
        for (int k = 0; k < CLASSES; k++) mms[k] = wave_sum<uint32_t>(mms[k]);
        cmps = wave_sum<unsigned long long>(cmps);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < CLASSES; k++) chunk_mm[(unsigned long long)k * A.n_chunks + ch] = mms[k];
            chunk_cmp[ch] = cmps;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_mm_count(MmWalkArgs A, uint32_t* __restrict__ chunk_mm, unsigned long long* __restrict__ chunk_cmp)
{
    mm_walk<false, false>(A, chunk_mm, chunk_cmp, nullptr, 0, nullptr);
}

__global__ __launch_bounds__(BLOCK) void k_mm_write(MmWalkArgs A, const unsigned long long* __restrict__ chunk_mm0, unsigned long long total,
                                                    gci_ivl* __restrict__ out)
{
    mm_walk<true, false>(A, nullptr, nullptr, chunk_mm0, total, out);
}

__global__ __launch_bounds__(BLOCK) void k_al_count(MmWalkArgs A, uint32_t* __restrict__ chunk_al, unsigned long long* __restrict__ chunk_cmp)
{
    mm_walk<false, true>(A, chunk_al, chunk_cmp, nullptr, 0, nullptr);
}

__global__ __launch_bounds__(BLOCK) void k_al_write(MmWalkArgs A, const unsigned long long* __restrict__ chunk_al0, unsigned long long total,
                                                    gci_ivl* __restrict__ out)
{
    mm_walk<true, true>(A, nullptr, nullptr, chunk_al0, total, out);
}

static inline MmWalkArgs mm_walk_args(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, uint32_t n_rec, unsigned long long n_chunks,
                                      const MmRecScratch& R, const MmChunkScratch& C, const uint8_t* d_codes)
{
    MmWalkArgs A;
    A.bam = d_stream; A.n_bytes = n_bytes; A.recs = R.recs; A.seqs = R.seqs; A.chunk0 = R.chunk0; A.n_rec = n_rec; A.n_chunks = n_chunks;
    A.ref0 = C.ref0; A.qry0 = C.qry0; A.contig_len = (const int64_t*)ctx->d_len.p; A.contig_off = (const int64_t*)ctx->d_off.p;
    A.n_contigs = ctx->n_contigs; A.codes = d_codes;
    return A;
}

struct MmMeasured {                      // on the host, after the synchronise
    unsigned long long n_chunks = 0, n_counted = 0, n_cmp = 0;
    unsigned long long end[4] = {0, 0, 0, 0};      // where the list of class k ends in the output: the events of classes 0 .. k
};

// what gci_bam_mismatch_size and gci_bam_allele_size do behind their argument checks, up to the synchronise: the parse, the chunks,
// the two axes, the count pass (one class, or four with ALLELES) and its scan, the records counted, the status word
template <bool ALLELES>
static int mm_measure(gci_ctx* ctx, DevBuf& rec_buf, DevBuf& chunk_buf, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off,
                      uint32_t n_rec, const int32_t* d_ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq, const uint8_t* d_codes,
                      uint64_t* d_status, MmMeasured& m)
{
    constexpr int CLASSES = ALLELES ? 4 : 1;
    RecFrame F;
    GCI_TRY(rec_frame_open(ctx, rec_buf, sizeof(CvSeq) * (size_t)n_rec, n_rec, F));
    const MmRecScratch R = mm_rec_scratch(F);
    unsigned long long n_chunks = 0, n_cmp = 0, n_counted = 0;
    if (n_rec) {
        const uint32_t groups = (n_rec + BLOCK - 1) / BLOCK;
        hipLaunchKernelGGL(k_mm_parse, dim3(groups), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, d_rec_off, n_rec, d_ref_sel, n_ref, excl_flags,
                           min_mapq, R.recs, R.seqs, R.nch, R.status);
        LAUNCHCHK("k_mm_parse");
        GCI_TRY(rec_frame_chunks(ctx, R, n_rec, n_chunks));
        const CigarSums* sums = nullptr;
        const unsigned long long* qry0 = nullptr;
        if (n_chunks) {
            GCI_TRY(gci_ensure(ctx, chunk_buf, mm_chunk_bytes(n_chunks, CLASSES)));
            const MmChunkScratch C = mm_chunk_scratch(chunk_buf, n_chunks, CLASSES);
            sums = C.sums; qry0 = C.qry0;
            hipLaunchKernelGGL(k_cigar_sums, cigar_sums_grid(n_chunks), dim3(BLOCK), 0, ctx->stream, d_stream, n_bytes, R.recs, R.chunk0, n_rec, n_chunks,
                               C.sums);
            LAUNCHCHK("k_cigar_sums");
            launch_chunk_lens(ctx, C.sums, n_chunks, C.ref, C.qry);
            LAUNCHCHK("k_chunk_lens");
            GCI_TRY((device_exclusive_scan<unsigned long long, unsigned long long>(ctx, C.ref, C.ref0, C.blk, (int64_t)n_chunks, true)));
            GCI_TRY((device_exclusive_scan<unsigned long long, unsigned long long>(ctx, C.qry, C.qry0, C.blk, (int64_t)n_chunks, true)));
            hipLaunchKernelGGL(ALLELES ? k_al_count : k_mm_count, wave_grid(n_chunks), dim3(BLOCK), 0, ctx->stream,
                               mm_walk_args(ctx, d_stream, n_bytes, n_rec, n_chunks, R, C, d_codes), C.n_mm, C.cmp);
            LAUNCHCHK(ALLELES ? "k_al_count" : "k_mm_count");
            // ONE scan over the classes' counts, class by class: the slot of every (class, chunk), and at (k + 1) * n_chunks list k's end
            GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, C.n_mm, C.mm0, C.blk, (int64_t)(CLASSES * n_chunks), true)));
            GCI_TRY((device_exclusive_scan<unsigned long long, unsigned long long>(ctx, C.cmp, C.cmp0, C.blk, (int64_t)n_chunks, true)));
            for (int k = 0; k < CLASSES; k++)
                HIPCHK(hipMemcpyAsync(&m.end[k], C.mm0 + (size_t)(k + 1) * n_chunks, 8, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(&n_cmp, C.cmp0 + n_chunks, 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        launch_rec_finish(ctx, n_rec, R.recs, R.chunk0, sums, R.seqs, qry0, R.counted, R.status);
        LAUNCHCHK("k_rec_finish");
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, R.counted, R.cnt0, R.blk, (int64_t)n_rec, true)));
        HIPCHK(hipMemcpyAsync(&n_counted, R.cnt0 + n_rec, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipMemcpyAsync(d_status, R.status, 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    m.n_chunks = n_chunks; m.n_counted = n_counted; m.n_cmp = n_cmp;
    return GCI_OK;
}

extern "C" int gci_bam_mismatch_size(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                                     const int32_t* d_ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq, const uint8_t* d_codes,
                                     uint64_t* h_counts, uint64_t* d_status)
{
    if (!ctx || !h_counts || !d_status || !d_codes || n_ref < 0 || has_seq != 1 || (n_rec && (!d_stream || !d_rec_off || !d_ref_sel)))
        return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    ctx->mm_valid = false;
    h_counts[0] = h_counts[1] = h_counts[2] = 0;
    MmMeasured m;
    GCI_TRY(mm_measure<false>(ctx, ctx->mm_rec, ctx->mm_chunk, d_stream, n_bytes, d_rec_off, n_rec, d_ref_sel, n_ref, excl_flags, min_mapq, d_codes,
                              d_status, m));
    ctx->mm_valid = true;
    ctx->mm_n_rec = n_rec; ctx->mm_n_bytes = n_bytes; ctx->mm_n_chunks = m.n_chunks; ctx->mm_n_mm = m.end[0];
    ctx->mm_stream = d_stream; ctx->mm_off = d_rec_off; ctx->mm_codes = d_codes;
    h_counts[0] = m.n_counted; h_counts[1] = m.end[0]; h_counts[2] = m.n_cmp;
    return GCI_OK;
}

extern "C" int gci_bam_mismatch_write(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                                      const uint8_t* d_codes, gci_ivl* d_out, uint64_t cap, uint64_t* d_status)
{
    if (!ctx || !d_status || !d_codes || has_seq != 1 || (n_rec && (!d_stream || !d_rec_off))) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    // not the input gci_bam_mismatch_size measured last on this context
    if (!ctx->mm_valid || n_rec != ctx->mm_n_rec || n_bytes != ctx->mm_n_bytes || d_stream != ctx->mm_stream || d_rec_off != ctx->mm_off ||
        d_codes != ctx->mm_codes)
        return GCI_E_INVALID;
    const unsigned long long total = ctx->mm_n_mm;
    if (total && !d_out) return GCI_E_INVALID;
    if (cap < total) return GCI_E_CAPACITY;
    const MmRecScratch R = mm_rec_scratch(rec_frame(ctx->mm_rec, n_rec));
    const unsigned long long n_chunks = ctx->mm_n_chunks;
    if (n_chunks && total) {
        const MmChunkScratch C = mm_chunk_scratch(ctx->mm_chunk, n_chunks, 1);
        hipLaunchKernelGGL(k_mm_write, wave_grid(n_chunks), dim3(BLOCK), 0, ctx->stream,
                           mm_walk_args(ctx, d_stream, n_bytes, n_rec, n_chunks, R, C, d_codes), C.mm0, total, d_out);
        LAUNCHCHK("k_mm_write");
    }
    HIPCHK(hipMemcpyAsync(d_status, R.status, 8, hipMemcpyDeviceToDevice, ctx->stream));
    return GCI_OK;
}

// allele_sites.py: the same two calls with the events ranked by the read's base; a scratch and a memo of their own (ctx->al_*), so a
// mismatch pair and an allele pair on one context do not end each other
extern "C" int gci_bam_allele_size(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                                   const int32_t* d_ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq, const uint8_t* d_codes,
                                   uint64_t* h_counts, uint64_t* d_status)
{
    if (!ctx || !h_counts || !d_status || !d_codes || n_ref < 0 || has_seq != 1 || (n_rec && (!d_stream || !d_rec_off || !d_ref_sel)))
        return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    ctx->al_valid = false;
    for (int k = 0; k < 6; k++) h_counts[k] = 0;
    MmMeasured m;
    GCI_TRY(mm_measure<true>(ctx, ctx->al_rec, ctx->al_chunk, d_stream, n_bytes, d_rec_off, n_rec, d_ref_sel, n_ref, excl_flags, min_mapq, d_codes,
                             d_status, m));
    ctx->al_valid = true;
    ctx->al_n_rec = n_rec; ctx->al_n_bytes = n_bytes; ctx->al_n_chunks = m.n_chunks; ctx->al_total = m.end[3];
    ctx->al_stream = d_stream; ctx->al_off = d_rec_off; ctx->al_codes = d_codes;
    h_counts[0] = m.n_counted; h_counts[5] = m.n_cmp;
    for (int k = 0; k < 4; k++) h_counts[1 + k] = m.end[k] - (k ? m.end[k - 1] : 0ull);
    return GCI_OK;
}

extern "C" int gci_bam_allele_write(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec, int has_seq,
                                    const uint8_t* d_codes, gci_ivl* d_out, uint64_t cap, uint64_t* d_status)
{
    if (!ctx || !d_status || !d_codes || has_seq != 1 || (n_rec && (!d_stream || !d_rec_off))) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    // not the input gci_bam_allele_size measured last on this context
    if (!ctx->al_valid || n_rec != ctx->al_n_rec || n_bytes != ctx->al_n_bytes || d_stream != ctx->al_stream || d_rec_off != ctx->al_off ||
        d_codes != ctx->al_codes)
        return GCI_E_INVALID;
    const unsigned long long total = ctx->al_total;
    if (total && !d_out) return GCI_E_INVALID;
    if (cap < total) return GCI_E_CAPACITY;
    const MmRecScratch R = mm_rec_scratch(rec_frame(ctx->al_rec, n_rec));
    const unsigned long long n_chunks = ctx->al_n_chunks;
    if (n_chunks && total) {
        const MmChunkScratch C = mm_chunk_scratch(ctx->al_chunk, n_chunks, 4);
        hipLaunchKernelGGL(k_al_write, wave_grid(n_chunks), dim3(BLOCK), 0, ctx->stream,
                           mm_walk_args(ctx, d_stream, n_bytes, n_rec, n_chunks, R, C, d_codes), C.mm0, total, d_out);
        LAUNCHCHK("k_al_write");
    }
    HIPCHK(hipMemcpyAsync(d_status, R.status, 8, hipMemcpyDeviceToDevice, ctx->stream));
    return GCI_OK;
}

// ---- the track side -----------------------------------------------------------------------------------------------------------------
struct MmEmit {
    static constexpr int LISTER = 3;
    static constexpr bool RUNS = true;
    gci_mismatch_site* out;
    __device__ __forceinline__ void operator()(unsigned long long slot, const SiteTile& x, int64_t q) const
    {
        gci_mismatch_site s;
        s.contig = x.contig; s.start = (int32_t)(q - x.contig_off);
        s.end = (int32_t)(x.run_hi - x.contig_off);    // where the run ends at the latest: k_site_runs_finish walks up to it
        s.mismatch = 0; s.depth = 0;
        out[slot] = s;
    }
};

// of a run: the largest mismatch count and the depth at the FIRST base that reaches it -- the largest key
// (count << 32) | (0xFFFFFFFF - distance from the start) is the largest count at the smallest distance
struct MmBest {
    const int32_t* depth;
    typedef unsigned long long Acc;
    __device__ __forceinline__ Acc init() const { return 0ull; }
    __device__ __forceinline__ void take(Acc& best, int2 v, int64_t e, int64_t q0) const
    {
        const unsigned long long key = ((unsigned long long)(uint32_t)v.x << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(e - q0));
        best = key > best ? key : best;
    }
    __device__ __forceinline__ void wave(Acc& best) const { best = wave_max(best); }
    __device__ __forceinline__ void store(gci_mismatch_site& s, const Acc& best, int64_t q0) const
    {
        s.mismatch = (int32_t)(best >> 32);
        s.depth = depth[q0 + (best ? (int64_t)(0xFFFFFFFFu - (uint32_t)best) : 0)];      // (best != 0: the start is hot)
    }
};

static inline SiteMemo mm_site_ask(const int32_t* d_mismatch, const int32_t* d_depth, int32_t min_reads, int32_t frac_ppm, uint32_t n_windows)
{
    SiteMemo m;
    m.track[0] = d_mismatch; m.track[1] = d_depth; m.min_reads = min_reads; m.frac = frac_ppm; m.n_windows = n_windows;
    return m;
}

extern "C" int gci_mismatch_sites_size(gci_ctx* ctx, const int32_t* d_mismatch, const int32_t* d_depth, int32_t min_reads, int32_t frac_ppm,
                                       const gci_window* h_windows, uint32_t n_windows, uint64_t* h_n_sites)
{
    if (!ctx || !d_mismatch || !d_depth || !h_n_sites || min_reads < 1 || frac_ppm < 0 || frac_ppm > 1000000 || (n_windows && !h_windows))
        return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    if ((((uintptr_t)d_mismatch) | ((uintptr_t)d_depth)) & 15u) return GCI_E_INVALID;                        // whole tracks, as allocated
    return site_size<MmEmit>(ctx, HotMismatch{d_mismatch, d_depth, min_reads, (int64_t)frac_ppm},
                                        mm_site_ask(d_mismatch, d_depth, min_reads, frac_ppm, n_windows), h_windows, h_n_sites,
                                        "k_sites_count (mismatch)");
}

extern "C" int gci_mismatch_sites_write(gci_ctx* ctx, const int32_t* d_mismatch, const int32_t* d_depth, int32_t min_reads, int32_t frac_ppm,
                                        const gci_window* h_windows, uint32_t n_windows, gci_mismatch_site* d_out, uint64_t cap)
{
    if (!ctx || !d_mismatch || !d_depth || min_reads < 1 || (n_windows && !h_windows)) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    const HotMismatch hot{d_mismatch, d_depth, min_reads, (int64_t)frac_ppm};
    GCI_TRY((site_write(ctx, hot, mm_site_ask(d_mismatch, d_depth, min_reads, frac_ppm, n_windows), MmEmit{d_out}, d_out, cap,
                                           "k_sites_write (mismatch)")));
    const unsigned long long total = ctx->site_memo.total;
    if (!total) return GCI_OK;
    hipLaunchKernelGGL((k_site_runs_finish<HotMismatch, MmBest, gci_mismatch_site>), wave_grid(total), dim3(BLOCK), 0, ctx->stream, hot,
                       MmBest{d_depth}, (const int64_t*)ctx->d_off.p, d_out, total);
    LAUNCHCHK("k_site_runs_finish (mismatch)");
    return GCI_OK;
}

// ---- the track side of allele_sites.py ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t al_best(int32_t a, int32_t c, int32_t g, int32_t t) { return max(max(a, c), max(g, t)); }

struct HotAllele {                       // the LARGEST of the four allele tracks >= min_reads and / depth >= frac_ppm / 10^6, in 64 bits
    const int32_t* a;
    const int32_t* c;
    const int32_t* g;
    const int32_t* t;
    const int32_t* depth;
    int32_t min_reads;
    int64_t frac_ppm;
    __device__ __forceinline__ bool hot(int32_t best, int32_t d) const { return best >= min_reads && (int64_t)best * 1000000ll >= frac_ppm * (int64_t)d; }
    __device__ __forceinline__ uint32_t four(int64_t p) const
    {
        const int4 va = *reinterpret_cast<const int4*>(a + p), vc = *reinterpret_cast<const int4*>(c + p);
        const int4 vg = *reinterpret_cast<const int4*>(g + p), vt = *reinterpret_cast<const int4*>(t + p);
        const int4 d = *reinterpret_cast<const int4*>(depth + p);
        return (hot(al_best(va.x, vc.x, vg.x, vt.x), d.x) ? 1u : 0u) | (hot(al_best(va.y, vc.y, vg.y, vt.y), d.y) ? 2u : 0u) |
               (hot(al_best(va.z, vc.z, vg.z, vt.z), d.z) ? 4u : 0u) | (hot(al_best(va.w, vc.w, vg.w, vt.w), d.w) ? 8u : 0u);
    }
    typedef int2 Val;                    // (best, depth)
    __device__ __forceinline__ Val load(int64_t q) const { return make_int2(al_best(a[q], c[q], g[q], t[q]), depth[q]); }
    __device__ __forceinline__ bool is(Val v) const { return hot(v.x, v.y); }
    __device__ __forceinline__ bool one(int64_t q) const { return is(load(q)); }
};

struct AlleleEmit {                      // single elements, as ClipEmit: adjacent hot bases are adjacent sites
    static constexpr int LISTER = 4;
    static constexpr bool RUNS = false;
    HotAllele h;
    const uint8_t* codes;
    gci_allele_site* out;
    __device__ __forceinline__ void operator()(unsigned long long slot, const SiteTile& x, int64_t q) const
    {
        gci_allele_site s;
        s.contig = x.contig; s.pos = (int32_t)(q - x.contig_off);
        s.n[0] = h.a[q]; s.n[1] = h.c[q]; s.n[2] = h.g[q]; s.n[3] = h.t[q];
        const int32_t best = al_best(s.n[0], s.n[1], s.n[2], s.n[3]);
        s.alt = s.n[0] == best ? 1 : s.n[1] == best ? 2 : s.n[2] == best ? 4 : 8;          // a tie goes to the earlier letter
        s.ref = codes[q]; s.depth = h.depth[q];
        out[slot] = s;
    }
};

static inline SiteMemo al_site_ask(const HotAllele& h, const uint8_t* d_codes, uint32_t n_windows)
{
    SiteMemo m;
    m.track[0] = h.a; m.track[1] = h.c; m.track[2] = h.g; m.track[3] = h.t; m.track[4] = h.depth; m.track[5] = d_codes;
    m.min_reads = h.min_reads; m.frac = (int32_t)h.frac_ppm; m.n_windows = n_windows;
    return m;
}

extern "C" int gci_allele_sites_size(gci_ctx* ctx, const int32_t* d_a, const int32_t* d_c, const int32_t* d_g, const int32_t* d_t, const int32_t* d_depth,
                                     const uint8_t* d_codes, int32_t min_reads, int32_t frac_ppm, const gci_window* h_windows, uint32_t n_windows,
                                     uint64_t* h_n_sites)
{
    if (!ctx || !d_a || !d_c || !d_g || !d_t || !d_depth || !d_codes || !h_n_sites || min_reads < 1 || frac_ppm < 0 || frac_ppm > 1000000 ||
        (n_windows && !h_windows))
        return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    if ((((uintptr_t)d_a) | ((uintptr_t)d_c) | ((uintptr_t)d_g) | ((uintptr_t)d_t) | ((uintptr_t)d_depth)) & 15u) return GCI_E_INVALID;      // whole tracks
    const HotAllele hot{d_a, d_c, d_g, d_t, d_depth, min_reads, (int64_t)frac_ppm};
    return site_size<AlleleEmit>(ctx, hot, al_site_ask(hot, d_codes, n_windows), h_windows, h_n_sites, "k_sites_count (alleles)");
}

extern "C" int gci_allele_sites_write(gci_ctx* ctx, const int32_t* d_a, const int32_t* d_c, const int32_t* d_g, const int32_t* d_t, const int32_t* d_depth,
                                      const uint8_t* d_codes, int32_t min_reads, int32_t frac_ppm, const gci_window* h_windows, uint32_t n_windows,
                                      gci_allele_site* d_out, uint64_t cap)
{
    if (!ctx || !d_a || !d_c || !d_g || !d_t || !d_depth || !d_codes || min_reads < 1 || (n_windows && !h_windows)) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    const HotAllele hot{d_a, d_c, d_g, d_t, d_depth, min_reads, (int64_t)frac_ppm};
    return site_write(ctx, hot, al_site_ask(hot, d_codes, n_windows), AlleleEmit{hot, d_codes, d_out}, d_out, cap, "k_sites_write (alleles)");
}
