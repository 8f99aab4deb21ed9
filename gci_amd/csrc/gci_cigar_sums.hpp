// gci_cigar_sums.hpp -- the base totals of every CIGAR chunk (gci_cover_chunks.hpp), one wave per chunk: what the kernels that need
// a record's totals under S, M / = / X, I, D and N share (k_reads.hip: the columns of a row; k_sweep.hip: the two quotients of the
// record filter and the covered bases).  A lane per record then adds the sums of chunk0[i] .. chunk0[i + 1].
#pragma once
#include "gci_cover_chunks.hpp"

struct CigarSums { unsigned long long S, M, I, D, N, bad; };      // (bad: the chunk holds an operation code 9 - 15)

// one wave per chunk: the bases under S, M / = / X, I, D and N, summed over the wave; whether it holds a code 9 - 15; no atomics
static __global__ __launch_bounds__(BLOCK) void k_cigar_sums(const uint8_t* __restrict__ bam, uint64_t n_bytes, const CoverRec* __restrict__ recs,
                                                             const unsigned long long* __restrict__ chunk0, uint32_t n_rec,
                                                             unsigned long long n_chunks, CigarSums* __restrict__ sums)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long ch = (unsigned long long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (ch >= n_chunks) return;                        // (the whole wave)
    const uint32_t rec = cv_rec_of_chunk(chunk0, n_rec, ch);
    const CoverRec r = recs[rec];
    const CvChunk c = cv_chunk_of(bam, r, (uint32_t)(ch - chunk0[rec]));
    unsigned long long s = 0, m = 0, ins = 0, del = 0, skip = 0;
    bool bad = false;
    for (uint32_t k0 = 0; k0 < c.n; k0 += 64) {
        const uint32_t k = k0 + lane;
        const uint32_t v = cv_op_word(bam, n_bytes, c, k, lane);
        const uint32_t op = v & 0xFu, len = k < c.n ? v >> 4 : 0u;
        bad |= k < c.n && op >= 9u;
        s += op == 4u ? len : 0u;
        m += ((0x181u >> op) & 1u) ? len : 0u;                                   // M = X
        ins += op == 1u ? len : 0u;
        del += op == 2u ? len : 0u;
        skip += op == 3u ? len : 0u;
    }
    CigarSums t;
    t.S = wave_sum<unsigned long long>(s);
    t.M = wave_sum<unsigned long long>(m);
    t.I = wave_sum<unsigned long long>(ins);
    t.D = wave_sum<unsigned long long>(del);
    t.N = wave_sum<unsigned long long>(skip);
    t.bad = __ballot(bad) != 0ull ? 1ull : 0ull;
    if (lane == 0) sums[ch] = t;
}

// the launch: a wave per chunk, BLOCK / 64 chunks a workgroup (n_chunks > 0)
static inline dim3 cigar_sums_grid(unsigned long long n_chunks) { return wave_grid(n_chunks); }

// one lane per chunk: its reference length M + D + N and, with QRY, its query length S + M + I -- scanned, they are the carries that
// place an operation of chunk k on the two axes.  (Templates: a file that includes this header need not launch them.)
template <bool QRY>
__global__ __launch_bounds__(BLOCK) void k_chunk_lens(const CigarSums* __restrict__ sums, unsigned long long n_chunks,
                                                             unsigned long long* __restrict__ chunk_ref, unsigned long long* __restrict__ chunk_qry)
{
    const unsigned long long ch = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (ch >= n_chunks) return;
    const CigarSums s = sums[ch];
    chunk_ref[ch] = s.M + s.D + s.N;                   // (every total is below 2^57)
    if (QRY) chunk_qry[ch] = s.S + s.M + s.I;
}

// one lane per record: whether it is counted; codes 9 - 15 in its chunks and, with QRY -- seqs and qry0, the scan of k_chunk_lens'
// query lengths (not read where there are no chunks) --, S + M + I != l_seq into the status word
template <bool QRY>
__global__ __launch_bounds__(BLOCK) void k_rec_finish(uint32_t n_rec, const CoverRec* __restrict__ recs, const unsigned long long* __restrict__ chunk0,
                                                             const CigarSums* __restrict__ sums, const CvSeq* __restrict__ seqs,
                                                             const unsigned long long* __restrict__ qry0, uint32_t* __restrict__ counted,
                                                             unsigned long long* __restrict__ status)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_rec) return;
    uint32_t c = 0;
    if (recs[i].contig >= 0) {
        c = 1;
        unsigned long long bad = 0;
        const unsigned long long first = chunk0[i], last = chunk0[i + 1];
        for (unsigned long long ch = first; ch < last; ch++) bad |= sums[ch].bad;
        if (QRY) {
            const unsigned long long q = last > first ? qry0[last] - qry0[first] : 0ull;
            if (seqs[i].l_seq != 0 && q != (unsigned long long)seqs[i].l_seq) bad = 1;
        }
        if (bad) cv_report(status, i, GCI_E_MALFORMED);
    }
    counted[i] = c;
}

// The two launches: the flag comes from the arguments, so it cannot disagree with them.  chunk_qry / seqs == nullptr: no query side
// (n_chunks, n_rec > 0; the caller's LAUNCHCHK follows).
static inline void launch_chunk_lens(gci_ctx* ctx, const CigarSums* sums, unsigned long long n_chunks, unsigned long long* chunk_ref,
                                     unsigned long long* chunk_qry)
{
    const dim3 grid((uint32_t)((n_chunks + BLOCK - 1) / BLOCK));
    if (chunk_qry) hipLaunchKernelGGL(k_chunk_lens<true>, grid, dim3(BLOCK), 0, ctx->stream, sums, n_chunks, chunk_ref, chunk_qry);
    else hipLaunchKernelGGL(k_chunk_lens<false>, grid, dim3(BLOCK), 0, ctx->stream, sums, n_chunks, chunk_ref, chunk_qry);
}

static inline void launch_rec_finish(gci_ctx* ctx, uint32_t n_rec, const CoverRec* recs, const unsigned long long* chunk0, const CigarSums* sums,
                                     const CvSeq* seqs, const unsigned long long* qry0, uint32_t* counted, unsigned long long* status)
{
    const dim3 grid((n_rec + BLOCK - 1) / BLOCK);
    if (seqs) hipLaunchKernelGGL(k_rec_finish<true>, grid, dim3(BLOCK), 0, ctx->stream, n_rec, recs, chunk0, sums, seqs, qry0, counted, status);
    else hipLaunchKernelGGL(k_rec_finish<false>, grid, dim3(BLOCK), 0, ctx->stream, n_rec, recs, chunk0, sums, seqs, qry0, counted, status);
}
