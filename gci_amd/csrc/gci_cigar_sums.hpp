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
static inline dim3 cigar_sums_grid(unsigned long long n_chunks) { return dim3((uint32_t)((n_chunks + BLOCK / 64 - 1) / (BLOCK / 64))); }
