// k_records.hip -- N1 on the GPU: the BAM record walk without its serial chain (what pysam / htslib do for the reference at
// GCI.py:150-151; k_inflate.hip inflates the stream this walks).
//
// gci_bam_record_offsets_device: the offsets of the records of an inflated BAM stream WITHOUT walking the block_size
// chain serially (137 k dependent loads of ~1 us each at chr19): every byte position is tested for "a record could
// start here" (block_size, refID, pos, l_read_name, l_seq, next_refID, next_pos consistent with the format -- SEQ / QUAL
// bytes never pass), each candidate's successor (offset + 4 + block_size) is looked up among the candidates, and the
// candidates reachable from the first record are found by pointer doubling.  The chain must end exactly at the end of
// the stream (or, for a chunk, in a record that runs past it); otherwise -- a record the strict test rejects -- the call
// reports GCI_E_MALFORMED and the caller takes the host path.
#include "gci_ctx.hpp"

namespace {

// "A BAM record could start at p": every field a well-formed record constrains (SAM spec 4.2) -- block_size >= 32, refID and
// next_refID in [-1, n_ref), pos and next_pos >= -1, l_read_name >= 1, l_seq >= 0, and the fixed part + name + CIGAR + SEQ +
// QUAL fit in block_size.
// One thread looks at 16 consecutive byte positions of the stream: their 52 bytes as four aligned 16-byte loads (`s_al` is the
// stream's address rounded down to 16 bytes, `delta` what was cut off), every field re-aligned in registers.  refID is
// tested first: SEQ / QUAL bytes and text almost never form a value in [-1, n_ref), so the full test runs for few positions.
__device__ __forceinline__ uint4 cand_load(const uint8_t* __restrict__ s_al, uint64_t q, uint64_t n_phys)
{
    if (q + 16 <= n_phys) return *reinterpret_cast<const uint4*>(s_al + q);
    uint32_t w[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    for (int k = 0; k < 16; k++)
        if (q + k < n_phys) w[k >> 2] = (w[k >> 2] & ~(0xFFu << (8 * (k & 3)))) | ((uint32_t)s_al[q + k] << (8 * (k & 3)));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(BLOCK) void k_rec_candidates(const uint8_t* __restrict__ s_al, uint32_t delta, uint64_t lo, uint64_t n, int32_t n_ref,
                                                          const uint32_t* __restrict__ tile_off, uint32_t* __restrict__ tile_count,
                                                          uint64_t* __restrict__ cand)
{
    __shared__ uint32_t wtot[BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t n_phys = n + delta;
    const uint64_t q0 = (uint64_t)blockIdx.x * TILE + (uint64_t)t * 16;      // physical offset of this thread's first position
    uint32_t d[17];
    {
        const uint4 v0 = cand_load(s_al, q0, n_phys), v1 = cand_load(s_al, q0 + 16, n_phys), v2 = cand_load(s_al, q0 + 32, n_phys),
                    v3 = cand_load(s_al, q0 + 48, n_phys);
        const uint32_t tmp[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
#pragma unroll
        for (int k = 0; k < 16; k++) d[k] = tmp[k];
        d[16] = 0xFFFFFFFFu;
    }
    uint32_t mask = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        // dword k of the record that would start at byte i of the window
#define FIELD(k) ((int32_t)__builtin_amdgcn_alignbyte(d[((i) >> 2) + (k) + 1], d[((i) >> 2) + (k)], (i) & 3))
        const int32_t ref_id = FIELD(1);
        if (ref_id < -1 || ref_id >= n_ref) continue;
        const uint64_t q = q0 + i;
        if (q < lo + delta || q + 36 > n_phys) continue;
        const int32_t block_size = FIELD(0), pos = FIELD(2), l_seq = FIELD(5), next_ref = FIELD(6), next_pos = FIELD(7);
        const uint32_t l_read_name = (uint32_t)FIELD(3) & 0xFFu, n_cigar = (uint32_t)FIELD(4) & 0xFFFFu;
#undef FIELD
        if (block_size < 32 || pos < -1 || l_read_name < 1 || l_seq < 0 || next_ref < -1 || next_ref >= n_ref || next_pos < -1) continue;
        const uint64_t need = 32ull + l_read_name + 4ull * n_cigar + (((uint64_t)(uint32_t)l_seq + 1) >> 1) + (uint64_t)(uint32_t)l_seq;
        if (need <= (uint64_t)(uint32_t)block_size) mask |= 1u << i;
    }
    const uint32_t cnt = (uint32_t)__builtin_popcount(mask);
    const uint32_t inc = wave_inclusive<uint32_t>(cnt, lane);
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    if (!cand) {                                                             // counting pass
        if (t == 0) tile_count[blockIdx.x] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
        return;
    }
    uint32_t w = tile_off[blockIdx.x] + inc - cnt;
    for (int k = 0; k < wave; k++) w += wtot[k];
    for (uint32_t m = mask; m; m &= m - 1) cand[w++] = q0 + (uint32_t)__builtin_ctz(m) - delta;
}

#define NODE_END 0xFFFFFFFEu          // the record ends exactly at the end of the stream
#define NODE_TAIL 0xFFFFFFFDu         // the record runs past the end of the stream (a chunk's partial last record)
#define NODE_HEAD 0xFFFFFFFCu         // the record is complete and fewer than 36 bytes follow it (a chunk's partial record head)
#define NODE_NONE 0xFFFFFFFFu         // its successor is not a candidate: not on the chain (or the chain is broken there)
__global__ __launch_bounds__(BLOCK) void k_rec_link(const uint8_t* __restrict__ s, uint64_t n, const uint64_t* __restrict__ cand, uint32_t nc,
                                                    uint32_t* __restrict__ next)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nc) return;
    const uint64_t p = cand[i];
    int32_t bs;
    __builtin_memcpy(&bs, s + p, 4);                                         // (a byte-wise copy: p has any alignment)
    const uint64_t q = p + 4 + (uint64_t)(uint32_t)bs;
    uint32_t r = NODE_NONE;
    if (q == n) r = NODE_END;
    else if (q > n) r = NODE_TAIL;
    else {
        uint32_t lo = i + 1, hi = nc;                                        // first candidate >= q
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (cand[mid] < q) lo = mid + 1; else hi = mid; }
        if (lo < nc && cand[lo] == q) r = lo;
        else if (q + 36 > n) r = NODE_HEAD;                                   // fewer than 36 bytes left: a partial record head
    }
    next[i] = r;
}

// jump_out[i] = jump_in[jump_in[i]] (terminal values stay)
__global__ __launch_bounds__(BLOCK) void k_rec_double(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t nc)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nc) return;
    const uint32_t a = in[i];
    out[i] = a < nc ? in[a] : a;
}

// marked nodes mark their 2^k-th successor
__global__ __launch_bounds__(BLOCK) void k_rec_mark(const uint32_t* __restrict__ jump, uint32_t* __restrict__ mark, uint32_t nc)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nc || !mark[i]) return;
    const uint32_t a = jump[i];
    if (a < nc) mark[a] = 1u;
}

__global__ __launch_bounds__(BLOCK) void k_rec_emit(const uint8_t* __restrict__ s, const uint64_t* __restrict__ cand,
                                                    const uint32_t* __restrict__ mark, const uint32_t* __restrict__ pos,
                                                    const uint32_t* __restrict__ next, uint32_t nc, uint64_t n, uint64_t* __restrict__ offs,
                                                    uint64_t cap, uint64_t* __restrict__ result)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nc || !mark[i]) return;
    const uint32_t nx = next[i];
    // the last record of the chain decides how the walk ended: result[1] = bytes consumed, result[2] = 0 ok / 1 broken
    if (nx == NODE_TAIL) { result[1] = cand[i]; return; }                    // partial last record: not emitted
    if (pos[i] < cap) offs[pos[i]] = cand[i];
    if (nx == NODE_END) result[1] = n;
    else if (nx == NODE_HEAD) { int32_t bs; __builtin_memcpy(&bs, s + cand[i], 4); result[1] = cand[i] + 4 + (uint64_t)(uint32_t)bs; }
    else if (nx == NODE_NONE) { result[1] = cand[i]; result[2] = 1; }
}

__global__ __launch_bounds__(BLOCK) void k_rec_flags(const uint32_t* __restrict__ mark, const uint32_t* __restrict__ next, uint32_t nc,
                                                     uint32_t* __restrict__ flag)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < nc) flag[i] = (mark[i] && next[i] != NODE_TAIL) ? 1u : 0u;
}

}  // namespace

// d_result (device, 3 x uint64): [0] = number of records, [1] = bytes consumed (n_bytes when the last record ends there, else
// the offset of the partial last record), [2] = 0 ok / 1 the chain broke at offset [1] (GCI_E_MALFORMED on the host side).
// d_offs: up to `cap` offsets; [0] may exceed cap (call again with more room).  first_record: offset of the first record
// (the end of the BAM header), which must pass the strict test itself.
extern "C" int gci_bam_record_offsets_device(gci_ctx* ctx, const uint8_t* d_stream, uint64_t n_bytes, uint64_t first_record, int32_t n_ref,
                                             uint64_t* d_offs, uint64_t cap, uint64_t* d_result)
{
    if (!ctx || !d_result || (n_bytes && !d_stream) || first_record > n_bytes || (cap && !d_offs)) return GCI_E_INVALID;
    hipStream_t st = ctx->stream;
    {
        const uint64_t init[3] = {0, first_record, 0};
        GCI_TRY(gci_upload_small(ctx, d_result, init, sizeof init));
    }
    if (n_bytes - first_record < 36) return GCI_OK;                            // no complete record head: everything is tail
    // the candidate test walks the stream in tiles of TILE bytes counted from its address rounded down to 16 bytes
    const uint32_t delta = (uint32_t)((uintptr_t)d_stream & 15u);
    const uint8_t* s_al = d_stream - delta;
    const uint64_t n_tiles64 = (n_bytes + delta + TILE - 1) / TILE;
    if (n_tiles64 > 0x7fffffffULL) return GCI_E_INVALID;
    const uint32_t n_tiles = (uint32_t)n_tiles64;
    GCI_TRY(gci_ensure(ctx, ctx->part_hist, (size_t)(n_tiles + 2) * 4));
    GCI_TRY(gci_ensure(ctx, ctx->part_blk, (size_t)(n_tiles / TILE + 2) * 4));
    uint32_t* d_tile = (uint32_t*)ctx->part_hist.p;
    hipLaunchKernelGGL(k_rec_candidates, dim3(n_tiles), dim3(BLOCK), 0, st, s_al, delta, first_record, n_bytes, n_ref, (const uint32_t*)nullptr,
                       d_tile, (uint64_t*)nullptr);
    LAUNCHCHK("k_rec_candidates(count)");
    int r = device_exclusive_scan<uint32_t, uint32_t>(ctx, d_tile, d_tile, (uint32_t*)ctx->part_blk.p, (int64_t)n_tiles, true);
    if (r) return r;
    uint32_t nc = 0;
    HIPCHK(hipMemcpyAsync(&nc, d_tile + n_tiles, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nc == 0) { const uint64_t res[3] = {0, first_record, 1}; return gci_upload_small(ctx, d_result, res, sizeof res); }
    // candidates (u64) | next, jump a, jump b, mark, flag, pos (u32 each)
    GCI_TRY(gci_ensure(ctx, ctx->part_a, (size_t)nc * 8 + 64));
    GCI_TRY(gci_ensure(ctx, ctx->part_b, (size_t)(nc + 1) * 4 * 6 + 64));
    uint64_t* d_cand = (uint64_t*)ctx->part_a.p;
    uint32_t* d_next = (uint32_t*)ctx->part_b.p;
    uint32_t* d_ja = d_next + (nc + 1);
    uint32_t* d_jb = d_ja + (nc + 1);
    uint32_t* d_mark = d_jb + (nc + 1);
    uint32_t* d_flag = d_mark + (nc + 1);
    uint32_t* d_pos = d_flag + (nc + 1);
    hipLaunchKernelGGL(k_rec_candidates, dim3(n_tiles), dim3(BLOCK), 0, st, s_al, delta, first_record, n_bytes, n_ref, (const uint32_t*)d_tile,
                       (uint32_t*)nullptr, d_cand);
    LAUNCHCHK("k_rec_candidates(write)");
    const dim3 grid((nc + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(k_rec_link, grid, dim3(BLOCK), 0, st, d_stream, n_bytes, (const uint64_t*)d_cand, nc, d_next);
    LAUNCHCHK("k_rec_link");
    // The first record must be the first candidate.  Marks spread from it by pointer doubling: the 2^k-step successor
    // tables are built bottom up and kept on the device one after the other would need K tables; instead the marks are
    // spread bottom up as well -- after round k every node within 2^(k+1) - 1 steps of a marked node is marked, because
    // round k marks the 2^k-th successors of ALL nodes marked so far (distances 0 .. 2^k - 1 from node 0 become
    // 0 .. 2^(k+1) - 1).
    HIPCHK(hipMemsetAsync(d_mark, 0, (size_t)nc * 4, st));
    {
        uint64_t first_cand = 0;
        HIPCHK(hipMemcpyAsync(&first_cand, d_cand, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (first_cand != first_record) { const uint64_t res[3] = {0, first_record, 1}; return gci_upload_small(ctx, d_result, res, sizeof res); }
        const uint32_t one = 1;
        GCI_TRY(gci_upload_small(ctx, d_mark, &one, 4));
    }
    HIPCHK(hipMemcpyAsync(d_ja, d_next, (size_t)nc * 4, hipMemcpyDeviceToDevice, st));
    uint32_t* jin = d_ja;
    uint32_t* jout = d_jb;
    for (uint64_t reach = 1; reach < (uint64_t)nc; reach <<= 1) {
        hipLaunchKernelGGL(k_rec_mark, grid, dim3(BLOCK), 0, st, (const uint32_t*)jin, d_mark, nc);
        hipLaunchKernelGGL(k_rec_double, grid, dim3(BLOCK), 0, st, (const uint32_t*)jin, jout, nc);
        uint32_t* t = jin; jin = jout; jout = t;
    }
    hipLaunchKernelGGL(k_rec_mark, grid, dim3(BLOCK), 0, st, (const uint32_t*)jin, d_mark, nc);
    LAUNCHCHK("k_rec_mark");
    hipLaunchKernelGGL(k_rec_flags, grid, dim3(BLOCK), 0, st, (const uint32_t*)d_mark, (const uint32_t*)d_next, nc, d_flag);
    LAUNCHCHK("k_rec_flags");
    GCI_TRY(gci_ensure(ctx, ctx->part_blk, (size_t)(nc / TILE + 2) * 4));
    r = device_exclusive_scan<uint32_t, uint32_t>(ctx, d_flag, d_pos, (uint32_t*)ctx->part_blk.p, (int64_t)nc, true);
    if (r) return r;
    hipLaunchKernelGGL(k_rec_emit, grid, dim3(BLOCK), 0, st, d_stream, (const uint64_t*)d_cand, (const uint32_t*)d_mark, (const uint32_t*)d_pos,
                       (const uint32_t*)d_next, nc, n_bytes, d_offs, cap, d_result);
    LAUNCHCHK("k_rec_emit");
    // the count: d_pos[nc] (u32) -> d_result[0] (u64)
    uint32_t n_rec = 0;
    HIPCHK(hipMemcpyAsync(&n_rec, d_pos + nc, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t n64 = n_rec;
    GCI_TRY(gci_upload_small(ctx, d_result, &n64, 8));
    return GCI_OK;
}
