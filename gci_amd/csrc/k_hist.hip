// k_hist.hip -- depth_dist.py: the depth histogram and the sum / min / max / count of a set of windows over a depth track, in ONE
// read of the windows.
//
// K8's windows and tiling (gci_set_windows, 4096-element tiles, int4 loads, bases outside [begin, end) masked off).  A workgroup
// takes GCI_HIST_CHUNK_TILES consecutive tiles of ONE window and keeps a private histogram of GCI_HIST_LDS_BINS uint32 counters in
// LDS for them (a chunk holds 2^18 elements, far below 2^32).  Depth is piecewise constant (about 20 events per tile), so the
// histogram is fed per RUN, not per base: a wave-instruction covers 256 consecutive elements, every lane flags the run heads among
// its four (k_bedgraph.hip's compare; the first in-window element of the wave's span is a head by position, so no predecessor is
// read), a ballot finds the lane of the next head, and the head adds the run's length inside the wave's span to its bin: a wave of
// one depth costs one LDS add, alternating depths one add per base.  Bins at or above GCI_HIST_LDS_BINS (n_bins may reach 65536;
// real data needs a few hundred) take the same per-run add as a 64-bit global atomic.  The two classes outside the bins -- over:
// depth >= n_bins, under: depth < 0 -- and the statistics are counted per base in registers.  At the end of its chunk the workgroup
// folds thread -> wave -> workgroup and flushes once: the non-zero bins, over and under with one 64-bit add each, then one add for
// the sum, one for the count, one signed atomicMin and one atomicMax.  Everything is an integer: exact, whatever the order.
#include "gci_ctx.hpp"

#define GCI_HIST_LDS_BINS 4096           // bins a workgroup keeps in LDS: 16 KB, nine workgroups (of the eight a CU's SIMDs hold) fit in 160 KB
static_assert((long long)GCI_HIST_CHUNK_TILES * TILE < (1ll << 32), "a chunk's counters are uint32");
static_assert(GCI_HIST_LDS_BINS % BLOCK == 0 && GCI_HIST_LDS_BINS <= GCI_HIST_MAX_BINS, "the flush walks the bins a workgroup at a time");

__device__ __forceinline__ int32_t hist_wave_min(int32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
    return v;
}

__device__ __forceinline__ int32_t hist_wave_max(int32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}

__global__ void k_hist_init(int64_t* __restrict__ stats, uint32_t n_win)
{
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_win) return;
    stats[4 * (size_t)w + 0] = 0;
    stats[4 * (size_t)w + 1] = INT32_MAX;
    stats[4 * (size_t)w + 2] = INT32_MIN;
    stats[4 * (size_t)w + 3] = 0;
}

// BINS: n_bins > 0 (the LDS histogram and the run heads); without it the per-base part alone (a statistics-only pass).
// hist == nullptr (legal with n_bins == 0 only): nothing is counted.
template <bool BINS>
__global__ __launch_bounds__(BLOCK) void k_depth_hist(const int32_t* __restrict__ depth, const gci_window* __restrict__ win,
                                                      const int64_t* __restrict__ win_tile_first,
                                                      const int64_t* __restrict__ win_chunk_first, int32_t n_win, uint32_t n_bins,
                                                      unsigned long long* __restrict__ hist, long long* __restrict__ stats)
{
    __shared__ uint32_t bins[BINS ? GCI_HIST_LDS_BINS : 1];
    __shared__ long long part_sum[BLOCK / 64];
    __shared__ int32_t part_min[BLOCK / 64], part_max[BLOCK / 64];
    __shared__ uint32_t part_over[BLOCK / 64], part_under[BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int32_t w = contig_of_tile(win_chunk_first, n_win, blockIdx.x);
    const gci_window W = win[w];
    const int64_t tiles = win_tile_first[w + 1] - win_tile_first[w];
    const int64_t t0 = ((int64_t)blockIdx.x - win_chunk_first[w]) * GCI_HIST_CHUNK_TILES;
    const int64_t t1 = min(t0 + GCI_HIST_CHUNK_TILES, tiles);
    const uint32_t lds_bins = min(n_bins, (uint32_t)GCI_HIST_LDS_BINS);
    unsigned long long* hw = hist ? hist + (size_t)w * ((size_t)n_bins + 2) : nullptr;
    if (BINS) {
        for (uint32_t b = t; b < lds_bins; b += BLOCK) bins[b] = 0;
        __syncthreads();
    }
    long long sum = 0;
    int32_t lo = INT32_MAX, hi = INT32_MIN;
    uint32_t over = 0, under = 0;
    for (int64_t tile = t0; tile < t1; tile++) {
        const int64_t p0 = (W.begin / TILE + tile) * TILE;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t p = p0 + (int64_t)(j * BLOCK + t) * 4;
            const int4 v = *reinterpret_cast<const int4*>(depth + p);
            const int32_t d[4] = {v.x, v.y, v.z, v.w};
            bool in[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                in[k] = (p + k >= W.begin) && (p + k < W.end);
                if (in[k]) {
                    sum += d[k];
                    lo = min(lo, d[k]);
                    hi = max(hi, d[k]);
                    under += d[k] < 0 ? 1u : 0u;
                    over += (d[k] >= 0 && (uint32_t)d[k] >= n_bins) ? 1u : 0u;
                }
            }
            if (!BINS) continue;
            // run heads inside the wave's span [ps, ps + 256): in the window, and the first such element or unlike the one before
            const int64_t ps = p - lane * 4;
            const int32_t prev = __shfl_up(v.w, 1, 64);                          // (lane 0: its own, unused -- its first in-window element is a head)
            const int64_t first = max(ps, W.begin);                             // the span's first in-window element, if it has one
            const int32_t span_end = (int32_t)min((int64_t)256, max((int64_t)0, W.end - ps));     // in-window elements end here, relative to ps
            uint32_t f = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const bool head = (p + k == first) || d[k] != (k ? d[k - 1] : prev);
                f |= (in[k] && head) ? (1u << k) : 0u;
            }
            const unsigned long long nz = __ballot(f != 0);
            if (nz == 0) continue;                                               // (the same in every lane: the span lies outside the window)
            const unsigned long long above = lane == 63 ? 0ull : nz & ~((2ull << lane) - 1ull);
            const int nl = above ? __builtin_ctzll(above) : lane;
            const int32_t their_first = __shfl(f ? __builtin_ctz(f) : 0, nl, 64);
            const int32_t next_head = above ? nl * 4 + their_first : span_end;   // relative to ps: where this lane's last run ends
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!((f >> k) & 1u)) continue;
                const uint32_t later = f >> (k + 1);
                const int32_t end = later ? lane * 4 + k + 1 + __builtin_ctz(later) : next_head;
                const uint32_t len = (uint32_t)(end - (lane * 4 + k));
                const uint32_t bin = (uint32_t)d[k];                             // (negative depths are above every n_bins)
                if (bin < lds_bins) atomicAdd(&bins[bin], len);
                else if (bin < n_bins) atomicAdd(hw + bin, (unsigned long long)len);
            }
        }
    }
    // fold: thread -> wave -> workgroup, then one flush for the chunk
    sum = wave_sum<long long>(sum);
    lo = hist_wave_min(lo);
    hi = hist_wave_max(hi);
    over = wave_sum<uint32_t>(over);
    under = wave_sum<uint32_t>(under);
    if (lane == 0) { part_sum[wave] = sum; part_min[wave] = lo; part_max[wave] = hi; part_over[wave] = over; part_under[wave] = under; }
    __syncthreads();                                                             // (and every LDS add of the chunk is done)
    if (BINS && hw) {
        for (uint32_t b = t; b < lds_bins; b += BLOCK) {
            const uint32_t c = bins[b];
            if (c) atomicAdd(hw + b, (unsigned long long)c);
        }
    }
    if (t == 0) {
        long long s = 0;
        int32_t mn = INT32_MAX, mx = INT32_MIN;
        uint32_t ov = 0, un = 0;
#pragma unroll
        for (int x = 0; x < BLOCK / 64; x++) { s += part_sum[x]; mn = min(mn, part_min[x]); mx = max(mx, part_max[x]); ov += part_over[x]; un += part_under[x]; }
        const int64_t a = max(W.begin, (W.begin / TILE + t0) * TILE), b = min(W.end, (W.begin / TILE + t1) * TILE);
        long long* st = stats + 4 * (size_t)w;
        if (s) atomicAdd((unsigned long long*)st, (unsigned long long)s);
        __hip_atomic_fetch_min(st + 1, (long long)mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(st + 2, (long long)mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicAdd((unsigned long long*)(st + 3), (unsigned long long)(b - a));
        if (hw) {
            if (ov) atomicAdd(hw + n_bins, (unsigned long long)ov);
            if (un) atomicAdd(hw + n_bins + 1, (unsigned long long)un);
        }
    }
}

extern "C" int gci_depth_hist(gci_ctx* ctx, const int32_t* d_depth, const gci_window* h_windows, uint32_t n_windows, uint32_t n_bins,
                              uint64_t* d_hist, int64_t* d_stats)
{
    if (!ctx || !d_depth || (n_windows && (!h_windows || !d_stats || (n_bins && !d_hist)))) return GCI_E_INVALID;
    if (n_bins > GCI_HIST_MAX_BINS) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    if (n_windows >= (1u << 31)) return GCI_E_INVALID;
    // a window's tiles in chunks of GCI_HIST_CHUNK_TILES, one workgroup each (the tiles as gci_set_windows counts them)
    std::vector<int64_t> chunk_first((size_t)n_windows + 1);
    int64_t chunks = 0;
    for (uint32_t i = 0; i < n_windows; i++) {
        gci_window w = h_windows[i];
        if (w.begin < 0) w.begin = 0;
        if (w.end > ctx->total) w.end = ctx->total;
        chunk_first[i] = chunks;
        if (w.end > w.begin) chunks += ((w.end + TILE - 1) / TILE - w.begin / TILE + GCI_HIST_CHUNK_TILES - 1) / GCI_HIST_CHUNK_TILES;
    }
    chunk_first[n_windows] = chunks;
    if (chunks > 0x7FFFFFFFll) return GCI_E_INVALID;
    GCI_TRY(gci_set_windows(ctx, h_windows, n_windows));
    ctx->win_flank = INT32_MIN;
    if (!n_windows) return GCI_OK;
    GCI_TRY(gci_ensure(ctx, ctx->hist_chunk_first, ((size_t)n_windows + 1) * 8));
    GCI_TRY(gci_upload_small(ctx, ctx->hist_chunk_first.p, chunk_first.data(), chunk_first.size() * 8));
    if (d_hist) HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)n_windows * ((size_t)n_bins + 2) * 8, ctx->stream));
    hipLaunchKernelGGL(k_hist_init, dim3((n_windows + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, ctx->stream, d_stats, n_windows);
    LAUNCHCHK("k_hist_init");
    if (chunks == 0) return GCI_OK;
    if (n_bins)
        hipLaunchKernelGGL(k_depth_hist<true>, dim3((uint32_t)chunks), dim3(BLOCK), 0, ctx->stream, d_depth, (const gci_window*)ctx->win.p,
                           (const int64_t*)ctx->win_tile_first.p, (const int64_t*)ctx->hist_chunk_first.p, (int32_t)n_windows, n_bins,
                           (unsigned long long*)d_hist, (long long*)d_stats);
    else
        hipLaunchKernelGGL(k_depth_hist<false>, dim3((uint32_t)chunks), dim3(BLOCK), 0, ctx->stream, d_depth, (const gci_window*)ctx->win.p,
                           (const int64_t*)ctx->win_tile_first.p, (const int64_t*)ctx->hist_chunk_first.p, (int32_t)n_windows, n_bins,
                           (unsigned long long*)d_hist, (long long*)d_stats);
    LAUNCHCHK("k_depth_hist");
    return GCI_OK;
}
