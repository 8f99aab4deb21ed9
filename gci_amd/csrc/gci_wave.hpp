// gci_wave.hpp -- scans and sums across a wave (64 lanes) and across a workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- wave-level scans and sums -------------------------------------------------------------------
// 32-bit values go through DPP (one v_add_*_dpp per step: row_shr 1/2/4/8 inside each 16-lane row, then
// row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3); 64-bit values through ds_bpermute.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int32_t dpp_add(int32_t v)
{
    return v + __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, true);
}

__device__ __forceinline__ int32_t wave_inclusive_i32(int32_t v)
{
    v = dpp_add<0x111, 0xF>(v);
    v = dpp_add<0x112, 0xF>(v);
    v = dpp_add<0x114, 0xF>(v);
    v = dpp_add<0x118, 0xF>(v);
    v = dpp_add<0x142, 0xA>(v);
    v = dpp_add<0x143, 0xC>(v);
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_inclusive(T v, int lane)
{
    if constexpr (sizeof(T) == 4) {
        return (T)wave_inclusive_i32((int32_t)v);
    } else {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { T n = __shfl_up(v, d, 64); if (lane >= d) v += n; }
        return v;
    }
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
    if constexpr (sizeof(T) == 4) {
        return (T)__builtin_amdgcn_readlane(wave_inclusive_i32((int32_t)v), 63);
    } else {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        return v;
    }
}

template <typename T>
__device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const T o = __shfl_xor(v, m, 64); v = o > v ? o : v; }
    return v;
}

// the lanes below `lane`, as a ballot's mask
__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// ---- workgroup exclusive scan -----------------------------------------------------------------------
// Exclusive prefix of `v` over the NWAVES * 64 threads of a one-dimensional workgroup, and in `total` the sum over all of
// them: a wave scan, the wave totals through LDS, then the totals of the waves in front.  All threads of the workgroup call it.
// The caller owns wtot[NWAVES] (LDS).  There is ONE barrier inside, between writing wtot and reading it; none follows the
// reads.  So a caller that hands the same array in again (a loop, a second scan) puts a __syncthreads() between the two calls.
// Whatever the caller wrote to LDS before the call is visible to the whole workgroup after it.
template <typename T, int NWAVES>
__device__ __forceinline__ T block_exclusive(T v, T* wtot, T& total)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const T inc = wave_inclusive<T>(v, lane);
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    T pre = inc - v, all = 0;
#pragma unroll
    for (int w = 0; w < NWAVES; w++) { if (w < wave) pre += wtot[w]; all += wtot[w]; }
    total = all;
    return pre;
}
