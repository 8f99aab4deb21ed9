// gci_ratio.hpp -- the comparison of a quotient of two base counts with a threshold as the reference makes it (GCI.py:165), shared
// by the record filter (k_filter.hip) and the per-record verdict (k_fate.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// (double)a / (double)b  <=  c  (le) or  >=  c  (!le), b != 0: the reference's IEEE f64 division and comparison (GCI.py:165),
// bit for bit.  An f64 division is ~40 instructions a wave executes for all its lanes, and almost no record is anywhere near a
// threshold: a single-precision quotient (relative error < 1e-6) decides whenever it is further than 1e-4 from the threshold --
// rounding is monotonic, so the f64 quotient falls on the same side -- and only the records in between take the division.
__device__ __forceinline__ bool ratio_cmp(int64_t a, int64_t b, double c, bool le)
{
    if (((a < 0 ? -a : a) | b) >> 30 == 0) {                     // both convert to f32 through the 32-bit path
        const float x = (float)(int32_t)a * __builtin_amdgcn_rcpf((float)(int32_t)b);
        const float cf = (float)c, m = 1e-4f * fmaxf(1.0f, fabsf(x));
        if (c == c && fabs(c) < 1e30) {                          // (a NaN or absurd threshold: the exact comparison below)
            if (x < cf - m) return le;
            if (x > cf + m) return !le;
        }
    }
    const double q = (double)a / (double)b;
    return le ? q <= c : q >= c;
}
