// cl_text.h -- decimal text of int64 values on the device, as Python's str(int) prints them: shared by the text kernels K14
// (k_track.hip) and K15 (k_convert.hip).
#pragma once
#include "cl_common.h"

__device__ __forceinline__ u64 cl_mag(long long v) { return v < 0 ? 0ull - (u64)v : (u64)v; }

__device__ __forceinline__ int cl_ndig(u64 m)                          // decimal digits of m (1 for 0)
{
    int d = 1;
    u64 p = 10;
#pragma unroll
    for (int k = 1; k < 20; ++k) { d += m >= p ? 1 : 0; p = k < 19 ? p * 10 : p; }
    return d;
}

__device__ __forceinline__ int cl_width(long long v) { return (v < 0 ? 1 : 0) + cl_ndig(cl_mag(v)); }

// v in decimal at s[pos ..] -> the position after it
__device__ __forceinline__ int cl_put(char* s, int pos, long long v)
{
    u64 m = cl_mag(v);
    if (v < 0) s[pos++] = '-';
    const int e = pos + cl_ndig(m);
    int k = e - 1;
    while (m >> 32) {                                                   // m / 10 by multiply-high (exact for every u64)
        const u64 q = __umul64hi(m, 0xCCCCCCCCCCCCCCCDull) >> 3;
        s[k--] = (char)('0' + (int)(m - q * 10));
        m = q;
    }
    u32 w = (u32)m;
    for (; k >= pos; --k) { s[k] = (char)('0' + (int)(w % 10)); w /= 10; }
    return e;
}
