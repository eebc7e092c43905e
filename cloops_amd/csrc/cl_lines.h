// cl_lines.h -- the text layer shared by the kernels that read lines of raw bytes, K15 (k_convert.hip) and K16 (k_ingest.hip): the
// '\n' SWAR mask, the line index (k15_count / k15_lines: a count per 16 KiB tile, the caller's exclusive scan of the counts, an
// ordered write of every line's end) and the word-cached byte reader K15Rd.
#pragma once
#include "cl_common.h"

#define K15_U 4                                  // 16-byte words per thread of an index tile
#define K15_TILE (TPB * K15_U * 16)              // bytes per index tile: 16 KiB
#define K15_PAD 64                               // device bytes past a chunk (16-byte loads of its last word, the added '\n')

// bit b: byte b of the 16 is '\n'; bytes at or past `left` do not count
__device__ __forceinline__ u32 k15_nlmask(uint4 v, long long left)
{
    const u32 w[4] = {v.x, v.y, v.z, v.w};
    u32 m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const u32 x = w[i] ^ 0x0a0a0a0au;
        const u32 t = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);    // 0x80 in exactly the bytes of x that are zero
        m |= (((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u)) << (4 * i);
    }
    return left >= 16 ? m : (left <= 0 ? 0u : m & ((1u << left) - 1u));
}

static __global__ void __launch_bounds__(TPB)
k15_count(const uint4* __restrict__ in, long long n, u32* __restrict__ tcnt)
{
    __shared__ int wc[TPB / 64];
    const long long t0 = (long long)blockIdx.x * K15_TILE;
    int cnt = 0;
#pragma unroll
    for (int u = 0; u < K15_U; ++u) {
        const long long pos = t0 + ((long long)u * TPB + threadIdx.x) * 16;
        if (pos < n) cnt += __popc(k15_nlmask(in[pos >> 4], n - pos));
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tcnt[blockIdx.x] = (u32)(wc[0] + wc[1] + wc[2] + wc[3]);
}

// the ends of the lines of every tile at toff[tile] onwards, in byte order (only the first lmax of the chunk are kept)
static __global__ void __launch_bounds__(TPB)
k15_lines(const uint4* __restrict__ in, long long n, const u32* __restrict__ toff, long long lmax, u32* __restrict__ ends)
{
    __shared__ u32 ws[K15_U][TPB / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long t0 = (long long)blockIdx.x * K15_TILE;
    u32 m[K15_U];
    int inc[K15_U];
#pragma unroll
    for (int u = 0; u < K15_U; ++u) {
        const long long pos = t0 + ((long long)u * TPB + threadIdx.x) * 16;
        m[u] = pos < n ? k15_nlmask(in[pos >> 4], n - pos) : 0u;
        int s = __popc(m[u]);
        for (int o = 1; o < 64; o <<= 1) {                            // inclusive scan over the wave
            const int t = __shfl_up(s, o);
            if (lane >= o) s += t;
        }
        inc[u] = s;
        if (lane == 63) ws[u][w] = (u32)s;
    }
    __syncthreads();
    u32 base = toff[blockIdx.x];
#pragma unroll
    for (int u = 0; u < K15_U; ++u) {
        u32 k = base + (u32)(inc[u] - __popc(m[u]));
        for (int v = 0; v < w; ++v) k += ws[u][v];
        const long long pos = t0 + ((long long)u * TPB + threadIdx.x) * 16;
        u32 mm = m[u];
        while (mm) {
            const int b = __builtin_ctz(mm);
            mm &= mm - 1;
            if ((long long)k < lmax) ends[k] = (u32)(pos + b);
            ++k;
        }
        for (int v = 0; v < TPB / 64; ++v) base += ws[u][v];
    }
}

// bytes of the chunk, one aligned 8-byte word per read: from the chunk in global memory (a0 = 0) or from the tile staged in LDS
// (chunk byte a0, a multiple of 16, at LDS byte 0)
struct K15Rd {
    const u64* g;
    long long a0, wi;
    u64 w;
    __device__ __forceinline__ u32 at(long long q)
    {
        const long long i = (q - a0) >> 3;
        if (i != wi) { wi = i; w = g[i]; }
        return (u32)(w >> ((q & 7) << 3)) & 0xffu;
    }
};
