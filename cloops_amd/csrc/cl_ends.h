// cl_ends.h -- the end points of a resident chromosome as sorted keys: the key pass, the LDS-or-global accessor over the sorted array
// and the galloping searches, shared by K20 (k_cover.hip) and K21 (k_peak.hip).
#pragma once
#include "cl_common.h"

#define K20_ITEMS 8                     // rows per thread of the key pass
#define K20_ROWS (TPB * K20_ITEMS)      // rows per workgroup of the key pass: 2048
#define K20_LIMIT ((1ll << 31) - 4096)  // end points a build takes (ranks and run numbers are 32-bit)

enum { K20_NENDS = 0, K20_MAXD = 1, K20_AREA = 2, K20_CTRS = 4 };       // c->cv.ctr, u64 each

__device__ __forceinline__ int k20_floor_div(int p, int res)
{
    const int q = p / res;
    return q - ((p % res) < 0 ? 1 : 0);
}

// the kept end points of every workgroup's rows as keys, in any order: slots [base, base + its count) from one atomic
static __global__ void __launch_bounds__(TPB)
k20_keys(const int* __restrict__ X, const int* __restrict__ Y, int n, long long cut, int ends, int res, int vmin, u32* __restrict__ key,
         u64* __restrict__ ctr)
{
    __shared__ u32 pre[K20_ITEMS * (TPB / 64)];
    __shared__ u32 base;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ne = (ends & 1) + ((ends >> 1) & 1);
    const long long t0 = (long long)blockIdx.x * K20_ROWS;
    u64 bal[K20_ITEMS];
    int xs[K20_ITEMS], ys[K20_ITEMS];
#pragma unroll
    for (int u = 0; u < K20_ITEMS; ++u) {
        const long long r = t0 + u * TPB + threadIdx.x;
        bool keep = false;
        xs[u] = ys[u] = 0;
        if (r < n) {
            xs[u] = X[r]; ys[u] = Y[r];
            keep = cut <= 0 || (long long)ys[u] - (long long)xs[u] >= cut;
        }
        bal[u] = __ballot(keep);
        if (lane == 0) pre[u * (TPB / 64) + w] = (u32)__popcll(bal[u]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 s = 0;
        for (int k = 0; k < K20_ITEMS * (TPB / 64); ++k) { const u32 v = pre[k]; pre[k] = s; s += v; }
        base = s ? (u32)atomicAdd(&ctr[K20_NENDS], (u64)s * (u64)ne) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < K20_ITEMS; ++u)
        if ((bal[u] >> lane) & 1) {
            const u32 rank = pre[u * (TPB / 64) + w] + (u32)__builtin_amdgcn_mbcnt_hi((u32)(bal[u] >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal[u], 0u));
            u32 slot = base + rank * (u32)ne;
            if (ends & 1) key[slot++] = (u32)((res ? k20_floor_div(xs[u], res) : xs[u]) - vmin);
            if (ends & 2) key[slot] = (u32)((res ? k20_floor_div(ys[u], res) : ys[u]) - vmin);
        }
}

// S through the LDS window [base, base + span) where it covers the element, through global memory elsewhere
struct K20Keys {
    const u32* __restrict__ g;
    const u32* l;
    int base, span, vmin;
    __device__ __forceinline__ int at(int j) const
    {
        const u32 o = (u32)(j - base);
        return (int)(o < (u32)span ? l[o] : g[j]) + vmin;
    }
};

// the first index of [j0, m] whose value exceeds v, given that every element below j0 does not: gallop upwards, then bisect
// (the gallop's probes are 64-bit: a step may reach past 2^31 before the test against m ends it)
__device__ __forceinline__ int k20_ub_up(const K20Keys& S, int m, int j0, int v)
{
    long long lo = j0, step = 1;
    while (lo + step - 1 < m && S.at((int)(lo + step - 1)) <= v) { lo += step; step <<= 1; }
    long long hi = lo + step - 1 < m ? lo + step - 1 : m;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (S.at((int)mid) <= v) lo = mid + 1; else hi = mid;
    }
    return (int)lo;
}

// the first index of [0, j0] whose value exceeds v, given that every element from j0 on does: gallop downwards, then bisect
__device__ __forceinline__ int k20_ub_down(const K20Keys& S, int j0, int v)
{
    long long hi = j0, step = 1;
    while (hi - step >= 0 && S.at((int)(hi - step)) > v) { hi -= step; step <<= 1; }
    long long lo = hi - step + 1 > 0 ? hi - step + 1 : 0;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (S.at((int)mid) <= v) lo = mid + 1; else hi = mid;
    }
    return (int)lo;
}
