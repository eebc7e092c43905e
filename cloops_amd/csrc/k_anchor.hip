// k_anchor.hip -- K13: the rows of a resident chromosome with an end inside a loop anchor (scripts/jd2cleanWashuPETs.py) --
// host merge of the anchors, kernels and C entry point.
#include "cl_chrom.h"

// ==========================================================================================
// K13: anchor membership of every PET (scripts/jd2cleanWashuPETs.py:162-227)
// ==========================================================================================
// The script merges the anchors of its loops until no two overlap or touch (mergeAllAnchors / getAnchors, quadratic in the anchor
// count), then collects the rows whose X or Y lies in a merged anchor with dicts of row lists and a set.  Here the merge is a sort
// and a sweep on the host, and the rows come back as a bit per row: bit r % 64 of word r / 64 is set iff X[r] or Y[r] lies in some
// merged [s_k, e_k] (closed on both ends).  One pass over 2048-row tiles, two membership tests per row, a ballot per mask word;
// integer work without atomics, so the mask does not depend on scheduling.  The merged anchors are disjoint and sorted, so the
// anchor that can hold v is the last one with s_k <= v.  The search for it takes one of two forms, chosen by the anchor count:
//   LDS        up to K13_LDS_MAX anchors: every workgroup stages s / e in LDS once and runs a fixed-length binary search there
//              (it wins on small sets only: the deeper searches of larger sets lose to the directory's short ones)
//   directory  more anchors: a bucket directory over the anchors' span (2^shift coordinates per bucket, about two buckets per
//              anchor) holds the first anchor ending at or after each bucket's start; v's bucket bounds the binary search in global
//              memory to the anchors between two directory entries
// Scratch (c->an) is the handle's own, apart from the sweep's layouts, q index, count cache and K8 tables, and stays with the
// handle between calls (freed with it): the anchor-filtering of a genome is one call per chromosome, and releasing device memory
// slows the process's later device-to-host copies (tools/d2h_after_free_probe.cpp).
#define K13_T 2048                      // rows per tile: 256 threads x 8
#define K13_GRID 1024                   // workgroups of the tile loop (each owns every gridDim-th tile)
#define K13_LDS_MAX 256                 // anchors staged in LDS (2 x 1 KB per workgroup); chosen from measured sizes: DESIGN.md, K13
#define K13_LIM (1 << 30)               // clamp of the uploaded anchors: every coordinate of a handle satisfies |v| < 2^29

struct K13Set {
    const int* __restrict__ s;          // merged anchors, ascending and disjoint: s[k + 1] > e[k]
    const int* __restrict__ e;
    const int* __restrict__ dir;        // directory form: nb + 1 entries, dir[nb] = na
    int na, lo, hi, shift, nb;          // lo = s[0], hi = e[na - 1]; bucket of v = (v - lo) >> shift
};

// LDS form: the last k with s[k] <= v by a binary search of fixed length (p = the power of two >= na), then v <= e[k]
__device__ __forceinline__ bool k13_in_lds(const int* s, const int* e, int na, int p, int v)
{
    int k = -1;
    for (int step = p; step > 0; step >>= 1) {
        const int j = k + step;
        if (j < na && s[j] <= v) k = j;
    }
    return k >= 0 && v <= e[k];
}

// directory form: only the anchors dir[b] .. dir[b + 1] can hold v (those before dir[b] end before the bucket starts; dir[b + 1]
// ends at or after the next bucket's start > v, so every later anchor starts beyond v)
__device__ __forceinline__ bool k13_in_dir(const K13Set& a, int v)
{
    if (v < a.lo || v > a.hi) return false;
    const int b = (int)((u32)(v - a.lo) >> a.shift);
    const int k0 = a.dir[b];
    int lo = k0, len = min(a.dir[b + 1] + 1, a.na) - k0;
    while (len > 0) {                                       // upper_bound of v over s[k0 .. k0 + len)
        const int h = len >> 1;
        if (a.s[lo + h] <= v) { lo += h + 1; len -= h + 1; } else len = h;
    }
    const int k = lo - 1;
    return k >= k0 && v <= a.e[k];
}

template <bool LDS>
__global__ void __launch_bounds__(256)
k13_mask(const int* __restrict__ X, const int* __restrict__ Y, int n, K13Set a, u64* __restrict__ mask, int* __restrict__ wsum)
{
    __shared__ int ls[LDS ? K13_LDS_MAX : 1], le[LDS ? K13_LDS_MAX : 1];
    __shared__ int l_c[4];
    int p = 0;
    if (LDS) {
        for (int k = threadIdx.x; k < a.na; k += blockDim.x) { ls[k] = a.s[k]; le[k] = a.e[k]; }
        p = 1; while (p < a.na) p <<= 1;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int cnt = 0;                                            // rows of this wave in an anchor (wave-uniform: a sum of ballots)
    for (long long t0 = (long long)blockIdx.x * K13_T; t0 < n; t0 += (long long)gridDim.x * K13_T) {
        int x[8], y[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long long r = t0 + u * 256 + threadIdx.x;
            x[u] = r < n ? X[r] : 0; y[u] = r < n ? Y[r] : 0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long long r = t0 + u * 256 + threadIdx.x;
            bool in = false;
            if (r < n) in = LDS ? (k13_in_lds(ls, le, a.na, p, x[u]) || k13_in_lds(ls, le, a.na, p, y[u]))
                                : (k13_in_dir(a, x[u]) || k13_in_dir(a, y[u]));
            const u64 bal = __ballot(in);
            if (lane == 0 && t0 + u * 256 + wv * 64 < n) mask[(t0 >> 6) + u * 4 + wv] = bal;   // bits past n are 0 (in = false)
            cnt += __popcll(bal);
        }
    }
    if (lane == 0) l_c[wv] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) wsum[blockIdx.x] = l_c[0] + l_c[1] + l_c[2] + l_c[3];      // one total per workgroup, summed by the host
}

// dir[b] = the first anchor with e >= lo + (b << shift) (lower_bound over the ascending ends), dir[nb] = na
__global__ void __launch_bounds__(TPB)
k13_dir(K13Set a, int* __restrict__ dir)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > a.nb) return;
    if (b == a.nb) { dir[b] = a.na; return; }
    const long long start = (long long)a.lo + ((long long)b << a.shift);
    int lo = 0, len = a.na;
    while (len > 0) {
        const int h = len >> 1;
        if ((long long)a.e[lo + h] < start) { lo += h + 1; len -= h + 1; } else len = h;
    }
    dir[b] = lo;
}

// the merge of scripts/jd2cleanWashuPETs.py:141-197 run to its fixed point: intervals that overlap or share an endpoint are one
static std::vector<std::pair<int64_t, int64_t>> k13_merge(int64_t n_iv, const int64_t* starts, const int64_t* ends)
{
    std::vector<std::pair<int64_t, int64_t>> iv((size_t)n_iv), out;
    for (int64_t k = 0; k < n_iv; ++k) iv[k] = {starts[k], ends[k]};
    std::sort(iv.begin(), iv.end());
    for (const auto& r : iv) {
        if (!out.empty() && r.first <= out.back().second) out.back().second = std::max(out.back().second, r.second);
        else out.push_back(r);
    }
    return out;
}

static int k13_lds_max()
{
#ifdef CLOOPS_DEVEL
    // developer A/B of the two search forms on one anchor set (CLOOPS_K13_LDS=0: the directory form for every set)
    if (const char* e = getenv("CLOOPS_K13_LDS")) return std::min(atoi(e), K13_LDS_MAX);
#endif
    return K13_LDS_MAX;
}

// ---- K13 host entry point -----------------------------------------------------------------------
// hs / he / ws: host staging of the copies, owned by the caller so that they outlive the stream synchronisation that follows an
// error return here
static int anchor_mask(cl_chrom* c, const std::vector<std::pair<int64_t, int64_t>>& merged, uint64_t* mask, int64_t* n_kept,
                       std::vector<int>& hs, std::vector<int>& he, std::vector<int>& ws)
{
    const int n = (int)c->n;
    const size_t nw = ((size_t)n + 63) / 64;
    // only anchors that reach the handle's domain (|v| < 2^29) can hold a row; clamping those to +-2^30 changes no membership
    for (const auto& r : merged)
        if (r.second > -(1ll << 29) && r.first < (1ll << 29)) {
            hs.push_back((int)std::max<int64_t>(r.first, -K13_LIM));
            he.push_back((int)std::min<int64_t>(r.second, K13_LIM));
        }
    const int na = (int)hs.size();
    if (na == 0) { std::memset(mask, 0, nw * 8); return CL_OK; }
    K13Set a;
    a.na = na; a.lo = hs[0]; a.hi = he[na - 1];
    const bool lds = na <= k13_lds_max();
    a.shift = 0; a.nb = 0;
    if (!lds) {                                              // about two buckets per anchor: (hi - lo) >> shift < 2 na
        const long long span = (long long)a.hi - a.lo;
        while ((span >> a.shift) >= 2ll * na) ++a.shift;
        a.nb = (int)(span >> a.shift) + 1;
    }
    const int grid = (int)std::max(1ll, std::min<long long>(K13_GRID, ((long long)n + K13_T - 1) / K13_T));
    int rc;
    if ((rc = c->an.s.ensure((size_t)na * 4)) || (rc = c->an.e.ensure((size_t)na * 4)) || (rc = c->an.mask.ensure(nw * 8)) ||
        (rc = c->an.wsum.ensure((size_t)grid * 4)) || (!lds && (rc = c->an.dir.ensure(((size_t)a.nb + 1) * 4))))
        return rc;
    a.s = c->an.s.as<int>(); a.e = c->an.e.as<int>(); a.dir = lds ? nullptr : c->an.dir.as<int>();
    HIP_TRY(hipMemcpyAsync(c->an.s.p, hs.data(), (size_t)na * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->an.e.p, he.data(), (size_t)na * 4, hipMemcpyHostToDevice, c->stream));
    if (lds) {
        hipLaunchKernelGGL(k13_mask<true>, dim3(grid), dim3(256), 0, c->stream, c->d_x, c->d_y, n, a, c->an.mask.as<u64>(), c->an.wsum.as<int>());
    } else {
        hipLaunchKernelGGL(k13_dir, dim3((a.nb + 1 + TPB - 1) / TPB), dim3(TPB), 0, c->stream, a, c->an.dir.as<int>());
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k13_mask<false>, dim3(grid), dim3(256), 0, c->stream, c->d_x, c->d_y, n, a, c->an.mask.as<u64>(), c->an.wsum.as<int>());
    }
    HIP_TRY(hipGetLastError());
    ws.assign(grid, 0);
    HIP_TRY(hipMemcpyAsync(mask, c->an.mask.p, nw * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(ws.data(), c->an.wsum.p, (size_t)grid * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    long long kept = 0;
    for (int w : ws) kept += w;
    *n_kept = kept;
    return CL_OK;
}

extern "C" int cl_anchor_mask(cl_chrom* c, int64_t n_iv, const int64_t* starts, const int64_t* ends, uint64_t* mask,
                              int64_t* n_merged, int64_t* n_kept)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_merged) *n_merged = 0;
    if (n_kept) *n_kept = 0;
    if (!mask || !n_merged || !n_kept || n_iv < 0 || (n_iv > 0 && (!starts || !ends)))
        return fail(CL_ERR_ARG, "cl_anchor_mask: bad arguments");
    for (int64_t k = 0; k < n_iv; ++k)
        if (starts[k] > ends[k]) return fail(CL_ERR_ARG, "cl_anchor_mask: an interval with start > end");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_anchor_mask: asynchronous runs still in flight");
    const std::vector<std::pair<int64_t, int64_t>> merged = k13_merge(n_iv, starts, ends);
    *n_merged = (int64_t)merged.size();
    if (c->n == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<int> hs, he, ws;
    const int rc = anchor_mask(c, merged, mask, n_kept, hs, he, ws);
    if (rc != CL_OK) (void)hipStreamSynchronize(c->stream);          // no copy from or to hs / he / ws / mask may still be pending
    return rc;
}
