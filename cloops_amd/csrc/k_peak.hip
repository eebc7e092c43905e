// k_peak.hip -- K21: peaks of the PET ends of a resident chromosome (1D DBSCAN in closed form over the sorted end points), counts of
// end points in intervals and summits of intervals -- kernels and C entry points.
#include "cl_chrom.h"
#include "cl_ends.h"

// ==========================================================================================
// K21: sequential 1D DBSCAN over ascending points as rank differences and prefix sums
// ==========================================================================================
// Definitions: include/cloops_hip.h, cl_peak_sort.  The reference has nothing of the kind; every number here is an integer that a few
// lines of numpy reproduce (tests/test_gpu_peaks.py).  S: the m kept end points in ascending order (keys v - base, K20's key pass and
// one radix sort over the bits in use), lb(x) = #{v < x}, ub(x) = #{v <= x}.
//   k21_core                  per element i: lo = lb(S[i] - eps) and hi = ub(S[i] + eps), so n(i) = hi - lo; core iff n(i) >= minPts.
//                             One workgroup per K21_TILE elements stages them and K21_HALO on either side in LDS; the two ranks come
//                             from K20's galloping searches, downwards from i and upwards from the larger of i + 1 and the rank of
//                             the thread's previous element, through the LDS-or-global accessor: a window with more points than the
//                             staged ones costs time, not exactness.  With w for eps the same kernel gives n_w for the summits.
//   exclusive scan            of the core flags: C (C[m] = the cores)
//   k21_heads                 core i opens a chain iff no core of a smaller index lies at a position >= S[i] - eps: C[i] == C[lo[i]]
//                             (by index, so equal positions cannot open two chains)
//   exclusive scan            of the head flags: H numbers the chains (H[m] = the peaks)
//   k21_chains                heads write their index as the first core of chain H[i]; core i closes chain H[i + 1] - 1 iff no core
//                             of a larger index lies at a position <= S[i] + eps: C[hi[i]] == C[i + 1]
//   k21_extents               per peak k with first / last core at a, b: i0 = max(lo[a], hi[b of peak k - 1]) -- lb of the larger of
//                             S[a] - eps and S[b'] + eps + 1, the border rule: what is within eps of the chain before belongs to it --
//                             and i1 = hi[b]; both are ranks k21_core has stored, so no search is left.  start = S[i0], end =
//                             S[i1 - 1] + 1, n_points = i1 - i0, n_cores = C[b + 1] - C[a]; the sum of n_points through one atomic
//                             per wave
//   k21_count                 one interval per lane: lb(e) - lb(s) by two binary searches, the bounds clamped to the keys' range in
//                             64 bits before the base is subtracted
//   k21_summit                per point of S: its interval by a search in the ascending starts (staged in LDS when they fit), the key
//                             (n_w << 32 | ~(position - the larger of the start and key 0's value)) whose maximum is the largest n_w
//                             at the smallest position; a segmented scan in the wave (the points are sorted, so an interval's points
//                             are consecutive), the segments that reach a wave's edge merged across the workgroup through LDS, then
//                             one 64-bit atomicMax per workgroup and interval; k21_summit_out unpacks the keys
// Only vector stores and ordinary HIP atomics.  Scratch (c->pk) is the handle's own, apart from the sweep's layouts, q index, count
// cache and the K8 / K13 / K14 / K19 / K20 state.
#define K21_TILE 1024                   // elements of S per workgroup of k21_core and k21_summit (4 per thread)
#define K21_HALO 1024                   // elements staged in LDS on either side of the tile of k21_core
#define K21_IVL 2048                    // interval starts that k21_summit stages in LDS (more: read from global memory)
#define K21_U (K21_TILE / TPB)          // elements per thread
#define K21_RUNS (K21_U * (TPB / 64))   // stretches of 64 consecutive elements per workgroup
#define K21_MAXW (1ll << 29)            // eps and w lie in [1, 2^29)

enum { K21_NENDS = 0, K21_CLUST = 1, K21_CTRS = 2 };                    // c->pk.ctr, u64 each
static_assert(K21_NENDS == K20_NENDS, "k20_keys counts into slot K20_NENDS");

__global__ void __launch_bounds__(TPB)
k21_core(const u32* __restrict__ skey, int m, int base, int eps, long long min_pts, u32* __restrict__ lo, u32* __restrict__ hi,
         u32* __restrict__ flag)
{
    __shared__ u32 win[K21_TILE + 2 * K21_HALO];
    const long long t0 = (long long)blockIdx.x * K21_TILE;
    K20Keys S;
    S.g = skey; S.l = win; S.vmin = base;
    S.base = (int)(t0 > K21_HALO ? t0 - K21_HALO : 0);
    const long long wend = t0 + K21_TILE + K21_HALO < m ? t0 + K21_TILE + K21_HALO : m;
    S.span = (int)(wend - S.base);
    for (int k = threadIdx.x; k < S.span; k += TPB) win[k] = skey[S.base + k];
    __syncthreads();
    int prev = 0;
#pragma unroll
    for (int u = 0; u < K21_U; ++u) {
        const long long il = t0 + u * TPB + threadIdx.x;
        if (il >= m) break;
        const int i = (int)il;
        const int v = S.at(i);
        const int l = k20_ub_down(S, i, v - eps - 1);                           // lb(v - eps): S[i] itself exceeds v - eps - 1
        const int h = k20_ub_up(S, m, prev > i + 1 ? prev : i + 1, v + eps);    // ub(v + eps): nothing below the start exceeds it
        prev = h;
        lo[i] = (u32)l; hi[i] = (u32)h;
        if (flag) flag[i] = (long long)(h - l) >= min_pts ? 1u : 0u;
    }
}

__global__ void __launch_bounds__(TPB)
k21_heads(const u32* __restrict__ flag, const u32* __restrict__ C, const u32* __restrict__ lo, int m, u32* __restrict__ head)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) {
        const u32 l = lo[i];
        head[i] = (flag[i] && l <= (u32)i && C[i] == C[l]) ? 1u : 0u;
    }
}

// C, H: m + 1 entries each; a[k], b[k]: the indices of the first and the last core of chain k < P
__global__ void __launch_bounds__(TPB)
k21_chains(const u32* __restrict__ C, const u32* __restrict__ H, const u32* __restrict__ hi, int m, u32 P, u32* __restrict__ a,
           u32* __restrict__ b)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) {
        const u32 c0 = C[i], c1 = C[i + 1];
        if (c1 == c0) continue;                                                 // not a core
        const u32 h0 = H[i], h1 = H[i + 1];
        if (h1 != h0 && h0 < P) a[h0] = (u32)i;
        const u32 h = hi[i];
        if (h <= (u32)m && C[h] == c1 && h1 >= 1 && h1 - 1 < P) b[h1 - 1] = (u32)i;
    }
}

__global__ void __launch_bounds__(TPB)
k21_extents(const u32* __restrict__ skey, int m, int base, const u32* __restrict__ C, const u32* __restrict__ lo,
            const u32* __restrict__ hi, const u32* __restrict__ a, const u32* __restrict__ b, u32 P, int* __restrict__ start,
            int* __restrict__ end, u32* __restrict__ np, u32* __restrict__ nc, u64* __restrict__ ctr)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    u64 pts = 0;
    if (k < P) {
        const u32 ia = a[k], ib = b[k];
        int s = 0, e = 0;
        u32 n = 0, cores = 0;
        if (ia <= ib && ib < (u32)m) {
            u32 i0 = lo[ia];
            if (k > 0) {
                const u32 pb = b[k - 1];
                if (pb < (u32)m) i0 = max(i0, hi[pb]);
            }
            const u32 i1 = hi[ib];
            if (i0 < i1 && i1 <= (u32)m) {
                s = (int)skey[i0] + base; e = (int)skey[i1 - 1] + base + 1;
                n = i1 - i0; cores = C[ib + 1] - C[ia];
            }
        }
        start[k] = s; end[k] = e; np[k] = n; nc[k] = cores;
        pts = n;
    }
    for (int o = 32; o > 0; o >>= 1) pts += (u64)__shfl_xor((long long)pts, o);
    if ((threadIdx.x & 63) == 0 && pts) atomicAdd(&ctr[K21_CLUST], pts);
}

// #{keys of S below position x}: x is clamped to the keys' range before the base is subtracted
__device__ __forceinline__ u32 k21_lb(const u32* __restrict__ skey, int m, int base, long long x)
{
    if (x <= (long long)base) return 0u;
    if (x > (long long)base + 0xffffffffll) return (u32)m;
    const u32 t = (u32)(x - (long long)base);
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (int)(((long long)lo + hi) >> 1);
        if (skey[mid] < t) lo = mid + 1; else hi = mid;
    }
    return (u32)lo;
}

__global__ void __launch_bounds__(TPB)
k21_count(const u32* __restrict__ skey, int m, int base, const long long* __restrict__ ivs, const long long* __restrict__ ive, long long n,
          u32* __restrict__ cnt)
{
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (long long)gridDim.x * blockDim.x) {
        const long long s = ivs[j], e = ive[j];
        cnt[j] = e > s ? k21_lb(skey, m, base, e) - k21_lb(skey, m, base, s) : 0u;
    }
}

// lo / hi: the ranks of k21_core for the half-width w; best[k]: the largest key of interval k, 0 while it has no point
__global__ void __launch_bounds__(TPB)
k21_summit(const u32* __restrict__ skey, int m, int base, const u32* __restrict__ lo, const u32* __restrict__ hi,
           const long long* __restrict__ ivs, const long long* __restrict__ ive, int n_iv, u64* __restrict__ best)
{
    __shared__ long long st[K21_IVL];
    __shared__ int rid[2 * K21_RUNS];
    __shared__ u64 rkey[2 * K21_RUNS];
    const bool staged = n_iv <= K21_IVL;                                        // (the same in every lane)
    if (staged)
        for (int k = threadIdx.x; k < n_iv; k += TPB) st[k] = ivs[k];
    if (threadIdx.x < 2 * K21_RUNS) rid[threadIdx.x] = -1;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long t0 = (long long)blockIdx.x * K21_TILE;
#pragma unroll
    for (int u = 0; u < K21_U; ++u) {                                           // (no early exit: every lane takes part in the shuffles)
        const long long il = t0 + u * TPB + threadIdx.x;
        int id = -1;
        u64 key = 0;
        if (il < m) {
            const long long p = (long long)skey[il] + base;
            int a = 0, b = n_iv;                                                // the intervals that start at or below p: [0, a)
            while (a < b) {
                const int mid = (int)(((long long)a + b) >> 1);
                if ((staged ? st[mid] : ivs[mid]) <= p) a = mid + 1; else b = mid;
            }
            if (a > 0 && p < ive[a - 1]) {
                id = a - 1;
                const long long s = staged ? st[id] : ivs[id];                  // (relative to the start or to key 0: below 2^32 either way)
                key = ((u64)(hi[il] - lo[il]) << 32) | (u64)(0xffffffffu - (u32)(p - (s > base ? s : (long long)base)));
            }
        }
        // the maximum of every stretch of equal ids up to this lane; the last lane of a stretch then holds the stretch's
        for (int o = 1; o < 64; o <<= 1) {
            const u64 ok = (u64)__shfl_up((long long)key, o);
            const int oi = __shfl_up(id, o);
            if (lane >= o && oi == id && ok > key) key = ok;
        }
        const int nid = __shfl_down(id, 1);
        const bool tail = lane == 63 || nid != id;
        const int fid = __shfl(id, 0);
        const u64 diff = __ballot(id != fid);
        const int flen = diff ? __ffsll((long long)diff) - 1 : 64;              // lanes of the stretch that starts at lane 0
        if (tail && id >= 0 && id < n_iv) {
            const int r = u * (TPB / 64) + w;
            if (lane == 63) { rid[2 * r + 1] = id; rkey[2 * r + 1] = key; }     // may go on in the next 64 elements
            else if (lane < flen) { rid[2 * r] = id; rkey[2 * r] = key; }       // may have begun in the 64 elements before
            else atomicMax(&best[id], key);                                     // complete inside these 64 elements
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                                     // the edge stretches in ascending order of their elements
        int cur = -1;
        u64 ck = 0;
        for (int k = 0; k < 2 * K21_RUNS; ++k) {
            const int id = rid[k];
            if (id < 0) continue;
            if (id != cur) {
                if (cur >= 0) atomicMax(&best[cur], ck);
                cur = id; ck = 0;
            }
            ck = rkey[k] > ck ? rkey[k] : ck;
        }
        if (cur >= 0) atomicMax(&best[cur], ck);
    }
}

__global__ void __launch_bounds__(TPB)
k21_summit_out(const u64* __restrict__ best, const long long* __restrict__ ivs, long long n, int base, int* __restrict__ pos,
               u32* __restrict__ cnt)
{
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (long long)gridDim.x * blockDim.x) {
        const u64 k = best[j];
        const long long s = ivs[j] > base ? ivs[j] : (long long)base;
        pos[j] = k ? (int)(s + (long long)(0xffffffffu - (u32)k)) : -1;
        cnt[j] = (u32)(k >> 32);
    }
}

// ---- K21 host side ------------------------------------------------------------------------------
static int k21_grid(long long work) { return (int)std::max(1ll, std::min<long long>(4096, (work + TPB - 1) / TPB)); }

static int peak_scan(cl_chrom* c, const u32* in, u32* out, size_t n, const char* what)
{
    return prim_run(c->pk.tmp, what, [&](void* tmp, size_t& bytes) {
        return rocprim::exclusive_scan(tmp, bytes, in, out, 0u, n, rocprim::plus<u32>(), c->stream);
    });
}

static int peak_sort(cl_chrom* c, long long cut, int ends, int64_t* n_ends, int64_t* vmin, int64_t* vmax)
{
    const int n = (int)c->n;
    const int ne = (ends & 1) + ((ends >> 1) & 1);
    if ((long long)n * ne > K20_LIMIT) return fail(CL_ERR_ARG, "cl_peak_sort: more than 2^31 - 4096 end points");
    const int base = std::min(c->st.xmin, c->st.ymin), pmax = std::max(c->st.xmax, c->st.ymax);
    const int ebit = std::max(1, bits_for((u32)(pmax - base)));
    int rc;
    if ((rc = c->pk.ctr.ensure(K21_CTRS * 8)) || (rc = c->pk.kin.ensure((size_t)n * ne * 4)) || (rc = c->pk.key.ensure((size_t)n * ne * 4))) return rc;
    u64* ctr = c->pk.ctr.as<u64>();
    HIP_TRY(hipMemsetAsync(ctr, 0, K21_CTRS * 8, c->stream));
    hipLaunchKernelGGL(k20_keys, dim3((unsigned)(((long long)n + K20_ROWS - 1) / K20_ROWS)), dim3(TPB), 0, c->stream, c->d_x, c->d_y, n, cut, ends,
                       0, base, c->pk.kin.as<u32>(), ctr);
    HIP_TRY(hipGetLastError());
    u64 hm = 0;
    HIP_TRY(hipMemcpyAsync(&hm, ctr + K21_NENDS, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const long long m = (long long)hm;
    if (m > (long long)n * ne) return fail(CL_ERR_HIP, "cl_peak_sort: the key pass counted more end points than rows allow");
    c->pk.st.base = base;
    if (m == 0) { c->pk.st.sorted = true; return CL_OK; }
    if ((rc = prim_run(c->pk.tmp, "radix_sort_keys(peaks)", [&](void* tmp, size_t& bytes) {
            return rocprim::radix_sort_keys(tmp, bytes, c->pk.kin.as<u32>(), c->pk.key.as<u32>(), (size_t)m, 0, ebit, c->stream);
        })))
        return rc;
    u32 k0 = 0, k1 = 0;
    HIP_TRY(hipMemcpyAsync(&k0, c->pk.key.as<u32>(), 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&k1, c->pk.key.as<u32>() + (m - 1), 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->pk.st.m = m;
    c->pk.st.sorted = true;
    *n_ends = m;
    *vmin = (long long)base + k0;
    *vmax = (long long)base + k1;
    return CL_OK;
}

extern "C" int cl_peak_sort(cl_chrom* c, int64_t cut, int32_t ends, int64_t* n_ends, int64_t* vmin, int64_t* vmax)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_ends) *n_ends = 0;
    if (vmin) *vmin = 0;
    if (vmax) *vmax = 0;
    if (!n_ends || !vmin || !vmax) return fail(CL_ERR_ARG, "cl_peak_sort: bad arguments");
    if (ends < 1 || ends > 3) return fail(CL_ERR_ARG, "cl_peak_sort: ends outside 1..3");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_peak_sort: asynchronous runs still in flight");
    HIP_TRY(hipSetDevice(c->device));
    c->pk.st = cl_chrom::Peak::State();                                      // (the buffers stay: the next sort reuses their memory, not their content)
    if (c->n == 0) { c->pk.st.sorted = true; return CL_OK; }
    const int rc = peak_sort(c, cut, ends, n_ends, vmin, vmax);
    if (rc != CL_OK) {
        (void)hipStreamSynchronize(c->stream);                          // no copy to the stack may still be pending
        peak_release(c);
    }
    return rc;
}

// lo / hi of every element for the half-width `width`, and the core flags if `flags`
static int peak_ranks(cl_chrom* c, int width, long long min_pts, bool flags)
{
    const long long m = c->pk.st.m;
    int rc;
    if ((rc = c->pk.lo.ensure((size_t)m * 4)) || (rc = c->pk.hi.ensure((size_t)m * 4))) return rc;
    if (flags && (rc = c->pk.flag.ensure(((size_t)m + 1) * 4))) return rc;
    if (flags) HIP_TRY(hipMemsetAsync(c->pk.flag.as<u32>() + m, 0, 4, c->stream));
    hipLaunchKernelGGL(k21_core, dim3((unsigned)((m + K21_TILE - 1) / K21_TILE)), dim3(TPB), 0, c->stream, c->pk.key.as<u32>(), (int)m, c->pk.st.base,
                       width, min_pts, c->pk.lo.as<u32>(), c->pk.hi.as<u32>(), flags ? c->pk.flag.as<u32>() : (u32*)nullptr);
    HIP_TRY(hipGetLastError());
    return CL_OK;
}

static int peak_call(cl_chrom* c, int eps, long long min_pts, int64_t* n_peaks, int64_t* n_cores, int64_t* n_clustered)
{
    const long long m = c->pk.st.m;
    int rc;
    if ((rc = peak_ranks(c, eps, min_pts, true))) return rc;
    if ((rc = c->pk.C.ensure(((size_t)m + 1) * 4)) || (rc = c->pk.head.ensure(((size_t)m + 1) * 4)) || (rc = c->pk.H.ensure(((size_t)m + 1) * 4)))
        return rc;
    if ((rc = peak_scan(c, c->pk.flag.as<u32>(), c->pk.C.as<u32>(), (size_t)m + 1, "exclusive_scan(peaks, cores)"))) return rc;
    HIP_TRY(hipMemsetAsync(c->pk.head.as<u32>() + m, 0, 4, c->stream));
    hipLaunchKernelGGL(k21_heads, dim3(k21_grid(m)), dim3(TPB), 0, c->stream, c->pk.flag.as<u32>(), c->pk.C.as<u32>(), c->pk.lo.as<u32>(), (int)m,
                       c->pk.head.as<u32>());
    HIP_TRY(hipGetLastError());
    if ((rc = peak_scan(c, c->pk.head.as<u32>(), c->pk.H.as<u32>(), (size_t)m + 1, "exclusive_scan(peaks, heads)"))) return rc;
    u32 hC = 0, hP = 0;
    u64* ctr = c->pk.ctr.as<u64>();
    HIP_TRY(hipMemsetAsync(ctr + K21_CLUST, 0, 8, c->stream));
    HIP_TRY(hipMemcpyAsync(&hC, c->pk.C.as<u32>() + m, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&hP, c->pk.H.as<u32>() + m, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const long long P = hP;
    u64 hclust = 0;
    if (P > 0) {
        if ((rc = c->pk.a.ensure((size_t)P * 4)) || (rc = c->pk.b.ensure((size_t)P * 4)) || (rc = c->pk.start.ensure((size_t)P * 4)) ||
            (rc = c->pk.end.ensure((size_t)P * 4)) || (rc = c->pk.np.ensure((size_t)P * 4)) || (rc = c->pk.nc.ensure((size_t)P * 4)))
            return rc;
        HIP_TRY(hipMemsetAsync(c->pk.a.p, 0xff, (size_t)P * 4, c->stream));                  // (an index no element has: refused by k21_extents)
        HIP_TRY(hipMemsetAsync(c->pk.b.p, 0xff, (size_t)P * 4, c->stream));
        hipLaunchKernelGGL(k21_chains, dim3(k21_grid(m)), dim3(TPB), 0, c->stream, c->pk.C.as<u32>(), c->pk.H.as<u32>(), c->pk.hi.as<u32>(), (int)m,
                           (u32)P, c->pk.a.as<u32>(), c->pk.b.as<u32>());
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k21_extents, dim3((unsigned)((P + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, c->pk.key.as<u32>(), (int)m, c->pk.st.base,
                           c->pk.C.as<u32>(), c->pk.lo.as<u32>(), c->pk.hi.as<u32>(), c->pk.a.as<u32>(), c->pk.b.as<u32>(), (u32)P,
                           c->pk.start.as<int>(), c->pk.end.as<int>(), c->pk.np.as<u32>(), c->pk.nc.as<u32>(), ctr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&hclust, ctr + K21_CLUST, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->pk.st.P = P;
    c->pk.st.called = true;
    *n_peaks = P;
    *n_cores = hC;
    *n_clustered = (int64_t)hclust;
    return CL_OK;
}

extern "C" int cl_peak_call(cl_chrom* c, int64_t eps, int64_t min_pts, int64_t* n_peaks, int64_t* n_cores, int64_t* n_clustered)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_peaks) *n_peaks = 0;
    if (n_cores) *n_cores = 0;
    if (n_clustered) *n_clustered = 0;
    if (!n_peaks || !n_cores || !n_clustered) return fail(CL_ERR_ARG, "cl_peak_call: bad arguments");
    if (eps < 1 || eps >= K21_MAXW) return fail(CL_ERR_ARG, "cl_peak_call: eps outside [1, 2^29)");
    if (min_pts < 1) return fail(CL_ERR_ARG, "cl_peak_call: min_pts below 1");
    if (!c->pk.st.sorted) return fail(CL_ERR_ARG, "cl_peak_call: no sorted end points on this handle (cl_peak_sort)");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_peak_call: asynchronous runs still in flight");
    c->pk.st.called = false; c->pk.st.P = 0;
    if (c->pk.st.m == 0) { c->pk.st.called = true; return CL_OK; }
    HIP_TRY(hipSetDevice(c->device));
    const int rc = peak_call(c, (int)eps, min_pts, n_peaks, n_cores, n_clustered);
    if (rc != CL_OK) (void)hipStreamSynchronize(c->stream);             // no copy to the stack may still be pending
    return rc;
}

extern "C" int cl_peak_get(cl_chrom* c, int64_t first, int64_t count, int32_t* start, int32_t* end, uint32_t* n_points, uint32_t* n_cores)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (!c->pk.st.sorted || !c->pk.st.called) return fail(CL_ERR_ARG, "cl_peak_get: no peaks called on this handle (cl_peak_sort, cl_peak_call)");
    if (!range_ok(first, count, c->pk.st.P)) return fail(CL_ERR_ARG, "cl_peak_get: range outside the peaks");
    if (count > 0 && (!start || !end || !n_points || !n_cores)) return fail(CL_ERR_ARG, "cl_peak_get: bad arguments");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_peak_get: asynchronous runs still in flight");
    if (count == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t nb = (size_t)count * 4;
    return read_back(c, "cl_peak_get", {{start, c->pk.start.as<int>() + first, nb}, {end, c->pk.end.as<int>() + first, nb},
                                        {n_points, c->pk.np.as<u32>() + first, nb}, {n_cores, c->pk.nc.as<u32>() + first, nb}});
}

// the n intervals of a count / summit call on the device (c->pk.ivs, c->pk.ive)
static int peak_intervals(cl_chrom* c, const int64_t* starts, const int64_t* ends, long long n)
{
    int rc;
    if ((rc = c->pk.ivs.ensure((size_t)n * 8)) || (rc = c->pk.ive.ensure((size_t)n * 8))) return rc;
    HIP_TRY(hipMemcpyAsync(c->pk.ivs.p, starts, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->pk.ive.p, ends, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    return CL_OK;
}

static int peak_count(cl_chrom* c, const int64_t* starts, const int64_t* ends, long long n, uint32_t* counts)
{
    int rc;
    if ((rc = peak_intervals(c, starts, ends, n)) || (rc = c->pk.ocnt.ensure((size_t)n * 4))) return rc;
    hipLaunchKernelGGL(k21_count, dim3(k21_grid(n)), dim3(TPB), 0, c->stream, c->pk.key.as<u32>(), (int)c->pk.st.m, c->pk.st.base,
                       c->pk.ivs.as<long long>(), c->pk.ive.as<long long>(), n, c->pk.ocnt.as<u32>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(counts, c->pk.ocnt.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CL_OK;
}

extern "C" int cl_peak_count(cl_chrom* c, const int64_t* starts, const int64_t* ends, int64_t n, uint32_t* counts)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n < 0 || n > K20_LIMIT || (n > 0 && (!starts || !ends || !counts))) return fail(CL_ERR_ARG, "cl_peak_count: bad arguments");
    if (!c->pk.st.sorted) return fail(CL_ERR_ARG, "cl_peak_count: no sorted end points on this handle (cl_peak_sort)");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_peak_count: asynchronous runs still in flight");
    if (n == 0) return CL_OK;
    if (c->pk.st.m == 0) { std::memset(counts, 0, (size_t)n * 4); return CL_OK; }
    HIP_TRY(hipSetDevice(c->device));
    const int rc = peak_count(c, starts, ends, n, counts);
    if (rc != CL_OK) (void)hipStreamSynchronize(c->stream);             // no copy from or to the caller's arrays may still be pending
    return rc;
}

static int peak_summits(cl_chrom* c, const int64_t* starts, const int64_t* ends, long long n, int w, int32_t* pos, uint32_t* cnt)
{
    const long long m = c->pk.st.m;
    int rc;
    if ((rc = peak_intervals(c, starts, ends, n)) || (rc = c->pk.best.ensure((size_t)n * 8)) || (rc = c->pk.opos.ensure((size_t)n * 4)) ||
        (rc = c->pk.ocnt.ensure((size_t)n * 4)))
        return rc;
    if ((rc = peak_ranks(c, w, 1, false))) return rc;
    HIP_TRY(hipMemsetAsync(c->pk.best.p, 0, (size_t)n * 8, c->stream));
    hipLaunchKernelGGL(k21_summit, dim3((unsigned)((m + K21_TILE - 1) / K21_TILE)), dim3(TPB), 0, c->stream, c->pk.key.as<u32>(), (int)m, c->pk.st.base,
                       c->pk.lo.as<u32>(), c->pk.hi.as<u32>(), c->pk.ivs.as<long long>(), c->pk.ive.as<long long>(), (int)n, c->pk.best.as<u64>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k21_summit_out, dim3(k21_grid(n)), dim3(TPB), 0, c->stream, c->pk.best.as<u64>(), c->pk.ivs.as<long long>(), n, c->pk.st.base,
                       c->pk.opos.as<int>(), c->pk.ocnt.as<u32>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(pos, c->pk.opos.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(cnt, c->pk.ocnt.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CL_OK;
}

extern "C" int cl_peak_summits(cl_chrom* c, const int64_t* starts, const int64_t* ends, int64_t n, int64_t w, int32_t* pos, uint32_t* cnt)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n < 0 || n > K20_LIMIT || (n > 0 && (!starts || !ends || !pos || !cnt))) return fail(CL_ERR_ARG, "cl_peak_summits: bad arguments");
    if (w < 1 || w >= K21_MAXW) return fail(CL_ERR_ARG, "cl_peak_summits: w outside [1, 2^29)");
    if (!c->pk.st.sorted) return fail(CL_ERR_ARG, "cl_peak_summits: no sorted end points on this handle (cl_peak_sort)");
    for (int64_t k = 0; k < n; ++k)
        if (ends[k] < starts[k] || (k > 0 && starts[k] < ends[k - 1]))
            return fail(CL_ERR_ARG, "cl_peak_summits: the intervals must be ascending and disjoint");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_peak_summits: asynchronous runs still in flight");
    if (n == 0) return CL_OK;
    if (c->pk.st.m == 0) {
        for (int64_t k = 0; k < n; ++k) { pos[k] = -1; cnt[k] = 0; }
        return CL_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    const int rc = peak_summits(c, starts, ends, n, (int)w, pos, cnt);
    if (rc != CL_OK) (void)hipStreamSynchronize(c->stream);             // no copy from or to the caller's arrays may still be pending
    return rc;
}

extern "C" int cl_peak_free(cl_chrom* c) { return unit_free(c, "cl_peak_free", peak_release); }
