// k_kdis.hip -- K23: the k-distance of every PET of a resident chromosome (the distance to its k-th nearest neighbour) and its
// log-binned histogram -- kernels and C entry points.
#include "cl_chrom.h"

// ==========================================================================================
// K23: exact k nearest neighbours under |dx| + |dy| by an outward walk over the X-sorted table
// ==========================================================================================
// Definitions: include/cloops_hip.h, cl_kdis_build.  The reference has nothing of the kind; every number here is an integer that a few
// lines of numpy reproduce (tests/kdis_cases.py).  Rows: K19's table (agg_table: the kept rows sorted by X with a stable sort, so rows
// of equal X stay in input order; c->ag.sx = X + 2^30, c->ag.sy = Y, c->ag.kept of them), shared with cl_agg_loops and cl_dom_tracks
// and keyed by the cut: nothing is sorted here.
//   k23_walk<CAP>             one lane per table row, K23_TILE rows per workgroup.  Lane i walks outward from its own index: step s
//                             reads row i + s and row i - s, so neighbouring lanes read neighbouring addresses (K23_AHEAD rows of
//                             either side per round, read before the first of them is judged).  It keeps its kmax
//                             smallest distances as an ascending list in LDS, laid out [slot][lane] (the slot is a run-time index, so
//                             a register array would go to scratch; lane-minor words never share a bank within a wave), and the
//                             kmax-th best as threshold T in a register (INT_MAX while fewer than kmax are held).
//                             Stopping rule: a side is finished when its index leaves the table, or when |dx| >= T there: a
//                             candidate has d >= |dx|, only d < T changes the list, and X is sorted, so nothing further out on that
//                             side can change it either.  T only falls, so a finished side stays finished.  A lane is done when both
//                             sides are; a wave runs until its last lane is done.  CAP = 8 / 16 / 32 / 64 list slots: 8 / 16 / 32 /
//                             64 KB of LDS per workgroup, so the common small k (minPts 5 .. 20) keeps several workgroups per CU.
//                             The lane then stores X, Y and, for every asked k, slot k - 1 (or -1 when the table has no k other rows).
//   k23_hist                  per asked k (blockIdx.y): the d of a grid-stride share of the rows into an LDS histogram of CL_KDIS_BINS
//                             counters by k7_logbin's rule, zeros and -1 counted apart, then one 64-bit atomic per counter that is
//                             not zero.  Integer adds: the order does not matter.
// Cost: a row reads the rows whose X lies within its d_kmax of its own X -- hundreds to a few thousand on ChIA-PET / HiChIP densities,
// whatever the size of the chromosome.  It is quadratic only where almost all X are equal (then |dx| = 0 never reaches T, and the walk
// is the brute force).
// Only vector stores and ordinary HIP atomics; every index is checked against its array before a load or store.  Scratch (c->kd) is
// the handle's own, apart from the sweep's layouts, q index, count cache and the K8 / K13 / K14 / K20 / K21 / K22 state.
#define K23_TILE TPB                    // table rows per workgroup of k23_walk, one per lane
#define K23_AHEAD 4                     // rows a lane reads ahead on either side per round of k23_walk
#define K23_HIST_BLOCKS 1024            // most workgroups per k of k23_hist
static_assert(CL_KDIS_BINS == 31 * 128, "k7_logbin of d < 2^31 lies below 31 octaves of 128 bins");
static_assert(CL_KDIS_KMAX * K23_TILE * 4 <= 64 * 1024, "the largest list must fit a workgroup's static LDS");

struct K23Ks { int n; int k[8]; };

template <int CAP>
__global__ void __launch_bounds__(K23_TILE)
k23_walk(const u32* __restrict__ sx, const int* __restrict__ sy, int m, int kmax, K23Ks ks, int* __restrict__ ox, int* __restrict__ oy,
         int* __restrict__ od)
{
    __shared__ int lst[CAP * K23_TILE];
    const long long gi = (long long)blockIdx.x * K23_TILE + threadIdx.x;
    if (gi >= m || kmax < 1 || kmax > CAP) return;                              // (no barrier below)
    const int i = (int)gi;
    int* L = lst + threadIdx.x;                                                 // slot s of this lane: L[s * K23_TILE]
    const u32 kx = sx[i];
    const int py = sy[i];
    int held = 0, T = INT_MAX;                                                  // every d <= 2^31 - 4 < INT_MAX
    int r = i + 1, l = i - 1;
    bool goR = r < m, goL = l >= 0;
    auto take = [&](int d) {                                                    // d < T: into the list, the kmax-th best drops out
        int s = held < kmax ? held : kmax - 1;                                  // the new last slot, or the one that drops out
        while (s > 0 && L[(s - 1) * K23_TILE] > d) { L[s * K23_TILE] = L[(s - 1) * K23_TILE]; --s; }
        L[s * K23_TILE] = d;
        if (held < kmax) ++held;
        if (held == kmax) T = L[(kmax - 1) * K23_TILE];
    };
    while (goR || goL) {
        // the next K23_AHEAD rows of either side are read before the first is judged: whether a row is needed depends on the rows
        // before it, so one read per round trip would leave the lane waiting for memory most of the time.  Indices are clamped into
        // the table; a value read beyond a side's end is never used (the side is finished before its turn).
        u32 xr[K23_AHEAD], xl[K23_AHEAD];
        int yr[K23_AHEAD], yl[K23_AHEAD];
#pragma unroll
        for (int b = 0; b < K23_AHEAD; ++b) {
            const int jr = min(r + b, m - 1), jl = max(l - b, 0);               // 0 <= jr, jl < m (r <= m < 2^31 - 1024: no overflow)
            xr[b] = goR ? sx[jr] : 0u; yr[b] = goR ? sy[jr] : 0;
            xl[b] = goL ? sx[jl] : 0u; yl[b] = goL ? sy[jl] : 0;
        }
#pragma unroll
        for (int b = 0; b < K23_AHEAD; ++b) {                                   // (a side that goes on has advanced b rows: row r is xr[b])
            if (goR) {
                const int dx = (int)(xr[b] - kx);                               // >= 0: the table ascends in X; < 2^30
                if (dx >= T) goR = false;
                else {
                    const int dy = yr[b] - py;
                    const int d = dx + (dy < 0 ? -dy : dy);
                    if (d < T) take(d);
                    ++r; goR = r < m;
                }
            }
            if (goL) {
                const int dx = (int)(kx - xl[b]);
                if (dx >= T) goL = false;
                else {
                    const int dy = yl[b] - py;
                    const int d = dx + (dy < 0 ? -dy : dy);
                    if (d < T) take(d);
                    --l; goL = l >= 0;
                }
            }
        }
    }
    ox[i] = (int)kx - (1 << 30);
    oy[i] = py;
    for (int w = 0; w < ks.n; ++w) {
        const int k = ks.k[w];                                                  // 1 <= k <= kmax
        od[(size_t)w * (size_t)m + (size_t)i] = (k >= 1 && k <= held) ? L[(k - 1) * K23_TILE] : -1;
    }
}

// out: per k CL_KDIS_BINS + 2 counters: the bins, then n_zero and n_none
__global__ void __launch_bounds__(TPB)
k23_hist(const int* __restrict__ d, int m, u64* __restrict__ out)
{
    __shared__ u32 h[CL_KDIS_BINS + 2];
    const int w = blockIdx.y;
    const int* dk = d + (size_t)w * (size_t)m;
    for (int b = threadIdx.x; b < CL_KDIS_BINS + 2; b += TPB) h[b] = 0u;
    __syncthreads();
    u32 nz = 0u, nn = 0u;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < m; i += (long long)gridDim.x * TPB) {
        const int v = dk[i];
        if (v > 0) atomicAdd(&h[k7_logbin((unsigned)v)], 1u);                   // v < 2^31: the bin lies below CL_KDIS_BINS
        else if (v == 0) ++nz;
        else ++nn;
    }
    if (nz) atomicAdd(&h[CL_KDIS_BINS], nz);
    if (nn) atomicAdd(&h[CL_KDIS_BINS + 1], nn);
    __syncthreads();
    u64* o = out + (size_t)w * (CL_KDIS_BINS + 2);
    for (int b = threadIdx.x; b < CL_KDIS_BINS + 2; b += TPB)
        if (h[b]) atomicAdd(&o[b], (u64)h[b]);
}

// ---- K23 host side ------------------------------------------------------------------------------
static int kdis_build(cl_chrom* c, cl_chrom::Kdis::State& st)
{
    int rc;
    if ((rc = agg_table(c, st.cut))) return rc;
    st.n_kept = c->ag.kept;
    if (c->ag.kept == 0) { st.ready = true; return CL_OK; }
    const int m = c->ag.kept;
    const size_t sm = (size_t)m, hw = (size_t)st.n_k * (CL_KDIS_BINS + 2);
    if ((rc = c->kd.x.ensure(sm * 4)) || (rc = c->kd.y.ensure(sm * 4)) || (rc = c->kd.d.ensure(sm * 4 * (size_t)st.n_k)) ||
        (rc = c->kd.hist.ensure(hw * 8))) return rc;
    HIP_TRY(hipMemsetAsync(c->kd.hist.p, 0, hw * 8, c->stream));
    K23Ks ks{};
    ks.n = st.n_k;
    for (int w = 0; w < st.n_k; ++w) ks.k[w] = st.ks[w];
    const int kmax = st.ks[st.n_k - 1];
    const dim3 grid((unsigned)(((long long)m + K23_TILE - 1) / K23_TILE)), block(K23_TILE);
    const u32* sx = c->ag.sx.as<u32>();
    const int* sy = c->ag.sy.as<int>();
    int *ox = c->kd.x.as<int>(), *oy = c->kd.y.as<int>(), *od = c->kd.d.as<int>();
    if (kmax <= 8) hipLaunchKernelGGL(k23_walk<8>, grid, block, 0, c->stream, sx, sy, m, kmax, ks, ox, oy, od);
    else if (kmax <= 16) hipLaunchKernelGGL(k23_walk<16>, grid, block, 0, c->stream, sx, sy, m, kmax, ks, ox, oy, od);
    else if (kmax <= 32) hipLaunchKernelGGL(k23_walk<32>, grid, block, 0, c->stream, sx, sy, m, kmax, ks, ox, oy, od);
    else hipLaunchKernelGGL(k23_walk<64>, grid, block, 0, c->stream, sx, sy, m, kmax, ks, ox, oy, od);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k23_hist, dim3((unsigned)std::max(1, std::min(K23_HIST_BLOCKS, nblocks(m))), (unsigned)st.n_k), dim3(TPB), 0, c->stream,
                       (const int*)od, m, c->kd.hist.as<u64>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    st.ready = true;
    return CL_OK;
}

extern "C" int cl_kdis_build(cl_chrom* c, int64_t cut, const int32_t* ks, int32_t n_k, int64_t* n_kept)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_kept) *n_kept = 0;
    if (!n_kept || !ks) return fail(CL_ERR_ARG, "cl_kdis_build: bad arguments");
    if (n_k < 1 || n_k > 8) return fail(CL_ERR_ARG, "cl_kdis_build: n_k outside [1, 8]");
    for (int w = 0; w < n_k; ++w) {
        if (ks[w] < 1 || ks[w] > CL_KDIS_KMAX) return fail(CL_ERR_ARG, "cl_kdis_build: k outside [1, 64]");
        if (w > 0 && ks[w] <= ks[w - 1]) return fail(CL_ERR_ARG, "cl_kdis_build: ks must be strictly ascending");
    }
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_kdis_build: asynchronous runs still in flight");
    cl_chrom::Kdis::State st;
    st.n_k = n_k;
    for (int w = 0; w < n_k; ++w) st.ks[w] = ks[w];
    st.cut = cut <= 0 ? 0 : (int)std::min<int64_t>(cut, 1ll << 30);             // |Y - X| < 2^30: a larger cut keeps no row either
    if (c->n == 0) {
        st.ready = true;
        c->kd.st = st;
        return CL_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    const int rc = kdis_build(c, st);
    if (rc != CL_OK) {
        (void)hipStreamSynchronize(c->stream);
        kdis_release(c);
        return rc;
    }
    c->kd.st = st;
    *n_kept = st.n_kept;
    return CL_OK;
}

extern "C" int cl_kdis_get(cl_chrom* c, int32_t which, int64_t first, int64_t count, int32_t* x, int32_t* y, int32_t* d)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (!c->kd.st.ready) return fail(CL_ERR_ARG, "cl_kdis_get: no k-distances on this handle (cl_kdis_build)");
    if (which < 0 || which >= c->kd.st.n_k) return fail(CL_ERR_ARG, "cl_kdis_get: which outside the ks of the build");
    if (!range_ok(first, count, c->kd.st.n_kept)) return fail(CL_ERR_ARG, "cl_kdis_get: range outside the kept rows");
    if (count > 0 && (!x || !y || !d)) return fail(CL_ERR_ARG, "cl_kdis_get: bad arguments");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_kdis_get: asynchronous runs still in flight");
    if (count == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)count * 4;
    const int* dk = c->kd.d.as<int>() + (size_t)which * (size_t)c->kd.st.n_kept;
    return read_back(c, "cl_kdis_get", {{x, c->kd.x.as<int>() + first, bytes}, {y, c->kd.y.as<int>() + first, bytes}, {d, dk + first, bytes}});
}

extern "C" int cl_kdis_hist(cl_chrom* c, int32_t which, uint64_t* hist, uint64_t* n_zero, uint64_t* n_none)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_zero) *n_zero = 0;
    if (n_none) *n_none = 0;
    if (!hist || !n_zero || !n_none) return fail(CL_ERR_ARG, "cl_kdis_hist: bad arguments");
    if (!c->kd.st.ready) return fail(CL_ERR_ARG, "cl_kdis_hist: no k-distances on this handle (cl_kdis_build)");
    if (which < 0 || which >= c->kd.st.n_k) return fail(CL_ERR_ARG, "cl_kdis_hist: which outside the ks of the build");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_kdis_hist: asynchronous runs still in flight");
    std::memset(hist, 0, (size_t)CL_KDIS_BINS * 8);
    if (c->kd.st.n_kept == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    static_assert(sizeof(uint64_t) == sizeof(u64), "the histogram is copied as it lies");
    const u64* src = c->kd.hist.as<u64>() + (size_t)which * (CL_KDIS_BINS + 2);
    uint64_t tail[2] = {0, 0};
    const int rc = read_back(c, "cl_kdis_hist", {{hist, src, (size_t)CL_KDIS_BINS * 8}, {tail, src + CL_KDIS_BINS, 16}});
    if (rc) return rc;                                                          // (synchronised: no copy to the stack is pending)
    *n_zero = tail[0]; *n_none = tail[1];
    return CL_OK;
}

extern "C" int cl_kdis_free(cl_chrom* c) { return unit_free(c, "cl_kdis_free", kdis_release); }
