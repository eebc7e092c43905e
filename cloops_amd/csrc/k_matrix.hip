// k_matrix.hip -- K24: contact matrices of a resident chromosome -- a dense window, the sparse non-empty cells and the virtual-4C
// profile of a viewpoint -- kernels and C entry points.
#include "cl_chrom.h"

// ==========================================================================================
// K24: binned counts of the kept rows over K19's X-sorted table
// ==========================================================================================
// Definitions: include/cloops_hip.h, cl_mat_window.  The reference has nothing of the kind; every number here is an integer count that
// a few lines of numpy reproduce (tests/matrix_cases.py).  Rows: K19's table (agg_table: the kept rows sorted by X, c->ag.sx = X + 2^30,
// c->ag.sy = Y, c->ag.kept of them), shared with cl_agg_loops, cl_dom_tracks and cl_kdis_build and keyed by the cut: nothing but the
// cells' keys is sorted here.
// Bins: floor(p / res) without dividing a negative number: with B = ceil(2^30 / res) the key p + 2^30 + (B res - 2^30) is p + B res >= 0
// and below 2^31, so its quotient by res (host-made multiply-shift, k12_div) minus B is the bin (K24Bin).
//   k24_ranges                the first table index with X key >= t for up to four t, one wave each (k19_lb_wave): the two ends of
//                             the rows whose bx lies in the window's X bins, and of those whose bx lies in its Y bins (the mirrored
//                             half).  The ranges stay on the device; the next kernel reads them.
//   k24_window                blockIdx.y = phase (0: a row counts at (bx - bx0, by - by0); 1, with mirror: a row with bx != by whose bx
//                             lies in the window's Y bins counts at (by - bx0, bx - by0)), one workgroup per K24_TILE rows of the
//                             phase's range.  Three wave-uniform paths per workgroup:
//                               whole   nx ny <= K24_CELLS: LDS counters over the whole window;
//                               tile    else (bins of the tile's first .. last X) x (the other side's bins) <= K24_CELLS: LDS counters
//                                       over that strip of the window -- a tile of X-sorted rows spans few X bins;
//                               global  else: one global atomic per row.
//                             The LDS paths end with one global atomic per counter that is not zero.
//   k24_v4c                   phase 0: the rows with X in [v0, v1) (a table range) add at by; phase 1: every row with Y in [v0, v1)
//                             adds at bx.  LDS counters over all nb bins when nb <= K24_CELLS; else phase 1 keeps the bins of the
//                             tile's first .. last X in LDS when they fit (K22's window), and everything else is a global atomic.
//                             n_x / n_y: one 64-bit atomic per workgroup.
//   k24_keys .. k24_counts    the cells: key = (bx - bmin) << b | (by - bmin) (folded: the smaller first), b the bits of the largest
//                             bin index over all rows of the handle, rocPRIM radix sort over the 2 b bits in use, head flags, ONE rocPRIM exclusive scan, run
//                             starts scattered by rank, counts as differences of neighbouring starts, their maximum reduced per workgroup.
// No aggregation of equal cells inside a wave in front of the atomics in the shipped form: on chr1 of the synthetic genome the
// aggregated kernel (k22_agg, the developer build's CLOOPS_K24_AGG) took 17.7 instead of 20.2 us on a 1000 x 1000 window at 5 kb and
// 128 instead of 127 us on the whole chromosome at 50 kb -- the rows of a wave share bx but rarely by -- inside calls of 250 - 350 us
// (DESIGN.md, K24).  70 000 rows in one cell are 64-deep LDS conflicts, not global ones.  The LDS paths stay: with every add a
// global atomic (CLOOPS_K24_GLOBAL) the same kernels took 36 and 778 us.
// Only vector stores and ordinary HIP atomics; every index is checked against its array before a load or store.  Scratch (c->mx) is
// the handle's own, apart from the sweep's layouts, q index, count cache and the K8 / K13 / K14 / K20 - K23 state.
#define K24_TILE 2048                   // table rows per workgroup of k24_window and k24_v4c (8 per thread)
#define K24_CELLS 8192                  // LDS counters per workgroup (32 KB: four workgroups per CU)
#define K24_U (K24_TILE / TPB)          // rows per thread
#define K24_MAXRES (1ll << 29)          // res lies below 2^29
#define K24_MAXB0 (1ll << 30)           // |bx0|, |by0|, |b0| <= 2^30
#define K24_MAXNB (1ll << 24)           // bins of a virtual 4C
static_assert(K24_CELLS * 4 <= 64 * 1024, "the counters must fit a workgroup's static LDS");
static_assert(CL_MAT_CELLS_MAX == (1 << 24) && CL_MAT_WMAX == 8192, "the limits of include/cloops_hip.h");

struct K24Bin { K12Div dv; u32 shift; int B; };             // bin of key k (= p + 2^30): k12_div(dv, k + shift) - B
struct K24Win { int bx0, by0, nx, ny; };
struct K24T { long long t[4]; int n; };                     // X keys to search for (any value: below 0 -> 0, above 2^32 - 1 -> m)

__device__ __forceinline__ int k24_bin(const K24Bin& b, u32 key) { return (int)k12_div(b.dv, key + b.shift) - b.B; }

__global__ void __launch_bounds__(TPB)
k24_ranges(const u32* __restrict__ sx, int m, K24T t, int* __restrict__ rng)
{
    const int w = threadIdx.x >> 6;                                             // (TPB / 64 = 4 waves)
    if (w >= t.n || w >= 4) return;
    const long long v = t.t[w];
    const int r = v <= 0 ? 0 : v > 0xffffffffll ? m : k19_lb_wave(sx, m, (u32)v);
    if ((threadIdx.x & 63) == 0) rng[w] = r;
}

// sum of v over the workgroup into *dst (one atomic); called by every thread
__device__ __forceinline__ void k24_total(u32 v, u32* part, u64* dst)
{
    for (int o = 32; o > 0; o >>= 1) v += (u32)__shfl_xor((int)v, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
        for (int k = 0; k < TPB / 64; ++k) s += part[k];
        if (s) atomicAdd(dst, s);
    }
}

// out: nx * ny counters, row-major; rng: {first, end} of phase 0, {first, end} of phase 1; n_in: hits of both phases.  AGG: the lanes of
// a wave that share the first active lane's cell leave the add to that lane (k22_agg); no_lds: every add goes to global memory
template <bool AGG>
__global__ void __launch_bounds__(TPB)
k24_window(const u32* __restrict__ sx, const int* __restrict__ sy, int m, const int* __restrict__ rng, K24Bin b, K24Win w, int no_lds,
           u32* __restrict__ out, u64* __restrict__ n_in)
{
    __shared__ u32 cell[K24_CELLS];
    __shared__ u32 part[TPB / 64];
    const int ph = blockIdx.y ? 1 : 0;
    const int r0 = max(rng[2 * ph], 0), r1 = min(rng[2 * ph + 1], m);
    const long long t0 = (long long)r0 + (long long)blockIdx.x * K24_TILE;
    if (t0 >= r1) return;                                                       // (the whole workgroup)
    const int tn = (int)(r1 - t0 < K24_TILE ? r1 - t0 : K24_TILE);
    // p: the side that X falls on (rows of the window in phase 0, columns in phase 1), s: the side of Y
    const int p0 = ph ? w.by0 : w.bx0, np = ph ? w.ny : w.nx, s0 = ph ? w.bx0 : w.by0, ns = ph ? w.nx : w.ny;
    const int pf = min(max(k24_bin(b, sx[t0]) - p0, 0), np - 1), pl = min(max(k24_bin(b, sx[t0 + tn - 1]) - p0, pf), np - 1);
    const int span = pl - pf + 1;
    const long long all = (long long)w.nx * w.ny;
    const bool whole = !no_lds && all <= K24_CELLS;                             // (the three are the same in every lane)
    const bool tile = !no_lds && !whole && (long long)span * ns <= K24_CELLS;
    const int need = whole ? (int)all : tile ? span * ns : 0;
    for (int k = threadIdx.x; k < need; k += TPB) cell[k] = 0u;
    __syncthreads();
    u32 hits = 0u;
#pragma unroll 2
    for (int u = 0; u < K24_U; ++u) {                                           // (no early exit: every lane takes part in the ballots)
        const int il = u * TPB + (int)threadIdx.x;
        int g = K22_NONE, p = 0, s = 0;                                         // the cell in out: < nx ny <= 2^24
        if (il < tn) {
            const int bx = k24_bin(b, sx[t0 + il]), by = k24_bin(b, (u32)(sy[t0 + il] + (1 << 30)));
            p = bx - p0; s = by - s0;                                           // |bins| <= 2^30 + 1 and |p0|, |s0| <= 2^30: no overflow
            if (p >= 0 && p < np && s >= 0 && s < ns && !(ph && bx == by)) { g = ph ? s * w.ny + p : p * w.ny + s; ++hits; }
        }
        const u32 v = AGG ? k22_agg(g, 1u) : (g != K22_NONE ? 1u : 0u);
        if (!v) continue;
        if (whole) atomicAdd(&cell[g], v);
        else {
            const int q = p - pf;
            const long long k = ph ? (long long)s * span + q : (long long)q * ns + s;
            if (tile && q >= 0 && q < span && k < need) atomicAdd(&cell[k], v);
            else atomicAdd(&out[g], v);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < need; k += TPB) {
        const u32 v = cell[k];
        if (!v) continue;
        size_t g;
        if (whole) g = (size_t)k;
        else if (!ph) g = (size_t)pf * w.ny + k;                                // the strip of rows pf .. pl is contiguous in out
        else { const int s = k / span; g = (size_t)s * w.ny + pf + (k - s * span); }
        if (g < (size_t)all) atomicAdd(&out[g], v);
    }
    k24_total(hits, part, n_in);
}

// out: nb counters for the bins b0 ..; rng: {first, end} of the rows with X in [v0, v1); ctr: {n_x, n_y}
__global__ void __launch_bounds__(TPB)
k24_v4c(const u32* __restrict__ sx, const int* __restrict__ sy, int m, const int* __restrict__ rng, K24Bin b, int v0, int v1, int b0,
        int nb, u32* __restrict__ out, u64* __restrict__ ctr)
{
    __shared__ u32 cell[K24_CELLS];
    __shared__ u32 part[TPB / 64];
    const int ph = blockIdx.y ? 1 : 0;
    const int r0 = ph ? 0 : max(rng[0], 0), r1 = ph ? m : min(rng[1], m);
    const long long t0 = (long long)r0 + (long long)blockIdx.x * K24_TILE;
    if (t0 >= r1) return;                                                       // (the whole workgroup)
    const int tn = (int)(r1 - t0 < K24_TILE ? r1 - t0 : K24_TILE);
    const bool whole = nb <= K24_CELLS;                                         // (the same in every lane, as wf, need)
    int wf = 0, need = whole ? nb : 0;                                          // LDS counter k stands for out[wf + k]
    if (!whole && ph) {                                                         // the bins of this tile's X, clipped to [b0, b0 + nb)
        const long long f = max((long long)k24_bin(b, sx[t0]) - b0, 0ll), l = min((long long)k24_bin(b, sx[t0 + tn - 1]) - b0, (long long)nb - 1);
        if (f <= l && l - f + 1 <= K24_CELLS) { wf = (int)f; need = (int)(l - f + 1); }
    }
    for (int k = threadIdx.x; k < need; k += TPB) cell[k] = 0u;
    __syncthreads();
    u32 hits = 0u;
#pragma unroll 2
    for (int u = 0; u < K24_U; ++u) {
        const int il = u * TPB + (int)threadIdx.x;
        if (il >= tn) continue;
        const u32 kx = sx[t0 + il];
        const int y = sy[t0 + il];
        if (ph && (y < v0 || y >= v1)) continue;                                // (phase 0: the range was searched for X in [v0, v1))
        ++hits;
        const long long g = (long long)(ph ? k24_bin(b, kx) : k24_bin(b, (u32)(y + (1 << 30)))) - b0;
        if (g < 0 || g >= nb) continue;
        const long long k = g - wf;
        if (k >= 0 && k < need) atomicAdd(&cell[k], 1u);
        else atomicAdd(&out[g], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < need; k += TPB) {
        const u32 v = cell[k];
        if (v && wf + k < nb) atomicAdd(&out[wf + k], v);
    }
    k24_total(hits, part, &ctr[ph]);
}

__global__ void __launch_bounds__(TPB)
k24_keys(const u32* __restrict__ sx, const int* __restrict__ sy, int m, K24Bin b, int bmin, int bits, int fold, u64* __restrict__ key)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= m) return;
    u32 cx = (u32)(k24_bin(b, sx[i]) - bmin), cy = (u32)(k24_bin(b, (u32)(sy[i] + (1 << 30))) - bmin);   // >= 0: bmin is the smallest bin
    if (fold && cy < cx) { const u32 t = cx; cx = cy; cy = t; }
    key[i] = ((u64)cx << bits) | (u64)cy;
}

// flag[i] = sorted key i opens a run, i < m; flag[m] = 0 (the scan's entry m is then the number of runs)
__global__ void __launch_bounds__(TPB)
k24_heads(const u64* __restrict__ key, int m, u32* __restrict__ flag)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i > m) return;
    flag[i] = (i < m && (i == 0 || key[i] != key[i - 1])) ? 1u : 0u;
}

// start[r] = index of the first row of run r, start[n_cells] = m; the run's bins
__global__ void __launch_bounds__(TPB)
k24_starts(const u64* __restrict__ key, const u32* __restrict__ flag, const u32* __restrict__ rank, int m, int n_cells, int bmin, int bits,
           int* __restrict__ start, int* __restrict__ bx, int* __restrict__ by)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i > m) return;
    const u32 r = rank[i];
    if (i == m) { if (r == (u32)n_cells) start[r] = m; return; }
    if (!flag[i] || r >= (u32)n_cells) return;
    const u64 k = key[i];
    start[r] = (int)i;
    bx[r] = (int)(k >> bits) + bmin;
    by[r] = (int)(k & ((1ull << bits) - 1ull)) + bmin;
}

// cnt[r] = rows of run r; their maximum: a grid-stride share per thread, reduced over the wave and the workgroup, one atomic per
// workgroup (one per wave of 64 cells was 87 000 atomics on one address for 5.6 M cells: 0.7 ms)
__global__ void __launch_bounds__(TPB)
k24_counts(const int* __restrict__ start, int n_cells, u32* __restrict__ cnt, int* __restrict__ maxc)
{
    __shared__ int part[TPB / 64];
    int v = 0;
    for (long long r = (long long)blockIdx.x * TPB + threadIdx.x; r < n_cells; r += (long long)gridDim.x * TPB) {
        const int k = start[r + 1] - start[r];
        cnt[r] = (u32)k;
        v = max(v, k);
    }
    v = dpp_reduce_wave(v, OpMax());
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < TPB / 64; ++k) v = max(v, part[k]);
        if (v > 0) atomicMax(maxc, v);
    }
}

// ---- K24 host side ------------------------------------------------------------------------------
static long long k24_floordiv(long long p, long long res)
{
    const long long q = p / res;
    return q - ((p - q * res) < 0 ? 1 : 0);
}

static K24Bin k24_binning(int res)
{
    K24Bin b;
    const long long B = ((1ll << 30) + res - 1) / res;
    b.dv = k12_divisor((u32)res);
    b.shift = (u32)(B * res - (1ll << 30));                                     // in [0, res)
    b.B = (int)B;                                                               // <= 2^30
    return b;
}

// developer A/B of the window kernel's forms (CLOOPS_K24_AGG=1: wave aggregation, CLOOPS_K24_GLOBAL=1: no LDS counters); the shipped
// library reads no environment variable
static int k24_knob(const char* name)
{
#ifdef CLOOPS_DEVEL
    if (const char* e = getenv(name)) return atoi(e);
#endif
    (void)name;
    return 0;
}

static int k24_cut(int64_t cut) { return cut <= 0 ? 0 : (int)std::min<int64_t>(cut, 1ll << 30); }   // |Y - X| < 2^30: a larger cut keeps no row either

// mx.ctr: four ints (table ranges), then two 64-bit counters; zeroed
static int mat_counters(cl_chrom* c)
{
    int rc;
    if ((rc = c->mx.ctr.ensure(32))) return rc;
    HIP_TRY(hipMemsetAsync(c->mx.ctr.p, 0, 32, c->stream));
    return CL_OK;
}

static int mat_window(cl_chrom* c, int res, const K24Win& w, bool mirror, uint32_t* out, int64_t* n_in)
{
    const int m = c->ag.kept;
    const size_t cells = (size_t)w.nx * (size_t)w.ny;
    int rc;
    if ((rc = c->mx.out.ensure(cells * 4)) || (rc = mat_counters(c))) return rc;
    HIP_TRY(hipMemsetAsync(c->mx.out.p, 0, cells * 4, c->stream));
    int* rng = c->mx.ctr.as<int>();
    u64* ctr = (u64*)(rng + 4);
    K24T t{};
    t.n = mirror ? 4 : 2;
    t.t[0] = (long long)w.bx0 * res + (1ll << 30); t.t[1] = ((long long)w.bx0 + w.nx) * res + (1ll << 30);
    t.t[2] = (long long)w.by0 * res + (1ll << 30); t.t[3] = ((long long)w.by0 + w.ny) * res + (1ll << 30);
    hipLaunchKernelGGL(k24_ranges, dim3(1), dim3(TPB), 0, c->stream, c->ag.sx.as<u32>(), m, t, rng);
    HIP_TRY(hipGetLastError());
    const dim3 grid((unsigned)(((long long)m + K24_TILE - 1) / K24_TILE), mirror ? 2u : 1u);
    const int no_lds = k24_knob("CLOOPS_K24_GLOBAL") ? 1 : 0;
    if (k24_knob("CLOOPS_K24_AGG"))
        hipLaunchKernelGGL(k24_window<true>, grid, dim3(TPB), 0, c->stream, c->ag.sx.as<u32>(), c->ag.sy.as<int>(), m, (const int*)rng,
                           k24_binning(res), w, no_lds, c->mx.out.as<u32>(), ctr);
    else
        hipLaunchKernelGGL(k24_window<false>, grid, dim3(TPB), 0, c->stream, c->ag.sx.as<u32>(), c->ag.sy.as<int>(), m, (const int*)rng,
                           k24_binning(res), w, no_lds, c->mx.out.as<u32>(), ctr);
    HIP_TRY(hipGetLastError());
    u64 h = 0;
    HIP_TRY(hipMemcpyAsync(out, c->mx.out.p, cells * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&h, ctr, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *n_in = (int64_t)h;
    return CL_OK;
}

extern "C" int cl_mat_window(cl_chrom* c, int64_t cut, int64_t res, int64_t bx0, int64_t by0, int64_t nx, int64_t ny, int32_t mirror,
                             uint32_t* out, int64_t* n_in, int64_t* n_kept)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_in) *n_in = 0;
    if (n_kept) *n_kept = 0;
    if (!out || !n_in || !n_kept) return fail(CL_ERR_ARG, "cl_mat_window: bad arguments");
    if (res < 1 || res >= K24_MAXRES) return fail(CL_ERR_ARG, "cl_mat_window: res outside [1, 2^29)");
    if (nx < 1 || ny < 1 || nx > CL_MAT_WMAX || ny > CL_MAT_WMAX || nx * ny > CL_MAT_CELLS_MAX)
        return fail(CL_ERR_ARG, "cl_mat_window: needs 1 <= nx, ny <= 8192 and nx ny <= 2^24");
    if (bx0 < -K24_MAXB0 || bx0 > K24_MAXB0 || by0 < -K24_MAXB0 || by0 > K24_MAXB0) return fail(CL_ERR_ARG, "cl_mat_window: |bx0|, |by0| above 2^30");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_mat_window: asynchronous runs still in flight");
    std::memset(out, 0, (size_t)(nx * ny) * 4);
    if (c->n == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc = agg_table(c, k24_cut(cut));
    if (rc == CL_OK) {
        *n_kept = c->ag.kept;
        if (c->ag.kept > 0) {
            const K24Win w{(int)bx0, (int)by0, (int)nx, (int)ny};
            rc = mat_window(c, (int)res, w, mirror != 0, out, n_in);
        }
    }
    if (rc != CL_OK) { (void)hipStreamSynchronize(c->stream); *n_in = 0; *n_kept = 0; }   // no copy to the outputs may still be pending
    return rc;
}

static int mat_v4c(cl_chrom* c, int res, int v0, int v1, int b0, int nb, uint32_t* out, int64_t* n_x, int64_t* n_y)
{
    const int m = c->ag.kept;
    int rc;
    if ((rc = c->mx.out.ensure(std::max<size_t>((size_t)nb * 4, 16))) || (rc = mat_counters(c))) return rc;
    if (nb > 0) HIP_TRY(hipMemsetAsync(c->mx.out.p, 0, (size_t)nb * 4, c->stream));
    int* rng = c->mx.ctr.as<int>();
    u64* ctr = (u64*)(rng + 4);
    K24T t{};
    t.n = 2;
    t.t[0] = (long long)v0 + (1ll << 30); t.t[1] = (long long)v1 + (1ll << 30);
    hipLaunchKernelGGL(k24_ranges, dim3(1), dim3(TPB), 0, c->stream, c->ag.sx.as<u32>(), m, t, rng);
    HIP_TRY(hipGetLastError());
    const dim3 grid((unsigned)(((long long)m + K24_TILE - 1) / K24_TILE), 2u);
    hipLaunchKernelGGL(k24_v4c, grid, dim3(TPB), 0, c->stream, c->ag.sx.as<u32>(), c->ag.sy.as<int>(), m, (const int*)rng, k24_binning(res), v0, v1,
                       b0, nb, c->mx.out.as<u32>(), ctr);
    HIP_TRY(hipGetLastError());
    u64 h[2] = {0, 0};
    if (nb > 0) HIP_TRY(hipMemcpyAsync(out, c->mx.out.p, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h, ctr, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *n_x = (int64_t)h[0]; *n_y = (int64_t)h[1];
    return CL_OK;
}

extern "C" int cl_mat_v4c(cl_chrom* c, int64_t cut, int64_t res, int64_t v0, int64_t v1, int64_t b0, int64_t nb, uint32_t* out,
                          int64_t* n_x, int64_t* n_y, int64_t* n_kept)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_x) *n_x = 0;
    if (n_y) *n_y = 0;
    if (n_kept) *n_kept = 0;
    if (!n_x || !n_y || !n_kept || nb < 0 || nb > K24_MAXNB || (nb > 0 && !out)) return fail(CL_ERR_ARG, "cl_mat_v4c: bad arguments (0 <= nb <= 2^24)");
    if (res < 1 || res >= K24_MAXRES) return fail(CL_ERR_ARG, "cl_mat_v4c: res outside [1, 2^29)");
    if (v0 > v1) return fail(CL_ERR_ARG, "cl_mat_v4c: the viewpoint needs v0 <= v1");
    if (b0 < -K24_MAXB0 || b0 > K24_MAXB0) return fail(CL_ERR_ARG, "cl_mat_v4c: |b0| above 2^30");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_mat_v4c: asynchronous runs still in flight");
    if (nb > 0) std::memset(out, 0, (size_t)nb * 4);
    if (c->n == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc = agg_table(c, k24_cut(cut));
    if (rc == CL_OK) {
        *n_kept = c->ag.kept;
        // every coordinate satisfies |p| < 2^29: a bound beyond +-2^30 selects the same rows as the bound clamped there
        const int a = (int)std::max<int64_t>(-(1ll << 30), std::min<int64_t>(v0, 1ll << 30)), e = (int)std::max<int64_t>(-(1ll << 30), std::min<int64_t>(v1, 1ll << 30));
        if (c->ag.kept > 0) rc = mat_v4c(c, (int)res, a, e, (int)b0, (int)nb, out, n_x, n_y);
    }
    if (rc != CL_OK) { (void)hipStreamSynchronize(c->stream); *n_x = 0; *n_y = 0; *n_kept = 0; }
    return rc;
}

static int mat_cells(cl_chrom* c, int res, bool fold, cl_chrom::Mat::State& st)
{
    const int m = c->ag.kept;
    const size_t sm = (size_t)m;
    int rc;
    // the bins of ALL rows of the handle (whatever the cut) bound those of the kept rows: bmin only has to lie at or below every bin, and
    // a cut that narrows the span costs at most a few key bits
    const long long bmin = k24_floordiv(std::min(c->st.xmin, c->st.ymin), res), bmax = k24_floordiv(std::max(c->st.xmax, c->st.ymax), res);
    if (bmax < bmin || bmax - bmin >= (1ll << 30)) return fail(CL_ERR_HIP, "cl_mat_cells: the handle's coordinate range is not one a handle can have");
    if ((rc = mat_counters(c))) return rc;
    const int bits = std::max(1, bits_for((unsigned)(bmax - bmin)));            // bmax - bmin < 2^30: 2 bits <= 60
    if ((rc = c->mx.key.ensure(sm * 8)) || (rc = c->mx.sorted.ensure(sm * 8)) || (rc = c->mx.flag.ensure((sm + 1) * 4)) ||
        (rc = c->mx.scan.ensure((sm + 1) * 4))) return rc;
    const K24Bin b = k24_binning(res);
    LAUNCH(k24_keys, m, c->ag.sx.as<u32>(), c->ag.sy.as<int>(), m, b, (int)bmin, bits, fold ? 1 : 0, c->mx.key.as<u64>());
    HIP_TRY(hipGetLastError());
    if ((rc = prim_run(c->mx.tmp, "radix_sort_keys(matrix cells)", [&](void* tmp, size_t& bytes) {
            return rocprim::radix_sort_keys(tmp, bytes, c->mx.key.as<u64>(), c->mx.sorted.as<u64>(), sm, 0, 2 * bits, c->stream);
        })))
        return rc;
    LAUNCH(k24_heads, (long long)m + 1, c->mx.sorted.as<u64>(), m, c->mx.flag.as<u32>());
    HIP_TRY(hipGetLastError());
    if ((rc = prim_run(c->mx.tmp, "exclusive_scan(matrix cells)", [&](void* tmp, size_t& bytes) {
            return rocprim::exclusive_scan(tmp, bytes, c->mx.flag.as<u32>(), c->mx.scan.as<u32>(), 0u, sm + 1, rocprim::plus<u32>(), c->stream);
        })))
        return rc;
    u32 nc = 0;
    HIP_TRY(hipMemcpyAsync(&nc, c->mx.scan.as<u32>() + sm, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (nc < 1 || nc > (u32)m) return fail(CL_ERR_HIP, "cl_mat_cells: the scan left a number of cells no table can have");
    const size_t sc = (size_t)nc;
    if ((rc = c->mx.start.ensure((sc + 1) * 4)) || (rc = c->mx.bx.ensure(sc * 4)) || (rc = c->mx.by.ensure(sc * 4)) || (rc = c->mx.cnt.ensure(sc * 4))) return rc;
    LAUNCH(k24_starts, (long long)m + 1, c->mx.sorted.as<u64>(), c->mx.flag.as<u32>(), c->mx.scan.as<u32>(), m, (int)nc, (int)bmin, bits,
           c->mx.start.as<int>(), c->mx.bx.as<int>(), c->mx.by.as<int>());
    HIP_TRY(hipGetLastError());
    int* maxc = c->mx.ctr.as<int>();                                            // (zeroed above)
    hipLaunchKernelGGL(k24_counts, dim3((unsigned)std::max(1, std::min(1024, nblocks((long long)nc)))), dim3(TPB), 0, c->stream, c->mx.start.as<int>(),
                       (int)nc, c->mx.cnt.as<u32>(), maxc);
    HIP_TRY(hipGetLastError());
    int hmax = 0;
    HIP_TRY(hipMemcpyAsync(&hmax, maxc, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    st.n_cells = nc; st.max_count = hmax;
    return CL_OK;
}

extern "C" int cl_mat_cells(cl_chrom* c, int64_t cut, int64_t res, int32_t fold, int64_t* n_cells, int64_t* n_kept, int64_t* max_count)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_cells) *n_cells = 0;
    if (n_kept) *n_kept = 0;
    if (max_count) *max_count = 0;
    if (!n_cells || !n_kept || !max_count) return fail(CL_ERR_ARG, "cl_mat_cells: bad arguments");
    if (res < 1 || res >= K24_MAXRES) return fail(CL_ERR_ARG, "cl_mat_cells: res outside [1, 2^29)");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_mat_cells: asynchronous runs still in flight");
    cl_chrom::Mat::State st;
    st.ready = true;
    st.res = (int)res; st.fold = fold != 0;
    if (c->n == 0) { bal_release(c); scc_release(c); c->mx.st = st; return CL_OK; }
    HIP_TRY(hipSetDevice(c->device));
    bal_release(c);                                                             // (K25's state belongs to the earlier cells; every K25 call ends synchronised)
    scc_release(c);                                                             // (K28's scratch was sized for them; cl_scc_moments ends synchronised)
    int rc = agg_table(c, k24_cut(cut));
    if (rc == CL_OK) {
        st.n_kept = c->ag.kept;
        c->mx.st.ready = false;                                                    // (the buffers of the earlier cells are written from here on)
        if (c->ag.kept > 0) rc = mat_cells(c, (int)res, fold != 0, st);
    }
    if (rc != CL_OK) {
        (void)hipStreamSynchronize(c->stream);
        mat_release(c);
        return rc;
    }
    c->mx.st = st;
    *n_cells = st.n_cells; *n_kept = st.n_kept; *max_count = st.max_count;
    return CL_OK;
}

extern "C" int cl_mat_cells_get(cl_chrom* c, int64_t first, int64_t count, int32_t* bx, int32_t* by, uint32_t* cnt)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (!c->mx.st.ready) return fail(CL_ERR_ARG, "cl_mat_cells_get: no cells on this handle (cl_mat_cells)");
    if (!range_ok(first, count, c->mx.st.n_cells)) return fail(CL_ERR_ARG, "cl_mat_cells_get: range outside the cells");
    if (count > 0 && (!bx || !by || !cnt)) return fail(CL_ERR_ARG, "cl_mat_cells_get: bad arguments");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_mat_cells_get: asynchronous runs still in flight");
    if (count == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)count * 4;
    return read_back(c, "cl_mat_cells_get", {{bx, c->mx.bx.as<int>() + first, bytes}, {by, c->mx.by.as<int>() + first, bytes},
                                             {cnt, c->mx.cnt.as<u32>() + first, bytes}});
}

extern "C" int cl_mat_free(cl_chrom* c) { return unit_free(c, "cl_mat_free", mat_release); }
