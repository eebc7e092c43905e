// k_dots.hip -- K29: loops called from the contact matrix itself, the donut enrichment test of HiCCUPS (Rao et al. 2014) over the folded
// cells that K24 left on the device, K25 weighted and K26 gave expected values -- kernels and C entry points.
#include <cmath>
#include "cl_chrom.h"

// ==========================================================================================
// K29: four neighbourhood sums of observed and expected around every pixel of a band; their histogram; the call
// ==========================================================================================
// Definitions: include/cloops_hip.h, cl_dot_lambdas.  The reference has nothing of the kind; tests/dots_cases.py restates the
// definitions in numpy.  Input: K24's cells, K25's bins b0 .. b0 + nb - 1 and ign, K26's effective weights ew (NaN on an invalid bin),
// its mask (one bit per bin) and expected[]; from the caller p < w and the diagonals [dmin, dmax).
//   band form       T[u][q], nb rows of W = dmax + 4w columns (fp64): column q holds V[u][u + q - 2w], the diagonals e = v - u of
//                   [-2w, dmax - 1 + 2w].  The footprint of a pixel of diagonal d < dmax reaches the diagonals d - 2w .. d + 2w.
//   k29_fill        one thread per cell: the raw count goes to the pixel's entry of the count plane (nb x (dmax - dmin) u32) when the
//                   cell lies in [dmin, dmax); the value (ew[bx] cnt) ew[by] of a used cell is stored at (u, e) when e <= dmax - 1 + 2w
//                   and at (v, -e) when 0 < e <= 2w -- the symmetric half where footprints reach across the diagonal.  The cells are
//                   distinct: plain stores into the cleared arrays.
//   k29_lambdas     one workgroup per tile of K29_TI bins x K29_TD diagonals; ONE fp64 tile in LDS with its halo (w rows above and
//                   below, 2w columns on each side), used twice: first it holds V from the band, and every thread takes the four
//                   sums NO_k of its pixels; then the workgroup overwrites it with E -- expected[|e|] where the row's bin and the
//                   column's bin are valid, made from a slice of expected[] and the validity of the tile's rows and columns, never
//                   stored in global memory -- and the same walk gives NE_k.  The walk of a pixel goes over its 2w + 1 rows
//                   ascending and over the columns of a row ascending, leaves out the inner (2p+1)^2 square, and adds an entry to
//                   each of the neighbourhoods that hold it (the union of the four is the (2w+1)^2 box less the inner square):
//                   T - (2p+1)^2 LDS reads of 8 bytes per pixel and matrix, T = (2w+1)^2, and per matrix 4 (w^2 - p^2) +
//                   (w^2 - p^2) + 2 * 6 (w - p) fp64 additions.  Only additions of non-negative terms, their order fixed by p and w:
//                   two runs give the same bytes.  A thread owns one diagonal of the tile and K29_TI / 8 of its bins: the 32 lanes
//                   of a half-wave read 32 consecutive doubles, and the row stride is odd.
//   k29_cells       la of the cells [first, first + count): a gather from the dense array.
//   k29_hist        one pass over the dense array: the chunk of each la by a branch-free search of the edges in LDS (padded to 64
//                   with +inf); the counts below K29_LC -- the zero-count column first of all -- in LDS counters per workgroup of
//                   16 384 pixels, flushed by one 64-bit atomic per non-zero counter; the larger counts, which are sparse, by 64-bit
//                   atomics straight to global memory.  (With the zero column alone in LDS a dense band spent its time in contended
//                   global atomics: 13.0 ms for 4.9 M pixels of which 3 M hold a cell.)
//   k29_flag / k29_scatter   one thread per cell: significant or not; an exclusive scan of the flags (rocPRIM) and the ascending list.
// LDS of k29_lambdas: (K29_TI + 2w) ((K29_TD + 4w) | 1) 8 bytes of tile, K29_TD + 4w doubles of expected, and the validity bytes: 50 656
// bytes at w = 16, below the 64 KiB a launch may ask for without an attribute.  Only vector stores and integer HIP atomics; every index
// is checked against its array before a load or store; plain launches in the handle's stream, no workgroup waits on another.
#define K29_TI 32                       // bins of a tile
#define K29_TD 32                       // diagonals of a tile: one per thread of a half-wave
#define K29_ROWS (TPB / K29_TD)         // threads of a diagonal (8): each takes K29_TI / K29_ROWS bins
#define K29_PER (K29_TI / K29_ROWS)
#define K29_HPT 64                      // pixels per thread of k29_hist
#define K29_LC 16                       // counts below it are counted in LDS (16 KiB of counters per workgroup)
#define K29_NC (CL_DOT_CMAX + 1)        // counts of a histogram row
static_assert(K29_TD == 32 && TPB == 256 && K29_TI % K29_ROWS == 0, "k29_lambdas maps thread t to diagonal t % 32 and bin row t / 32");
static_assert((K29_TI + 2 * CL_DOT_WMAX) * ((K29_TD + 4 * CL_DOT_WMAX) | 1) * 8 + (K29_TD + 4 * CL_DOT_WMAX) * 8 +
              (K29_TI + 2 * CL_DOT_WMAX) + (K29_TI + 2 * CL_DOT_WMAX + K29_TD + 4 * CL_DOT_WMAX) + 16 <= 65536,
              "the tile, the expected slice and the validity bytes fit the default LDS of a launch");
static_assert(CL_DOT_CHUNKS_MAX == 64, "the chunk search takes six halving steps and one more comparison");

struct K29Geo { long long b0; int nb, ign, p, w, dmin, dmax, W, ND; };          // W = dmax + 4w, ND = dmax - dmin

__device__ __forceinline__ bool k29_valid(const u64* __restrict__ mask, int nb, long long bin)
{
    return bin >= 0 && bin < nb && ((mask[bin >> 6] >> (bin & 63)) & 1ull);
}

__global__ void __launch_bounds__(TPB)
k29_fill(const int* __restrict__ bx, const int* __restrict__ by, const u32* __restrict__ cnt, long long n, K29Geo g, const double* __restrict__ ew,
         double* __restrict__ T, u32* __restrict__ pix)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const long long u = (long long)bx[i] - g.b0, v = (long long)by[i] - g.b0;
    if (u < 0 || v < 0 || u >= g.nb || v >= g.nb || v < u) return;              // (folded cells of the bins: never)
    const long long e = v - u;
    const u32 c = cnt[i];
    if (e >= g.dmin && e < g.dmax) pix[(size_t)u * g.ND + (size_t)(e - g.dmin)] = c;
    if (e < g.ign) return;
    const double wx = ew[u], wy = ew[v];
    if (wx != wx || wy != wy) return;
    const double val = (wx * (double)c) * wy;                                   // K25's order of operations
    if (e <= (long long)g.dmax - 1 + 2 * g.w) T[(size_t)u * g.W + (size_t)(e + 2 * g.w)] = val;
    if (e > 0 && e <= 2 * g.w) T[(size_t)v * g.W + (size_t)(2 * g.w - e)] = val;
}

// the four sums around the pixel whose entry of the tile is (r0, c0): row r0 + a holds the pixel's column at c0 - a
__device__ __forceinline__ void k29_walk(const double* __restrict__ tile, int stride, int r0, int c0, int p, int w, double s[4])
{
    double donut = 0.0, ll = 0.0, hz = 0.0, vt = 0.0;
    for (int a = -w; a <= w; ++a) {
        const double* __restrict__ row = tile + (r0 + a) * stride + (c0 - a);
        const bool ain = a >= -p && a <= p;
        for (int b = -w; b <= w; ++b) {
            const bool bin = b >= -p && b <= p;
            if (ain && bin) continue;                                           // (the same in every thread)
            const double x = row[b];
            if (a != 0 && b != 0) donut += x;
            if (a >= 1 && b <= -1) ll += x;
            if (!bin && a >= -1 && a <= 1) hz += x;
            if (!ain && b >= -1 && b <= 1) vt += x;
        }
    }
    s[0] = donut; s[1] = ll; s[2] = hz; s[3] = vt;
}

// la: four planes of nb x ND; ctr: {candidates, full pixels}
__global__ void __launch_bounds__(TPB)
k29_lambdas(const double* __restrict__ T, const u64* __restrict__ mask, const double* __restrict__ ew, const double* __restrict__ expected, K29Geo g,
            double nan, double* __restrict__ la, u64* __restrict__ ctr)
{
    extern __shared__ __align__(16) double lds29[];
    __shared__ u32 nct[2];
    const int w = g.w, rows = K29_TI + 2 * w, cols = K29_TD + 4 * w, stride = cols | 1;
    const long long i0 = (long long)blockIdx.x * K29_TI;                        // first bin of the tile
    const int d0 = g.dmin + (int)blockIdx.y * K29_TD;                           // first diagonal of the tile (< dmax)
    const size_t plane = (size_t)g.nb * (size_t)g.ND;
    const int dl = threadIdx.x & (K29_TD - 1), rl = threadIdx.x / K29_TD;
    const long long d = (long long)d0 + dl;
    if (i0 + d0 >= g.nb) {                                                      // no pixel (i, i + d) of the tile lies in the window (the whole workgroup)
        if (d < g.dmax)
            for (int k = 0; k < K29_PER; ++k) {
                const long long i = i0 + rl + k * K29_ROWS;
                if (i >= g.nb) break;
                const size_t at = (size_t)i * g.ND + (size_t)(d - g.dmin);
                for (int m = 0; m < 4; ++m) la[m * plane + at] = nan;
            }
        return;
    }
    double* __restrict__ tile = lds29;
    double* __restrict__ ex = lds29 + rows * stride;                            // expected of the tile's columns, 0 where E is 0 whatever the bins
    unsigned char* __restrict__ vr = (unsigned char*)(ex + cols);               // validity of the rows' bins i0 - w + r
    unsigned char* __restrict__ vb = vr + rows;                                 // ... of the bins i0 + d0 - 3w + k, k < rows + cols: entry (r, c) pairs with k = r + c
    if (threadIdx.x < 2) nct[threadIdx.x] = 0u;
    // the value tile: row r is bin i0 - w + r, column c is band column d0 + c (diagonal d0 - 2w + c)
    for (int t = threadIdx.x; t < rows * cols; t += TPB) {
        const int r = t / cols, cc = t - r * cols;
        const long long u = i0 - w + r;
        const int q = d0 + cc;
        double v = 0.0;
        if (u >= 0 && u < g.nb && q < g.W) v = T[(size_t)u * g.W + (size_t)q];
        tile[r * stride + cc] = v;
    }
    for (int t = threadIdx.x; t < cols; t += TPB) {
        const long long e = (long long)d0 - 2 * w + t, ae = e < 0 ? -e : e;
        double v = 0.0;
        if (ae >= g.ign && ae < g.nb) v = expected[ae];
        ex[t] = (v >= 0.0 && v <= 1.7976931348623157e308) ? v : 0.0;            // (a diagonal without a number has no valid pair: cl_dot_lambdas)
    }
    for (int t = threadIdx.x; t < rows; t += TPB) vr[t] = k29_valid(mask, g.nb, i0 - w + t) ? 1 : 0;
    for (int t = threadIdx.x; t < rows + cols; t += TPB) vb[t] = k29_valid(mask, g.nb, i0 + d0 - 3 * w + t) ? 1 : 0;
    __syncthreads();
    double no[K29_PER][4], ne[4];
    if (d < g.dmax)
        for (int k = 0; k < K29_PER; ++k) k29_walk(tile, stride, rl + k * K29_ROWS + w, dl + 2 * w, g.p, w, no[k]);
    __syncthreads();
    // E over the same entries
    for (int t = threadIdx.x; t < rows * cols; t += TPB) {
        const int r = t / cols, cc = t - r * cols;
        tile[r * stride + cc] = (vr[r] && vb[r + cc]) ? ex[cc] : 0.0;
    }
    __syncthreads();
    u32 ncand = 0u, nfull = 0u;
    if (d < g.dmax) {
        for (int k = 0; k < K29_PER; ++k) {
            const int il = rl + k * K29_ROWS;
            const long long i = i0 + il;
            if (i >= g.nb) break;                                               // (i ascends with k)
            const size_t at = (size_t)i * g.ND + (size_t)(d - g.dmin);
            const bool cand = i + d < g.nb && vr[il + w] && vb[il + dl + 3 * w];
            double out[4] = {nan, nan, nan, nan};
            if (cand) {
                k29_walk(tile, stride, il + w, dl + 2 * w, g.p, w, ne);
                const double ed = ex[dl + 2 * w], ww = ew[i] * ew[i + d];
                bool full = true;
                for (int m = 0; m < 4; ++m) {
                    if (ne[m] != 0.0) out[m] = ((no[k][m] / ne[m]) * ed) / ww;
                    full = full && out[m] == out[m];
                }
                ncand += 1u; nfull += full ? 1u : 0u;
            }
            for (int m = 0; m < 4; ++m) la[m * plane + at] = out[m];
        }
    }
    if (ncand) atomicAdd(&nct[0], ncand);
    if (nfull) atomicAdd(&nct[1], nfull);
    __syncthreads();
    if (threadIdx.x < 2 && nct[threadIdx.x]) atomicAdd(ctr + threadIdx.x, (u64)nct[threadIdx.x]);
}

// the entry of a cell's pixel in a plane of the dense array, or -1 when the cell lies outside the bins or the diagonals
__device__ __forceinline__ long long k29_pixel(const int* __restrict__ bx, const int* __restrict__ by, long long i, const K29Geo& g)
{
    const long long u = (long long)bx[i] - g.b0, v = (long long)by[i] - g.b0;
    if (u < 0 || v < 0 || u >= g.nb || v >= g.nb) return -1;
    const long long e = v - u;
    if (e < g.dmin || e >= g.dmax) return -1;
    return u * g.ND + (e - g.dmin);
}

__global__ void __launch_bounds__(TPB)
k29_cells(const int* __restrict__ bx, const int* __restrict__ by, long long first, long long count, long long n, K29Geo g, const double* __restrict__ la,
          double nan, double* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= count || first + i >= n) return;
    const long long at = k29_pixel(bx, by, first + i, g);
    const size_t plane = (size_t)g.nb * (size_t)g.ND;
    for (int m = 0; m < 4; ++m) out[4 * i + m] = at < 0 ? nan : la[m * plane + (size_t)at];
}

// se: the edges, +inf from n_chunks on -> the number of edges below x = the smallest l with x <= edges[l] (n_chunks: beyond)
__device__ __forceinline__ int k29_chunk(const double* __restrict__ se, double x)
{
    int l = 0;
#pragma unroll
    for (int step = CL_DOT_CHUNKS_MAX / 2; step >= 1; step >>= 1) l += se[l + step - 1] < x ? step : 0;
    return l + (se[l] < x ? 1 : 0);                                             // (l <= 63)
}

__device__ __forceinline__ void k29_edges_to_lds(double* se, const double* __restrict__ edges, int nch)
{
    for (int t = threadIdx.x; t < CL_DOT_CHUNKS_MAX; t += TPB) se[t] = t < nch ? edges[t] : __longlong_as_double(0x7ff0000000000000ll);
}

// hist: [4][nch][K29_NC]
__global__ void __launch_bounds__(TPB)
k29_hist(const double* __restrict__ la, const u32* __restrict__ pix, size_t npix, const double* __restrict__ edges, int nch, u64* __restrict__ hist,
         u64* __restrict__ beyond)
{
    __shared__ double se[CL_DOT_CHUNKS_MAX];
    __shared__ u32 zc[4 * CL_DOT_CHUNKS_MAX * K29_LC];                          // [kernel][chunk][count < K29_LC]
    __shared__ u32 sbey;
    k29_edges_to_lds(se, edges, nch);
    for (int t = threadIdx.x; t < 4 * CL_DOT_CHUNKS_MAX * K29_LC; t += TPB) zc[t] = 0u;
    if (threadIdx.x == 0) sbey = 0u;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * (TPB * K29_HPT);
    for (int it = 0; it < K29_HPT; ++it) {
        const size_t at = base + (size_t)it * TPB + threadIdx.x;
        if (at >= npix) break;
        double x[4];
        bool full = true;
        for (int m = 0; m < 4; ++m) { x[m] = la[m * npix + at]; full = full && x[m] == x[m]; }
        if (!full) continue;
        int l[4];
        bool bey = false;
        for (int m = 0; m < 4; ++m) { l[m] = k29_chunk(se, x[m]); bey = bey || l[m] >= nch; }
        if (bey) { atomicAdd(&sbey, 1u); continue; }
        const u32 c = min(pix[at], (u32)CL_DOT_CMAX);
        for (int m = 0; m < 4; ++m) {
            if (c < (u32)K29_LC) atomicAdd(&zc[(m * CL_DOT_CHUNKS_MAX + l[m]) * K29_LC + (int)c], 1u);
            else atomicAdd(hist + ((size_t)m * nch + (size_t)l[m]) * K29_NC + c, 1ull);
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 4 * CL_DOT_CHUNKS_MAX * K29_LC; t += TPB) {
        const int ml = t / K29_LC, c = t - ml * K29_LC, m = ml / CL_DOT_CHUNKS_MAX, ll = ml - m * CL_DOT_CHUNKS_MAX;
        if (zc[t] && ll < nch) atomicAdd(hist + ((size_t)m * nch + (size_t)ll) * K29_NC + c, (u64)zc[t]);
    }
    if (threadIdx.x == 0 && sbey) atomicAdd(beyond, (u64)sbey);
}

// flag[i] = 1 iff cell i is significant (flag[n] = 0: the scan's last entry is the total)
__global__ void __launch_bounds__(TPB)
k29_flag(const int* __restrict__ bx, const int* __restrict__ by, const u32* __restrict__ cnt, long long n, K29Geo g, const double* __restrict__ la,
         const double* __restrict__ edges, int nch, const u32* __restrict__ thr, u32* __restrict__ flag)
{
    __shared__ double se[CL_DOT_CHUNKS_MAX];
    k29_edges_to_lds(se, edges, nch);
    __syncthreads();
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i > n) return;
    u32 f = 0u;
    if (i < n) {
        const long long at = k29_pixel(bx, by, i, g);
        if (at >= 0) {
            const size_t plane = (size_t)g.nb * (size_t)g.ND;
            const u32 c = cnt[i];
            f = 1u;
            for (int m = 0; m < 4; ++m) {
                const double x = la[m * plane + (size_t)at];
                const int l = k29_chunk(se, x);
                if (!(x == x) || l >= nch || c < thr[m * nch + (l < nch ? l : 0)]) f = 0u;
            }
        }
    }
    flag[i] = f;
}

__global__ void __launch_bounds__(TPB)
k29_scatter(const u32* __restrict__ flag, const u32* __restrict__ scan, long long n, long long* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const u32 at = scan[i];
    if ((long long)at < n) out[at] = i;
}

// ---- K29 host side ------------------------------------------------------------------------------
// the checks every K29 call shares; -> CL_OK with c usable
static int dot_enter(cl_chrom* c, const char* who, bool need_lambdas)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, who, "asynchronous runs still in flight");
    if (!c->bl.st.ready || !c->ex.st.ready || !c->ex.st.expected) return fail(CL_ERR_ARG, who, "no expected values on this handle (cl_exp_set)");
    if (need_lambdas && !c->dt.st.lambdas) return fail(CL_ERR_ARG, who, "no lambdas on this handle (cl_dot_lambdas)");
    return CL_OK;
}

static K29Geo dot_geo(const cl_chrom* c)
{
    const cl_chrom::Dot::State& st = c->dt.st;
    return K29Geo{c->bl.st.b0, (int)c->bl.st.nb, c->bl.st.ignore_diags, st.p, st.w, (int)st.dmin, (int)st.dmax, (int)(st.dmax + 4 * st.w),
                  (int)(st.dmax - st.dmin)};
}

static int dot_lambdas(cl_chrom* c, const K29Geo& g, long long* n_cand, long long* n_full)
{
    const size_t npix = (size_t)g.nb * (size_t)g.ND, band = (size_t)g.nb * (size_t)g.W;
    const long long n = c->bl.st.n_cells;
    const double nan = std::nan("");
    int rc;
    if ((rc = c->dt.band.ensure(band * 8)) || (rc = c->dt.la.ensure(4 * npix * 8)) || (rc = c->dt.pix.ensure(npix * 4)) || (rc = c->dt.ctr.ensure(64)))
        return rc;
    HIP_TRY(hipMemsetAsync(c->dt.band.p, 0, band * 8, c->stream));
    HIP_TRY(hipMemsetAsync(c->dt.pix.p, 0, npix * 4, c->stream));
    HIP_TRY(hipMemsetAsync(c->dt.ctr.p, 0, 64, c->stream));
    if (n > 0) {
        LAUNCH(k29_fill, n, c->mx.bx.as<int>(), c->mx.by.as<int>(), c->mx.cnt.as<u32>(), n, g, (const double*)c->ex.w.as<double>(), c->dt.band.as<double>(),
               c->dt.pix.as<u32>());
        HIP_TRY(hipGetLastError());
    }
    const int rows = K29_TI + 2 * g.w, cols = K29_TD + 4 * g.w, stride = cols | 1;
    const size_t lds = (size_t)rows * stride * 8 + (size_t)cols * 8 + (size_t)rows + (size_t)(rows + cols);
    const dim3 grid((unsigned)((g.nb + K29_TI - 1) / K29_TI), (unsigned)((g.ND + K29_TD - 1) / K29_TD));
    hipLaunchKernelGGL(k29_lambdas, grid, dim3(TPB), lds, c->stream, (const double*)c->dt.band.as<double>(), (const u64*)c->ex.mask.as<u64>(),
                       (const double*)c->ex.w.as<double>(), (const double*)c->ex.exp.as<double>(), g, nan, c->dt.la.as<double>(), c->dt.ctr.as<u64>());
    HIP_TRY(hipGetLastError());
    u64 h[2] = {0, 0};
    if ((rc = read_back(c, "cl_dot_lambdas", {{h, c->dt.ctr.p, 16}}))) return rc;
    *n_cand = (long long)h[0]; *n_full = (long long)h[1];
    return CL_OK;
}

extern "C" int cl_dot_lambdas(cl_chrom* c, int32_t p, int32_t w, int64_t dmin, int64_t dmax, int64_t* n_cand, int64_t* n_full)
{
    if (n_cand) *n_cand = 0;
    if (n_full) *n_full = 0;
    int rc = dot_enter(c, "cl_dot_lambdas", false);
    if (rc != CL_OK) return rc;
    if (!n_cand || !n_full) return fail(CL_ERR_ARG, "cl_dot_lambdas: bad arguments");
    if (p < 0 || p >= w || w > CL_DOT_WMAX) return fail(CL_ERR_ARG, "cl_dot_lambdas: needs 0 <= p < w <= 16");
    const long long nb = c->bl.st.nb, ign = c->bl.st.ignore_diags;
    if (nb == 0 ? (dmin != 0 || dmax != 0) : !(ign <= dmin && dmin < dmax && dmax <= nb))
        return fail(CL_ERR_ARG, "cl_dot_lambdas: needs ignore_diags <= dmin < dmax <= nb (dmin = dmax = 0 with nb = 0)");
    cl_chrom::Dot::State st;
    st.lambdas = true; st.p = p; st.w = w; st.dmin = dmin; st.dmax = dmax;
    if (nb == 0) { dot_release(c); c->dt.st = st; return CL_OK; }                // (no bins: no HIP call)
    if (nb * (dmax + 4 * (int64_t)w) > CL_DOT_BAND_MAX) return fail(CL_ERR_ARG, "cl_dot_lambdas: the band nb (dmax + 4 w) has more than 2^27 entries");
    HIP_TRY(hipSetDevice(c->device));
    {   // the rule on the expected values, on the host
        const size_t m = (size_t)std::min<long long>(nb, dmax + 2 * (long long)w);
        std::vector<long long> pairs(m);
        std::vector<double> e(m);
        if ((rc = read_back(c, "cl_dot_lambdas", {{pairs.data(), c->ex.pairs.p, m * 8}, {e.data(), c->ex.exp.p, m * 8}}))) return rc;
        for (size_t k = (size_t)ign; k < m; ++k)
            if (pairs[k] > 0 && !(e[k] >= 0.0 && std::isfinite(e[k])))
                return fail(CL_ERR_ARG, "cl_dot_lambdas: an expected value of the band is NaN, infinite or negative on a diagonal with valid pairs");
    }
    c->dt.st = cl_chrom::Dot::State();                                          // (the earlier state's buffers are written from here on)
    c->dt.st.p = p; c->dt.st.w = w; c->dt.st.dmin = dmin; c->dt.st.dmax = dmax;
    long long nc = 0, nf = 0;
    rc = dot_lambdas(c, dot_geo(c), &nc, &nf);
    if (rc != CL_OK) {
        (void)hipStreamSynchronize(c->stream);
        dot_release(c);
        return rc;
    }
    c->dt.st = st;
    *n_cand = nc; *n_full = nf;
    return CL_OK;
}

extern "C" int cl_dot_lambdas_get(cl_chrom* c, int32_t kernel, int64_t first_bin, int64_t n_bins, double* la)
{
    int rc = dot_enter(c, "cl_dot_lambdas_get", true);
    if (rc != CL_OK) return rc;
    if (kernel < 0 || kernel > 3) return fail(CL_ERR_ARG, "cl_dot_lambdas_get: kernel outside [0, 3]");
    if (!range_ok(first_bin, n_bins, c->bl.st.nb)) return fail(CL_ERR_ARG, "cl_dot_lambdas_get: range outside the bins");
    const size_t nd = (size_t)(c->dt.st.dmax - c->dt.st.dmin);
    if (n_bins > 0 && !la) return fail(CL_ERR_ARG, "cl_dot_lambdas_get: bad arguments");
    if (n_bins == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t plane = (size_t)c->bl.st.nb * nd;
    return read_back(c, "cl_dot_lambdas_get", {{la, c->dt.la.as<double>() + (size_t)kernel * plane + (size_t)first_bin * nd, (size_t)n_bins * nd * 8}});
}

extern "C" int cl_dot_cells_get(cl_chrom* c, int64_t first, int64_t count, double* la4)
{
    int rc = dot_enter(c, "cl_dot_cells_get", true);
    if (rc != CL_OK) return rc;
    if (!range_ok(first, count, c->bl.st.n_cells)) return fail(CL_ERR_ARG, "cl_dot_cells_get: range outside the cells");
    if (count > 0 && !la4) return fail(CL_ERR_ARG, "cl_dot_cells_get: bad arguments");
    if (count == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->dt.out.ensure((size_t)count * 32))) return rc;
    LAUNCH(k29_cells, count, c->mx.bx.as<int>(), c->mx.by.as<int>(), (long long)first, (long long)count, c->bl.st.n_cells, dot_geo(c),
           (const double*)c->dt.la.as<double>(), std::nan(""), c->dt.out.as<double>());
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(CL_ERR_HIP, "cl_dot_cells_get", hipGetErrorString(e));
    return read_back(c, "cl_dot_cells_get", {{la4, c->dt.out.p, (size_t)count * 32}});
}

static int dot_hist(cl_chrom* c, const double* edges, int nch, uint64_t* hist, uint64_t* n_beyond)
{
    const K29Geo g = dot_geo(c);
    const size_t npix = (size_t)g.nb * (size_t)g.ND, hbytes = (size_t)4 * nch * K29_NC * 8;
    int rc;
    if ((rc = c->dt.edges.ensure(CL_DOT_CHUNKS_MAX * 8)) || (rc = c->dt.hist.ensure(hbytes)) || (rc = c->dt.ctr.ensure(64))) return rc;
    HIP_TRY(hipMemcpyAsync(c->dt.edges.p, edges, (size_t)nch * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->dt.hist.p, 0, hbytes, c->stream));
    HIP_TRY(hipMemsetAsync(c->dt.ctr.p, 0, 64, c->stream));
    hipLaunchKernelGGL(k29_hist, dim3((unsigned)((npix + (size_t)TPB * K29_HPT - 1) / ((size_t)TPB * K29_HPT))), dim3(TPB), 0, c->stream,
                       (const double*)c->dt.la.as<double>(), (const u32*)c->dt.pix.as<u32>(), npix, (const double*)c->dt.edges.as<double>(), nch,
                       c->dt.hist.as<u64>(), c->dt.ctr.as<u64>());
    HIP_TRY(hipGetLastError());
    return read_back(c, "cl_dot_hist", {{hist, c->dt.hist.p, hbytes}, {n_beyond, c->dt.ctr.p, 8}});
}

extern "C" int cl_dot_hist(cl_chrom* c, const double* edges, int32_t n_chunks, uint64_t* hist, uint64_t* n_beyond)
{
    if (n_beyond) *n_beyond = 0;
    int rc = dot_enter(c, "cl_dot_hist", true);
    if (rc != CL_OK) return rc;
    if (n_chunks < 1 || n_chunks > CL_DOT_CHUNKS_MAX) return fail(CL_ERR_ARG, "cl_dot_hist: n_chunks outside [1, 64]");
    if (!edges) return fail(CL_ERR_ARG, "cl_dot_hist: bad arguments");
    for (int l = 0; l < n_chunks; ++l)
        if (!(std::isfinite(edges[l]) && edges[l] > 0.0 && (l == 0 || edges[l] > edges[l - 1])))
            return fail(CL_ERR_ARG, "cl_dot_hist: the edges must be finite, above 0 and strictly ascending");
    const bool empty = c->bl.st.nb == 0;
    if (!empty && (!hist || !n_beyond)) return fail(CL_ERR_ARG, "cl_dot_hist: bad arguments");
    c->dt.st.hist = c->dt.st.called = false;
    if (empty) {
        if (hist) std::memset(hist, 0, (size_t)4 * n_chunks * K29_NC * 8);
    } else {
        HIP_TRY(hipSetDevice(c->device));
        rc = dot_hist(c, edges, n_chunks, hist, n_beyond);
        if (rc != CL_OK) {
            (void)hipStreamSynchronize(c->stream);
            *n_beyond = 0;
            return rc;
        }
    }
    c->dt.st.hist = true; c->dt.st.n_chunks = n_chunks;
    return CL_OK;
}

static int dot_call(cl_chrom* c, const uint32_t* thr, long long* n_sig)
{
    const long long n = c->bl.st.n_cells;
    const size_t sn = (size_t)n;
    const int nch = c->dt.st.n_chunks;
    int rc;
    if ((rc = c->dt.thr.ensure((size_t)4 * nch * 4)) || (rc = c->dt.flag.ensure((sn + 1) * 4)) || (rc = c->dt.scan.ensure((sn + 1) * 4)) ||
        (rc = c->dt.sig.ensure(sn * 8)))
        return rc;
    HIP_TRY(hipMemcpyAsync(c->dt.thr.p, thr, (size_t)4 * nch * 4, hipMemcpyHostToDevice, c->stream));
    LAUNCH(k29_flag, n + 1, c->mx.bx.as<int>(), c->mx.by.as<int>(), c->mx.cnt.as<u32>(), n, dot_geo(c), (const double*)c->dt.la.as<double>(),
           (const double*)c->dt.edges.as<double>(), nch, (const u32*)c->dt.thr.as<u32>(), c->dt.flag.as<u32>());
    HIP_TRY(hipGetLastError());
    if ((rc = prim_run(c->dt.tmp, "exclusive_scan(dots)", [&](void* tmp, size_t& bytes) {
            return rocprim::exclusive_scan(tmp, bytes, c->dt.flag.as<u32>(), c->dt.scan.as<u32>(), 0u, sn + 1, rocprim::plus<u32>(), c->stream);
        })))
        return rc;
    LAUNCH(k29_scatter, n, (const u32*)c->dt.flag.as<u32>(), (const u32*)c->dt.scan.as<u32>(), n, c->dt.sig.as<long long>());
    HIP_TRY(hipGetLastError());
    u32 total = 0;
    if ((rc = read_back(c, "cl_dot_call", {{&total, c->dt.scan.as<u32>() + sn, 4}}))) return rc;
    *n_sig = (long long)total;
    return CL_OK;
}

extern "C" int cl_dot_call(cl_chrom* c, const uint32_t* thr, int64_t* n_sig)
{
    if (n_sig) *n_sig = 0;
    int rc = dot_enter(c, "cl_dot_call", true);
    if (rc != CL_OK) return rc;
    if (!c->dt.st.hist) return fail(CL_ERR_ARG, "cl_dot_call: no histogram on this handle (cl_dot_hist)");
    if (!thr || !n_sig) return fail(CL_ERR_ARG, "cl_dot_call: bad arguments");
    c->dt.st.called = false; c->dt.st.n_sig = 0;
    long long ns = 0;
    if (c->bl.st.n_cells > 0 && c->bl.st.nb > 0) {
        HIP_TRY(hipSetDevice(c->device));
        rc = dot_call(c, thr, &ns);
        if (rc != CL_OK) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    }
    c->dt.st.called = true; c->dt.st.n_sig = ns;
    *n_sig = ns;
    return CL_OK;
}

extern "C" int cl_dot_sig_get(cl_chrom* c, int64_t first, int64_t count, int64_t* cell_index)
{
    int rc = dot_enter(c, "cl_dot_sig_get", true);
    if (rc != CL_OK) return rc;
    if (!c->dt.st.called) return fail(CL_ERR_ARG, "cl_dot_sig_get: no call on this handle (cl_dot_call)");
    if (!range_ok(first, count, c->dt.st.n_sig)) return fail(CL_ERR_ARG, "cl_dot_sig_get: range outside the significant cells");
    if (count > 0 && !cell_index) return fail(CL_ERR_ARG, "cl_dot_sig_get: bad arguments");
    if (count == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    return read_back(c, "cl_dot_sig_get", {{cell_index, c->dt.sig.as<long long>() + first, (size_t)count * 8}});
}

extern "C" int cl_dot_free(cl_chrom* c) { return unit_free(c, "cl_dot_free", dot_release); }
