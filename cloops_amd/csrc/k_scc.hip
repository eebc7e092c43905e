// k_scc.hip -- K28: the moments of the stratum-adjusted correlation (HiCRep's SCC) of two samples' contact matrices, from the folded cells
// that K24 left on both handles -- kernels and C entry points.
#include "cl_chrom.h"

// ==========================================================================================
// K28: both matrices under a (2h+1)^2 box sum; per diagonal the six integer moments of the two smoothed values
// ==========================================================================================
// Definitions: include/cloops_hip.h, cl_scc_moments.  The reference has nothing of the kind; tests/similarity_cases.py restates the
// definitions in numpy.  Input: the folded cells (bx, by, cnt) of two handles, a window of nb bins from b0, the box half-width h and D
// diagonals.  Everything is an integer; the host has checked that no sum can pass 2^64 (scc_smax) before anything is launched.
//   band form       T_s[u][q], nb rows of W = D + 4h columns (u32): column q holds A_s[u][u + q - 2h], the diagonals e = v - u of
//                   [-2h, D - 1 + 2h].  A box of half-width h around a pixel of diagonal d < D reaches the diagonals d - 2h .. d + 2h
//                   and nothing else.
//   k28_fill        one thread per cell: inside the window the cell is stored at (u, e) when e <= D - 1 + 2h, and at (v, -e) when
//                   0 < e <= 2h -- the symmetric half where boxes reach across the diagonal.  The cells are distinct, so no two
//                   threads store to one entry: plain stores into the cleared array.
//   k28_moments     one workgroup per tile of K28_TI bins x K28_TD diagonals.  Both samples' tiles with their halo (h rows above and
//                   below, 2h columns on each side) are staged in LDS, rows and columns outside the band as zero.  The box is
//                   separable: R[u][e] = sum over |t| <= h of T[u][e + t] is a running sum along a band row (one thread per row
//                   walks it and stores R over the entries it has finished with); S[i][d] = sum over |t| <= h of R[i + t][d - t] is
//                   an anti-diagonal walk in band coordinates, taken in registers.  A thread owns one diagonal of the tile and
//                   K28_TI / 8 of its bins; its moments are summed over the 8 threads of the diagonal (one shuffle, then LDS) and
//                   added to the accumulators of the diagonal with six 64-bit integer atomics per tile.  Integer addition is exact
//                   and has no order: two runs give the same bytes.
// The row stride in LDS is odd, so the threads that walk different rows, and the 32 diagonals a half-wave reads, fall into
// different banks.  LDS per workgroup: 2 (K28_TI + 2h) (K28_TD + 4h + 1) 4 bytes, at most 65088 (h = 20), always below the 64 KiB a
// launch may ask for without an attribute.  Only vector stores and integer HIP atomics; every index is checked against its array
// before a load or store; plain launches in the first handle's stream, no workgroup waits on another.
#define K28_TI 32                       // bins of a tile
#define K28_TD 32                       // diagonals of a tile: one per thread of a half-wave
#define K28_ROWS (TPB / K28_TD)         // threads of a diagonal (8): each takes K28_TI / K28_ROWS bins
#define K28_WAVES (TPB / 64)
static_assert(K28_TD == 32 && TPB == 256 && K28_TI % K28_ROWS == 0, "k28_moments maps thread t to diagonal t % 32 and bin row t / 32");
static_assert(K28_WAVES * 6 * K28_TD * 8 <= 2 * K28_TI * (K28_TD | 1) * 4, "the partial sums fit the tiles of h = 0");
static_assert(2 * (K28_TI + 2 * CL_SCC_HMAX) * ((K28_TD + 4 * CL_SCC_HMAX) | 1) * 4 <= 65536, "the tiles of both samples fit the default LDS of a launch");

struct K28Geo { long long b0, nb; int h, D, W; };          // W = D + 4h

__global__ void __launch_bounds__(TPB)
k28_fill(const int* __restrict__ bx, const int* __restrict__ by, const u32* __restrict__ cnt, long long n, K28Geo g, u32* __restrict__ T)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const long long u = (long long)bx[i] - g.b0, v = (long long)by[i] - g.b0;
    if (u < 0 || v < 0 || u >= g.nb || v >= g.nb || v < u) return;             // (folded cells: bx <= by)
    const long long e = v - u;
    const u32 c = cnt[i];
    if (e <= (long long)g.D - 1 + 2 * g.h) T[(size_t)u * g.W + (size_t)(e + 2 * g.h)] = c;
    if (e > 0 && e <= 2 * g.h) T[(size_t)v * g.W + (size_t)(2 * g.h - e)] = c;
}

__device__ __forceinline__ u64 k28_xor32(u64 v) { return (u64)__shfl_xor((unsigned long long)v, 32); }

// acc: six arrays of D u64 (n, sx, sy, sxx, syy, sxy)
__global__ void __launch_bounds__(TPB)
k28_moments(const u32* __restrict__ Ta, const u32* __restrict__ Tb, K28Geo g, u64* __restrict__ acc)
{
    extern __shared__ __align__(8) u32 lds[];
    const int h = g.h, rows = K28_TI + 2 * h, cols = K28_TD + 4 * h, stride = cols | 1;
    const long long i0 = (long long)blockIdx.x * K28_TI;                        // first bin of the tile
    const int d0 = (int)blockIdx.y * K28_TD;                                    // first diagonal of the tile (< D)
    if (i0 + d0 >= g.nb) return;                                                // no position (i, i + d) of the tile lies in the window (the whole workgroup, before any barrier)
    u32* __restrict__ sa = lds;
    u32* __restrict__ sb = lds + rows * stride;
    // the tiles: row r is bin i0 - h + r, column j is band column d0 + j (diagonal d0 - 2h + j)
    for (int t = threadIdx.x; t < rows * cols; t += TPB) {
        const int r = t / cols, j = t - r * cols;
        const long long u = i0 - h + r;
        const int q = d0 + j;
        u32 va = 0u, vb = 0u;
        if (u >= 0 && u < g.nb && q < g.W) {
            const size_t at = (size_t)u * g.W + (size_t)q;
            va = Ta[at]; vb = Tb[at];
        }
        sa[r * stride + j] = va; sb[r * stride + j] = vb;
    }
    __syncthreads();
    // R of the columns h .. cols - 1 - h of a row, stored from column 0 on: R(j) lands at j - h, an entry the running sum has left
    for (int t = threadIdx.x; t < 2 * rows; t += TPB) {
        u32* __restrict__ row = (t < rows ? sa + t * stride : sb + (t - rows) * stride);
        u32 run = 0u;
        for (int j = 0; j < 2 * h; ++j) run += row[j];
        for (int j = h; j < cols - h; ++j) {
            run += row[j + h];
            const u32 out = row[j - h];
            row[j - h] = run;
            run -= out;
        }
    }
    __syncthreads();
    const int dl = threadIdx.x & (K28_TD - 1), rl = threadIdx.x / K28_TD;
    const long long d = (long long)d0 + dl;
    u64 n = 0, sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
    if (d < g.D) {
        for (int k = 0; k < K28_TI / K28_ROWS; ++k) {
            const int il = rl + k * K28_ROWS;
            const long long i = i0 + il;
            if (i + d >= g.nb) break;                                           // (i ascends with k)
            // S[i][d]: rows il .. il + 2h of the tile (bins i - h .. i + h); R of diagonal d - t sits at column dl - t + h
            u32 x = 0u, y = 0u;
            for (int t = -h; t <= h; ++t) {
                const int at = (il + h + t) * stride + (dl - t + h);
                x += sa[at]; y += sb[at];
            }
            if (x | y) {
                n += 1; sx += x; sy += y;
                sxx += (u64)x * x; syy += (u64)y * y; sxy += (u64)x * y;
            }
        }
    }
    // the two threads of a diagonal inside a wave, then the four waves
    n += k28_xor32(n); sx += k28_xor32(sx); sy += k28_xor32(sy); sxx += k28_xor32(sxx); syy += k28_xor32(syy); sxy += k28_xor32(sxy);
    __syncthreads();                                                            // (the tiles are done with: their LDS takes the partial sums)
    u64 (*red)[6][K28_TD] = (u64 (*)[6][K28_TD])lds;                            // [K28_WAVES][6][K28_TD]: 6 KiB, below the smallest tiles' 8.25 KiB
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) < K28_TD) {
        red[wave][0][dl] = n; red[wave][1][dl] = sx; red[wave][2][dl] = sy; red[wave][3][dl] = sxx; red[wave][4][dl] = syy; red[wave][5][dl] = sxy;
    }
    __syncthreads();
    if (threadIdx.x < 6 * K28_TD) {
        const int m = threadIdx.x / K28_TD, dd = threadIdx.x - m * K28_TD;      // moment m of diagonal d0 + dd
        u64 s = 0;
        for (int w = 0; w < K28_WAVES; ++w) s += red[w][m][dd];
        if (s && (long long)d0 + dd < g.D) atomicAdd(acc + (size_t)m * g.D + (size_t)(d0 + dd), s);
    }
}

// ---- K28 host side ------------------------------------------------------------------------------
// the largest box sum a sample can have: min((2h+1)^2 max_count, 2 n_kept) -- a box holds at most (2h+1)^2 entries, and every kept
// row stands in at most two entries of the symmetric matrix
static unsigned __int128 scc_smax(const cl_chrom::Mat::State& st, int h)
{
    const unsigned __int128 box = (unsigned __int128)((2 * h + 1) * (2 * h + 1)) * (unsigned __int128)st.max_count;
    const unsigned __int128 all = (unsigned __int128)2 * (unsigned __int128)st.n_kept;
    return box < all ? box : all;
}

static int scc_fill(cl_chrom* a, cl_chrom* s, const K28Geo& g, DevBuf& band)
{
    cl_chrom* c = a;                                                            // (LAUNCH: everything runs in a's stream)
    const size_t bytes = (size_t)g.nb * (size_t)g.W * 4;
    int rc;
    if ((rc = band.ensure(bytes))) return rc;
    HIP_TRY(hipMemsetAsync(band.p, 0, bytes, c->stream));
    const long long n = s->mx.st.n_cells;
    if (n > 0) {
        LAUNCH(k28_fill, n, s->mx.bx.as<int>(), s->mx.by.as<int>(), s->mx.cnt.as<u32>(), n, g, band.as<u32>());
        HIP_TRY(hipGetLastError());
    }
    return CL_OK;
}

static int scc_moments(cl_chrom* a, cl_chrom* b, const K28Geo& g, int64_t* n, uint64_t* sx, uint64_t* sy, uint64_t* sxx, uint64_t* syy, uint64_t* sxy)
{
    cl_chrom* c = a;
    const size_t sd = (size_t)g.D;
    int rc;
    // b's stream has been waited for: its cells are at rest, and a's stream may read them
    if ((rc = scc_fill(a, a, g, a->sc.ta))) return rc;
    if (b != a && (rc = scc_fill(a, b, g, a->sc.tb))) return rc;
    if ((rc = a->sc.acc.ensure(6 * sd * 8))) return rc;
    HIP_TRY(hipMemsetAsync(a->sc.acc.p, 0, 6 * sd * 8, c->stream));
    const int rows = K28_TI + 2 * g.h, stride = (K28_TD + 4 * g.h) | 1;
    const size_t lds = (size_t)2 * rows * stride * 4;
    const dim3 grid((unsigned)((g.nb + K28_TI - 1) / K28_TI), (unsigned)((g.D + K28_TD - 1) / K28_TD));
    hipLaunchKernelGGL(k28_moments, grid, dim3(TPB), lds, c->stream, (const u32*)a->sc.ta.as<u32>(),
                       (const u32*)(b != a ? a->sc.tb.as<u32>() : a->sc.ta.as<u32>()), g, a->sc.acc.as<u64>());
    HIP_TRY(hipGetLastError());
    const u64* acc = a->sc.acc.as<u64>();
    return read_back(c, "cl_scc_moments", {{n, acc, sd * 8}, {sx, acc + sd, sd * 8}, {sy, acc + 2 * sd, sd * 8}, {sxx, acc + 3 * sd, sd * 8},
                                           {syy, acc + 4 * sd, sd * 8}, {sxy, acc + 5 * sd, sd * 8}});
}

extern "C" int cl_scc_moments(cl_chrom* a, cl_chrom* b, int64_t b0, int64_t nb, int32_t h, int64_t n_diags, int64_t* n, uint64_t* sx,
                              uint64_t* sy, uint64_t* sxx, uint64_t* syy, uint64_t* sxy)
{
    void* const outs[6] = {n, sx, sy, sxx, syy, sxy};
    if (n_diags >= 1 && n_diags <= CL_SCC_BAND_MAX)
        for (void* o : outs) if (o) std::memset(o, 0, (size_t)n_diags * 8);
    if (!a || !b) return fail(CL_ERR_ARG, "null chromosome handle");
    if (a->device != b->device) return fail(CL_ERR_ARG, "cl_scc_moments: the two handles are on different devices");
    if (a->enq != a->deq || b->enq != b->deq) return fail(CL_ERR_ARG, "cl_scc_moments: asynchronous runs still in flight");
    if (!a->mx.st.ready || !b->mx.st.ready) return fail(CL_ERR_ARG, "cl_scc_moments: no cells on a handle (cl_mat_cells)");
    if (!a->mx.st.fold || !b->mx.st.fold) return fail(CL_ERR_ARG, "cl_scc_moments: the cells of a handle are not folded (cl_mat_cells, fold = 1)");
    if (a->mx.st.res != b->mx.st.res) return fail(CL_ERR_ARG, "cl_scc_moments: the cells of the two handles have different res");
    if (h < 0 || h > CL_SCC_HMAX) return fail(CL_ERR_ARG, "cl_scc_moments: h outside [0, 20]");
    if (nb < 0 || nb > CL_SCC_BAND_MAX) return fail(CL_ERR_ARG, "cl_scc_moments: nb outside [0, 2^28]");
    if (n_diags < 0 || n_diags > nb || (n_diags == 0 && nb > 0)) return fail(CL_ERR_ARG, "cl_scc_moments: needs 1 <= n_diags <= nb (0 with nb = 0)");
    if (b0 < -(1ll << 30) || b0 > (1ll << 30)) return fail(CL_ERR_ARG, "cl_scc_moments: |b0| above 2^30");
    if (nb == 0) return CL_OK;
    for (void* o : outs) if (!o) return fail(CL_ERR_ARG, "cl_scc_moments: bad arguments");
    if (nb * (n_diags + 4 * (int64_t)h) > CL_SCC_BAND_MAX)
        return fail(CL_ERR_ARG, "cl_scc_moments: the band nb (n_diags + 4 h) has more than 2^28 entries");
    // the overflow rule, in exact arithmetic: a diagonal sums at most nb squares of box sums
    const unsigned __int128 sa = scc_smax(a->mx.st, h), sb = scc_smax(b->mx.st, h), sm = sa > sb ? sa : sb;
    if (sm >> 32 || sm * sm * (unsigned __int128)nb >> 64)
        return fail(CL_ERR_ARG, "cl_scc_moments: overflow rule: the squared box sums of a diagonal could pass 2^64 (smaller h, larger res or fewer bins)");
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(hipStreamSynchronize(a->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    const K28Geo g{(long long)b0, (long long)nb, (int)h, (int)n_diags, (int)(n_diags + 4 * (int64_t)h)};
    const int rc = scc_moments(a, b, g, n, sx, sy, sxx, syy, sxy);
    if (rc != CL_OK) {
        (void)hipStreamSynchronize(a->stream);                                  // no copy to the outputs may still be pending
        for (void* o : outs) std::memset(o, 0, (size_t)n_diags * 8);
        scc_release(a);
    }
    return rc;
}

extern "C" int cl_scc_free(cl_chrom* a) { return unit_free(a, "cl_scc_free", scc_release); }
