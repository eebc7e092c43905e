// k_saddle.hip -- K30: saddle tables -- per pair of bin classes the bin pairs, the cells and the sum of the O/E of the folded cells that
// K24 left on the device, K25 weighted and K26 gave expected values -- kernels and C entry points.
#include <cmath>
#include <vector>
#include "cl_chrom.h"

// ==========================================================================================
// K30: three n_cls x n_cls tables over the pairs of a band: pairs (exact), cells (exact), sum of O/E (fp64, keyed reduction)
// ==========================================================================================
// Definitions: include/cloops_hip.h, cl_sad_sums.  The reference has nothing of the kind; tests/saddle_cases.py restates the
// definitions in numpy.  Input: K24's cells as they lie (c->mx.bx / by / cnt, ascending by bx then by), K26's effective weights
// c->ex.w (NaN = invalid bin) and expected values c->ex.exp, and the caller's classes.  One array drives everything: kc[i], the
// effective class of bin i -- the caller's class on a valid bin, -1 on every other bin (made on the host, which looks at K26's state
// for the rule on the expected values anyway).
//   k30_hist / k30_scan   the per-class prefix counts at the bounds of tiles of K30_PT bins: one wave per tile, lane = class, counts the
//                   tile's bins of its class; then one lane per class adds the tiles in tile order.  C_b(k) = the bins below k of class
//                   b = tb[k / PT][b] + a count over the at most PT - 1 bins from the tile's start (k30_prefix).
//   k30_pairs       pairs[a][.] += for every bin i of class a the per-class counts D of the bins in [i + lo, min(i + hi, nb)).  One wave
//                   per tile of K30_PT bins, lane = class b: D of the tile's first bin is a difference of two prefix counts; from a
//                   bin to the next the window slides by one bin at either end, so D changes by at most one in two classes.  nb n_cls
//                   look-ups in all, whatever the band's width.  The tile's table in LDS (u64), then integer atomics for its non-zero
//                   entries.
//   k30_sums        the hot path: the cells once, as they lie.  The cells are cut into tiles of K30_TILE = 256 and the tiles into
//                   K30_CHUNKS chunks of consecutive tiles -- a constant of this unit, not the CU count; one workgroup per chunk with
//                   its own fp64 table (and a u32 table of cell counts) in LDS.  A step takes one tile, one cell per thread: key = a
//                   n_cls + b and the O/E term made on the fly, or no key outside P.  Inside a wave the 64 cells are folded key by
//                   key: the lowest pending lane broadcasts its key, the lanes with that key are summed by a fixed butterfly (the other
//                   lanes add zeros: exact), and the wave notes (key, sum, lanes) in its list.  The loop runs once per distinct key
//                   of the step: row-major cells share cls[bx] along a row and cls[by] changes slowly on a smooth track.  Then wave 0
//                   adds the four lists to the table in wave order (the keys of one list are distinct: no two lanes meet).  The
//                   order of the additions of an entry is: chunk, tile, wave, butterfly -- fixed by the cells' positions alone.
//   k30_fold        the chunk tables in chunk order, one thread per entry.
// Only vector stores and integer HIP atomics; every index is checked against its array before a load or store; plain launches in the
// handle's stream, no workgroup waits on another.
#define K30_PT 256                      // bins per workgroup of the pair counts (one wave, lane = class)
#define K30_TILE TPB                    // cells per step of a workgroup of the sums: one per thread
#define K30_CHUNKS 1024                 // most workgroups (= chunk tables) of the sums
#define K30_WAVES (TPB / 64)
static_assert(CL_SAD_CLASSES_MAX == 64, "a class is a lane of the pair kernels; a table is 64 x 64 entries at most");
static_assert(CL_SAD_CLASSES_MAX * CL_SAD_CLASSES_MAX * 12 + 4096 <= 65536, "the two LDS tables and the lists of k30_sums");

struct K30In {                          // what k30_sums reads
    const int* bx; const int* by; const u32* cnt;                               // n cells
    const double* ew; const double* ex;                                         // nb effective weights, nb expected values
    const int* kc;                                                              // nb effective classes
    int n, b0, nb, ncls, lo, hi;
};

// th[t][b] = the bins of tile t with class b
__global__ void __launch_bounds__(64)
k30_hist(const int* __restrict__ kc, int nb, int ncls, u32* __restrict__ th)
{
    const int b = threadIdx.x;
    const long long j0 = (long long)blockIdx.x * K30_PT, j1 = j0 + K30_PT < nb ? j0 + K30_PT : nb;
    u32 c = 0u;
    for (long long j = j0; j < j1; ++j) c += kc[j] == b ? 1u : 0u;
    if (b < ncls) th[(size_t)blockIdx.x * ncls + b] = c;
}

// tb[t][b] = the bins of the tiles before t with class b, t = 0 .. ntiles, in tile order
__global__ void __launch_bounds__(64)
k30_scan(const u32* __restrict__ th, int ntiles, int ncls, u32* __restrict__ tb)
{
    const int b = threadIdx.x;
    if (b >= ncls) return;
    u32 s = 0u;
    for (int t = 0; t <= ntiles; ++t) {
        tb[(size_t)t * ncls + b] = s;
        if (t < ntiles) s += th[(size_t)t * ncls + b];
    }
}

// C_b(k): the bins below k of class b, 0 <= k <= nb (all lanes of a wave with one k: the loads are one address)
__device__ __forceinline__ long long k30_prefix(const int* __restrict__ kc, const u32* __restrict__ tb, int nb, int ncls, long long k, int b)
{
    if (k <= 0) return 0;
    if (k > nb) k = nb;
    const long long t = k / K30_PT;
    long long c = tb[(size_t)t * ncls + b];
    for (long long j = t * K30_PT; j < k; ++j) c += kc[j] == b ? 1 : 0;
    return c;
}

__global__ void __launch_bounds__(64)
k30_pairs(const int* __restrict__ kc, const u32* __restrict__ tb, int nb, int ncls, int lo, int hi, u64* __restrict__ pairs)
{
    __shared__ u64 acc[CL_SAD_CLASSES_MAX * CL_SAD_CLASSES_MAX];
    const int b = threadIdx.x, K = ncls * ncls;
    const long long i0 = (long long)blockIdx.x * K30_PT, i1 = i0 + K30_PT < nb ? i0 + K30_PT : nb;
    if (i0 >= nb || ncls < 1 || ncls > CL_SAD_CLASSES_MAX) return;              // (the whole workgroup)
    for (int e = b; e < K; e += 64) acc[e] = 0ull;
    __syncthreads();
    long long D = 0;                                                            // the bins of class b in [i + lo, min(i + hi, nb))
    if (b < ncls) D = k30_prefix(kc, tb, nb, ncls, i0 + hi, b) - k30_prefix(kc, tb, nb, ncls, i0 + lo, b);
    for (long long i = i0; i < i1; ++i) {
        const int a = kc[i];                                                    // (one address: the same in every lane)
        if (a >= 0 && a < ncls && b < ncls) acc[a * ncls + b] += (u64)D;
        if (i + hi < nb) D += kc[i + hi] == b ? 1 : 0;
        if (i + lo < nb) D -= kc[i + lo] == b ? 1 : 0;
    }
    __syncthreads();
    for (int e = b; e < K; e += 64)
        if (acc[e]) atomicAdd(&pairs[e], acc[e]);
}

__global__ void __launch_bounds__(TPB)
k30_sums(K30In in, int ntiles, int per, double* __restrict__ psum, u32* __restrict__ pcnt)
{
    extern __shared__ __align__(16) unsigned char k30_lds[];                    // K fp64 sums, then K u32 cell counts
    __shared__ double ls[K30_WAVES][64];                                        // per wave the list of a step: sum, key, lanes; its length
    __shared__ int lk[K30_WAVES][64];
    __shared__ u32 lc[K30_WAVES][64];
    __shared__ int ln[K30_WAVES];
    const int K = in.ncls * in.ncls;
    double* tab = (double*)k30_lds;
    u32* tc = (u32*)(tab + K);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < K; e += TPB) { tab[e] = 0.0; tc[e] = 0u; }
    __syncthreads();
    const long long t0 = (long long)blockIdx.x * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
    for (long long t = t0; t < t1; ++t) {
        const long long i = t * K30_TILE + threadIdx.x;
        int key = -1;
        double term = 0.0;
        if (i < in.n) {
            const long long ix = (long long)in.bx[i] - in.b0, d = (long long)in.by[i] - in.bx[i], iy = ix + d;
            if (d >= in.lo && d < in.hi && ix >= 0 && iy < in.nb) {             // (lo >= 1: ix < iy; hi <= nb)
                const int a = in.kc[ix], b = in.kc[iy];
                if (a >= 0 && a < in.ncls && b >= 0 && b < in.ncls) {           // (a class: the bin is valid, its weight a number)
                    key = a * in.ncls + b;
                    term = ((in.ew[ix] * (double)in.cnt[i]) * in.ew[iy]) / in.ex[d];   // (K26's order of operations; the host checked ex[d])
                }
            }
        }
        u64 pend = __ballot(key >= 0);
        int m = 0;
        while (pend) {                                                          // (the same in every lane of the wave)
            const int leader = __ffsll((long long)pend) - 1;
            const int k = __shfl(key, leader);
            const bool mine = key == k;
            const u64 same = __ballot(mine);
            double v = mine ? term : 0.0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0 && m < 64) { ls[wave][m] = v; lk[wave][m] = k; lc[wave][m] = (u32)__popcll(same); }
            ++m;
            pend &= ~same;
        }
        if (lane == 0) ln[wave] = m;
        __syncthreads();
        if (wave == 0) {
            for (int w = 0; w < K30_WAVES; ++w) {
                if (lane < ln[w]) {
                    const int k = lk[w][lane];
                    if (k >= 0 && k < K) { tab[k] += ls[w][lane]; tc[k] += lc[w][lane]; }
                }
            }
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < K; e += TPB) {
        psum[(size_t)blockIdx.x * K + e] = tab[e];
        pcnt[(size_t)blockIdx.x * K + e] = tc[e];
    }
}

// sum[e] / cells[e] = the chunk tables' entries e in chunk order
__global__ void __launch_bounds__(TPB)
k30_fold(const double* __restrict__ psum, const u32* __restrict__ pcnt, int nchunks, int K, double* __restrict__ sum, u64* __restrict__ cells)
{
    const int e = blockIdx.x * TPB + threadIdx.x;
    if (e >= K) return;
    double s = 0.0;
    u64 n = 0ull;
    for (int g = 0; g < nchunks; ++g) { s += psum[(size_t)g * K + e]; n += pcnt[(size_t)g * K + e]; }
    sum[e] = s;
    cells[e] = n;
}

// ---- K30 host side ------------------------------------------------------------------------------
// the checks every K30 call shares; -> CL_OK with c usable
static int sad_enter(cl_chrom* c, const char* who, bool need_sums)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, who, "asynchronous runs still in flight");
    if (!c->bl.st.ready || !c->ex.st.ready || !c->ex.st.expected) return fail(CL_ERR_ARG, who, "no expected values on this handle (cl_exp_set)");
    if (need_sums && !c->sd.st.ready) return fail(CL_ERR_ARG, who, "no tables on this handle (cl_sad_sums)");
    return CL_OK;
}

// the three tables of kc on the stream -> st.sum / pairs / cells (out: K fp64 sums, K u64 pairs, K u64 cells)
static int sad_sums(cl_chrom* c, const std::vector<int>& kc, cl_chrom::Sad::State& st)
{
    const cl_chrom::Bal::State& bl = c->bl.st;
    const int n = (int)bl.n_cells, nb = (int)bl.nb, ncls = st.n_cls, K = ncls * ncls;
    const size_t sK = (size_t)K;
    const int ptiles = (nb + K30_PT - 1) / K30_PT;
    const int ntiles = (int)(((long long)n + K30_TILE - 1) / K30_TILE);
    const int per = std::max(1, (ntiles + K30_CHUNKS - 1) / K30_CHUNKS), nchunks = (ntiles + per - 1) / per;
    int rc;
    if ((rc = c->sd.cls.ensure((size_t)nb * 4)) || (rc = c->sd.th.ensure((size_t)ptiles * ncls * 4)) ||
        (rc = c->sd.tb.ensure(((size_t)ptiles + 1) * ncls * 4)) || (rc = c->sd.part.ensure(std::max<size_t>((size_t)nchunks * sK * 12, 16))) ||
        (rc = c->sd.out.ensure(sK * 24))) return rc;
    double* d_sum = c->sd.out.as<double>();
    u64 *d_pairs = (u64*)(d_sum + sK), *d_cells = d_pairs + sK;
    const int* d_kc = c->sd.cls.as<int>();
    HIP_TRY(hipMemcpyAsync(c->sd.cls.p, kc.data(), (size_t)nb * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->sd.out.p, 0, sK * 24, c->stream));
    if (st.hi > st.lo) {
        hipLaunchKernelGGL(k30_hist, dim3((unsigned)ptiles), dim3(64), 0, c->stream, d_kc, nb, ncls, c->sd.th.as<u32>());
        hipLaunchKernelGGL(k30_scan, dim3(1), dim3(64), 0, c->stream, (const u32*)c->sd.th.as<u32>(), ptiles, ncls, c->sd.tb.as<u32>());
        hipLaunchKernelGGL(k30_pairs, dim3((unsigned)ptiles), dim3(64), 0, c->stream, d_kc, (const u32*)c->sd.tb.as<u32>(), nb, ncls, (int)st.lo,
                           (int)st.hi, d_pairs);
        HIP_TRY(hipGetLastError());
        if (nchunks > 0) {
            K30In in{c->mx.bx.as<int>(), c->mx.by.as<int>(), c->mx.cnt.as<u32>(), c->ex.w.as<double>(), c->ex.exp.as<double>(), d_kc,
                     n, (int)bl.b0, nb, ncls, (int)st.lo, (int)st.hi};
            double* psum = c->sd.part.as<double>();
            u32* pcnt = (u32*)(psum + (size_t)nchunks * sK);
            hipLaunchKernelGGL(k30_sums, dim3((unsigned)nchunks), dim3(TPB), sK * 12, c->stream, in, ntiles, per, psum, pcnt);
            HIP_TRY(hipGetLastError());
            LAUNCH(k30_fold, K, (const double*)psum, (const u32*)pcnt, nchunks, K, d_sum, d_cells);
            HIP_TRY(hipGetLastError());
        }
    }
    st.sum.assign(sK, 0.0); st.pairs.assign(sK, 0); st.cells.assign(sK, 0);
    if ((rc = read_back(c, "cl_sad_sums", {{st.sum.data(), d_sum, sK * 8}, {st.pairs.data(), d_pairs, sK * 8}, {st.cells.data(), d_cells, sK * 8}})))
        return rc;
    for (size_t e = 0; e < sK; ++e) { st.n_pairs += st.pairs[e]; st.n_in += st.cells[e]; }
    return CL_OK;
}

extern "C" int cl_sad_sums(cl_chrom* c, const int32_t* cls, int64_t count, int32_t n_cls, int64_t lo, int64_t hi, int64_t* n_binned,
                           int64_t* n_pairs, int64_t* n_in)
{
    if (n_binned) *n_binned = 0;
    if (n_pairs) *n_pairs = 0;
    if (n_in) *n_in = 0;
    int rc = sad_enter(c, "cl_sad_sums", false);
    if (rc != CL_OK) return rc;
    if (!n_binned || !n_pairs || !n_in) return fail(CL_ERR_ARG, "cl_sad_sums: bad arguments");
    if (n_cls < 1 || n_cls > CL_SAD_CLASSES_MAX) return fail(CL_ERR_ARG, "cl_sad_sums: n_cls outside [1, CL_SAD_CLASSES_MAX]");
    const cl_chrom::Bal::State& bl = c->bl.st;
    if (count != bl.nb) return fail(CL_ERR_ARG, "cl_sad_sums: count is not the number of bins");
    if (count > 0 && !cls) return fail(CL_ERR_ARG, "cl_sad_sums: bad arguments");
    const long long near = std::max<long long>(bl.ignore_diags, 1);
    if (bl.nb == 0 ? (lo != 0 || hi != 0) : (lo < near || lo > hi || hi > bl.nb))
        return fail(CL_ERR_ARG, "cl_sad_sums: the band must hold max(ignore_diags, 1) <= lo <= hi <= nb (lo = hi = 0 without bins)");
    for (int64_t i = 0; i < count; ++i)
        if (cls[i] < -1 || cls[i] >= n_cls) return fail(CL_ERR_ARG, "cl_sad_sums: a class outside [-1, n_cls)");
    cl_chrom::Sad::State st;
    st.ready = true; st.n_cls = n_cls; st.lo = lo; st.hi = hi;
    const size_t sK = (size_t)n_cls * (size_t)n_cls;
    if (bl.nb == 0) {                                                           // (no bins: no band, no HIP call)
        st.sum.assign(sK, 0.0); st.pairs.assign(sK, 0); st.cells.assign(sK, 0);
        sad_release(c); c->sd.st = st;
        return CL_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    // the host's look at K26's state: the valid bins, and the expected values of the band's diagonals that hold a valid pair
    const size_t snb = (size_t)bl.nb;
    std::vector<double> ew(snb), ex(snb);
    std::vector<long long> pairs(snb);
    if ((rc = read_back(c, "cl_sad_sums", {{ew.data(), c->ex.w.p, snb * 8}, {ex.data(), c->ex.exp.p, snb * 8}, {pairs.data(), c->ex.pairs.p, snb * 8}})))
        return rc;
    for (long long d = lo; d < hi; ++d)
        if (pairs[(size_t)d] > 0 && !(ex[(size_t)d] > 0.0 && std::isfinite(ex[(size_t)d])))
            return fail(CL_ERR_ARG, "cl_sad_sums: a diagonal of the band has valid pairs and no finite positive expected value (lower hi)");
    std::vector<int> kc(snb);
    for (size_t i = 0; i < snb; ++i) {
        kc[i] = ew[i] == ew[i] ? cls[i] : -1;
        st.n_binned += kc[i] >= 0 ? 1 : 0;
    }
    c->sd.st = cl_chrom::Sad::State();                                          // (the earlier state's buffers are written from here on)
    rc = sad_sums(c, kc, st);
    if (rc != CL_OK) {
        (void)hipStreamSynchronize(c->stream);
        sad_release(c);
        return rc;
    }
    c->sd.st = st;
    *n_binned = st.n_binned; *n_pairs = st.n_pairs; *n_in = st.n_in;
    return CL_OK;
}

extern "C" int cl_sad_get(cl_chrom* c, double* sum, int64_t* pairs, int64_t* cells)
{
    int rc = sad_enter(c, "cl_sad_get", true);
    if (rc != CL_OK) return rc;
    if (!sum || !pairs || !cells) return fail(CL_ERR_ARG, "cl_sad_get: bad arguments");
    const cl_chrom::Sad::State& st = c->sd.st;
    for (size_t e = 0; e < st.sum.size(); ++e) { sum[e] = st.sum[e]; pairs[e] = st.pairs[e]; cells[e] = st.cells[e]; }
    return CL_OK;
}

extern "C" int cl_sad_free(cl_chrom* c) { return unit_free(c, "cl_sad_free", sad_release); }
