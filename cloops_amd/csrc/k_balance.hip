// k_balance.hip -- K25: matrix balancing (iterative correction, ICE) of the folded cells that K24 left on the device -- kernels and C
// entry points.
#include <cmath>
#include "cl_segsum.h"

// ==========================================================================================
// K25: one weight per bin so that the rows of the weighted contact matrix have equal sums
// ==========================================================================================
// Definitions: include/cloops_hip.h, cl_bal_marginals.  The reference has nothing of the kind; tests/balance_cases.py restates the
// definitions in numpy.  Input: K24's cells (c->mx.bx, c->mx.by, c->mx.cnt: ascending by (bx, by), bx <= by).
// A marginal of bin i has a row part (the cells with bx == i: a run of the cells as they lie) and a column part (the cells with by ==
// i and bx != i: a run of the cells sorted by (by, bx), the transposed order that cl_bal_marginals builds once with one rocPRIM radix
// sort of (key, cell index) pairs over the bits in use and one gather).  Both are sums over runs of equal sorted keys:
//   k25_marg<V>, k25_fold<V>   the segmented sums over the runs of one order and the fold of the tiles' carry records: cl_segsum.h
//                   (shared with K26, k_expected.hip).
//                   V = K25I (sum as u64 and nnz as u32: the raw marginals) or K25D (fp64: (w[bx] cnt) w[by], the iteration's s).
//   k25_stat1       s[i] = row part + column part (and both parts back to zero for the next pass); count and sum of the s != 0: a
//                   fixed share of the bins per thread in ascending order, a fixed tree over the workgroup -> one partial per workgroup.
//   k25_stat2       every workgroup folds the partials in index order to the mean, then w[i] /= s[i] / mean and the partial sums of
//                   (s / mean - 1)^2 the same way.
//   k25_stat3       one workgroup: folds those to var, counts the iteration and sets `stop` in the loop's record when var < tol (or
//                   when no s differs from zero).  Every kernel of the loop begins by reading `stop` and returns at once when it is set:
//                   the host enqueues K25_BLOCK iterations at a time and reads the 32-byte record after each block.
// Every fp64 sum is taken in an order that depends on the cells and nb alone: two runs give the same bytes.  No fp64 atomics, no
// workgroup waits on another, plain launches in the handle's stream.  Only vector stores and integer HIP atomics (the count of used
// cells); every index is checked against its array before a load or store.
#define K25_PARTS 1024                  // most workgroups (= partial sums) of k25_stat1 / k25_stat2
#define K25_BLOCK 16                    // iterations enqueued between two reads of the record
static_assert(CL_BAL_BINS_MAX == (1 << 24), "the limit of include/cloops_hip.h");

struct K25I {                           // the integer pass
    u64 s; u32 n;
    struct Out { u64* s; u32* n; };
    struct Ctx { int ign; };
    __device__ __forceinline__ static K25I zero() { return K25I{0ull, 0u}; }
    __device__ __forceinline__ static K25I add(const K25I& a, const K25I& b) { return K25I{a.s + b.s, a.n + b.n}; }
    __device__ __forceinline__ static K25I up(const K25I& a, int d)
    {
        K25I r;
        r.s = (u64)__shfl_up((unsigned long long)a.s, (unsigned)d);
        r.n = (u32)__shfl_up((int)a.n, (unsigned)d);
        return r;
    }
    __device__ __forceinline__ static void store(const Out& o, size_t i, const K25I& v) { o.s[i] = v.s; o.n[i] = v.n; }
};
struct K25D {                           // the fp64 pass
    double s;
    struct Out { double* s; };
    __device__ __forceinline__ static K25D zero() { return K25D{0.0}; }
    __device__ __forceinline__ static K25D add(const K25D& a, const K25D& b) { return K25D{a.s + b.s}; }
    __device__ __forceinline__ static K25D up(const K25D& a, int d) { return K25D{__shfl_up(a.s, (unsigned)d)}; }
    __device__ __forceinline__ static void store(const Out& o, size_t i, const K25D& v) { o.s[i] = v.s; }
};
// what a cell adds to the run of `k` (o: its other bin)
__device__ __forceinline__ K25I k25_term(const K25In& in, int ph, int k, int o, u32 c, K25I*)
{
    const int d = ph ? k - o : o - k;                                           // by - bx >= 0
    return (d >= in.ign && !(ph && d == 0)) ? K25I{(u64)c, 1u} : K25I::zero();
}
__device__ __forceinline__ K25D k25_term(const K25In& in, int ph, int k, int o, u32 c, K25D*)
{
    const int d = ph ? k - o : o - k;
    const long long ix = (long long)(ph ? o : k) - in.b0, iy = (long long)(ph ? k : o) - in.b0;
    if (d < in.ign || (ph && d == 0) || ix < 0 || ix >= in.nb || iy < 0 || iy >= in.nb) return K25D::zero();
    return K25D{(in.w[ix] * (double)c) * in.w[iy]};
}

// tby / tbx / tcnt[i] = by / bx / cnt of cell order[i]
__global__ void __launch_bounds__(TPB)
k25_keys(const int* __restrict__ bx, const int* __restrict__ by, int n, int b0, int bits, u64* __restrict__ key, u32* __restrict__ val)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    key[i] = ((u64)(u32)(by[i] - b0) << bits) | (u64)(u32)(bx[i] - b0);         // b0 <= bx <= by
    val[i] = (u32)i;
}

__global__ void __launch_bounds__(TPB)
k25_gather(const u32* __restrict__ order, const int* __restrict__ bx, const int* __restrict__ by, const u32* __restrict__ cnt, int n,
           int* __restrict__ tbx, int* __restrict__ tby, u32* __restrict__ tcnt)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const u32 j = order[i];
    if (j >= (u32)n) return;
    tbx[i] = bx[j]; tby[i] = by[j]; tcnt[i] = cnt[j];
}

// sum / nnz = row part + column part
__global__ void __launch_bounds__(TPB)
k25_join(const u64* __restrict__ ps, const u32* __restrict__ pn, int nb, u64* __restrict__ sum, u32* __restrict__ nnz)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= nb) return;
    sum[i] = ps[i] + ps[(size_t)nb + i];
    nnz[i] = pn[i] + pn[(size_t)nb + i];
}

__global__ void __launch_bounds__(TPB)
k25_init(const u32* __restrict__ valid, int nb, double* __restrict__ w, double* __restrict__ parts2, K25Rec* __restrict__ rec, double nan)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i == 0) { rec->iters = 0; rec->converged = 0; rec->stop = 0; rec->pad = 0; rec->var = nan; rec->scale = nan; }
    if (i >= nb) return;
    w[i] = valid[i] ? 1.0 : 0.0;
    parts2[i] = 0.0; parts2[(size_t)nb + i] = 0.0;
}

// sum of (a, b) over the workgroup in a fixed tree; the result in thread 0
__device__ __forceinline__ void k25_wg_sum(double& a, double& b, double* la, double* lb)
{
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, (unsigned)o); b += __shfl_down(b, (unsigned)o); }
    if ((threadIdx.x & 63) == 0) { la[threadIdx.x >> 6] = a; lb[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) { a = la[0]; b = lb[0]; for (int q = 1; q < TPB / 64; ++q) { a += la[q]; b += lb[q]; } }
    __syncthreads();
}

// the bins of workgroup g: [g per, min((g + 1) per, nb)), per a multiple of TPB; thread t takes them at stride TPB, ascending
__global__ void __launch_bounds__(TPB)
k25_stat1(double* __restrict__ parts2, int nb, int per, double* __restrict__ s, double* __restrict__ pcnt, double* __restrict__ psum,
          const K25Rec* __restrict__ rec)
{
    __shared__ double la[TPB / 64], lb[TPB / 64];
    if (rec->stop) return;
    const long long lo = (long long)blockIdx.x * per, hi = lo + per < nb ? lo + per : nb;
    double n = 0.0, t = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += TPB) {
        const double v = parts2[i] + parts2[(size_t)nb + i];
        parts2[i] = 0.0; parts2[(size_t)nb + i] = 0.0;
        s[i] = v;
        if (v != 0.0) { n += 1.0; t += v; }
    }
    k25_wg_sum(n, t, la, lb);
    if (threadIdx.x == 0) { pcnt[blockIdx.x] = n; psum[blockIdx.x] = t; }
}

// the partials p[0 .. np) folded in index order by the workgroup: thread t takes p[t], p[t + TPB], ..; then the tree
__device__ __forceinline__ void k25_fold_parts(const double* __restrict__ pa, const double* __restrict__ pb, int np, double& a, double& b,
                                               double* la, double* lb)
{
    a = 0.0; b = 0.0;
    for (int q = threadIdx.x; q < np; q += TPB) { a += pa[q]; b += pb[q]; }
    k25_wg_sum(a, b, la, lb);
}

__global__ void __launch_bounds__(TPB)
k25_stat2(const double* __restrict__ s, int nb, int per, int np, const double* __restrict__ pcnt, const double* __restrict__ psum,
          double* __restrict__ w, double* __restrict__ pvar, const K25Rec* __restrict__ rec)
{
    __shared__ double la[TPB / 64], lb[TPB / 64];
    __shared__ double l_mean;
    if (rec->stop) return;
    double n, t;
    k25_fold_parts(pcnt, psum, np, n, t, la, lb);
    if (threadIdx.x == 0) l_mean = n > 0.0 ? t / n : 0.0;
    __syncthreads();
    const double mean = l_mean;
    double dv = 0.0, unused = 0.0;
    if (mean != 0.0) {                                                          // (n == 0: no bin to update; k25_stat3 ends the loop)
        const long long lo = (long long)blockIdx.x * per, hi = lo + per < nb ? lo + per : nb;
        for (long long i = lo + threadIdx.x; i < hi; i += TPB) {
            const double v = s[i];
            if (v == 0.0) continue;
            const double q = v / mean;
            w[i] = w[i] / q;
            dv += (q - 1.0) * (q - 1.0);
        }
    }
    k25_wg_sum(dv, unused, la, lb);
    if (threadIdx.x == 0) pvar[blockIdx.x] = dv;
}

__global__ void __launch_bounds__(TPB)
k25_stat3(int np, const double* __restrict__ pcnt, const double* __restrict__ psum, const double* __restrict__ pvar, double tol,
          K25Rec* __restrict__ rec)
{
    __shared__ double la[TPB / 64], lb[TPB / 64];
    if (rec->stop) return;
    double n, t, dv, unused;
    k25_fold_parts(pcnt, psum, np, n, t, la, lb);
    k25_fold_parts(pvar, pvar, np, dv, unused, la, lb);
    if (threadIdx.x != 0) return;
    if (!(n > 0.0)) { rec->stop = 1; return; }                                  // no s differs from zero: the record stays as k25_init left it
    const double var = dv / n;
    rec->iters += 1;
    rec->var = var;
    rec->scale = t / n;
    if (var < tol) { rec->converged = 1; rec->stop = 1; }
}

// weight[i] = w[i] / root where w[i] > 0 (root = sqrt(scale), taken on the host), NaN elsewhere
__global__ void __launch_bounds__(TPB)
k25_weights(const double* __restrict__ w, int nb, double root, double nan, double* __restrict__ weight)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= nb) return;
    const double v = w[i];
    weight[i] = v > 0.0 ? v / root : nan;
}

__global__ void __launch_bounds__(TPB)
k25_cells(const int* __restrict__ bx, const int* __restrict__ by, const u32* __restrict__ cnt, long long first, long long count, long long n,
          int b0, int nb, const double* __restrict__ weight, double nan, double* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= count || first + i >= n) return;
    const long long ix = (long long)bx[first + i] - b0, iy = (long long)by[first + i] - b0;
    out[i] = (ix < 0 || ix >= nb || iy < 0 || iy >= nb) ? nan : ((double)cnt[first + i] * weight[ix]) * weight[iy];
}

// ---- K25 host side ------------------------------------------------------------------------------
static long long k25_floordiv(long long p, long long res)
{
    const long long q = p / res;
    return q - ((p - q * res) < 0 ? 1 : 0);
}

static K25In k25_input(cl_chrom* c, const cl_chrom::Bal::State& st)
{
    K25In in{};
    in.key[0] = c->mx.bx.as<int>(); in.oth[0] = c->mx.by.as<int>(); in.cnt[0] = c->mx.cnt.as<u32>();
    in.key[1] = c->bl.tby.as<int>(); in.oth[1] = c->bl.tbx.as<int>(); in.cnt[1] = c->bl.tcnt.as<u32>();
    in.n = (int)st.n_cells; in.ign = st.ignore_diags; in.b0 = (int)st.b0; in.nb = (int)st.nb;
    in.w = nullptr;
    in.vec = 1;
    for (int ph = 0; ph < 2; ++ph)
        for (const void* p : {(const void*)in.key[ph], (const void*)in.oth[ph], (const void*)in.cnt[ph]}) if ((uintptr_t)p % 16) in.vec = 0;
    return in;
}

// workgroups of k25_stat1 / k25_stat2 over nb bins and the bins of each (a multiple of TPB)
static void k25_parts(long long nb, int& np, int& per)
{
    long long p = (nb + K25_PARTS - 1) / K25_PARTS;
    p = (p + TPB - 1) / TPB * TPB;
    per = (int)std::max<long long>(p, TPB);
    np = (int)std::max<long long>((nb + per - 1) / per, 1);
}

static int bal_marginals(cl_chrom* c, cl_chrom::Bal::State& st)
{
    const int n = (int)st.n_cells;
    const size_t sn = (size_t)n;
    int rc;
    int hb0 = 0;
    HIP_TRY(hipMemcpyAsync(&hb0, c->mx.bx.as<int>(), 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // the bins of all rows of the handle bound those of the cells (as in cl_mat_cells): by - b0 fits the key's bits
    const long long bmax = k25_floordiv(std::max(c->st.xmax, c->st.ymax), c->mx.st.res);
    if (bmax < hb0 || bmax - hb0 >= (1ll << 30)) return fail(CL_ERR_HIP, "cl_bal_marginals: the cells' bins are not ones this handle can have");
    const int bits = std::max(1, bits_for((unsigned)(bmax - hb0)));
    if ((rc = c->bl.kin.ensure(sn * 8)) || (rc = c->bl.kout.ensure(sn * 8)) || (rc = c->bl.vin.ensure(sn * 4)) || (rc = c->bl.vout.ensure(sn * 4)) ||
        (rc = c->bl.tby.ensure(sn * 4)) || (rc = c->bl.tbx.ensure(sn * 4)) || (rc = c->bl.tcnt.ensure(sn * 4)) || (rc = c->bl.rec.ensure(64))) return rc;
    LAUNCH(k25_keys, n, c->mx.bx.as<int>(), c->mx.by.as<int>(), n, hb0, bits, c->bl.kin.as<u64>(), c->bl.vin.as<u32>());
    HIP_TRY(hipGetLastError());
    if ((rc = prim_run(c->bl.tmp, "radix_sort_pairs(balance)", [&](void* tmp, size_t& bytes) {
            return rocprim::radix_sort_pairs(tmp, bytes, c->bl.kin.as<u64>(), c->bl.kout.as<u64>(), c->bl.vin.as<u32>(), c->bl.vout.as<u32>(), sn, 0,
                                             2 * bits, c->stream);
        })))
        return rc;
    LAUNCH(k25_gather, n, c->bl.vout.as<u32>(), c->mx.bx.as<int>(), c->mx.by.as<int>(), c->mx.cnt.as<u32>(), n, c->bl.tbx.as<int>(),
           c->bl.tby.as<int>(), c->bl.tcnt.as<u32>());
    HIP_TRY(hipGetLastError());
    int hb1 = 0;
    HIP_TRY(hipMemcpyAsync(&hb1, c->bl.tby.as<int>() + (sn - 1), 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (hb1 < hb0 || (long long)hb1 > bmax) return fail(CL_ERR_HIP, "cl_bal_marginals: the transposed order ends with a bin no cell can have");
    st.b0 = hb0; st.nb = (long long)hb1 - hb0 + 1;
    if (st.nb > CL_BAL_BINS_MAX) return fail(CL_ERR_ARG, "cl_bal_marginals: more than CL_BAL_BINS_MAX bins (use a coarser res)");
    const size_t snb = (size_t)st.nb;
    const int ntiles = (int)((sn + K25_TILE - 1) / K25_TILE);
    // bl.out serves as the two integer parts here (sum: 2 nb u64, then nnz: 2 nb u32); later as the balanced values of a get
    if ((rc = c->bl.out.ensure(snb * 24)) || (rc = c->bl.sum.ensure(snb * 8)) || (rc = c->bl.nnz.ensure(snb * 4)) ||
        (rc = c->bl.icar.ensure((size_t)ntiles * 2 * sizeof(K25Car<K25I>)))) return rc;
    HIP_TRY(hipMemsetAsync(c->bl.out.p, 0, snb * 24, c->stream));
    HIP_TRY(hipMemsetAsync(c->bl.rec.p, 0, 64, c->stream));
    u64* d_used = c->bl.rec.as<u64>() + 4;                                      // (behind the loop's record)
    K25I::Out out{c->bl.out.as<u64>(), (u32*)(c->bl.out.as<u64>() + 2 * snb)};
    const K25In in = k25_input(c, st);
    hipLaunchKernelGGL(k25_marg<K25I>, dim3((unsigned)ntiles, 2u), dim3(TPB), 0, c->stream, in, out, c->bl.icar.as<K25Car<K25I>>(), ntiles, d_used,
                       (const K25Rec*)nullptr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k25_fold<K25I>, dim3((unsigned)nblocks(ntiles), 2u), dim3(TPB), 0, c->stream, (const K25Car<K25I>*)c->bl.icar.as<K25Car<K25I>>(),
                       ntiles, in.b0, in.nb, out, (const K25Rec*)nullptr);
    HIP_TRY(hipGetLastError());
    LAUNCH(k25_join, st.nb, (const u64*)out.s, (const u32*)out.n, in.nb, c->bl.sum.as<u64>(), c->bl.nnz.as<u32>());
    HIP_TRY(hipGetLastError());
    u64 hu = 0;
    HIP_TRY(hipMemcpyAsync(&hu, d_used, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    st.n_used = (long long)hu;
    return CL_OK;
}

// the checks every K25 call shares; -> CL_OK with c usable
static int bal_enter(cl_chrom* c, const char* who, bool need_marginals)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, who, "asynchronous runs still in flight");
    if (!c->mx.st.ready) return fail(CL_ERR_ARG, who, "no cells on this handle (cl_mat_cells)");
    if (!c->mx.st.fold) return fail(CL_ERR_ARG, who, "the cells are not folded (cl_mat_cells with fold = 1)");
    if (need_marginals && !c->bl.st.ready) return fail(CL_ERR_ARG, who, "no marginals on this handle (cl_bal_marginals)");
    return CL_OK;
}

extern "C" int cl_bal_marginals(cl_chrom* c, int32_t ignore_diags, int64_t* b0, int64_t* nb, int64_t* n_used)
{
    if (b0) *b0 = 0;
    if (nb) *nb = 0;
    if (n_used) *n_used = 0;
    int rc = bal_enter(c, "cl_bal_marginals", false);
    if (rc != CL_OK) return rc;
    if (!b0 || !nb || !n_used) return fail(CL_ERR_ARG, "cl_bal_marginals: bad arguments");
    if (ignore_diags < 0) return fail(CL_ERR_ARG, "cl_bal_marginals: ignore_diags below 0");
    cl_chrom::Bal::State st;
    st.ready = true;
    st.ignore_diags = ignore_diags;
    st.n_cells = c->mx.st.n_cells;
    if (st.n_cells == 0) { bal_release(c); c->bl.st = st; return CL_OK; }          // (no rows, or a cut that keeps none: no HIP call)
    HIP_TRY(hipSetDevice(c->device));
    exp_release(c);                                                             // (every K26 call ends synchronised)
    c->bl.st.ready = false; c->bl.st.iterated = false;                                // (the earlier state's buffers are written from here on)
    rc = bal_marginals(c, st);
    if (rc != CL_OK) {
        (void)hipStreamSynchronize(c->stream);
        bal_release(c);
        return rc;
    }
    c->bl.st = st;
    *b0 = st.b0; *nb = st.nb; *n_used = st.n_used;
    return CL_OK;
}

extern "C" int cl_bal_marginals_get(cl_chrom* c, int64_t first, int64_t count, uint64_t* sum, uint32_t* nnz)
{
    int rc = bal_enter(c, "cl_bal_marginals_get", true);
    if (rc != CL_OK) return rc;
    if (!range_ok(first, count, c->bl.st.nb)) return fail(CL_ERR_ARG, "cl_bal_marginals_get: range outside the bins");
    if (count > 0 && (!sum || !nnz)) return fail(CL_ERR_ARG, "cl_bal_marginals_get: bad arguments");
    if (count == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    return read_back(c, "cl_bal_marginals_get", {{sum, c->bl.sum.as<u64>() + first, (size_t)count * 8},
                                                 {nnz, c->bl.nnz.as<u32>() + first, (size_t)count * 4}});
}

static int bal_iterate(cl_chrom* c, const uint32_t* valid, int max_iters, double tol, K25Rec& h)
{
    const cl_chrom::Bal::State& st = c->bl.st;
    const size_t snb = (size_t)st.nb;
    const int ntiles = (int)(((size_t)st.n_cells + K25_TILE - 1) / K25_TILE);
    int np, per, rc;
    k25_parts(st.nb, np, per);
    // bl.w: w, then the weights; bl.s: the two parts of s, then s; bl.part: count, sum and var partials
    if ((rc = c->bl.valid.ensure(snb * 4)) || (rc = c->bl.w.ensure(snb * 16)) || (rc = c->bl.s.ensure(snb * 24)) ||
        (rc = c->bl.part.ensure((size_t)np * 24)) || (rc = c->bl.dcar.ensure((size_t)ntiles * 2 * sizeof(K25Car<K25D>))) ||
        (rc = c->bl.rec.ensure(64))) return rc;
    const double nan = std::nan("");
    double *w = c->bl.w.as<double>(), *weight = w + snb, *parts2 = c->bl.s.as<double>(), *s = parts2 + 2 * snb;
    double *pcnt = c->bl.part.as<double>(), *psum = pcnt + np, *pvar = psum + np;
    K25Rec* rec = c->bl.rec.as<K25Rec>();
    HIP_TRY(hipMemcpyAsync(c->bl.valid.p, valid, snb * 4, hipMemcpyHostToDevice, c->stream));
    LAUNCH(k25_init, st.nb, (const u32*)c->bl.valid.as<u32>(), (int)st.nb, w, parts2, rec, nan);
    HIP_TRY(hipGetLastError());
    K25In in = k25_input(c, st);
    in.w = w;
    K25D::Out out{parts2};
    K25Car<K25D>* car = c->bl.dcar.as<K25Car<K25D>>();
    h = K25Rec{0, 0, 0, 0, nan, nan};
    for (int done = 0; done < max_iters && !h.stop;) {
        const int blk = std::min(K25_BLOCK, max_iters - done);
        for (int k = 0; k < blk; ++k) {
            hipLaunchKernelGGL(k25_marg<K25D>, dim3((unsigned)ntiles, 2u), dim3(TPB), 0, c->stream, in, out, car, ntiles, (u64*)nullptr, (const K25Rec*)rec);
            hipLaunchKernelGGL(k25_fold<K25D>, dim3((unsigned)nblocks(ntiles), 2u), dim3(TPB), 0, c->stream, (const K25Car<K25D>*)car, ntiles, in.b0, in.nb,
                               out, (const K25Rec*)rec);
            hipLaunchKernelGGL(k25_stat1, dim3((unsigned)np), dim3(TPB), 0, c->stream, parts2, in.nb, per, s, pcnt, psum, (const K25Rec*)rec);
            hipLaunchKernelGGL(k25_stat2, dim3((unsigned)np), dim3(TPB), 0, c->stream, (const double*)s, in.nb, per, np, (const double*)pcnt,
                               (const double*)psum, w, pvar, (const K25Rec*)rec);
            hipLaunchKernelGGL(k25_stat3, dim3(1), dim3(TPB), 0, c->stream, np, (const double*)pcnt, (const double*)psum, (const double*)pvar, tol, rec);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(&h, rec, sizeof(K25Rec), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        done += blk;
        if (h.iters < 0 || h.iters > done) return fail(CL_ERR_HIP, "cl_bal_iterate: the record holds a count no loop can have");
    }
    const double root = std::sqrt(h.scale);                                     // (NaN when nothing was iterated: every weight NaN)
    LAUNCH(k25_weights, st.nb, (const double*)w, (int)st.nb, root, nan, weight);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CL_OK;
}

extern "C" int cl_bal_iterate(cl_chrom* c, const uint32_t* valid, int32_t max_iters, double tol, int32_t* iters, int32_t* converged,
                              double* var, double* scale)
{
    const double nan = std::nan("");
    if (iters) *iters = 0;
    if (converged) *converged = 0;
    if (var) *var = nan;
    if (scale) *scale = nan;
    int rc = bal_enter(c, "cl_bal_iterate", true);
    if (rc != CL_OK) return rc;
    if (!iters || !converged || !var || !scale) return fail(CL_ERR_ARG, "cl_bal_iterate: bad arguments");
    if (max_iters < 0) return fail(CL_ERR_ARG, "cl_bal_iterate: max_iters below 0");
    if (!(tol >= 0.0)) return fail(CL_ERR_ARG, "cl_bal_iterate: tol below 0 or not a number");
    if (c->bl.st.nb > 0 && !valid) return fail(CL_ERR_ARG, "cl_bal_iterate: no mask");
    exp_release(c);                                                             // (K26's diagonals were those of the earlier weights)
    if (c->bl.st.nb == 0) { c->bl.st.iterated = true; return CL_OK; }
    HIP_TRY(hipSetDevice(c->device));
    c->bl.st.iterated = false;
    K25Rec h{};
    rc = bal_iterate(c, valid, max_iters, tol, h);
    if (rc != CL_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    c->bl.st.iterated = true;
    *iters = h.iters; *converged = h.converged; *var = h.var; *scale = h.scale;
    return CL_OK;
}

extern "C" int cl_bal_weights_get(cl_chrom* c, int64_t first, int64_t count, double* weight)
{
    int rc = bal_enter(c, "cl_bal_weights_get", true);
    if (rc != CL_OK) return rc;
    if (!c->bl.st.iterated) return fail(CL_ERR_ARG, "cl_bal_weights_get: no weights on this handle (cl_bal_iterate)");
    if (!range_ok(first, count, c->bl.st.nb)) return fail(CL_ERR_ARG, "cl_bal_weights_get: range outside the bins");
    if (count > 0 && !weight) return fail(CL_ERR_ARG, "cl_bal_weights_get: bad arguments");
    if (count == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    return read_back(c, "cl_bal_weights_get", {{weight, c->bl.w.as<double>() + (size_t)c->bl.st.nb + first, (size_t)count * 8}});
}

extern "C" int cl_bal_cells_get(cl_chrom* c, int64_t first, int64_t count, double* balanced)
{
    int rc = bal_enter(c, "cl_bal_cells_get", true);
    if (rc != CL_OK) return rc;
    if (!c->bl.st.iterated) return fail(CL_ERR_ARG, "cl_bal_cells_get: no weights on this handle (cl_bal_iterate)");
    if (!range_ok(first, count, c->bl.st.n_cells)) return fail(CL_ERR_ARG, "cl_bal_cells_get: range outside the cells");
    if (count > 0 && !balanced) return fail(CL_ERR_ARG, "cl_bal_cells_get: bad arguments");
    if (count == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->bl.out.ensure((size_t)count * 8))) return rc;
    LAUNCH(k25_cells, count, c->mx.bx.as<int>(), c->mx.by.as<int>(), c->mx.cnt.as<u32>(), (long long)first, (long long)count, c->bl.st.n_cells,
           (int)c->bl.st.b0, (int)c->bl.st.nb, (const double*)(c->bl.w.as<double>() + (size_t)c->bl.st.nb), std::nan(""), c->bl.out.as<double>());
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(CL_ERR_HIP, "cl_bal_cells_get", hipGetErrorString(e));
    return read_back(c, "cl_bal_cells_get", {{balanced, c->bl.out.p, (size_t)count * 8}});
}

extern "C" int cl_bal_free(cl_chrom* c)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_bal_free: asynchronous runs still in flight");
    if (c->n > 0) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    bal_release(c);
    return CL_OK;
}
