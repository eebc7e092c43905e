// k_expected.hip -- K26: expected contacts by distance and observed / expected of the folded cells that K24 left on the device and K25
// weighted -- kernels and C entry points.
#include <cmath>
#include "cl_segsum.h"

// ==========================================================================================
// K26: per diagonal the valid bin pairs, the count sum and the (balanced) value sum; O/E of every cell
// ==========================================================================================
// Definitions: include/cloops_hip.h, cl_exp_diagonals.  The reference has nothing of the kind; tests/expected_cases.py restates the
// definitions in numpy.  Input: K24's cells (c->mx.bx, c->mx.by, c->mx.cnt), K25's bins b0 .. b0 + nb - 1 and ignore_diags, and either
// K25's weights (balanced) or the caller's mask (raw).  One array drives everything that follows: ew[i], the effective weight of bin
// i -- the ICE weight, or 1 on a valid bin of the raw mode, NaN on every other bin.  A bin is valid iff ew[i] is a number; a cell is
// used iff by - bx >= ignore_diags and both of its bins are valid; its value is (ew[bx] cnt) ew[by].
//   k26_mask        ew, and the mask packed to one bit per bin: one __ballot per 64 bins (the bits behind nb are zero).
//   k26_pairs       n_pairs[d] = sum over the mask words j of popcount(m[j] & (m >> d)[j]): the autocorrelation of the mask.  A
//                   workgroup owns K26_DB = 256 consecutive diagonals, one per thread: the 64 diagonals of a wave share the word
//                   offset d / 64 and differ in the bit shift d % 64 = the lane, so every LDS read of the loop is one address per
//                   wave (a broadcast).  The words come through LDS windows of K26_WIN words: m[J .. J + WIN) once, and per wave the
//                   WIN + 1 words from J + d / 64 that it shifts (word j of m >> d is a funnel of the words j + d / 64 and
//                   j + d / 64 + 1), laid out so that the loop reads 16 bytes at a time.  A word index is checked against the mask's
//                   length before its load; what lies behind the mask reads as zero.  One plain store per diagonal.  The work is
//                   nb^2 / 128 word operations (the words with a partner: half of nb^2 / 64).
//   k26_keys / k26_gather   the diagonal order: (d, cell index) pairs through one rocPRIM radix sort over the bits of nb - 1 (stable:
//                   inside a diagonal the cells keep their ascending (bx, by) order), then d, bx - b0 and cnt of every cell in that
//                   order; the used cells are counted on the way (integer atomics, one per workgroup).
//   k25_marg<K26V> / k25_fold<K26V>   the sums over the runs of equal d (cl_segsum.h, K25's tile scan and carry fold): count sum
//                   (u64) and value sum (fp64) of a diagonal in one pass.  The order of the fp64 additions depends on the cells and nb
//                   alone: two runs give the same bytes.  No fp64 atomics.
//   k26_oe          O/E of the cells [first, first + count) as they lie: one gather of expected[by - bx], the multiply chain and one
//                   divide per cell.
// Only vector stores and integer HIP atomics; every index is checked against its array before a load or store; plain launches in the
// handle's stream, no workgroup waits on another.
#define K26_DB TPB                      // diagonals per workgroup of k26_pairs: one per thread
#define K26_WIN 512                     // mask words per LDS window (4 KiB; with the four waves' shifted copies 20 KiB per workgroup: 7 per CU)
#define K26_WAVES (TPB / 64)

struct K26V {                           // a diagonal's count sum and value sum
    double s; u64 c;
    struct Out { double* s; u64* c; };
    __device__ __forceinline__ static K26V zero() { return K26V{0.0, 0ull}; }
    __device__ __forceinline__ static K26V add(const K26V& a, const K26V& b) { return K26V{a.s + b.s, a.c + b.c}; }
    __device__ __forceinline__ static K26V up(const K26V& a, int d)
    {
        K26V r;
        r.s = __shfl_up(a.s, (unsigned)d);
        r.c = (u64)__shfl_up((unsigned long long)a.c, (unsigned)d);
        return r;
    }
    __device__ __forceinline__ static void store(const Out& o, size_t i, const K26V& v) { o.s[i] = v.s; o.c[i] = v.c; }
};

// a cell's value and whether it is used: d = by - bx, ix = bx - b0 (iy = ix + d), ew: nb effective weights
__device__ __forceinline__ bool k26_value(const double* __restrict__ ew, int nb, int ign, long long ix, long long d, u32 c, double& v)
{
    const long long iy = ix + d;
    if (d < ign || ix < 0 || iy >= nb) return false;                            // (d >= ign >= 0: ix <= iy)
    const double wx = ew[ix], wy = ew[iy];
    if (wx != wx || wy != wy) return false;
    v = (wx * (double)c) * wy;
    return true;
}

// what a cell adds to the run of diagonal `k` (o: bx - b0); in.b0 = 0 and in.nb = nd = nb: the store's index is the diagonal
__device__ __forceinline__ K26V k25_term(const K25In& in, int, int k, int o, u32 c, K26V*)
{
    double v;
    return k26_value(in.w, in.nb, in.ign, o, k, c, v) ? K26V{v, (u64)c} : K26V::zero();
}

// ew[i] = weight[i] (balanced; NaN on an invalid bin), or 1 where valid[i] != 0 (all bins without a mask) and NaN elsewhere; m: the
// valid bins, one bit each.  The grid covers 64 W bins: every lane of a wave reaches the ballot
__global__ void __launch_bounds__(TPB)
k26_mask(const u32* __restrict__ valid, const double* __restrict__ weight, int nb, int W, double nan, double* __restrict__ ew, u64* __restrict__ m)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    bool ok = false;
    if (i < nb) {
        const double v = weight ? weight[i] : ((!valid || valid[i]) ? 1.0 : nan);
        ew[i] = v;
        ok = v == v;
    }
    const u64 b = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && (i >> 6) < W) m[i >> 6] = b;
}

__global__ void __launch_bounds__(TPB)
k26_pairs(const u64* __restrict__ m, int W, int nb, int ign, long long* __restrict__ n_pairs)
{
    __shared__ __align__(16) u64 wa[K26_WIN];                                   // m[J .. J + WIN)
    __shared__ __align__(16) u64 wb[K26_WAVES][K26_WIN + 2];                    // per wave w: m[J + q + 1 ..] (WIN words), then m[J + q], q = q0 + w
    const long long d0 = (long long)blockIdx.x * K26_DB, d = d0 + threadIdx.x;
    if (d0 >= nb) return;                                                       // (the whole workgroup)
    const int q0 = (int)(d0 >> 6), wave = threadIdx.x >> 6;
    const u32 rr = threadIdx.x & 31;                                            // d = 64 (q0 + wave) + r, r = the lane: r % 32, and r >= 32
    const bool upper = (threadIdx.x & 32) != 0;
    const int jend = W - q0;                                                    // the words j with j + q0 < W (d0 < nb: at least one)
    u32 acc = 0u;                                                               // (at most nb <= 2^24)
    for (int J = 0; J < jend; J += K26_WIN) {
        __syncthreads();
        for (int t = threadIdx.x; t < K26_WIN; t += TPB) {
            const long long ja = (long long)J + t;
            wa[t] = ja < W ? m[ja] : 0ull;
        }
        for (int t = threadIdx.x; t < K26_WAVES * (K26_WIN + 1); t += TPB) {
            const int w = t / (K26_WIN + 1), k = t - w * (K26_WIN + 1);         // (w < K26_WAVES, k <= WIN)
            const long long jb = (long long)J + q0 + w + (k < K26_WIN ? k + 1 : 0);
            wb[w][k] = jb < W ? m[jb] : 0ull;
        }
        __syncthreads();
        const int cnt = jend - J < K26_WIN ? jend - J : K26_WIN;
        // word j of m >> d is bits [r, r + 64) of the 128 bits (hi, lo) = (m[j + q + 1], m[j + q]): as dwords, (a, b) for r < 32 and
        // (b, c) from there on, each a 32-bit funnel shift by r % 32; the c of a word is the a of the next.  The copy of a wave
        // starts at its word q + 1, so that both LDS reads of two consecutive j are 16-byte aligned
        const u64* __restrict__ mine = wb[wave];
        u64 lo = mine[K26_WIN];
        u32 a = __builtin_amdgcn_alignbit((u32)(lo >> 32), (u32)lo, rr);
#pragma unroll 8
        for (int j = 0; j < cnt; ++j) {
            const u64 hi = mine[j];
            const u32 b = __builtin_amdgcn_alignbit((u32)hi, (u32)(lo >> 32), rr);
            const u32 c = __builtin_amdgcn_alignbit((u32)(hi >> 32), (u32)hi, rr);
            const u64 wj = wa[j];
            acc += (u32)__popc((u32)wj & (upper ? b : a)) + (u32)__popc((u32)(wj >> 32) & (upper ? c : b));
            a = c; lo = hi;
        }
    }
    if (d < nb) n_pairs[d] = d >= ign ? (long long)acc : 0ll;
}

__global__ void __launch_bounds__(TPB)
k26_keys(const int* __restrict__ bx, const int* __restrict__ by, int n, u32* __restrict__ key, u32* __restrict__ val)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    key[i] = (u32)(by[i] - bx[i]);                                              // bx <= by
    val[i] = (u32)i;
}

// dk / dx / dc[i] = by - bx / bx - b0 / cnt of cell order[i]; *n_used += the used cells
__global__ void __launch_bounds__(TPB)
k26_gather(const u32* __restrict__ order, const int* __restrict__ bx, const int* __restrict__ by, const u32* __restrict__ cnt, int n, int b0,
           int nb, int ign, const double* __restrict__ ew, int* __restrict__ dk, int* __restrict__ dx, u32* __restrict__ dc, u64* __restrict__ n_used)
{
    __shared__ u32 wu[K26_WAVES];
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    u32 used = 0u;
    if (i < n) {
        const u32 j = order[i];
        if (j < (u32)n) {
            const int x = bx[j], d = by[j] - x;
            const u32 c = cnt[j];
            dk[i] = d; dx[i] = x - b0; dc[i] = c;
            double v;
            used = k26_value(ew, nb, ign, (long long)x - b0, d, c, v) ? 1u : 0u;
        }
    }
    for (int o = 32; o > 0; o >>= 1) used += (u32)__shfl_xor((int)used, o);
    if ((threadIdx.x & 63) == 0) wu[threadIdx.x >> 6] = used;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
        for (int q = 0; q < K26_WAVES; ++q) s += wu[q];
        if (s) atomicAdd(n_used, s);
    }
}

__global__ void __launch_bounds__(TPB)
k26_oe(const int* __restrict__ bx, const int* __restrict__ by, const u32* __restrict__ cnt, long long first, long long count, long long n,
       int b0, int nb, int ign, const double* __restrict__ ew, const double* __restrict__ expected, double nan, double* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= count || first + i >= n) return;
    const long long x = bx[first + i], d = (long long)by[first + i] - x;
    double v, r = nan;
    if (k26_value(ew, nb, ign, x - b0, d, cnt[first + i], v)) {                 // (used: 0 <= d < nb)
        const double e = expected[d];
        if (e == e && e != 0.0) r = v / e;
    }
    out[i] = r;
}

// ---- K26 host side ------------------------------------------------------------------------------
// the checks every K26 call shares; -> CL_OK with c usable.  (K25's marginals imply K24's folded cells: mat_release drops both)
static int exp_enter(cl_chrom* c, const char* who, bool need_diagonals)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, who, "asynchronous runs still in flight");
    if (!c->bl.st.ready) return fail(CL_ERR_ARG, who, "no marginals on this handle (cl_bal_marginals)");
    if (need_diagonals && !c->ex.st.ready) return fail(CL_ERR_ARG, who, "no diagonals on this handle (cl_exp_diagonals)");
    return CL_OK;
}

static int exp_diagonals(cl_chrom* c, const uint32_t* valid, int balanced, cl_chrom::Exp::State& st)
{
    const cl_chrom::Bal::State& bl = c->bl.st;
    const int n = (int)bl.n_cells, nb = (int)bl.nb, W = (nb + 63) / 64;
    const size_t sn = (size_t)n, snb = (size_t)nb;
    const int ntiles = (int)((sn + K25_TILE - 1) / K25_TILE);
    const double nan = std::nan("");
    int rc;
    if ((rc = c->ex.w.ensure(snb * 8)) || (rc = c->ex.mask.ensure((size_t)W * 8)) || (rc = c->ex.pairs.ensure(snb * 8)) ||
        (rc = c->ex.cnt.ensure(snb * 8)) || (rc = c->ex.val.ensure(snb * 8)) || (rc = c->ex.exp.ensure(snb * 8)) || (rc = c->ex.ctr.ensure(64)) ||
        (rc = c->ex.kin.ensure(sn * 4)) || (rc = c->ex.kout.ensure(sn * 4)) || (rc = c->ex.vin.ensure(sn * 4)) || (rc = c->ex.vout.ensure(sn * 4)) ||
        (rc = c->ex.dk.ensure(sn * 4)) || (rc = c->ex.dx.ensure(sn * 4)) || (rc = c->ex.dc.ensure(sn * 4)) ||
        (rc = c->ex.car.ensure((size_t)ntiles * sizeof(K25Car<K26V>)))) return rc;
    const u32* d_valid = nullptr;
    if (valid) {
        if ((rc = c->ex.valid.ensure(snb * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(c->ex.valid.p, valid, snb * 4, hipMemcpyHostToDevice, c->stream));
        d_valid = c->ex.valid.as<u32>();
    }
    const double* d_weight = balanced ? c->bl.w.as<double>() + snb : nullptr;   // (the weights of cl_bal_iterate: behind w)
    double* ew = c->ex.w.as<double>();
    LAUNCH(k26_mask, (long long)W * 64, d_valid, d_weight, nb, W, nan, ew, c->ex.mask.as<u64>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k26_pairs, dim3((unsigned)((nb + K26_DB - 1) / K26_DB)), dim3(TPB), 0, c->stream, (const u64*)c->ex.mask.as<u64>(), W, nb,
                       bl.ignore_diags, c->ex.pairs.as<long long>());
    HIP_TRY(hipGetLastError());
    // the diagonal order
    LAUNCH(k26_keys, n, c->mx.bx.as<int>(), c->mx.by.as<int>(), n, c->ex.kin.as<u32>(), c->ex.vin.as<u32>());
    HIP_TRY(hipGetLastError());
    const int bits = std::max(1, bits_for((unsigned)(nb - 1)));
    if ((rc = prim_run(c->ex.tmp, "radix_sort_pairs(expected)", [&](void* tmp, size_t& bytes) {
            return rocprim::radix_sort_pairs(tmp, bytes, c->ex.kin.as<u32>(), c->ex.kout.as<u32>(), c->ex.vin.as<u32>(), c->ex.vout.as<u32>(), sn, 0,
                                             bits, c->stream);
        })))
        return rc;
    HIP_TRY(hipMemsetAsync(c->ex.ctr.p, 0, 64, c->stream));
    HIP_TRY(hipMemsetAsync(c->ex.cnt.p, 0, snb * 8, c->stream));                // (a diagonal without cells has no run)
    HIP_TRY(hipMemsetAsync(c->ex.val.p, 0, snb * 8, c->stream));
    u64* d_used = c->ex.ctr.as<u64>();
    LAUNCH(k26_gather, n, (const u32*)c->ex.vout.as<u32>(), c->mx.bx.as<int>(), c->mx.by.as<int>(), c->mx.cnt.as<u32>(), n, (int)bl.b0, nb,
           bl.ignore_diags, (const double*)ew, c->ex.dk.as<int>(), c->ex.dx.as<int>(), c->ex.dc.as<u32>(), d_used);
    HIP_TRY(hipGetLastError());
    // the sums per diagonal: runs of equal d, the keys being the diagonals themselves (b0 = 0, nb = nd)
    K25In in{};
    for (int ph = 0; ph < 2; ++ph) { in.key[ph] = c->ex.dk.as<int>(); in.oth[ph] = c->ex.dx.as<int>(); in.cnt[ph] = c->ex.dc.as<u32>(); }
    in.n = n; in.ign = bl.ignore_diags; in.b0 = 0; in.nb = nb; in.w = ew;
    in.vec = 1;
    for (const void* p : {(const void*)in.key[0], (const void*)in.oth[0], (const void*)in.cnt[0]}) if ((uintptr_t)p % 16) in.vec = 0;
    K26V::Out out{c->ex.val.as<double>(), c->ex.cnt.as<u64>()};
    K25Car<K26V>* car = c->ex.car.as<K25Car<K26V>>();
    hipLaunchKernelGGL(k25_marg<K26V>, dim3((unsigned)ntiles, 1u), dim3(TPB), 0, c->stream, in, out, car, ntiles, (u64*)nullptr, (const K25Rec*)nullptr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k25_fold<K26V>, dim3((unsigned)nblocks(ntiles), 1u), dim3(TPB), 0, c->stream, (const K25Car<K26V>*)car, ntiles, 0, nb, out,
                       (const K25Rec*)nullptr);
    HIP_TRY(hipGetLastError());
    u64 hu = 0;
    HIP_TRY(hipMemcpyAsync(&hu, d_used, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    st.nd = nb; st.n_used = (long long)hu;
    return CL_OK;
}

extern "C" int cl_exp_diagonals(cl_chrom* c, const uint32_t* valid, int32_t balanced, int64_t* nd, int64_t* n_used)
{
    if (nd) *nd = 0;
    if (n_used) *n_used = 0;
    int rc = exp_enter(c, "cl_exp_diagonals", false);
    if (rc != CL_OK) return rc;
    if (!nd || !n_used) return fail(CL_ERR_ARG, "cl_exp_diagonals: bad arguments");
    if (balanced != 0 && balanced != 1) return fail(CL_ERR_ARG, "cl_exp_diagonals: balanced must be 0 or 1");
    if (balanced && !c->bl.st.iterated) return fail(CL_ERR_ARG, "cl_exp_diagonals: no weights on this handle (cl_bal_iterate)");
    if (balanced && valid) return fail(CL_ERR_ARG, "cl_exp_diagonals: the balanced mode takes its mask from the weights (valid must be NULL)");
    cl_chrom::Exp::State st;
    st.ready = true;
    st.balanced = balanced;
    if (c->bl.st.nb == 0) { exp_release(c); c->ex.st = st; return CL_OK; }            // (no cells: no HIP call)
    HIP_TRY(hipSetDevice(c->device));
    eig_release(c);                                                                  // (K27's matrix was made of the earlier diagonals)
    dot_release(c);                                                                  // (... and K29's lambdas)
    sad_release(c);                                                                  // (... and K30's tables)
    c->ex.st = cl_chrom::Exp::State();                                               // (the earlier state's buffers are written from here on; every K26 call ends synchronised)
    rc = exp_diagonals(c, valid, balanced, st);
    if (rc != CL_OK) {
        (void)hipStreamSynchronize(c->stream);
        exp_release(c);
        return rc;
    }
    c->ex.st = st;
    *nd = st.nd; *n_used = st.n_used;
    return CL_OK;
}

extern "C" int cl_exp_diagonals_get(cl_chrom* c, int64_t first, int64_t count, int64_t* n_pairs, uint64_t* cnt_sum, double* val_sum)
{
    int rc = exp_enter(c, "cl_exp_diagonals_get", true);
    if (rc != CL_OK) return rc;
    if (!range_ok(first, count, c->ex.st.nd)) return fail(CL_ERR_ARG, "cl_exp_diagonals_get: range outside the diagonals");
    if (count > 0 && (!n_pairs || !cnt_sum || !val_sum)) return fail(CL_ERR_ARG, "cl_exp_diagonals_get: bad arguments");
    if (count == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    return read_back(c, "cl_exp_diagonals_get", {{n_pairs, c->ex.pairs.as<long long>() + first, (size_t)count * 8},
                                                 {cnt_sum, c->ex.cnt.as<u64>() + first, (size_t)count * 8},
                                                 {val_sum, c->ex.val.as<double>() + first, (size_t)count * 8}});
}

extern "C" int cl_exp_set(cl_chrom* c, const double* expected, int64_t count)
{
    int rc = exp_enter(c, "cl_exp_set", true);
    if (rc != CL_OK) return rc;
    if (count != c->ex.st.nd) return fail(CL_ERR_ARG, "cl_exp_set: count is not the number of diagonals");
    if (count > 0 && !expected) return fail(CL_ERR_ARG, "cl_exp_set: bad arguments");
    eig_release(c);                                                             // (K27's matrix was made of the earlier expected values)
    dot_release(c);                                                             // (... and K29's lambdas)
    sad_release(c);                                                             // (... and K30's tables)
    if (count > 0) {
        HIP_TRY(hipSetDevice(c->device));
        c->ex.st.expected = false;
        HIP_TRY(hipMemcpyAsync(c->ex.exp.p, expected, (size_t)count * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->ex.st.expected = true;
    return CL_OK;
}

extern "C" int cl_exp_cells_get(cl_chrom* c, int64_t first, int64_t count, double* oe)
{
    int rc = exp_enter(c, "cl_exp_cells_get", true);
    if (rc != CL_OK) return rc;
    if (!c->ex.st.expected) return fail(CL_ERR_ARG, "cl_exp_cells_get: no expected values on this handle (cl_exp_set)");
    if (!range_ok(first, count, c->bl.st.n_cells)) return fail(CL_ERR_ARG, "cl_exp_cells_get: range outside the cells");
    if (count > 0 && !oe) return fail(CL_ERR_ARG, "cl_exp_cells_get: bad arguments");
    if (count == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->ex.out.ensure((size_t)count * 8))) return rc;
    LAUNCH(k26_oe, count, c->mx.bx.as<int>(), c->mx.by.as<int>(), c->mx.cnt.as<u32>(), (long long)first, (long long)count, c->bl.st.n_cells,
           (int)c->bl.st.b0, (int)c->bl.st.nb, c->bl.st.ignore_diags, (const double*)c->ex.w.as<double>(), (const double*)c->ex.exp.as<double>(), std::nan(""),
           c->ex.out.as<double>());
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(CL_ERR_HIP, "cl_exp_cells_get", hipGetErrorString(e));
    return read_back(c, "cl_exp_cells_get", {{oe, c->ex.out.p, (size_t)count * 8}});
}

extern "C" int cl_exp_free(cl_chrom* c) { return unit_free(c, "cl_exp_free", exp_release); }
