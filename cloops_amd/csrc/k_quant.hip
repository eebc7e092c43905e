// k_quant.hip -- K11: interval counts for re-quantifying a loop set on a dataset (scripts/quantifyLoops.py) and for differential
// loops (scripts/deLoops), on the chromosome resident in HBM -- kernel and C entry point.
#include "cl_chrom.h"

// ==========================================================================================
// K11: directed counts of the 11 x 11 window pairs (cLoops/cModel.py:60-80, scripts/quantifyLoops.py:124-134)
// ==========================================================================================
// quantifyLoops' local background is getPETsforRegions(A_k, B_l) over the 10 x 10 shifted window pairs of
// getNearbyPairRegions, and what it keeps of each call is the DIRECTED count rab = |{X in A_k} & {Y in B_l}| -- not
// the union-based |S(A_k) & S(B_l)| that K8 returns.  One workgroup per record: the PETs with X inside the span of
// the A windows are one contiguous slice of K8's X-sorted table (entry = X << 32 | Y); every PET of it gets an 11-bit
// mask of the A windows holding X and one of the B windows holding Y, and bumps the set-bit pairs of the 11 x 11 grid
// in LDS.  Shifted windows overlap by about half a step, so a coordinate lies in only a few windows.
// ra = |S(A_0)| = |{X in A_0}| (a difference of two bounds in the X table) + the PETs of the Y slice of A_0 whose X
// is not in A_0 (so a PET with both ends inside is counted once); rb likewise.  Integer work only, LDS atomics only.
#define QNT_OUT (2 + SIG_W * SIG_W)     // [0] ra, [1] rb, [2 + 11 k + l] |{X in A_k} & {Y in B_l}|

__device__ __forceinline__ void k11_decode(u64 kv, int& first, int& second)
{
    first = (int)(u32)(kv >> 32) - (1 << 30);
    second = (int)(u32)(kv & 0xffffffffu) - (1 << 30);
}

__global__ void __launch_bounds__(TPB)
k11_quant(const u64* __restrict__ tx, const u64* __restrict__ ty, const int* __restrict__ d_m, int nrec,
          const SigWin* __restrict__ wins, int* __restrict__ out)
{
    __shared__ int wlo[2 * SIG_W], whi[2 * SIG_W];
    __shared__ int c_ab[SIG_W * SIG_W];
    __shared__ int rng[6];              // X slice of the A span; Y slice of A_0; Y slice of B_0
    __shared__ int c_r[2];              // ra, rb
    const int rec = blockIdx.x;
    if (rec >= nrec) return;
    const int m = d_m[0];
    if (threadIdx.x < 2 * SIG_W) { wlo[threadIdx.x] = wins[rec].lo[threadIdx.x]; whi[threadIdx.x] = wins[rec].hi[threadIdx.x]; }
    for (int k = threadIdx.x; k < SIG_W * SIG_W; k += blockDim.x) c_ab[k] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        int lo = wlo[0], hi = whi[0];
        for (int k = 1; k < SIG_W; ++k) { lo = min(lo, wlo[k]); hi = max(hi, whi[k]); }
        rng[0] = k8_lb(tx, m, lo);
        rng[1] = k8_ub(tx, m, hi);
    } else if (threadIdx.x == 1 || threadIdx.x == 2) {
        const int w = (threadIdx.x - 1) * SIG_W;
        rng[2 * threadIdx.x] = k8_lb(ty, m, wlo[w]);
        rng[2 * threadIdx.x + 1] = k8_ub(ty, m, whi[w]);
    } else if (threadIdx.x == 3 || threadIdx.x == 4) {
        const int w = (threadIdx.x - 3) * SIG_W;                   // |{X in W}|: the same bounds as getCounts' searchsorted
        c_r[threadIdx.x - 3] = max(0, k8_ub(tx, m, whi[w]) - k8_lb(tx, m, wlo[w]));
    }
    __syncthreads();
    for (int j = rng[0] + (int)threadIdx.x; j < rng[1]; j += blockDim.x) {
        int x, y;
        k11_decode(tx[j], x, y);
        unsigned ma = 0, mb = 0;
#pragma unroll
        for (int k = 0; k < SIG_W; ++k) {
            ma |= (unsigned)((x >= wlo[k]) & (x <= whi[k])) << k;
            mb |= (unsigned)((y >= wlo[SIG_W + k]) & (y <= whi[SIG_W + k])) << k;
        }
        if (!mb) continue;
        for (unsigned a = ma; a; a &= a - 1) {
            const int k = __ffs(a) - 1;
            for (unsigned b = mb; b; b &= b - 1) atomicAdd(&c_ab[k * SIG_W + (__ffs(b) - 1)], 1);
        }
    }
    // the Y-side halves of ra and rb: PETs with Y in the window whose X is not (those with X in it are in c_r already)
    int extra[2] = {0, 0};
    for (int s = 0; s < 2; ++s) {
        const int lo = wlo[s * SIG_W], hi = whi[s * SIG_W];
        for (int j = rng[2 + 2 * s] + (int)threadIdx.x; j < rng[3 + 2 * s]; j += blockDim.x) {
            int y, x;
            k11_decode(ty[j], y, x);
            extra[s] += (x < lo) | (x > hi);
        }
    }
    for (int o = 32; o > 0; o >>= 1) { extra[0] += __shfl_down(extra[0], o); extra[1] += __shfl_down(extra[1], o); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&c_r[0], extra[0]); atomicAdd(&c_r[1], extra[1]); }
    __syncthreads();
    int* o = out + (size_t)rec * QNT_OUT;
    if (threadIdx.x < 2) o[threadIdx.x] = c_r[threadIdx.x];
    for (int k = threadIdx.x; k < SIG_W * SIG_W; k += blockDim.x) o[2 + k] = c_ab[k];
}

// ---- K11 host entry point -----------------------------------------------------------------------
extern "C" int cl_quant_counts(cl_chrom* c, int32_t cut, int32_t n_records, const int32_t* windows, int32_t* out,
                               int64_t* n_pets)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_pets) *n_pets = 0;
    if (n_records < 0 || (n_records > 0 && (!windows || !out))) return fail(CL_ERR_ARG, "cl_quant_counts: bad arguments");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_quant_counts: asynchronous runs still in flight");
    if (c->n == 0) { if (n_records) memset(out, 0, (size_t)n_records * QNT_OUT * 4); return CL_OK; }
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = sig_tables(c, cut))) return rc;                          // K8's sorted tables of (chromosome, cut), shared
    int hm = 0;
    HIP_TRY(hipMemcpyAsync(&hm, c->sig.m.p, 4, hipMemcpyDeviceToHost, c->stream));
    if (n_records > 0) {
        if ((rc = c->sig.win.ensure((size_t)n_records * sizeof(SigWin))) || (rc = c->sig.out.ensure((size_t)n_records * QNT_OUT * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(c->sig.win.p, windows, (size_t)n_records * sizeof(SigWin), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k11_quant, dim3(n_records), dim3(TPB), 0, c->stream, c->sig.tx.as<u64>(), c->sig.ty.as<u64>(), c->sig.m.as<int>(),
                           n_records, c->sig.win.as<SigWin>(), c->sig.out.as<int>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, c->sig.out.p, (size_t)n_records * QNT_OUT * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n_pets) *n_pets = hm;
    return CL_OK;
}
