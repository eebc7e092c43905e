// k_fingerprint.hip -- K12: the histogram of contact-matrix cell counts behind scripts/jd2fingerprint, on the chromosome resident
// in HBM -- kernels and C entry point.
#include "cl_chrom.h"

// ==========================================================================================
// K12: cell-count histogram of the upper contact matrix (scripts/jd2fingerprint:32-50)
// ==========================================================================================
// The script bins every kept PET into the cell ((x - minC) // bs, (y - minC) // bs), minC the minimum of both coordinate columns
// of the kept rows, and keeps the count of every non-empty cell.  The fingerprint only needs those counts in ascending order, so
// K12 returns their HISTOGRAM: the distinct counts v with the number of cells H[v] holding v PETs (sum of H = cells, sum of
// v H[v] = kept PETs).  Four passes, integer work only, so the result is exact and does not depend on scheduling:
//   k12_minmax  min / max of both columns and the number of kept rows (one wave-reduced atomic per wave)
//   k12_keys    cell key cx << b | cy of every kept row (b = bits of the largest cell index; division by the bin size is a
//               host-made multiply-shift), compacted with one atomic per chunk of 2048 rows -- the order is restored by the sort
//   rocPRIM radix sort of the keys over their 2b bits
//   k12_runs    every run end of the sorted keys finds its run start by exponential search backwards (O(log count) reads; a
//               cell of count 1 reads two neighbours), and adds its count to a workgroup-private LDS histogram of counts
//               1 .. K12_HB - 1, wave-aggregated (one LDS atomic per distinct count in a wave: Guideline 12); larger counts go to a
//               compact overflow list (at most m / K12_HB entries: every entry is a distinct cell of >= K12_HB PETs)
// The overflow list is sorted and run-length coded on the device, and both parts are compacted to (value, multiplicity) pairs, so
// the device-to-host copy is O(distinct counts).  Distinct counts D satisfy D (D + 1) / 2 <= kept PETs.
// Scratch (c->fp) is the handle's own, apart from the sweep's layouts, q index, count cache and K8 tables, and is freed when the
// call returns: a fingerprint is one call per chromosome, and the handle's footprint between sweep steps stays what it was.
#define K12_HB 2048                     // LDS histogram bins (8 KB per workgroup): counts 1 .. 2047
#define K12_GRID 1024                   // workgroups of the grid-stride kernels
enum { K12_MIN = 0, K12_MAX = 1, K12_KEPT = 2, K12_POS = 3, K12_NOVF = 4, K12_NPAIR = 5, K12_HDR = 16 };   // fp.small: header, then hist

// (K12Div, k12_div, k12_divisor: cl_chrom.h, shared with K24)
__device__ __forceinline__ bool k12_keep(int x, int y, int cut)
{
    return cut <= 0 || (long long)y - (long long)x >= (long long)cut;        // parseJd(jd, cut), cLoops/io.py:213-216
}

__device__ __forceinline__ int k12_lane_rank(u64 mask)               // set bits of `mask` below this lane
{
    return __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
}

__global__ void k12_init(int* s)
{
    s[K12_MIN] = INT_MAX; s[K12_MAX] = INT_MIN;
    for (int k = K12_KEPT; k < K12_HDR; ++k) s[k] = 0;
}

__global__ void __launch_bounds__(TPB)
k12_minmax(const int* __restrict__ X, const int* __restrict__ Y, int n, int cut, int* __restrict__ s)
{
    int lo = INT_MAX, hi = INT_MIN, kept = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int x = X[i], y = Y[i];
        if (k12_keep(x, y, cut)) { lo = min(lo, min(x, y)); hi = max(hi, max(x, y)); ++kept; }
    }
    lo = dpp_reduce_wave(lo, OpMin());
    hi = dpp_reduce_wave(hi, OpMax());
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
    if ((threadIdx.x & 63) == 0 && kept) { atomicMin(&s[K12_MIN], lo); atomicMax(&s[K12_MAX], hi); atomicAdd(&s[K12_KEPT], kept); }
}

#define K12_ITEMS 8                     // rows per thread and chunk of k12_keys: one atomic per TPB * K12_ITEMS rows
__global__ void __launch_bounds__(TPB)
k12_keys(const int* __restrict__ X, const int* __restrict__ Y, int n, int cut, int minc, K12Div d, int b, int m,
         int* __restrict__ s, u64* __restrict__ keys)
{
    __shared__ int wbase[TPB / 64];
    __shared__ int bbase;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // chunks of TPB * K12_ITEMS rows; the loop bound is uniform per workgroup (barriers inside)
    for (long long base = (long long)blockIdx.x * TPB * K12_ITEMS; base < n; base += (long long)gridDim.x * TPB * K12_ITEMS) {
        int x[K12_ITEMS], y[K12_ITEMS], cnt = 0;
        unsigned flags = 0;
#pragma unroll
        for (int k = 0; k < K12_ITEMS; ++k) {
            const long long i = base + k * TPB + threadIdx.x;
            x[k] = 0; y[k] = 0;
            if (i < n) { x[k] = X[i]; y[k] = Y[i]; if (k12_keep(x[k], y[k], cut)) { flags |= 1u << k; ++cnt; } }
        }
        int incl = cnt;                                  // inclusive scan of the kept counts over the wave
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        if (lane == 63) wbase[w] = incl;
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
            for (int k = 0; k < TPB / 64; ++k) { const int t = wbase[k]; wbase[k] = tot; tot += t; }
            bbase = tot ? atomicAdd(&s[K12_POS], tot) : 0;
        }
        __syncthreads();
        int p = bbase + wbase[w] + incl - cnt;
#pragma unroll
        for (int k = 0; k < K12_ITEMS; ++k) {
            if (((flags >> k) & 1u) && p < m) {
                const u64 cx = k12_div(d, (u32)x[k] - (u32)minc), cy = k12_div(d, (u32)y[k] - (u32)minc);
                keys[p] = cx << b | cy;
            }
            p += (flags >> k) & 1u;
        }
        __syncthreads();                                 // wbase / bbase are rewritten by the next chunk
    }
}

// first index of the run holding position i of the sorted array t (t[i] is the run's value): exponential search backwards
template <typename T>
__device__ __forceinline__ long long k12_run_start(const T* __restrict__ t, long long i)
{
    const T v = t[i];
    long long hi = i, lo = -1, step = 1;
    for (;;) {                                       // t[hi] == v; widen until t[lo] != v (or lo = -1)
        const long long j = hi - step;
        if (j < 0) break;
        if (t[j] != v) { lo = j; break; }
        hi = j;
        step <<= 1;
    }
    // t is sorted, t[lo] != v (or lo = -1), t[hi] == v: the first v lies in (lo, hi]
    while (hi - lo > 1) { const long long mid = lo + ((hi - lo) >> 1); if (t[mid] == v) hi = mid; else lo = mid; }
    return hi;
}

__global__ void __launch_bounds__(TPB)
k12_runs(const u64* __restrict__ keys, int m, u32* __restrict__ hist, int* __restrict__ s, u32* __restrict__ ovf, int ovf_cap)
{
    __shared__ u32 lh[K12_HB];
    for (int k = threadIdx.x; k < K12_HB; k += blockDim.x) lh[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int base = blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < m; base += gridDim.x * blockDim.x) {
        const int i = base + lane;
        int cnt = 0;
        if (i < m && (i == m - 1 || keys[i] != keys[i + 1])) cnt = (int)((long long)i + 1 - k12_run_start(keys, i));
        if (cnt >= K12_HB) {
            const int p = atomicAdd(&s[K12_NOVF], 1);
            if (p < ovf_cap) ovf[p] = (u32)cnt;
        }
        bool pend = cnt > 0 && cnt < K12_HB;
        for (;;) {                                   // wave aggregation: one LDS atomic per distinct count of the wave
            const u64 act = __ballot(pend);
            if (!act) break;
            const int v = __shfl(cnt, __ffsll((long long)act) - 1);
            const bool same = pend && cnt == v;
            const u64 grp = __ballot(same);
            if (lane == __ffsll((long long)act) - 1) atomicAdd(&lh[v], (u32)__popcll(grp));
            if (same) pend = false;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K12_HB; k += blockDim.x)
        if (lh[k]) atomicAdd(&hist[k], lh[k]);
}

// (value, multiplicity) pairs of the non-empty histogram bins, appended to `pv` / `pm` (one atomic per wave)
__global__ void __launch_bounds__(TPB)
k12_hist_pairs(const u32* __restrict__ hist, int* __restrict__ s, u32* __restrict__ pv, u32* __restrict__ pm, int cap)
{
    const int lane = threadIdx.x & 63;
    for (int base = blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < K12_HB; base += gridDim.x * blockDim.x) {
        const int k = base + lane;
        const u32 h = k < K12_HB ? hist[k] : 0u;
        const u64 mask = __ballot(h != 0);
        if (!mask) continue;
        int first = 0;
        if (lane == 0) first = atomicAdd(&s[K12_NPAIR], __popcll(mask));
        first = __shfl(first, 0);
        const int p = first + k12_lane_rank(mask);
        if (h && p < cap) { pv[p] = (u32)k; pm[p] = h; }
    }
}

// ... and of the runs of the sorted overflow list
__global__ void __launch_bounds__(TPB)
k12_ovf_pairs(const u32* __restrict__ ov, int k, int* __restrict__ s, u32* __restrict__ pv, u32* __restrict__ pm, int cap)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < k; i += gridDim.x * blockDim.x) {
        if (i != k - 1 && ov[i] == ov[i + 1]) continue;
        const int len = (int)((long long)i + 1 - k12_run_start(ov, i));
        const int p = atomicAdd(&s[K12_NPAIR], 1);
        if (p < cap) { pv[p] = ov[i]; pm[p] = (u32)len; }
    }
}

static int k12_grid(long long n) { return (int)std::max(1ll, std::min<long long>(K12_GRID, (n + TPB - 1) / TPB)); }

// ---- K12 host entry point -----------------------------------------------------------------------
static int contact_hist(cl_chrom* c, int cut, int bin_size, int64_t cap, int64_t* values, int64_t* mult, int64_t* n_distinct,
                        int64_t* n_cells, int64_t* n_kept, int32_t* min_c)
{
    const int n = (int)c->n;
    int rc;
    if ((rc = c->fp.small.ensure((K12_HDR + K12_HB) * 4))) return rc;
    int* s = c->fp.small.as<int>();
    u32* hist = (u32*)(s + K12_HDR);
    hipLaunchKernelGGL(k12_init, dim3(1), dim3(1), 0, c->stream, s);
    HIP_TRY(hipMemsetAsync(hist, 0, K12_HB * 4, c->stream));
    hipLaunchKernelGGL(k12_minmax, dim3(k12_grid(n)), dim3(TPB), 0, c->stream, c->d_x, c->d_y, n, cut, s);
    HIP_TRY(hipGetLastError());
    int hs[3];
    HIP_TRY(hipMemcpyAsync(hs, s, 12, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int m = hs[K12_KEPT];
    if (n_kept) *n_kept = m;
    if (m == 0) return CL_OK;                                        // np.min of no rows: the caller raises
    if (min_c) *min_c = hs[K12_MIN];
    const int minc = hs[K12_MIN];
    const u32 top = ((u32)hs[K12_MAX] - (u32)minc) / (u32)bin_size;  // largest cell index
    const int b = std::max(1, bits_for(top));
    const K12Div dv = k12_divisor((u32)bin_size);
    // keys of the kept rows, sorted over their 2b bits
    if ((rc = c->fp.keys.ensure((size_t)m * 8)) || (rc = c->fp.sorted.ensure((size_t)m * 8))) return rc;
    hipLaunchKernelGGL(k12_keys, dim3(k12_grid((n + K12_ITEMS - 1) / K12_ITEMS)), dim3(TPB), 0, c->stream, c->d_x, c->d_y, n, cut, minc, dv, b, m, s,
                       c->fp.keys.as<u64>());
    HIP_TRY(hipGetLastError());
    if ((rc = prim_run(c->fp.tmp, "radix_sort_keys(cells)", [&](void* tmp, size_t& bytes) {
            return rocprim::radix_sort_keys(tmp, bytes, c->fp.keys.as<u64>(), c->fp.sorted.as<u64>(), (size_t)m, 0, 2 * b, c->stream);
        })))
        return rc;
    // run lengths -> LDS histogram + overflow list (fp.keys is free again: the overflow list lives there)
    const int ovf_cap = m / K12_HB + 1;
    u32* ovf = (u32*)c->fp.keys.p;                                    // ovf_cap u32 <= m * 8 bytes
    u32* ovs = ovf + ovf_cap;                                         // the sorted copy
    hipLaunchKernelGGL(k12_runs, dim3(k12_grid(m)), dim3(TPB), 0, c->stream, c->fp.sorted.as<u64>(), m, hist, s, ovf, ovf_cap);
    HIP_TRY(hipGetLastError());
    int novf = 0;
    HIP_TRY(hipMemcpyAsync(&novf, s + K12_NOVF, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (novf > ovf_cap) return fail(CL_ERR_HIP, "cl_contact_hist: overflow list exceeded its bound");
    // (value, multiplicity) pairs: at most K12_HB - 1 histogram bins + novf overflow runs
    const int pcap = K12_HB + novf;
    if ((rc = c->fp.pairs.ensure((size_t)pcap * 8))) return rc;
    u32* pv = c->fp.pairs.as<u32>();
    u32* pm = pv + pcap;
    if (novf > 0) {
        if ((rc = prim_run(c->fp.tmp, "radix_sort_keys(overflow)", [&](void* tmp, size_t& bytes) {
                return rocprim::radix_sort_keys(tmp, bytes, ovf, ovs, (size_t)novf, 0, 32, c->stream);
            })))
            return rc;
        hipLaunchKernelGGL(k12_ovf_pairs, dim3(k12_grid(novf)), dim3(TPB), 0, c->stream, ovs, novf, s, pv, pm, pcap);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k12_hist_pairs, dim3(K12_HB / TPB), dim3(TPB), 0, c->stream, hist, s, pv, pm, pcap);
    HIP_TRY(hipGetLastError());
    int np = 0;
    HIP_TRY(hipMemcpyAsync(&np, s + K12_NPAIR, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (np > pcap) return fail(CL_ERR_HIP, "cl_contact_hist: pair list exceeded its bound");
    *n_distinct = np;
    if (np > cap) return fail(CL_ERR_ARG, "cl_contact_hist: capacity below the number of distinct counts (*n_distinct)");
    std::vector<u32> hv(np), hm(np);
    if (np > 0) {
        HIP_TRY(hipMemcpyAsync(hv.data(), pv, (size_t)np * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(hm.data(), pm, (size_t)np * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    // the pairs arrive in atomic order; their values are distinct, so sorting by value fixes the result
    std::vector<int> ord(np);
    for (int k = 0; k < np; ++k) ord[k] = k;
    std::sort(ord.begin(), ord.end(), [&](int a, int b2) { return hv[a] < hv[b2]; });
    long long cells = 0, pets = 0;
    for (int k = 0; k < np; ++k) {
        values[k] = hv[ord[k]]; mult[k] = hm[ord[k]];
        cells += hm[ord[k]]; pets += (long long)hv[ord[k]] * hm[ord[k]];
    }
    if (pets != m) return fail(CL_ERR_HIP, "cl_contact_hist: histogram does not account for every kept PET");
    if (n_cells) *n_cells = cells;
    return CL_OK;
}

extern "C" int cl_contact_hist(cl_chrom* c, int32_t cut, int32_t bin_size, int64_t cap, int64_t* values, int64_t* mult,
                               int64_t* n_distinct, int64_t* n_cells, int64_t* n_kept, int32_t* min_c)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_distinct) *n_distinct = 0;
    if (n_cells) *n_cells = 0;
    if (n_kept) *n_kept = 0;
    if (min_c) *min_c = 0;
    if (bin_size < 1) return fail(CL_ERR_ARG, "cl_contact_hist: bin_size < 1");
    if (cap < 0 || (cap > 0 && (!values || !mult)) || !n_distinct) return fail(CL_ERR_ARG, "cl_contact_hist: bad arguments");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_contact_hist: asynchronous runs still in flight");
    if (c->n == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    const int rc = contact_hist(c, cut, bin_size, cap, values, mult, n_distinct, n_cells, n_kept, min_c);
    if (rc != CL_OK) (void)hipStreamSynchronize(c->stream);          // nothing of ours may still be running when the scratch goes
    c->fp = cl_chrom::Fp();
    return rc;
}
