// k_domain.hip -- K22: the integers of a domain call on a resident chromosome -- three insulation tracks over its bins and the PETs
// of called domains -- kernels and C entry points.
#include "cl_chrom.h"

// ==========================================================================================
// K22: cross / up / down per bin boundary as range adds over difference arrays, and counts per domain
// ==========================================================================================
// Definitions: include/cloops_hip.h, cl_dom_tracks.  The reference has nothing of the kind; every number here is an integer that a few
// lines of numpy reproduce (tests/domains_cases.py).  Rows: K19's table (agg_table: the kept rows sorted by X, c->ag.sx = X + 2^30,
// c->ag.sy = Y, c->ag.kept of them), shared with cl_agg_loops and keyed by the cut, so another w or res sorts nothing.
//   k22_range                 the smallest / largest Y of the kept rows (one atomicMin / atomicMax per workgroup) and the first / last X
//   k22_tracks                one workgroup per K22_TILE consecutive sorted rows.  A row with bx <= by adds +1 at the first bin and -1
//                             behind the last bin of its three intervals (clipped to bmin .. bmax + 1): six updates, all at bins of
//                             [bx - w + 1, bx + w + 1].  The tile's updates go into three LDS windows of K22_BW counters over the bins
//                             [bx_first - w + 1, bx_last + w + 1] and reach the global difference arrays with one atomic per counter
//                             that is not zero; a tile whose bins do not fit (sparse rows) adds to global memory directly.  Before an
//                             atomic the lanes of a wave that share the first active lane's target leave it to that lane (the rows are
//                             sorted, so a pile-up of equal X is one add per wave, not 64).
//   inclusive scan            ONE rocPRIM scan over the three difference arrays laid end to end (n_bins + 1 entries each): every +1 has
//                             its -1 inside its own array, so the running sum is back at 0 where the next array begins.  u32 with
//                             wrap-around: -1 is 0xffffffff.
//   k22_count                 one workgroup per K22_TILE sorted rows: the domain of X and of Y by a search in the ascending starts
//                             (staged in LDS up to K22_DL of them, read from global memory beyond), the three counters of the
//                             K22_DW domains from the domain of the tile's first X on in LDS (X ascends, and Y mostly lies near),
//                             any other domain in global memory, the same per-wave aggregation, and one global atomic per LDS
//                             counter that is not zero: one domain holding every row costs three atomics per workgroup.
// Only vector stores and ordinary HIP atomics; every index is checked against its array before a store.  Scratch (c->dm) is the
// handle's own, apart from the sweep's layouts, q index, count cache and the K8 / K13 / K14 / K20 / K21 state.
#define K22_TILE 2048                   // sorted rows per workgroup of k22_tracks and k22_count (8 per thread)
#define K22_BW 3072                     // bins per LDS window of k22_tracks (three windows: 36 KB, four workgroups per CU)
#define K22_DL 2048                     // domain starts that k22_count stages in LDS (more: read from global memory)
#define K22_DW 1024                     // domains whose counters k22_count keeps in LDS (three arrays: 12 KB)
#define K22_U (K22_TILE / TPB)          // rows per thread
#define K22_WMAX 1024                   // w lies in [1, 1024]: 2 w + 1 <= K22_BW
#define K22_MAXRES (1ll << 29)          // res and w res lie below 2^29
#define K22_MAXBINS (1ll << 24)         // bins of a handle at one res
static_assert(2 * K22_WMAX + 1 <= K22_BW, "the window of one bin must fit the LDS window");

__device__ __forceinline__ int k22_bin(int p, int res)          // floor(p / res), res >= 1
{
    const int q = p / res;
    return q - ((p - q * res) < 0 ? 1 : 0);
}

// (k22_agg, K22_NONE: cl_chrom.h, shared with K24)

// rng: {min Y key, max Y key, first X key, last X key}, keys = coordinate + 2^30; rng[0] preset to ~0 and rng[1] to 0
__global__ void __launch_bounds__(TPB)
k22_range(const u32* __restrict__ sx, const int* __restrict__ sy, int m, u32* __restrict__ rng)
{
    __shared__ u32 lo[TPB / 64], hi[TPB / 64];
    u32 a = 0xffffffffu, b = 0u;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) {
        const u32 k = (u32)(sy[i] + (1 << 30));
        a = min(a, k); b = max(b, k);
    }
    for (int o = 32; o > 0; o >>= 1) {
        a = min(a, (u32)__shfl_xor((int)a, o));
        b = max(b, (u32)__shfl_xor((int)b, o));
    }
    if ((threadIdx.x & 63) == 0) { lo[threadIdx.x >> 6] = a; hi[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < TPB / 64; ++k) { a = min(a, lo[k]); b = max(b, hi[k]); }
        if (a <= b) { atomicMin(&rng[0], a); atomicMax(&rng[1], b); }
        if (blockIdx.x == 0 && m > 0) { rng[2] = sx[0]; rng[3] = sx[m - 1]; }
    }
}

// diff: three arrays of nb + 1 counters, for cross, up and down; entry g stands for bin bmin + g
__global__ void __launch_bounds__(TPB)
k22_tracks(const u32* __restrict__ sx, const int* __restrict__ sy, int m, int res, int w, int bmin, int nb, u32* __restrict__ diff)
{
    __shared__ u32 win[3 * K22_BW];
    const long long t0 = (long long)blockIdx.x * K22_TILE;
    if (t0 >= m) return;                                                        // (the whole workgroup)
    const int tn = (int)(m - t0 < K22_TILE ? m - t0 : K22_TILE);
    const int bxf = k22_bin((int)sx[t0] - (1 << 30), res), bxl = k22_bin((int)sx[t0 + tn - 1] - (1 << 30), res);
    const int wb0 = bxf - w + 1;                                                // the window: bins [wb0, wb0 + need)
    const long long span = (long long)bxl - bxf + 2ll * w + 1;
    const bool lds = span <= K22_BW;                                            // (the same in every lane)
    const int need = lds ? (int)span : 0;
    for (int k = threadIdx.x; k < need; k += TPB) { win[k] = 0u; win[K22_BW + k] = 0u; win[2 * K22_BW + k] = 0u; }
    __syncthreads();
    const int btop = bmin + nb - 1;                                             // bmax + 1: the last bin with an entry
#pragma unroll 2
    for (int u = 0; u < K22_U; ++u) {                                           // (no early exit: every lane takes part in the ballots)
        const int il = u * TPB + (int)threadIdx.x;
        int tb[6] = {K22_NONE, K22_NONE, K22_NONE, K22_NONE, K22_NONE, K22_NONE};   // +1 / -1 of cross, up, down
        if (il < tn) {
            const int bx = k22_bin((int)sx[t0 + il] - (1 << 30), res), by = k22_bin(sy[t0 + il], res);
            if (bx <= by) {
                const int lo3[3] = {max(bx + 1, by - w + 1), by + 1, by - w + 1};
                const int hi3[3] = {min(bx + w, by), bx + w, bx};
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const int lo = max(lo3[t], bmin), hi = min(hi3[t], btop);
                    if (lo <= hi) { tb[2 * t] = lo; tb[2 * t + 1] = hi + 1; }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const u32 v = k22_agg(tb[q], (q & 1) ? 0xffffffffu : 1u);
            if (v) {
                const int t = q >> 1;
                const int k = tb[q] - wb0;
                if (lds && k >= 0 && k < need) atomicAdd(&win[t * K22_BW + k], v);
                else {
                    const int g = tb[q] - bmin;
                    if (g >= 0 && g <= nb) atomicAdd(&diff[(size_t)t * ((size_t)nb + 1) + g], v);
                }
            }
        }
    }
    if (!lds) return;
    __syncthreads();
    for (int k = threadIdx.x; k < need; k += TPB) {
        const int g = wb0 + k - bmin;
        if (g < 0 || g > nb) continue;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const u32 v = win[t * K22_BW + k];
            if (v) atomicAdd(&diff[(size_t)t * ((size_t)nb + 1) + g], v);
        }
    }
}

// the interval of the ascending, disjoint [st[k], ive[k]) that holds p, or K22_NONE: only the last one that starts at or below p can
__device__ __forceinline__ int k22_dom(const long long* st, const long long* __restrict__ ive, int n, long long p)
{
    int a = 0, b = n;
    while (a < b) {
        const int mid = (int)(((long long)a + b) >> 1);
        if (st[mid] <= p) a = mid + 1; else b = mid;
    }
    return (a > 0 && p < ive[a - 1]) ? a - 1 : K22_NONE;
}

// cnt: three arrays of n counters, for intra, nx and ny
__global__ void __launch_bounds__(TPB)
k22_count(const u32* __restrict__ sx, const int* __restrict__ sy, int m, const long long* __restrict__ ivs,
          const long long* __restrict__ ive, int n, u32* __restrict__ cnt)
{
    __shared__ long long st[K22_DL];
    __shared__ u32 acc[3 * K22_DW];
    const long long t0 = (long long)blockIdx.x * K22_TILE;
    if (t0 >= m) return;                                                        // (the whole workgroup)
    const int tn = (int)(m - t0 < K22_TILE ? m - t0 : K22_TILE);
    const bool staged = n <= K22_DL;                                            // (the same in every lane)
    if (staged)
        for (int k = threadIdx.x; k < n; k += TPB) st[k] = ivs[k];
    for (int k = threadIdx.x; k < 3 * K22_DW; k += TPB) acc[k] = 0u;
    __syncthreads();
    const long long* S = staged ? (const long long*)st : ivs;
    int base;                                                                   // the last domain that starts at or below the tile's first X
    {
        const long long p = (long long)((int)sx[t0] - (1 << 30));
        int a = 0, b = n;
        while (a < b) {
            const int mid = (int)(((long long)a + b) >> 1);
            if (S[mid] <= p) a = mid + 1; else b = mid;
        }
        base = a > 0 ? a - 1 : 0;
    }
#pragma unroll 2
    for (int u = 0; u < K22_U; ++u) {                                           // (no early exit: every lane takes part in the ballots)
        const int il = u * TPB + (int)threadIdx.x;
        int id[3] = {K22_NONE, K22_NONE, K22_NONE};                             // intra, nx, ny
        if (il < tn) {
            id[1] = k22_dom(S, ive, n, (long long)((int)sx[t0 + il] - (1 << 30)));
            id[2] = k22_dom(S, ive, n, (long long)sy[t0 + il]);
            if (id[1] == id[2]) id[0] = id[1];
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const u32 v = k22_agg(id[t], 1u);
            if (v && id[t] >= 0 && id[t] < n) {
                const int k = id[t] - base;
                if (k >= 0 && k < K22_DW) atomicAdd(&acc[t * K22_DW + k], v);
                else atomicAdd(&cnt[(size_t)t * (size_t)n + id[t]], v);
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 3 * K22_DW; k += TPB) {
        const u32 v = acc[k];
        if (!v) continue;
        const int t = k / K22_DW;
        const long long d = (long long)base + (k - t * K22_DW);
        if (d < n) atomicAdd(&cnt[(size_t)t * (size_t)n + (size_t)d], v);
    }
}

// ---- K22 host side ------------------------------------------------------------------------------
static long long k22_floordiv(long long p, long long res)
{
    const long long q = p / res;
    return q - ((p - q * res) < 0 ? 1 : 0);
}

// the kept rows of `cut` sorted by X (shared with K19) and the range of their coordinates -> st (ready stays false)
static int dom_rows(cl_chrom* c, int cut, cl_chrom::Dom::State& st)
{
    int rc;
    if ((rc = agg_table(c, cut))) return rc;
    st.cut = cut;
    st.n_kept = c->ag.kept;
    if (c->ag.kept == 0) return CL_OK;
    if (c->dm.st.ready && c->dm.st.cut == cut && c->dm.st.n_kept == c->ag.kept) { st.pmin = c->dm.st.pmin; st.pmax = c->dm.st.pmax; return CL_OK; }
    const int m = c->ag.kept;
    if ((rc = c->dm.rng.ensure(64))) return rc;
    u32* rng = c->dm.rng.as<u32>();
    HIP_TRY(hipMemsetAsync(rng, 0xff, 4, c->stream));
    HIP_TRY(hipMemsetAsync(rng + 1, 0, 12, c->stream));
    hipLaunchKernelGGL(k22_range, dim3((unsigned)std::max(1, std::min(1024, nblocks(m)))), dim3(TPB), 0, c->stream, c->ag.sx.as<u32>(),
                       c->ag.sy.as<int>(), m, rng);
    HIP_TRY(hipGetLastError());
    u32 h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, rng, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const long long lim = 1ll << 29;
    long long v[4];
    for (int k = 0; k < 4; ++k) v[k] = (long long)h[k] - (1ll << 30);
    if (v[0] > v[1] || v[2] > v[3] || v[0] <= -lim || v[1] >= lim || v[2] <= -lim || v[3] >= lim)
        return fail(CL_ERR_HIP, "cl_dom_tracks: the range pass left coordinates no row can have");
    st.pmin = (int)std::min(v[0], v[2]);
    st.pmax = (int)std::max(v[1], v[3]);
    return CL_OK;
}

static int dom_tracks(cl_chrom* c, int cut, int res, int w, cl_chrom::Dom::State& st)
{
    int rc;
    if ((rc = dom_rows(c, cut, st))) return rc;
    st.res = res; st.w = w;
    if (st.n_kept == 0) { st.ready = true; return CL_OK; }
    const long long bmin = k22_floordiv(st.pmin, res), bmax = k22_floordiv(st.pmax, res);
    const long long nb = bmax - bmin + 2;
    if (nb < 2 || nb > K22_MAXBINS) return fail(CL_ERR_HIP, "cl_dom_tracks: the kept rows span more bins than all rows");
    const size_t words = 3 * ((size_t)nb + 1);
    if ((rc = c->dm.diff.ensure(words * 4)) || (rc = c->dm.trk.ensure(words * 4))) return rc;
    HIP_TRY(hipMemsetAsync(c->dm.diff.p, 0, words * 4, c->stream));
    const int m = (int)st.n_kept;
    hipLaunchKernelGGL(k22_tracks, dim3((unsigned)(((long long)m + K22_TILE - 1) / K22_TILE)), dim3(TPB), 0, c->stream, c->ag.sx.as<u32>(),
                       c->ag.sy.as<int>(), m, res, w, (int)bmin, (int)nb, c->dm.diff.as<u32>());
    HIP_TRY(hipGetLastError());
    if ((rc = prim_run(c->dm.tmp, "inclusive_scan(domains)", [&](void* tmp, size_t& bytes) {
            return rocprim::inclusive_scan(tmp, bytes, c->dm.diff.as<u32>(), c->dm.trk.as<u32>(), words, rocprim::plus<u32>(), c->stream);
        })))
        return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    st.bmin = bmin; st.n_bins = nb;
    st.ready = true;
    return CL_OK;
}

extern "C" int cl_dom_tracks(cl_chrom* c, int64_t cut, int64_t res, int64_t w, int64_t* n_bins, int64_t* bin0, int64_t* n_kept)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_bins) *n_bins = 0;
    if (bin0) *bin0 = 0;
    if (n_kept) *n_kept = 0;
    if (!n_bins || !bin0 || !n_kept) return fail(CL_ERR_ARG, "cl_dom_tracks: bad arguments");
    if (res < 1 || res >= K22_MAXRES) return fail(CL_ERR_ARG, "cl_dom_tracks: res outside [1, 2^29)");
    if (w < 1 || w > K22_WMAX) return fail(CL_ERR_ARG, "cl_dom_tracks: w outside [1, 1024]");
    if (w * res >= K22_MAXRES) return fail(CL_ERR_ARG, "cl_dom_tracks: w res must lie below 2^29");
    if (c->n > 0) {
        const long long lo = std::min(c->st.xmin, c->st.ymin), hi = std::max(c->st.xmax, c->st.ymax);
        if (k22_floordiv(hi, res) - k22_floordiv(lo, res) + 2 > K22_MAXBINS)
            return fail(CL_ERR_ARG, "cl_dom_tracks: the rows of this handle span more than 2^24 bins at this res");
    }
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_dom_tracks: asynchronous runs still in flight");
    cl_chrom::Dom::State st;
    if (c->n == 0) {
        st.ready = true; st.res = (int)res; st.w = (int)w;
        c->dm.st = st;
        return CL_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    const int cut32 = cut <= 0 ? 0 : (int)std::min<int64_t>(cut, 1ll << 30);    // |Y - X| < 2^30: a larger cut keeps no row either
    const int rc = dom_tracks(c, cut32, (int)res, (int)w, st);
    if (rc != CL_OK) {
        (void)hipStreamSynchronize(c->stream);                          // no copy to the stack may still be pending
        dom_release(c);
        return rc;
    }
    c->dm.st = st;
    *n_bins = st.n_bins; *bin0 = st.bmin; *n_kept = st.n_kept;
    return CL_OK;
}

extern "C" int cl_dom_get(cl_chrom* c, int64_t first, int64_t count, uint32_t* cross, uint32_t* up, uint32_t* down)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (!c->dm.st.ready) return fail(CL_ERR_ARG, "cl_dom_get: no tracks on this handle (cl_dom_tracks)");
    if (!range_ok(first, count, c->dm.st.n_bins)) return fail(CL_ERR_ARG, "cl_dom_get: range outside the bins");
    if (count > 0 && (!cross || !up || !down)) return fail(CL_ERR_ARG, "cl_dom_get: bad arguments");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_dom_get: asynchronous runs still in flight");
    if (count == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t stride = (size_t)c->dm.st.n_bins + 1;
    const u32* trk = c->dm.trk.as<u32>();
    const size_t nb = (size_t)count * 4;
    return read_back(c, "cl_dom_get", {{cross, trk + first, nb}, {up, trk + stride + first, nb}, {down, trk + 2 * stride + first, nb}});
}

static int dom_count(cl_chrom* c, const int64_t* starts, const int64_t* ends, long long n, uint32_t* intra, uint32_t* nx, uint32_t* ny)
{
    int rc;
    if ((rc = agg_table(c, c->dm.st.cut))) return rc;                      // (cl_agg_loops at another cut has rebuilt it for itself since)
    if (c->ag.kept != c->dm.st.n_kept) return fail(CL_ERR_HIP, "cl_dom_count: the sorted rows are not those of the tracks");
    const int m = c->ag.kept;
    const size_t sn = (size_t)n;
    if ((rc = c->dm.ivs.ensure(sn * 8)) || (rc = c->dm.ive.ensure(sn * 8)) || (rc = c->dm.cnt.ensure(3 * sn * 4))) return rc;
    HIP_TRY(hipMemcpyAsync(c->dm.ivs.p, starts, sn * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->dm.ive.p, ends, sn * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->dm.cnt.p, 0, 3 * sn * 4, c->stream));
    hipLaunchKernelGGL(k22_count, dim3((unsigned)(((long long)m + K22_TILE - 1) / K22_TILE)), dim3(TPB), 0, c->stream, c->ag.sx.as<u32>(),
                       c->ag.sy.as<int>(), m, c->dm.ivs.as<long long>(), c->dm.ive.as<long long>(), (int)n, c->dm.cnt.as<u32>());
    HIP_TRY(hipGetLastError());
    const u32* cnt = c->dm.cnt.as<u32>();
    HIP_TRY(hipMemcpyAsync(intra, cnt, sn * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(nx, cnt + sn, sn * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(ny, cnt + 2 * sn, sn * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CL_OK;
}

extern "C" int cl_dom_count(cl_chrom* c, const int64_t* starts, const int64_t* ends, int64_t n, uint32_t* intra, uint32_t* nx, uint32_t* ny)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n < 0 || n > (1ll << 31) - 4096 || (n > 0 && (!starts || !ends || !intra || !nx || !ny))) return fail(CL_ERR_ARG, "cl_dom_count: bad arguments");
    if (!c->dm.st.ready) return fail(CL_ERR_ARG, "cl_dom_count: no tracks on this handle (cl_dom_tracks)");
    for (int64_t k = 0; k < n; ++k)
        if (ends[k] < starts[k] || (k > 0 && starts[k] < ends[k - 1]))
            return fail(CL_ERR_ARG, "cl_dom_count: the intervals must be ascending and disjoint");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_dom_count: asynchronous runs still in flight");
    if (n == 0) return CL_OK;
    if (c->dm.st.n_kept == 0) {
        std::memset(intra, 0, (size_t)n * 4); std::memset(nx, 0, (size_t)n * 4); std::memset(ny, 0, (size_t)n * 4);
        return CL_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    const int rc = dom_count(c, starts, ends, n, intra, nx, ny);
    if (rc != CL_OK) (void)hipStreamSynchronize(c->stream);             // no copy from or to the caller's arrays may still be pending
    return rc;
}

extern "C" int cl_dom_free(cl_chrom* c) { return unit_free(c, "cl_dom_free", dom_release); }
