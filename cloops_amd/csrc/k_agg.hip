// k_agg.hip -- K19: aggregate pile-up of the PETs of a resident chromosome around loop centres (the APA of Rao et al. 2014) --
// the X-sorted table, kernels and C entry point.
#include "cl_chrom.h"

// ==========================================================================================
// K19: (2w + 1) x (2w + 1) bins of `res` bp around every loop centre, piled into one matrix
// ==========================================================================================
// Definitions: include/cloops_hip.h, cl_agg_loops.  The reference has nothing of the kind; every number here is an integer count
// that a few lines of numpy reproduce (tests/test_gpu_agg.py).
// Table: the rows that pass the cut, sorted by X with Y as payload (key = X + 2^30 as u32, rows that fail the cut sort to the end as
// ~0; one rocPRIM radix sort of pairs), built at the first call and kept with the handle, keyed by the cut (c->ag: scratch of its
// own, apart from the sweep's layouts, q index, count cache and K8 tables, freed with the handle).  K8's tables hold the same rows
// as 64-bit keys next to a Y-sorted copy, and exist only after cl_sig_counts / cl_quant_counts: they are neither read nor built here.
// Loops: the centres are sorted by cx ON THE DEVICE (rocPRIM pairs of (clamped cx, loop number); 10^5 loops take tens of
// microseconds, a host sort milliseconds), so that the workgroups running at one time read neighbouring X ranges (L2).
// Kernel: K19_GRID persistent workgroups, workgroup b takes loops b, b + grid, ... of that order.  Per loop: waves 0 / 1 find the two
// ends of [ox, ox + W res) in the sorted X by a 64-way search (one ballot per round: 4 dependent loads for 16 M rows instead of 24),
// the threads stride over that range with coalesced loads of (X, Y), test Y, bin with a multiply-shift division and count into W W
// int32 counters in LDS with LDS atomics (at most 41 x 41 x 4 B = 6.7 KB).  After a barrier every thread reads the cells it owns
// (cell c belongs to thread c % NT): the loop's matrix goes out if wanted, the six statistics are reduced through LDS, and the
// counts are added to the thread's 64-bit registers, which reach the global matrix once, when the workgroup is done: at most
// grid x W W global atomics per call instead of loops x W W.  Integer addition commutes, so neither S nor any per-loop value
// depends on how the loops are scheduled (tested by calling twice).  Only vector stores and ordinary HIP atomics.
// Form: NT = 256 (a workgroup per loop) in the shipped library; NT = 64 (a wave per loop, four times the workgroups) was measured
// against it in the developer build.
#define K19_WMAX 41                     // 2 * 20 + 1
#define K19_CELLS (K19_WMAX * K19_WMAX)
#define K19_GRID 2048                   // persistent workgroups of the 256-thread form: 8 per CU (32 waves, 8 x 8.5 KB of LDS)
#define K19_LIM (1 << 30)               // clamp of the centres: every coordinate of a handle satisfies |v| < 2^29 and W res < 2^29, so a
                                        // window whose centre lies at or beyond +-2^30 holds no row, and neither does its clamped twin
#define K19_NONE 0xffffffffu            // key of a row that fails the cut

struct K19Par {
    int res, w, W, WW, corner;
    u32 span;                           // W * res
    u32 magic; int sh1, sh2;            // v / res by multiply-shift (Granlund-Montgomery, exact for all u32)
};

__device__ __forceinline__ u32 k19_div(const K19Par& p, u32 v)
{
    const u32 t1 = __umulhi(p.magic, v);
    return (t1 + ((v - t1) >> p.sh1)) >> p.sh2;
}

__global__ void k19_split(const int* __restrict__ X, const int* __restrict__ Y, int n, int cut, u32* __restrict__ key, int* __restrict__ val)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int x = X[r], y = Y[r];
    key[r] = (cut <= 0 || (y - x) >= cut) ? (u32)(x + (1 << 30)) : K19_NONE;      // parseJd(f, cut), io.py:213-216
    val[r] = y;
}

// number of rows that pass the cut = lower bound of the sentinel in the sorted keys
__global__ void k19_count_valid(const u32* __restrict__ sx, int n, int* __restrict__ d_m)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int lo = 0, hi = n;
        while (lo < hi) { const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1); if (sx[mid] != K19_NONE) lo = mid + 1; else hi = mid; }
        d_m[0] = lo;
    }
}

__global__ void k19_loop_keys(const int* __restrict__ cx, int n_loops, int* __restrict__ key, u32* __restrict__ idx)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_loops) return;
    key[k] = max(-K19_LIM, min(K19_LIM, cx[k]));
    idx[k] = (u32)k;
}

// (k19_lb_wave: cl_chrom.h, shared with K24)
enum { K19_LL = 1, K19_UL = 2, K19_UR = 4, K19_LR = 8 };

template <int NT>
__global__ void __launch_bounds__(NT)
k19_pile(const u32* __restrict__ sx, const int* __restrict__ sy, int m, K19Par p, int n_loops, const u32* __restrict__ order,
         const int* __restrict__ cx, const int* __restrict__ cy, u64* __restrict__ S, int* __restrict__ stats, int* __restrict__ mats)
{
    constexpr int CPT = (K19_CELLS + NT - 1) / NT;          // cells a thread owns: c = tid + s NT
    __shared__ int cnt[K19_CELLS];
    __shared__ unsigned char cls[K19_CELLS];                // corner membership of every cell
    __shared__ int st[6];
    __shared__ int rng[2];
    const int tid = threadIdx.x, wv = tid >> 6;
    u64 acc[CPT];
#pragma unroll
    for (int s = 0; s < CPT; ++s) {
        acc[s] = 0;
        const int c = tid + s * NT;
        if (c < p.WW) {
            const int i = c / p.W, j = c - i * p.W;
            const bool top = i < p.corner, bot = i >= p.W - p.corner, left = j < p.corner, right = j >= p.W - p.corner;
            cls[c] = (unsigned char)((bot && left ? K19_LL : 0) | (top && left ? K19_UL : 0) | (top && right ? K19_UR : 0) | (bot && right ? K19_LR : 0));
            cnt[c] = 0;
        }
    }
    if (tid < 6) st[tid] = 0;
    __syncthreads();
    const int half = p.w * p.res + (p.res >> 1);            // < W res < 2^29
    const int centre = p.w * p.W + p.w;
    for (int k = blockIdx.x; k < n_loops; k += gridDim.x) {
        const u32 l = order[k];
        const int ox = max(-K19_LIM, min(K19_LIM, cx[l])) - half, oy = max(-K19_LIM, min(K19_LIM, cy[l])) - half;   // in (-2^30 - 2^29, 2^30]
        const long long tlo = (long long)ox + (1ll << 30);   // the window's first X as a key: in (-2^29, 2^31]
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if (NT == 64 || wv == s) {
                const long long t = tlo + (s ? (long long)p.span : 0);                    // < 2^31 + 2^29
                const int r = t <= 0 ? 0 : k19_lb_wave(sx, m, (u32)t);
                if ((tid & 63) == 0) rng[s] = r;
            }
        __syncthreads();
        const int b = rng[0], e = rng[1];
        for (int j = b + tid; j < e; j += NT) {
            const u32 dx = sx[j] - (u32)tlo;                 // in [0, span): the range was searched for it
            const u32 dy = (u32)sy[j] - (u32)oy;             // the true difference lies in (-2^31 + 2^29, 2^31): a negative one wraps beyond span
            if (dy < p.span && dx < p.span) atomicAdd(&cnt[(int)k19_div(p, dx) * p.W + (int)k19_div(p, dy)], 1);
        }
        __syncthreads();
        int part[5] = {0, 0, 0, 0, 0};                       // total, ll, ul, ur, lr of this thread's cells
#pragma unroll
        for (int s = 0; s < CPT; ++s) {
            const int c = tid + s * NT;
            if (c < p.WW) {
                const int v = cnt[c];
                if (mats) mats[(size_t)l * p.WW + c] = v;
                if (stats && c == centre) st[1] = v;
                if (v) {
                    cnt[c] = 0;
                    acc[s] += (u64)v;
                    const int f = cls[c];
                    part[0] += v;
                    part[1] += (f & K19_LL) ? v : 0; part[2] += (f & K19_UL) ? v : 0;
                    part[3] += (f & K19_UR) ? v : 0; part[4] += (f & K19_LR) ? v : 0;
                }
            }
        }
        if (stats) {                                         // (uniform)
            if (part[0]) atomicAdd(&st[0], part[0]);
#pragma unroll
            for (int q = 1; q < 5; ++q) if (part[q]) atomicAdd(&st[q + 1], part[q]);
            __syncthreads();
            if (tid < 6) { stats[(size_t)l * 6 + tid] = st[tid]; st[tid] = 0; }
            // (the next loop's two barriers stand between this reset and its adds; rng is rewritten only after every thread has
            // passed the barrier above, behind its last read of b / e)
        }
    }
#pragma unroll
    for (int s = 0; s < CPT; ++s) {
        const int c = tid + s * NT;
        if (c < p.WW && acc[s]) atomicAdd(&S[c], acc[s]);
    }
}

static bool k19_wave_form()
{
#ifdef CLOOPS_DEVEL
    // developer A/B of the two forms on one loop set (CLOOPS_K19_WAVE=1: a wave per loop)
    if (const char* e = getenv("CLOOPS_K19_WAVE")) return atoi(e) != 0;
#endif
    return false;
}

// the X-sorted table of (chromosome, cut) unless the handle holds it already; c->n > 0 (declared in cl_chrom.h: K22 shares it)
int agg_table(cl_chrom* c, int cut)
{
    if (c->ag.ready && c->ag.cut == cut) return CL_OK;
    c->ag.ready = false;
    const int n = (int)c->n;
    int rc;
    if ((rc = c->ag.kin.ensure((size_t)n * 4)) || (rc = c->ag.vin.ensure((size_t)n * 4)) || (rc = c->ag.sx.ensure((size_t)n * 4)) ||
        (rc = c->ag.sy.ensure((size_t)n * 4)) || (rc = c->ag.m.ensure(64))) return rc;
    LAUNCH(k19_split, n, c->d_x, c->d_y, n, cut, c->ag.kin.as<u32>(), c->ag.vin.as<int>());
    HIP_TRY(hipGetLastError());
    if ((rc = prim_run(c->ag.tmp, "radix_sort_pairs(agg table)", [&](void* tmp, size_t& bytes) {
            return rocprim::radix_sort_pairs<SortConfig>(tmp, bytes, c->ag.kin.as<u32>(), c->ag.sx.as<u32>(), c->ag.vin.as<int>(), c->ag.sy.as<int>(),
                                                         (size_t)n, 0, 32, c->stream);
        })))
        return rc;
    hipLaunchKernelGGL(k19_count_valid, dim3(1), dim3(64), 0, c->stream, c->ag.sx.as<u32>(), n, c->ag.m.as<int>());
    HIP_TRY(hipGetLastError());
    int hm = 0;
    HIP_TRY(hipMemcpyAsync(&hm, c->ag.m.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->ag.kept = hm; c->ag.cut = cut; c->ag.ready = true;
    return CL_OK;
}

// ---- K19 host entry point -----------------------------------------------------------------------
static int agg_loops(cl_chrom* c, const K19Par& p, int n_loops, const int32_t* cx, const int32_t* cy, int64_t* sum_out,
                     int32_t* stats_out, int32_t* mats_out)
{
    const size_t nl = (size_t)n_loops, ww = (size_t)p.WW;
    int rc;
    if ((rc = c->ag.cx.ensure(nl * 4)) || (rc = c->ag.cy.ensure(nl * 4)) || (rc = c->ag.lkin.ensure(nl * 4)) || (rc = c->ag.lkout.ensure(nl * 4)) ||
        (rc = c->ag.lvin.ensure(nl * 4)) || (rc = c->ag.order.ensure(nl * 4)) || (rc = c->ag.sum.ensure(ww * 8)) ||
        (stats_out && (rc = c->ag.stats.ensure(nl * 6 * 4))) || (mats_out && (rc = c->ag.mats.ensure(nl * ww * 4)))) return rc;
    HIP_TRY(hipMemcpyAsync(c->ag.cx.p, cx, nl * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->ag.cy.p, cy, nl * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->ag.sum.p, 0, ww * 8, c->stream));
    LAUNCH(k19_loop_keys, n_loops, c->ag.cx.as<int>(), n_loops, c->ag.lkin.as<int>(), c->ag.lvin.as<u32>());
    HIP_TRY(hipGetLastError());
    if ((rc = prim_run(c->ag.ltmp, "radix_sort_pairs(agg loops)", [&](void* tmp, size_t& bytes) {
            return rocprim::radix_sort_pairs<SortConfig>(tmp, bytes, c->ag.lkin.as<int>(), c->ag.lkout.as<int>(), c->ag.lvin.as<u32>(),
                                                         c->ag.order.as<u32>(), nl, 0, 32, c->stream);
        })))
        return rc;
    int* d_stats = stats_out ? c->ag.stats.as<int>() : nullptr;
    int* d_mats = mats_out ? c->ag.mats.as<int>() : nullptr;
    if (k19_wave_form())
        hipLaunchKernelGGL(k19_pile<64>, dim3(std::min(n_loops, 4 * K19_GRID)), dim3(64), 0, c->stream, c->ag.sx.as<u32>(), c->ag.sy.as<int>(), c->ag.kept,
                           p, n_loops, c->ag.order.as<u32>(), c->ag.cx.as<int>(), c->ag.cy.as<int>(), c->ag.sum.as<u64>(), d_stats, d_mats);
    else
        hipLaunchKernelGGL(k19_pile<256>, dim3(std::min(n_loops, K19_GRID)), dim3(256), 0, c->stream, c->ag.sx.as<u32>(), c->ag.sy.as<int>(), c->ag.kept,
                           p, n_loops, c->ag.order.as<u32>(), c->ag.cx.as<int>(), c->ag.cy.as<int>(), c->ag.sum.as<u64>(), d_stats, d_mats);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sum_out, c->ag.sum.p, ww * 8, hipMemcpyDeviceToHost, c->stream));
    if (stats_out) HIP_TRY(hipMemcpyAsync(stats_out, d_stats, nl * 6 * 4, hipMemcpyDeviceToHost, c->stream));
    if (mats_out) HIP_TRY(hipMemcpyAsync(mats_out, d_mats, nl * ww * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CL_OK;
}

extern "C" int cl_agg_loops(cl_chrom* c, int32_t cut, int32_t res, int32_t w, int32_t corner, int64_t n_loops, const int32_t* cx,
                            const int32_t* cy, int64_t* sum_out, int32_t* stats_out, int32_t* mats_out, int64_t* n_kept)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_kept) *n_kept = 0;
    if (!sum_out || n_loops < 0 || (n_loops > 0 && (!cx || !cy))) return fail(CL_ERR_ARG, "cl_agg_loops: bad arguments");
    if (res < 1 || w < 1 || w > 20 || corner < 1 || corner > w || (long long)(2 * w + 1) * res >= (1ll << 29))
        return fail(CL_ERR_ARG, "cl_agg_loops: needs res >= 1, 1 <= w <= 20, 1 <= corner <= w and (2 w + 1) res < 2^29");
    if (n_loops > INT_MAX - 1024) return fail(CL_ERR_ARG, "cl_agg_loops: more than 2^31 loops");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_agg_loops: asynchronous runs still in flight");
    K19Par p;
    p.res = res; p.w = w; p.W = 2 * w + 1; p.WW = p.W * p.W; p.corner = corner; p.span = (u32)p.W * (u32)res;
    {
        const unsigned d = (unsigned)res;
        int l = 0; while ((1ull << l) < d) ++l;                          // ceil(log2 d)
        p.magic = (u32)((((1ull << 32) * ((1ull << l) - d)) / d) + 1);
        p.sh1 = l < 1 ? l : 1; p.sh2 = l > 1 ? l - 1 : 0;
    }
    const auto zero_outputs = [&]() {                                // no row in any window: every count is 0
        std::memset(sum_out, 0, (size_t)p.WW * 8);
        if (stats_out && n_loops) std::memset(stats_out, 0, (size_t)n_loops * 6 * 4);
        if (mats_out && n_loops) std::memset(mats_out, 0, (size_t)n_loops * p.WW * 4);
    };
    if (c->n == 0) { zero_outputs(); return CL_OK; }
    HIP_TRY(hipSetDevice(c->device));
    int rc = agg_table(c, cut);
    if (rc == CL_OK) {
        if (n_kept) *n_kept = c->ag.kept;
        if (n_loops > 0 && c->ag.kept > 0) rc = agg_loops(c, p, (int)n_loops, cx, cy, sum_out, stats_out, mats_out);
        else zero_outputs();
    }
    if (rc != CL_OK) (void)hipStreamSynchronize(c->stream);          // no copy from cx / cy or to the outputs may still be pending
    return rc;
}
