// k_cover.hip -- K20: 1D coverage of the genome by the PET ends of a resident chromosome, as the runs of a bedGraph and their text,
// made on the device -- kernels and C entry points.
#include "cl_chrom.h"
#include "cl_text.h"
#include "cl_ends.h"

// ==========================================================================================
// K20: maximal runs of constant depth > 0 of the intervals the PET ends stand for
// ==========================================================================================
// Definitions: include/cloops_hip.h, cl_cov_build.  The reference has nothing of the kind; every number here is an integer that a
// few lines of numpy reproduce (tests/test_gpu_coverage.py).
// Units: window mode works on base pairs, an end point p standing for [max(0, p - ext), p + ext); bin mode works on bin numbers
// b = floor(p / res), standing for [b, b + 1), and multiplies every position by res when it writes a run.  Both are the interval
// [max(0, v - lo), v + hi) of a value v with (lo, hi) = (ext, ext) or (0, 1), so one set of kernels serves both.
//   k20_keys + radix sort     the end points of the rows that pass the cut as keys v - vmin, in any order (a workgroup reserves the
//                             slots of its 2048 rows with one atomic), then sorted over the bits in use: S, m = n_ends values
//   k20_breaks                depth(t) = ub(t + lo) - ub(t - hi) for t >= 0, ub(x) = #{v <= x}: a rank difference between two
//                             places of S.  The depth can only change at a start A = max(0, v - lo) or an end B = v + hi > 0, and
//                             both are monotone in v, so S is at once the sorted starts and the sorted ends.  The first element i
//                             of every group of equal v computes, for its A and for its B, the depth at t and at t - 1 from four
//                             ranks, two of which are i and the end of its group; the other two lie lo + hi further down (A) or up
//                             (B) in S and are found by a galloping search that starts where the last one ended.  An end B whose
//                             position is also some start (v' = B + lo is in S: ub(t + lo) > ub(t - 1 + lo)) leaves the position
//                             to that start, so equal positions of the two sides collapse into one break point wherever their
//                             elements lie.  A break point is a candidate with depth(t) != depth(t - 1); it opens a run if
//                             depth(t) > 0 and closes the run before it if depth(t - 1) > 0.  Per candidate: the two depths, and
//                             the number of candidates of the OTHER side with a smaller position (again one of the four ranks).
//                             Keys are staged in LDS, the tile's K20_TILE elements and K20_HALO on either side; a search that leaves
//                             that window (dense data, a wide ext, all points equal) reads global memory instead -- one accessor,
//                             so the result does not depend on whether the window fits.
//   exclusive scan            of the "opens a run" flags, starts' flags first, ends' flags behind them: F
//   k20_runs                  the break point of side A at element i has F[i] + (FB[xr] - FB[0]) runs opening before it, the other
//                             side likewise: that is the index r of the run it opens, and r - 1 the run it closes.  Neighbouring
//                             runs differ in depth or do not abut by construction: between two break points the depth is constant
//   k20_area                  sum of depth * (end - start) over the runs
// Text (cl_cov_text / chunks / render) follows K14: line lengths, their running sum, K14's bounds kernel, a render of 256 lines per
// workgroup through LDS with 16-byte stores.  Only vector stores and ordinary HIP atomics.
// Scratch (c->cv) is the handle's own, apart from the sweep's layouts, q index, count cache and the K8 / K13 / K14 / K19 state.
#define K20_TILE 1024                   // elements of S per workgroup of k20_breaks (4 per thread)
#define K20_HALO 1024                   // elements staged in LDS on either side of the tile
#define K20_T 256                       // lines per render tile (one per lane)
#define K20_POS 10                      // longest position: 2^30
#define K20_VAL 20                      // longest value: depth < 2^32 as it is, or (depth * 2^30 + den / 2) / den < 2^62 with ".ddd"

struct K20Par {
    int lo, hi;                         // the interval of a value v is [max(0, v - lo), v + hi)
    int mul;                            // positions are multiplied by it when a run is written (bin mode: res)
    int vmin;                           // value of key 0
};

// per element i of S: the candidate of its start (slot i) and of its end (slot m + i): depth at the position, depth one base below
// it, candidates of the other side below it; zeros for an element that is not the first of its group or whose candidate is void
__global__ void __launch_bounds__(TPB)
k20_breaks(const u32* __restrict__ skey, int m, K20Par p, u32* __restrict__ dcur, u32* __restrict__ dprev, u32* __restrict__ xr,
           u32* __restrict__ flag, u64* __restrict__ ctr)
{
    __shared__ u32 win[K20_TILE + 2 * K20_HALO];
    const long long t0 = (long long)blockIdx.x * K20_TILE;
    K20Keys S;
    S.g = skey; S.l = win; S.vmin = p.vmin;
    S.base = (int)(t0 > K20_HALO ? t0 - K20_HALO : 0);
    const long long wend = t0 + K20_TILE + K20_HALO < m ? t0 + K20_TILE + K20_HALO : m;
    S.span = (int)(wend - S.base);
    for (int k = threadIdx.x; k < S.span; k += TPB) win[k] = skey[S.base + k];
    __syncthreads();
    u32 dmax = 0;
#pragma unroll
    for (int u = 0; u < K20_TILE / TPB; ++u) {
        const long long il = t0 + u * TPB + threadIdx.x;
        if (il >= m) break;
        const int i = (int)il;
        const int v = S.at(i);
        u32 ac = 0, ap = 0, ax = 0, bc = 0, bp = 0, bx = 0;
        if (i == 0 || S.at(i - 1) != v) {
            const int ge = k20_ub_up(S, m, i + 1, v);                    // ub(v): the end of the group
            if (v + p.hi > 0) {                                          // the end t = v + hi: ub(t - hi) = ge, ub(t - 1 - hi) = i
                const int r3 = k20_ub_up(S, m, ge, v + p.hi + p.lo - 1); // ub(t - 1 + lo)
                const int r1 = k20_ub_up(S, m, r3, v + p.hi + p.lo);     // ub(t + lo)
                if (r1 == r3) { bc = (u32)(r1 - ge); bp = (u32)(r3 - i); bx = (u32)r3; }   // (else a start stands at t and speaks for it)
            }
            if (v - p.lo > 0) {                                          // the start t = v - lo: ub(t + lo) = ge, ub(t - 1 + lo) = i
                const int r2 = k20_ub_down(S, i, v - p.lo - p.hi);       // ub(t - hi)
                const int r4 = k20_ub_down(S, r2, v - p.lo - p.hi - 1);  // ub(t - 1 - hi)
                ac = (u32)(ge - r2); ap = (u32)(i - r4); ax = (u32)r4;
            } else if (i == 0) {                                         // the clamped starts: t = 0, nothing lies below it
                const int r1 = k20_ub_up(S, m, ge, p.lo);
                const int r2 = k20_ub_up(S, m, 0, -p.hi);
                ac = (u32)(r1 - r2);
            }
        }
        dcur[i] = ac; dprev[i] = ap; xr[i] = ax; flag[i] = (ac != ap && ac > 0) ? 1u : 0u;
        dcur[(size_t)m + i] = bc; dprev[(size_t)m + i] = bp; xr[(size_t)m + i] = bx; flag[(size_t)m + i] = (bc != bp && bc > 0) ? 1u : 0u;
        dmax = max(dmax, max(ac, bc));
    }
    for (int o = 32; o > 0; o >>= 1) dmax = max(dmax, (u32)__shfl_xor((int)dmax, o));
    if ((threadIdx.x & 63) == 0 && dmax) atomicMax(&ctr[K20_MAXD], (u64)dmax);
}

// every break point writes the start and depth of the run it opens and the end of the run it closes; F: the exclusive scan of
// the 2 m flags (+ the total at F[2 m]); R = F[2 m]
__global__ void __launch_bounds__(TPB)
k20_runs(const u32* __restrict__ skey, int m, K20Par p, const u32* __restrict__ dcur, const u32* __restrict__ dprev,
         const u32* __restrict__ xr, const u32* __restrict__ F, long long R, int* __restrict__ start, int* __restrict__ end,
         u32* __restrict__ depth)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= 2ll * m) return;
    const u32 dc = dcur[k], dp = dprev[k];
    if (dc == dp) return;
    const int side = k >= m ? 1 : 0;
    const int i = (int)(k - (side ? m : 0));
    const int v = (int)skey[i] + p.vmin;
    const int t = side ? v + p.hi : (v - p.lo > 0 ? v - p.lo : 0);
    const u32 fb0 = F[m], x = xr[k];
    const long long r = side ? (long long)(F[k] - fb0) + F[x] : (long long)F[k] + (F[(size_t)m + x] - fb0);
    const int pos = t * p.mul;
    if (dc > 0 && r < R) { start[r] = pos; depth[r] = dc; }
    if (dp > 0 && r >= 1 && r <= R) end[r - 1] = pos;
}

__global__ void __launch_bounds__(TPB)
k20_area(const int* __restrict__ start, const int* __restrict__ end, const u32* __restrict__ depth, long long R, u64* __restrict__ ctr)
{
    u64 a = 0;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < R; j += (long long)gridDim.x * blockDim.x)
        a += (u64)depth[j] * (u64)(end[j] - start[j]);
    for (int o = 32; o > 0; o >>= 1) a += (u64)__shfl_xor((long long)a, o);
    if ((threadIdx.x & 63) == 0 && a) atomicAdd(&ctr[K20_AREA], a);
}

// ---- text ----------------------------------------------------------------------------------------
struct K20Tpl {
    const int* __restrict__ start;
    const int* __restrict__ end;
    const u32* __restrict__ depth;
    const char* __restrict__ name;
    u64 num, den;                       // den == 0: the depth as it is
    int la;
};

__device__ __forceinline__ u64 k20_fixed(const K20Tpl& t, u32 d) { return ((u64)d * t.num + t.den / 2) / t.den; }   // thousandths

__global__ void __launch_bounds__(TPB)
k20_lens(K20Tpl t, long long R, long long* __restrict__ len)
{
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < R; j += (long long)gridDim.x * blockDim.x) {
        const u32 d = t.depth[j];
        const int vw = t.den ? cl_ndig(k20_fixed(t, d) / 1000) + 4 : cl_ndig(d);
        len[j] = t.la + 4 + cl_ndig((u64)t.start[j]) + cl_ndig((u64)t.end[j]) + vw;    // name\tstart\tend\tvalue\n
    }
}

// lines [r0, r1) of the text (byte b0 = the start of line r0) -> out[0 ..); K20_T lines per workgroup, staged in LDS as in k14_render
__global__ void __launch_bounds__(K20_T)
k20_render(K20Tpl t, long long r0, long long r1, long long b0, const long long* __restrict__ lend, char* __restrict__ out)
{
    extern __shared__ uint4 k20_lds[];
    __shared__ char nm[CL_TRACK_NAME_MAX];
    char* buf = (char*)k20_lds;
    for (int k = threadIdx.x; k < CL_TRACK_NAME_MAX; k += blockDim.x) nm[k] = t.name[k];
    const TextTile tile = text_tile(lend, r0, r1, b0, K20_T);
    __syncthreads();
    const long long j = tile.q0 + threadIdx.x;
    if (j < tile.q1) {
        int pos = (int)((j > 0 ? lend[j - 1] : 0) - b0 - tile.a0);
        for (int k = 0; k < t.la; ++k) buf[pos + k] = nm[k];
        pos += t.la; buf[pos++] = '\t';
        pos = cl_put(buf, pos, t.start[j]); buf[pos++] = '\t';
        pos = cl_put(buf, pos, t.end[j]); buf[pos++] = '\t';
        const u32 d = t.depth[j];
        if (t.den) {
            const u64 q = k20_fixed(t, d);
            const u64 whole = q / 1000;
            u32 frac = (u32)(q - whole * 1000);
            pos = cl_put(buf, pos, (long long)whole); buf[pos++] = '.';
            buf[pos + 2] = (char)('0' + frac % 10); frac /= 10;
            buf[pos + 1] = (char)('0' + frac % 10); frac /= 10;
            buf[pos] = (char)('0' + frac);
            pos += 3;
        } else {
            pos = cl_put(buf, pos, (long long)d);
        }
        buf[pos++] = '\n';
    }
    __syncthreads();
    text_flush(out, k20_lds, tile.g0, tile.g1, tile.a0);
}

// ---- K20 host side ------------------------------------------------------------------------------
static int k20_lcap(const cl_chrom* c) { return c->cv.st.la + 4 + 2 * K20_POS + K20_VAL; }   // longest line the template allows

static int k20_grid(long long work) { return (int)std::max(1ll, std::min<long long>(4096, (work + TPB - 1) / TPB)); }

static K20Tpl k20_tpl(cl_chrom* c)
{
    K20Tpl t;
    t.start = c->cv.start.as<int>(); t.end = c->cv.end.as<int>(); t.depth = c->cv.depth.as<u32>();
    t.name = c->cv.name.as<char>();
    t.num = (u64)c->cv.st.num; t.den = (u64)c->cv.st.den; t.la = c->cv.st.la;
    return t;
}

static int cov_build(cl_chrom* c, long long cut, int ends, int ext, int res, int64_t* n_runs, uint32_t* max_depth, int64_t* n_ends,
                     int64_t* area)
{
    const int n = (int)c->n;
    const int ne = (ends & 1) + ((ends >> 1) & 1);
    if ((long long)n * ne > K20_LIMIT) return fail(CL_ERR_ARG, "cl_cov_build: more than 2^31 - 4096 end points");
    K20Par p;
    const int pmin = std::min(c->st.xmin, c->st.ymin), pmax = std::max(c->st.xmax, c->st.ymax);
    const auto fdiv = [](int a, int b) { const int q = a / b; return q - ((a % b) < 0 ? 1 : 0); };
    p.lo = res ? 0 : ext; p.hi = res ? 1 : ext; p.mul = res ? res : 1;
    p.vmin = res ? fdiv(pmin, res) : pmin;
    const int vmax = res ? fdiv(pmax, res) : pmax;
    const int ebit = std::max(1, bits_for((u32)(vmax - p.vmin)));
    int rc;
    if ((rc = c->cv.ctr.ensure(K20_CTRS * 8)) || (rc = c->cv.kin.ensure((size_t)n * ne * 4)) || (rc = c->cv.key.ensure((size_t)n * ne * 4))) return rc;
    u64* ctr = c->cv.ctr.as<u64>();
    HIP_TRY(hipMemsetAsync(ctr, 0, K20_CTRS * 8, c->stream));
    hipLaunchKernelGGL(k20_keys, dim3((unsigned)(((long long)n + K20_ROWS - 1) / K20_ROWS)), dim3(TPB), 0, c->stream, c->d_x, c->d_y, n, cut, ends,
                       res, p.vmin, c->cv.kin.as<u32>(), ctr);
    HIP_TRY(hipGetLastError());
    u64 hctr[K20_CTRS] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(hctr, ctr, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const long long m = (long long)hctr[K20_NENDS];
    *n_ends = m;
    if (m == 0) { c->cv.st.built = true; return CL_OK; }
    if (m > (long long)n * ne) return fail(CL_ERR_HIP, "cl_cov_build: the key pass counted more end points than rows allow");
    // S: the end points in ascending order, sorted over the bits in use
    if ((rc = prim_run(c->cv.tmp, "radix_sort_keys(coverage)", [&](void* tmp, size_t& bytes) {
            return rocprim::radix_sort_keys(tmp, bytes, c->cv.kin.as<u32>(), c->cv.key.as<u32>(), (size_t)m, 0, ebit, c->stream);
        })))
        return rc;
    // candidates, flags, their scan
    const size_t m2 = 2 * (size_t)m;
    if ((rc = c->cv.dcur.ensure(m2 * 4)) || (rc = c->cv.dprev.ensure(m2 * 4)) || (rc = c->cv.xr.ensure(m2 * 4)) ||
        (rc = c->cv.flag.ensure((m2 + 1) * 4)) || (rc = c->cv.scan.ensure((m2 + 1) * 4)))
        return rc;
    HIP_TRY(hipMemsetAsync(c->cv.flag.as<u32>() + m2, 0, 4, c->stream));
    hipLaunchKernelGGL(k20_breaks, dim3((unsigned)((m + K20_TILE - 1) / K20_TILE)), dim3(TPB), 0, c->stream, c->cv.key.as<u32>(), (int)m, p,
                       c->cv.dcur.as<u32>(), c->cv.dprev.as<u32>(), c->cv.xr.as<u32>(), c->cv.flag.as<u32>(), ctr);
    HIP_TRY(hipGetLastError());
    if ((rc = prim_run(c->cv.tmp, "exclusive_scan(coverage)", [&](void* tmp, size_t& bytes) {
            return rocprim::exclusive_scan(tmp, bytes, c->cv.flag.as<u32>(), c->cv.scan.as<u32>(), 0u, m2 + 1, rocprim::plus<u32>(), c->stream);
        })))
        return rc;
    u32 hR = 0;
    HIP_TRY(hipMemcpyAsync(&hR, c->cv.scan.as<u32>() + m2, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&hctr[K20_MAXD], ctr + K20_MAXD, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const long long R = hR;
    if (R > 0) {
        if ((rc = c->cv.start.ensure((size_t)R * 4)) || (rc = c->cv.end.ensure((size_t)R * 4)) || (rc = c->cv.depth.ensure((size_t)R * 4))) return rc;
        hipLaunchKernelGGL(k20_runs, dim3((unsigned)((m2 + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, c->cv.key.as<u32>(), (int)m, p,
                           c->cv.dcur.as<u32>(), c->cv.dprev.as<u32>(), c->cv.xr.as<u32>(), c->cv.scan.as<u32>(), R, c->cv.start.as<int>(),
                           c->cv.end.as<int>(), c->cv.depth.as<u32>());
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k20_area, dim3(k20_grid(R)), dim3(TPB), 0, c->stream, c->cv.start.as<int>(), c->cv.end.as<int>(), c->cv.depth.as<u32>(), R, ctr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&hctr[K20_AREA], ctr + K20_AREA, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->cv.st.R = R;
    c->cv.st.built = true;
    *n_runs = R;
    *max_depth = (uint32_t)hctr[K20_MAXD];
    *area = (int64_t)hctr[K20_AREA];
    return CL_OK;
}

extern "C" int cl_cov_build(cl_chrom* c, int64_t cut, int32_t ends, int64_t ext, int64_t res, int64_t* n_runs, uint32_t* max_depth,
                            int64_t* n_ends, int64_t* area)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_runs) *n_runs = 0;
    if (max_depth) *max_depth = 0;
    if (n_ends) *n_ends = 0;
    if (area) *area = 0;
    if (!n_runs || !max_depth || !n_ends || !area) return fail(CL_ERR_ARG, "cl_cov_build: bad arguments");
    if (ends < 1 || ends > 3) return fail(CL_ERR_ARG, "cl_cov_build: ends outside 1..3");
    if (res < 0 || res >= (1ll << 29)) return fail(CL_ERR_ARG, "cl_cov_build: res outside [0, 2^29)");
    if (res > 0 && ext != 0) return fail(CL_ERR_ARG, "cl_cov_build: bin mode (res >= 1) takes ext = 0");
    if (res == 0 && (ext < 1 || ext >= (1ll << 29))) return fail(CL_ERR_ARG, "cl_cov_build: window mode (res = 0) needs 1 <= ext < 2^29");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_cov_build: asynchronous runs still in flight");
    HIP_TRY(hipSetDevice(c->device));
    c->cv.st = cl_chrom::Cov::State();                                      // (the buffers stay: the next build reuses their memory, not their content)
    text_reset(c->cv.txt);
    if (c->n == 0) { c->cv.st.built = true; return CL_OK; }
    const int rc = cov_build(c, cut, ends, (int)ext, (int)res, n_runs, max_depth, n_ends, area);
    if (rc != CL_OK) {
        (void)hipStreamSynchronize(c->stream);                          // no copy to the stack may still be pending
        cov_release(c);
    }
    return rc;
}

extern "C" int cl_cov_runs(cl_chrom* c, int64_t first, int64_t count, int32_t* start_out, int32_t* end_out, uint32_t* depth_out)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (!c->cv.st.built) return fail(CL_ERR_ARG, "cl_cov_runs: no coverage built on this handle");
    if (!range_ok(first, count, c->cv.st.R)) return fail(CL_ERR_ARG, "cl_cov_runs: range outside the runs");
    if (count > 0 && (!start_out || !end_out || !depth_out)) return fail(CL_ERR_ARG, "cl_cov_runs: bad arguments");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_cov_runs: asynchronous runs still in flight");
    if (count == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    return read_back(c, "cl_cov_runs", {{start_out, c->cv.start.as<int>() + first, (size_t)count * 4},
                                        {end_out, c->cv.end.as<int>() + first, (size_t)count * 4},
                                        {depth_out, c->cv.depth.as<u32>() + first, (size_t)count * 4}});
}

static int cov_text(cl_chrom* c, std::vector<char>& hn, int64_t* n_bytes)
{
    cl_chrom::Cov::State& s = c->cv.st;
    const long long R = s.R;
    int rc;
    TextOut& txt = c->cv.txt;
    if ((rc = c->cv.name.ensure(CL_TRACK_NAME_MAX)) || (rc = txt.len.ensure((size_t)R * 8)) || (rc = txt.end.ensure((size_t)R * 8))) return rc;
    HIP_TRY(hipMemcpyAsync(c->cv.name.p, hn.data(), CL_TRACK_NAME_MAX, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k20_lens, dim3(k20_grid(R)), dim3(TPB), 0, c->stream, k20_tpl(c), R, txt.len.as<long long>());
    HIP_TRY(hipGetLastError());
    if ((rc = text_scan(txt, c->cv.tmp, R, c->stream)) || (rc = text_total(txt, R, c->stream))) return rc;
    s.text = true;
    *n_bytes = txt.total;
    return CL_OK;
}

extern "C" int cl_cov_text(cl_chrom* c, const char* name, int64_t scale_num, int64_t scale_den, int64_t* n_bytes)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_bytes) *n_bytes = 0;
    if (!name || !n_bytes) return fail(CL_ERR_ARG, "cl_cov_text: bad arguments");
    if (!c->cv.st.built) return fail(CL_ERR_ARG, "cl_cov_text: no coverage built on this handle");
    const size_t la = strlen(name);
    if (la > CL_TRACK_NAME_MAX) return fail(CL_ERR_ARG, "cl_cov_text: chromosome name longer than CL_TRACK_NAME_MAX");
    if (scale_den < 0 || scale_num < 0 || scale_num > (1ll << 30) || (scale_den > 0 && scale_num < 1))
        return fail(CL_ERR_ARG, "cl_cov_text: needs scale_den >= 0 and 1 <= scale_num <= 2^30 (0 allowed with scale_den = 0)");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_cov_text: asynchronous runs still in flight");
    cl_chrom::Cov::State& s = c->cv.st;
    s.text = false;
    text_reset(c->cv.txt);
    s.la = (int)la; s.num = scale_num; s.den = scale_den;
    if (s.R == 0) { s.text = true; return CL_OK; }
    HIP_TRY(hipSetDevice(c->device));
    std::vector<char> hn(CL_TRACK_NAME_MAX, 0);
    std::memcpy(hn.data(), name, la);
    const int rc = cov_text(c, hn, n_bytes);
    if (rc != CL_OK) (void)hipStreamSynchronize(c->stream);            // no copy from hn may still be pending
    return rc;
}

extern "C" int cl_cov_chunks(cl_chrom* c, int64_t budget, int64_t cap, int64_t* run_bounds, int64_t* byte_bounds, int64_t* n_chunks)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_chunks) *n_chunks = 0;
    if (!n_chunks || (!run_bounds) != (!byte_bounds)) return fail(CL_ERR_ARG, "cl_cov_chunks: bad arguments");
    if (!c->cv.st.built || !c->cv.st.text) return fail(CL_ERR_ARG, "cl_cov_chunks: no coverage text on this handle (cl_cov_build, cl_cov_text)");
    if (budget < k20_lcap(c)) return fail(CL_ERR_ARG, "cl_cov_chunks: budget below the longest line the template allows");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_cov_chunks: asynchronous runs still in flight");
    if (c->cv.txt.R > 0) HIP_TRY(hipSetDevice(c->device));
    return text_chunks(c->cv.txt, c->stream, budget, k20_lcap(c), cap, run_bounds, byte_bounds, n_chunks, "cl_cov_chunks");
}

extern "C" int cl_cov_render(cl_chrom* c, int64_t chunk, char* out, int64_t cap, int64_t* n_bytes)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_bytes) *n_bytes = 0;
    if (!out || !n_bytes) return fail(CL_ERR_ARG, "cl_cov_render: bad arguments");
    cl_chrom::Cov::State& s = c->cv.st;
    TextOut& txt = c->cv.txt;
    if (!s.built || !s.text || txt.crec.empty()) return fail(CL_ERR_ARG, "cl_cov_render: no chunks made on this handle (cl_cov_chunks)");
    if (chunk < 0 || chunk + 1 >= (int64_t)txt.crec.size()) return fail(CL_ERR_ARG, "cl_cov_render: chunk index out of range");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_cov_render: asynchronous runs still in flight");
    const TextChunk k = text_chunk(txt, chunk);
    if (cap < k.nb) return fail(CL_ERR_ARG, "cl_cov_render: capacity below the chunk's bytes");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = text_reserve(txt, k.nb))) return rc;
    const long long tiles = (k.r1 - k.r0 + K20_T - 1) / K20_T;
    const size_t lds = (((size_t)K20_T * k20_lcap(c) + 16 + 15) / 16) * 16;   // the span plus the shift of its first word
    hipLaunchKernelGGL(k20_render, dim3((unsigned)tiles), dim3(K20_T), lds, c->stream, k20_tpl(c), k.r0, k.r1, k.b0, txt.end.as<long long>(),
                       txt.out.as<char>());
    HIP_TRY(hipGetLastError());
    if ((rc = text_copy_out(txt, c->stream, out, k.nb, "cl_cov_render"))) return rc;
    *n_bytes = k.nb;
    return CL_OK;
}

extern "C" int cl_cov_free(cl_chrom* c) { return unit_free(c, "cl_cov_free", cov_release); }
