// k_track.hip -- K14: browser-track text of the PETs of a resident chromosome (cLoops/io.py jd2washU / jd2hic) rendered on the
// device -- kernels and C entry points.
#define CL_TEXTOUT_KERNELS                // k14_bounds is defined in this unit
#include "cl_chrom.h"
#include "cl_text.h"

// ==========================================================================================
// K14: PET lines for the washU long-range track and for `juicer_tools pre` (cLoops/io.py:206-217, :292-348)
// ==========================================================================================
// The reference loops over every PET in Python, writes two text lines per PET for washU (one per end) or one for juicer, and lets
// `bedtools sort` order the washU text.  Here the rows stay in HBM and the text is made on the device, in four steps at build time
// and one per chunk:
//   k14_count / k14_compact   the rows passing parseJd's cut (Y - X >= cut if cut > 0), in row order (a count per 2048-row tile,
//                             an exclusive scan of the counts, a ballot-ranked write of every tile's rows)
//   k14_keys + radix sort     washU only: record g = 2 i + side of kept row i, anchored at p = X (side 0) or Y (side 1), gets the
//                             key (p - pmin) << gbits | g.  start = max(0, p - ext) and end = p + ext are both monotone in p, so
//                             the key order is the pinned order (start, end, generation); only the bits in use are sorted
//   k14_len + inclusive scan  the byte length of every line (digits of its int64 fields + the template's literal bytes, names
//                             included) and their running sum: line j occupies [end[j - 1], end[j]) of the track's text
//   k14_bounds                chunks: chunk k holds the lines that START in [k S, (k + 1) S), S = budget - Lcap + 1, Lcap the
//                             longest line the template allows, so no chunk exceeds the budget and no line is split; the host
//                             drops empty chunks
//   k14_render                one chunk: every workgroup renders 256 consecutive lines into LDS (one line per lane), placed so
//                             that LDS and the output agree modulo 16, then writes the tile's byte span with 16-byte stores
//                             (byte stores only in the two words it shares with its neighbours)
// k14_bounds, the tile bounds and span flush of k14_render and the host side of the text (running sum, chunks, copy-out) are
// cl_textout.h's, shared with K20 and K15.
// Scratch (c->tk, the text in c->tk.txt) is the handle's own, apart from the sweep's layouts, q index, count cache and K8 tables:
// it lives from cl_track_build to the next build, cl_track_free or the handle's destruction.
#define K14_ITEMS 8                     // rows per thread of the filter passes
#define K14_ROWS (TPB * K14_ITEMS)      // rows per tile: 2048
#define K14_T 256                       // lines per render tile (one per lane)
#define K14_NAME_MAX CL_TRACK_NAME_MAX  // bytes of a chromosome name
#define K14_FIELD 20                    // longest decimal int64: "-9223372036854775808"

struct K14Tpl {
    const u32* __restrict__ krow;       // kept rows, ascending
    const u64* __restrict__ keys;       // washU: sorted keys (record order); juice: unused (record j = kept row j)
    const int* __restrict__ X;
    const int* __restrict__ Y;
    const long long* __restrict__ ids;  // NULL: the ids are the row numbers
    const char* __restrict__ names;     // name a at 0, name b at K14_NAME_MAX
    long long ext;
    u64 gmask;                          // washU: generation bits of a key
    int kind, la, lb;
};

__device__ __forceinline__ bool k14_keep(int x, int y, long long cut)
{
    return cut <= 0 || (long long)y - (long long)x >= cut;              // parseJd(f, cut), cLoops/io.py:213-216
}

__device__ __forceinline__ int k14_lane_rank(u64 mask)                 // set bits of `mask` below this lane
{
    return __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
}

__device__ __forceinline__ int k14_str(char* s, int pos, const char* t, int len)
{
    for (int k = 0; k < len; ++k) s[pos + k] = t[k];
    return pos + len;
}

__device__ __forceinline__ long long k14_add(long long a, long long b) { return (long long)((u64)a + (u64)b); }   // numpy int64 wraps
__device__ __forceinline__ long long k14_sub(long long a, long long b) { return (long long)((u64)a - (u64)b); }

struct K14F { long long f0, f1, f2, f3, f4; };                   // the int64 fields of a line (no array: it would live in scratch)

// the fields of record j: washU (start, end, partner start, partner end, id) and its side; juice (X, Y)
template <int KIND>
__device__ __forceinline__ void k14_fields(const K14Tpl& t, long long j, K14F& f, int& side)
{
    if (KIND == CL_TRACK_WASHU) {
        const u64 g = t.keys[j] & t.gmask;
        side = (int)(g & 1);
        const u32 row = t.krow[g >> 1];
        const long long x = t.X[row], y = t.Y[row];
        const long long sw = (x ^ y) & -(long long)side;               // side 1 swaps the ends
        const long long p = x ^ sw, q = y ^ sw;
        const long long s = k14_sub(p, t.ext), ps = k14_sub(q, t.ext);
        f.f0 = s > 0 ? s : 0; f.f1 = k14_add(p, t.ext);                 // max([0, t[1] - ext]), t[1] + ext (io.py:307-308)
        f.f2 = ps > 0 ? ps : 0; f.f3 = k14_add(q, t.ext);
        f.f4 = t.ids ? t.ids[row] : (long long)row;
    } else {
        side = 0;
        const u32 row = t.krow[j];
        f.f0 = t.X[row]; f.f1 = t.Y[row]; f.f2 = f.f3 = f.f4 = 0;
    }
}

template <int KIND>
__device__ __forceinline__ int k14_len(const K14Tpl& t, const K14F& f)
{
    if (KIND == CL_TRACK_WASHU)                                       // a\ts\te\tb:ps-pe,1\tid\t.\n
        return t.la + t.lb + 11 + cl_width(f.f0) + cl_width(f.f1) + cl_width(f.f2) + cl_width(f.f3) + cl_width(f.f4);
    return t.la + t.lb + 12 + cl_width(f.f0) + cl_width(f.f1);       // 0\ta\tX\t0\t1\tb\tY\t1\n
}

__global__ void __launch_bounds__(TPB)
k14_count(const int* __restrict__ X, const int* __restrict__ Y, int n, long long cut, u32* __restrict__ tcnt)
{
    __shared__ int wc[TPB / 64];
    const long long t0 = (long long)blockIdx.x * K14_ROWS;
    int cnt = 0;
#pragma unroll
    for (int u = 0; u < K14_ITEMS; ++u) {
        const long long r = t0 + u * TPB + threadIdx.x;
        if (r < n && k14_keep(X[r], Y[r], cut)) ++cnt;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tcnt[blockIdx.x] = (u32)(wc[0] + wc[1] + wc[2] + wc[3]);
}

// the kept rows of every tile at toff[tile] onwards, ascending: rows of a tile are ordered (u, lane of the workgroup)
__global__ void __launch_bounds__(TPB)
k14_compact(const int* __restrict__ X, const int* __restrict__ Y, int n, long long cut, const u32* __restrict__ toff,
            u32* __restrict__ krow)
{
    __shared__ u32 pre[K14_ITEMS * (TPB / 64)];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long t0 = (long long)blockIdx.x * K14_ROWS;
    u64 bal[K14_ITEMS];
#pragma unroll
    for (int u = 0; u < K14_ITEMS; ++u) {
        const long long r = t0 + u * TPB + threadIdx.x;
        bal[u] = __ballot(r < n && k14_keep(X[r], Y[r], cut));
        if (lane == 0) pre[u * (TPB / 64) + w] = (u32)__popcll(bal[u]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 s = toff[blockIdx.x];
        for (int k = 0; k < K14_ITEMS * (TPB / 64); ++k) { const u32 v = pre[k]; pre[k] = s; s += v; }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < K14_ITEMS; ++u)
        if ((bal[u] >> lane) & 1)
            krow[pre[u * (TPB / 64) + w] + (u32)k14_lane_rank(bal[u])] = (u32)(t0 + u * TPB + threadIdx.x);
}

__global__ void __launch_bounds__(TPB)
k14_keys(const u32* __restrict__ krow, long long m, const int* __restrict__ X, const int* __restrict__ Y, int pmin, int gbits,
         u64* __restrict__ keys)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) {
        const u32 row = krow[i];
        keys[2 * i] = ((u64)(u32)(X[row] - pmin) << gbits) | (u64)(2 * i);
        keys[2 * i + 1] = ((u64)(u32)(Y[row] - pmin) << gbits) | (u64)(2 * i + 1);
    }
}

template <int KIND>
__global__ void __launch_bounds__(TPB)
k14_lens(K14Tpl t, long long R, long long* __restrict__ len)
{
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < R; j += (long long)gridDim.x * blockDim.x) {
        K14F f;
        int side;
        k14_fields<KIND>(t, j, f, side);
        len[j] = k14_len<KIND>(t, f);
    }
}

// lines [r0, r1) of the track (byte b0 = the start of line r0) -> out[0 ..); K14_T lines per workgroup, staged in LDS
template <int KIND>
__global__ void __launch_bounds__(K14_T)
k14_render(K14Tpl t, long long r0, long long r1, long long b0, const long long* __restrict__ end, char* __restrict__ out)
{
    extern __shared__ uint4 k14_lds[];
    __shared__ char nm[2 * K14_NAME_MAX];
    char* buf = (char*)k14_lds;
    for (int k = threadIdx.x; k < 2 * K14_NAME_MAX; k += blockDim.x) nm[k] = t.names[k];
    const TextTile tile = text_tile(end, r0, r1, b0, K14_T);
    __syncthreads();
    const long long j = tile.q0 + threadIdx.x;
    if (j < tile.q1) {
        K14F f;
        int side;
        k14_fields<KIND>(t, j, f, side);
        int p = (int)((j > 0 ? end[j - 1] : 0) - b0 - tile.a0);
        if (KIND == CL_TRACK_WASHU) {
            const char* own = side ? nm + K14_NAME_MAX : nm;
            const char* par = side ? nm : nm + K14_NAME_MAX;
            const int lo = side ? t.lb : t.la, lp = side ? t.la : t.lb;
            p = k14_str(buf, p, own, lo); buf[p++] = '\t';
            p = cl_put(buf, p, f.f0); buf[p++] = '\t';
            p = cl_put(buf, p, f.f1); buf[p++] = '\t';
            p = k14_str(buf, p, par, lp); buf[p++] = ':';
            p = cl_put(buf, p, f.f2); buf[p++] = '-';
            p = cl_put(buf, p, f.f3); buf[p++] = ','; buf[p++] = '1'; buf[p++] = '\t';
            p = cl_put(buf, p, f.f4); buf[p++] = '\t'; buf[p++] = '.'; buf[p++] = '\n';
        } else {
            buf[p++] = '0'; buf[p++] = '\t';
            p = k14_str(buf, p, nm, t.la); buf[p++] = '\t';
            p = cl_put(buf, p, f.f0);
            buf[p++] = '\t'; buf[p++] = '0'; buf[p++] = '\t'; buf[p++] = '1'; buf[p++] = '\t';
            p = k14_str(buf, p, nm + K14_NAME_MAX, t.lb); buf[p++] = '\t';
            p = cl_put(buf, p, f.f1);
            buf[p++] = '\t'; buf[p++] = '1'; buf[p++] = '\n';
        }
    }
    __syncthreads();
    text_flush(out, k14_lds, tile.g0, tile.g1, tile.a0);
}

// ---- K14 host side ------------------------------------------------------------------------------
static int k14_lcap(const cl_chrom* c)                                   // longest line the template allows
{
    return c->tk.st.la + c->tk.st.lb + (c->tk.st.kind == CL_TRACK_WASHU ? 11 + 5 * K14_FIELD : 12 + 2 * K14_FIELD);
}

static K14Tpl k14_tpl(cl_chrom* c)
{
    K14Tpl t;
    t.krow = c->tk.row.as<u32>();
    t.keys = c->tk.st.kind == CL_TRACK_WASHU ? c->tk.sorted.as<u64>() : nullptr;
    t.X = c->d_x; t.Y = c->d_y;
    t.ids = c->tk.st.ids ? c->tk.ids.as<long long>() : nullptr;
    t.names = c->tk.names.as<char>();
    t.ext = c->tk.st.ext;
    t.gmask = c->tk.st.gbits >= 64 ? ~0ull : ((1ull << c->tk.st.gbits) - 1);
    t.kind = c->tk.st.kind; t.la = c->tk.st.la; t.lb = c->tk.st.lb;
    return t;
}

static int k14_grid(long long work) { return (int)std::max(1ll, std::min<long long>(4096, (work + TPB - 1) / TPB)); }

// hn: host staging of the names, owned by the caller so that it outlives the stream synchronisation after an error return
static int track_build(cl_chrom* c, const int64_t* ids, std::vector<char>& hn, int64_t* n_records, int64_t* n_bytes)
{
    const int n = (int)c->n;
    cl_chrom::Track::State& s = c->tk.st;
    int rc;
    if ((rc = c->tk.names.ensure(2 * K14_NAME_MAX))) return rc;
    HIP_TRY(hipMemcpyAsync(c->tk.names.p, hn.data(), 2 * K14_NAME_MAX, hipMemcpyHostToDevice, c->stream));
    if (ids) {
        if ((rc = c->tk.ids.ensure((size_t)n * 8))) return rc;
        HIP_TRY(hipMemcpyAsync(c->tk.ids.p, ids, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    }
    // rows passing the cut, ascending
    const long long tiles = ((long long)n + K14_ROWS - 1) / K14_ROWS;
    if ((rc = c->tk.tcnt.ensure((size_t)(tiles + 1) * 4)) || (rc = c->tk.toff.ensure((size_t)(tiles + 1) * 4)) ||
        (rc = c->tk.row.ensure((size_t)n * 4)))
        return rc;
    HIP_TRY(hipMemsetAsync(c->tk.tcnt.as<u32>() + tiles, 0, 4, c->stream));
    hipLaunchKernelGGL(k14_count, dim3((unsigned)tiles), dim3(TPB), 0, c->stream, c->d_x, c->d_y, n, (long long)s.cut, c->tk.tcnt.as<u32>());
    HIP_TRY(hipGetLastError());
    if ((rc = prim_run(c->tk.tmp, "exclusive_scan(tiles)", [&](void* tmp, size_t& bytes) {
            return rocprim::exclusive_scan(tmp, bytes, c->tk.tcnt.as<u32>(), c->tk.toff.as<u32>(), 0u, (size_t)tiles + 1, rocprim::plus<u32>(), c->stream);
        })))
        return rc;
    hipLaunchKernelGGL(k14_compact, dim3((unsigned)tiles), dim3(TPB), 0, c->stream, c->d_x, c->d_y, n, (long long)s.cut, c->tk.toff.as<u32>(),
                       c->tk.row.as<u32>());
    HIP_TRY(hipGetLastError());
    u32 m = 0;
    HIP_TRY(hipMemcpyAsync(&m, c->tk.toff.as<u32>() + tiles, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const long long R = s.kind == CL_TRACK_WASHU ? 2ll * m : (long long)m;
    if (R == 0) { s.built = true; *n_records = 0; *n_bytes = 0; return CL_OK; }
    // washU: records in key order (p, generation), sorted over the bits in use
    if (s.kind == CL_TRACK_WASHU) {
        const int pmin = std::min(c->st.xmin, c->st.ymin), pmax = std::max(c->st.xmax, c->st.ymax);
        s.gbits = std::max(1, bits_for((unsigned)(R - 1)));
        const int ebit = bits_for((u32)(pmax - pmin)) + s.gbits;
        if ((rc = c->tk.keys.ensure((size_t)R * 8)) || (rc = c->tk.sorted.ensure((size_t)R * 8))) return rc;
        hipLaunchKernelGGL(k14_keys, dim3(k14_grid(m)), dim3(TPB), 0, c->stream, c->tk.row.as<u32>(), (long long)m, c->d_x, c->d_y, pmin,
                           s.gbits, c->tk.keys.as<u64>());
        HIP_TRY(hipGetLastError());
        if ((rc = prim_run(c->tk.tmp, "radix_sort_keys(track)", [&](void* tmp, size_t& bytes) {
                return rocprim::radix_sort_keys(tmp, bytes, c->tk.keys.as<u64>(), c->tk.sorted.as<u64>(), (size_t)R, 0, ebit, c->stream);
            })))
            return rc;
    }
    // line lengths and their running sum
    TextOut& txt = c->tk.txt;
    if ((rc = txt.len.ensure((size_t)R * 8)) || (rc = txt.end.ensure((size_t)R * 8))) return rc;
    if (s.kind == CL_TRACK_WASHU)
        hipLaunchKernelGGL(k14_lens<CL_TRACK_WASHU>, dim3(k14_grid(R)), dim3(TPB), 0, c->stream, k14_tpl(c), R, txt.len.as<long long>());
    else
        hipLaunchKernelGGL(k14_lens<CL_TRACK_JUICE>, dim3(k14_grid(R)), dim3(TPB), 0, c->stream, k14_tpl(c), R, txt.len.as<long long>());
    HIP_TRY(hipGetLastError());
    if ((rc = text_scan(txt, c->tk.tmp, R, c->stream)) || (rc = text_total(txt, R, c->stream))) return rc;
    s.built = true;
    *n_records = R;
    *n_bytes = txt.total;
    return CL_OK;
}

extern "C" int cl_track_build(cl_chrom* c, int32_t kind, int64_t cut, int64_t ext, const int64_t* ids, const char* name_a,
                              const char* name_b, int64_t* n_records, int64_t* n_bytes)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_records) *n_records = 0;
    if (n_bytes) *n_bytes = 0;
    if (!n_records || !n_bytes || !name_a || !name_b) return fail(CL_ERR_ARG, "cl_track_build: bad arguments");
    if (kind != CL_TRACK_WASHU && kind != CL_TRACK_JUICE) return fail(CL_ERR_ARG, "cl_track_build: unknown kind");
    if (cut < 0) return fail(CL_ERR_ARG, "cl_track_build: cut < 0");
    const size_t la = strlen(name_a), lb = strlen(name_b);
    if (la > K14_NAME_MAX || lb > K14_NAME_MAX) return fail(CL_ERR_ARG, "cl_track_build: chromosome name longer than CL_TRACK_NAME_MAX");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_track_build: asynchronous runs still in flight");
    HIP_TRY(hipSetDevice(c->device));
    track_release(c);
    cl_chrom::Track::State& s = c->tk.st;
    s.kind = kind; s.cut = cut; s.ext = ext; s.la = (int)la; s.lb = (int)lb; s.ids = ids != nullptr;
    if (c->n == 0) { s.built = true; return CL_OK; }
    std::vector<char> hn(2 * K14_NAME_MAX, 0);
    std::memcpy(hn.data(), name_a, la);
    std::memcpy(hn.data() + K14_NAME_MAX, name_b, lb);
    const int rc = track_build(c, ids, hn, n_records, n_bytes);
    if (rc != CL_OK) {
        (void)hipStreamSynchronize(c->stream);                          // no copy from hn / ids may still be pending
        track_release(c);
    }
    return rc;
}

extern "C" int cl_track_chunks(cl_chrom* c, int64_t budget, int64_t cap, int64_t* rec_bounds, int64_t* byte_bounds, int64_t* n_chunks)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_chunks) *n_chunks = 0;
    if (!n_chunks || (!rec_bounds) != (!byte_bounds)) return fail(CL_ERR_ARG, "cl_track_chunks: bad arguments");
    if (!c->tk.st.built) return fail(CL_ERR_ARG, "cl_track_chunks: no track built on this handle");
    if (budget < k14_lcap(c)) return fail(CL_ERR_ARG, "cl_track_chunks: budget below the longest line the template allows");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_track_chunks: asynchronous runs still in flight");
    if (c->tk.txt.R > 0) HIP_TRY(hipSetDevice(c->device));
    return text_chunks(c->tk.txt, c->stream, budget, k14_lcap(c), cap, rec_bounds, byte_bounds, n_chunks, "cl_track_chunks");
}

extern "C" int cl_track_render(cl_chrom* c, int64_t chunk, char* out, int64_t cap, int64_t* n_bytes)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (n_bytes) *n_bytes = 0;
    if (!out || !n_bytes) return fail(CL_ERR_ARG, "cl_track_render: bad arguments");
    cl_chrom::Track::State& s = c->tk.st;
    TextOut& txt = c->tk.txt;
    if (!s.built || txt.crec.empty()) return fail(CL_ERR_ARG, "cl_track_render: no chunks made on this handle (cl_track_chunks)");
    if (chunk < 0 || chunk + 1 >= (int64_t)txt.crec.size()) return fail(CL_ERR_ARG, "cl_track_render: chunk index out of range");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, "cl_track_render: asynchronous runs still in flight");
    const TextChunk k = text_chunk(txt, chunk);
    if (cap < k.nb) return fail(CL_ERR_ARG, "cl_track_render: capacity below the chunk's bytes");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = text_reserve(txt, k.nb))) return rc;
    const long long tiles = (k.r1 - k.r0 + K14_T - 1) / K14_T;
    const size_t lds = (((size_t)K14_T * k14_lcap(c) + 16 + 15) / 16) * 16;   // the span plus the shift of its first word
    if (s.kind == CL_TRACK_WASHU)
        hipLaunchKernelGGL(k14_render<CL_TRACK_WASHU>, dim3((unsigned)tiles), dim3(K14_T), lds, c->stream, k14_tpl(c), k.r0, k.r1, k.b0,
                           txt.end.as<long long>(), txt.out.as<char>());
    else
        hipLaunchKernelGGL(k14_render<CL_TRACK_JUICE>, dim3((unsigned)tiles), dim3(K14_T), lds, c->stream, k14_tpl(c), k.r0, k.r1, k.b0,
                           txt.end.as<long long>(), txt.out.as<char>());
    HIP_TRY(hipGetLastError());
    if ((rc = text_copy_out(txt, c->stream, out, k.nb, "cl_track_render"))) return rc;
    *n_bytes = k.nb;
    return CL_OK;
}

extern "C" int cl_track_free(cl_chrom* c) { return unit_free(c, "cl_track_free", track_release); }
