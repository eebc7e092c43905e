// k_convert.hip -- K15: the pairs-to-BEDPE converters of the reference (scripts/hicpropairs2bedpe, scripts/juicerLong2bedpe.py) on
// the device: a line index over raw bytes, a field tokenizer with exact integer parsing, and a lane-per-line renderer -- kernels and
// the C entry points of the cl_conv handle.  CL_CONV_PAIRS (4DN pairs text, no script of the reference) is the HiC-Pro rule on
// other columns, with '#' header lines.
#include "cl_chrom.h"
#include "cl_text.h"
#include "cl_pairs.h"

// ==========================================================================================
// K15: one chunk of complete lines per cl_conv_feed, its text made by cl_conv_render
// ==========================================================================================
// The reference reads one line at a time in Python, splits it, parses two integers and writes one BEDPE line.  Here the host hands
// over a chunk of complete lines (page-locked, up to the handle's byte budget) and the device does the rest, in four steps:
//   k15_count / k15_lines   the line index: 16 KiB tiles of input bytes read with 16-byte loads, '\n' found by an exact SWAR byte
//                           compare and counted by popcount; a count per tile, an exclusive scan of the counts, an ordered write
//                           of every line's end (the position of its '\n')
//   k15_parse<FMT>          256 lines per workgroup, one per lane: the tile's bytes staged in LDS with 16-byte loads (a tile wider
//                           than the LDS reads global memory instead), each lane walks its own line 8 bytes per read, splits it as
//                           the script does (up to field 6), parses the two positions and writes one record and its output
//                           length; the first bad line: a wave minimum, a workgroup minimum, one atomicMin per workgroup
//   inclusive scan          the int64 running sum of the lengths: line j occupies [end[j - 1], end[j]) of the chunk's text
//   k15_render<FMT>         K14's LDS tile: one lane per line assembles its text in LDS, the workgroup writes its span with
//                           16-byte stores; copied fields are read from the chunk, still in HBM (a span wider than the LDS is
//                           written straight to global memory)
// The reading rules are Python 2's on bytes: lines end at '\n' only, whitespace is ASCII \t \n \v \f \r and space,
// an integer is optional whitespace, an optional sign, ASCII digits, optional whitespace, and must fit int64 with +-ext applied.
#define K15_T 256                                // lines per parse / render workgroup (one per lane)
#define K15_LDS (40 * 1024)                      // bytes of a staged input or output tile: 4 workgroups per CU
#define K15_HEADER 4u                            // K15Rec.flags: a '#' line of a pairs file (a record of no text)

struct K15Rec {                                  // one parsed line
    u32 off[5], len[5];                          // copied fields (chunk offsets): hicpro f0 f1 f3 f4 f6; pairs f0 f1 f5 f3 f6; juicer f1 f5
    long long v[4];                              // the four printed integers
    u32 flags;                                   // juicer: bit 0 / 1 = field 0 / 4 is "0"; pairs: K15_HEADER; a bad line: its error kind << 8
    u32 pad;
};

// the copied fields and the output length of a tab-separated line whose ends are v: f0, chromosome A, strand A, chromosome B, strand B
__device__ __forceinline__ void k15_tab_rec(const long long* fs, const long long* fe, int c1, int s1, int c2, int s2, const long long* v, K15Rec& r,
                                            long long& olen)
{
    const int f[5] = {0, c1, s1, c2, s2};
#pragma unroll
    for (int k = 0; k < 5; ++k) { r.off[k] = (u32)fs[f[k]]; r.len[k] = (u32)(fe[f[k]] - fs[f[k]]); }
    r.v[0] = v[0]; r.v[1] = v[1]; r.v[2] = v[2]; r.v[3] = v[3];
    r.flags = 0;
    olen = (long long)r.len[0] + r.len[1] + r.len[2] + r.len[3] + r.len[4] + cl_width(v[0]) + cl_width(v[1]) + cl_width(v[2]) + cl_width(v[3]) + 11;
}

// scripts/hicpropairs2bedpe:15-34: line.strip().split('\t'); A from f1, f2, f3 and B from f4, f5, f6; f0 . f3 f6 copied
__device__ __forceinline__ int k15_hicpro(K15Rd& rd, long long s, long long e, long long ext, K15Rec& r, long long& olen)
{
    long long fs[7], fe[7], v[4];
    if (!k15_tabs7(rd, s, e, fs, fe)) return CL_CONV_E_FIELDS;
    const int bad = k15_ends<2, 3, 5, 6>(rd, fs, fe, ext, v);
    if (bad) return bad;
    k15_tab_rec(fs, fe, 1, 3, 4, 6, v, r, olen);
    return 0;
}

// 4DN pairs (readID chr1 pos1 chr2 pos2 strand1 strand2): the rule above on f0 f1 f2 f5 f3 f4 f6; a line whose first byte is '#'
// is a header line: no text
__device__ __forceinline__ int k15_pairs(K15Rd& rd, long long s, long long e, long long ext, K15Rec& r, long long& olen)
{
    if (s < e && rd.at(s) == '#') { r.flags = K15_HEADER; olen = 0; return 0; }
    long long fs[7], fe[7], v[4];
    if (!k15_tabs7(rd, s, e, fs, fe)) return CL_CONV_E_FIELDS;
    const int bad = k15_ends<2, 5, 4, 6>(rd, fs, fe, ext, v);
    if (bad) return bad;
    k15_tab_rec(fs, fe, 1, 5, 3, 6, v, r, olen);
    return 0;
}

// scripts/juicerLong2bedpe.py:12-31: line.split(); f1 max(0, p1 - ext) p1 + ext f5 max(0, p2 - ext) p2 + ext . . s1 s2
__device__ __forceinline__ int k15_juicer(K15Rd& rd, long long s, long long e, long long ext, K15Rec& r, long long& olen)
{
    long long fs[7], fe[7];
    long long q = s;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        if (ok)
            while (q < e && k15_ws(rd.at(q))) ++q;
        ok = ok && q < e;
        fs[k] = q;
        if (ok)
            while (q < e && !k15_ws(rd.at(q))) ++q;
        fe[k] = q;
    }
    if (!ok) return CL_CONV_E_FIELDS;
    long long p1 = 0, p2 = 0;
    int bad = k15_int(rd, fs[2], fe[2], p1);
    if (!bad) bad = k15_int(rd, fs[6], fe[6], p2);
    if (bad) return bad;
    long long lo1, hi1, lo2, hi2;
    const int ovf = (int)__builtin_sub_overflow(p1, ext, &lo1) | (int)__builtin_add_overflow(p1, ext, &hi1) |
                    (int)__builtin_sub_overflow(p2, ext, &lo2) | (int)__builtin_add_overflow(p2, ext, &hi2);
    if (ovf) return CL_CONV_E_RANGE;
    r.v[0] = lo1 > 0 ? lo1 : 0; r.v[1] = hi1;
    r.v[2] = lo2 > 0 ? lo2 : 0; r.v[3] = hi2;
    const bool z1 = fe[0] - fs[0] == 1 && rd.at(fs[0]) == '0';
    const bool z2 = fe[4] - fs[4] == 1 && rd.at(fs[4]) == '0';
    r.flags = (z1 ? 1u : 0u) | (z2 ? 2u : 0u);
    r.off[0] = (u32)fs[1]; r.len[0] = (u32)(fe[1] - fs[1]);
    r.off[1] = (u32)fs[5]; r.len[1] = (u32)(fe[5] - fs[5]);
    r.off[2] = r.off[3] = r.off[4] = 0;
    r.len[2] = r.len[3] = r.len[4] = 0;
    olen = (long long)r.len[0] + r.len[1] + cl_width(r.v[0]) + cl_width(r.v[1]) + cl_width(r.v[2]) + cl_width(r.v[3]) + 14;
    return 0;
}

template <int FMT>
__device__ __forceinline__ int k15_line(K15Rd& rd, long long s, long long e, long long ext, K15Rec& r, long long& olen)
{
    if (FMT == CL_CONV_PAIRS) return k15_pairs(rd, s, e, ext, r, olen);
    return FMT == CL_CONV_HICPRO ? k15_hicpro(rd, s, e, ext, r, olen) : k15_juicer(rd, s, e, ext, r, olen);
}

// lines [256 b, 256 b + 256) of the chunk -> their records and output lengths (0 for a bad line); the first bad line -> *err
template <int FMT>
__global__ void __launch_bounds__(K15_T)
k15_parse(const uint4* __restrict__ in, const u32* __restrict__ ends, long long L, long long ext, K15Rec* __restrict__ rec,
          long long* __restrict__ len, int* __restrict__ err)
{
    extern __shared__ uint4 k15_lds[];
    __shared__ int wmin[K15_T / 64];
    const long long q0 = (long long)blockIdx.x * K15_T;
    const long long q1 = q0 + K15_T < L ? q0 + K15_T : L;
    const long long a0 = (q0 > 0 ? (long long)ends[q0 - 1] + 1 : 0) & ~15ll;
    const long long a1 = ((long long)ends[q1 - 1] + 1 + 15) & ~15ll;        // the tile's bytes, its last '\n' included
    const bool fits = a1 - a0 <= K15_LDS;
    if (fits)
        for (long long i = threadIdx.x; i < (a1 - a0) >> 4; i += K15_T) k15_lds[i] = in[(a0 >> 4) + i];
    __syncthreads();
    const long long j = q0 + threadIdx.x;
    int bad = INT_MAX;
    if (j < q1) {
        const long long s = j > 0 ? (long long)ends[j - 1] + 1 : 0, e = ends[j];
        K15Rec r = {};
        long long olen = 0;
        int kind;
        if (fits) {
            K15Rd rd{(const u64*)k15_lds, a0, -1, 0};
            kind = k15_line<FMT>(rd, s, e, ext, r, olen);
        } else {
            K15Rd rd{(const u64*)in, 0, -1, 0};
            kind = k15_line<FMT>(rd, s, e, ext, r, olen);
        }
        if (kind) { r.flags = (u32)kind << 8; olen = 0; bad = (int)j; }
        rec[j] = r;
        len[j] = olen;
    }
    bad = dpp_reduce_wave(bad, OpMin());
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int m = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
        if (m != INT_MAX) atomicMin(err, m);
    }
}

__device__ __forceinline__ int k15_copy(char* d, int p, K15Rd& rd, u32 off, u32 n)
{
    for (u32 k = 0; k < n; ++k) d[p + k] = (char)rd.at((long long)off + k);
    return p + (int)n;
}

// the text of one record at d[p ..]
template <int FMT>
__device__ __forceinline__ void k15_emit(char* d, int p, const uint4* in, const K15Rec& r)
{
    K15Rd rd{(const u64*)in, 0, -1, 0};
    if (FMT == CL_CONV_PAIRS && (r.flags & K15_HEADER)) return;
    if (FMT != CL_CONV_JUICER) {                                       // A0 A1 A2 B0 B1 B2 f0 . sA sB (hicpro f3 f6, pairs f5 f6)
        p = k15_copy(d, p, rd, r.off[1], r.len[1]); d[p++] = '\t';
        p = cl_put(d, p, r.v[0]); d[p++] = '\t';
        p = cl_put(d, p, r.v[1]); d[p++] = '\t';
        p = k15_copy(d, p, rd, r.off[3], r.len[3]); d[p++] = '\t';
        p = cl_put(d, p, r.v[2]); d[p++] = '\t';
        p = cl_put(d, p, r.v[3]); d[p++] = '\t';
        p = k15_copy(d, p, rd, r.off[0], r.len[0]); d[p++] = '\t'; d[p++] = '.'; d[p++] = '\t';
        p = k15_copy(d, p, rd, r.off[2], r.len[2]); d[p++] = '\t';
        p = k15_copy(d, p, rd, r.off[4], r.len[4]); d[p++] = '\n';
    } else {                                                           // f1 lo1 hi1 f5 lo2 hi2 . . s1 s2
        p = k15_copy(d, p, rd, r.off[0], r.len[0]); d[p++] = '\t';
        p = cl_put(d, p, r.v[0]); d[p++] = '\t';
        p = cl_put(d, p, r.v[1]); d[p++] = '\t';
        p = k15_copy(d, p, rd, r.off[1], r.len[1]); d[p++] = '\t';
        p = cl_put(d, p, r.v[2]); d[p++] = '\t';
        p = cl_put(d, p, r.v[3]); d[p++] = '\t';
        d[p++] = '.'; d[p++] = '\t'; d[p++] = '.'; d[p++] = '\t';
        d[p++] = (r.flags & 1u) ? '+' : '-'; d[p++] = '\t';
        d[p++] = (r.flags & 2u) ? '+' : '-'; d[p++] = '\n';
    }
}

// lines [0, R) of the chunk -> out[0 .. end[R - 1]); 256 lines per workgroup, staged in LDS when their span fits
template <int FMT>
__global__ void __launch_bounds__(K15_T)
k15_render(const uint4* __restrict__ in, const K15Rec* __restrict__ rec, const long long* __restrict__ end, long long R,
           char* __restrict__ out)
{
    extern __shared__ uint4 k15_lds[];
    char* buf = (char*)k15_lds;
    const TextTile tile = text_tile(end, 0, R, 0, K15_T);
    const bool fits = tile.g1 - tile.a0 <= K15_LDS;
    const long long j = tile.q0 + threadIdx.x;
    if (j < tile.q1) {
        const long long p0 = j > 0 ? end[j - 1] : 0;
        const K15Rec r = rec[j];
        if (fits) k15_emit<FMT>(buf, (int)(p0 - tile.a0), in, r);
        else k15_emit<FMT>(out + p0, 0, in, r);
    }
    if (!fits) return;                                                  // uniform over the workgroup
    __syncthreads();
    text_flush(out, k15_lds, tile.g0, tile.g1, tile.a0);
}

// ---- K15 host side ------------------------------------------------------------------------------
struct cl_conv {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int fmt = 0;
    long long ext = 0, budget = 0, lmax = 0;
    DevBuf in, tcnt, toff, ends, rec, tmp, err;
    TextOut txt;                                  // the last feed's text: txt.R lines of txt.total bytes (a feed is its own chunk)
    long long lines = 0;                          // lines of every feed so far: cl_conv_error's line numbers
    bool fed = false;                             // the last feed's lines can be rendered
    long long err_line = 0;
    int err_kind = 0;
    hipEvent_t ev[6] = {};                        // feed: copy start / copy end / kernels end; render: start / kernel end / copy end
    float ms_h2d = 0, ms_feed = 0, ms_render = 0, ms_d2h = 0;
};

// `delete c` frees the buffers; the events and the stream are noted first and ended afterwards (as free_chrom does)
static void conv_free(cl_conv* c)
{
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    const std::vector<hipEvent_t> events(std::begin(c->ev), std::end(c->ev));
    const hipStream_t own = c->own_stream ? c->stream : nullptr;
    delete c;
    for (hipEvent_t e : events)
        if (e) (void)hipEventDestroy(e);
    if (own) (void)hipStreamDestroy(own);
}

extern "C" int cl_conv_create(int device, void* stream, int32_t format, int64_t ext, int64_t budget, cl_conv** out)
{
    if (!out) return fail(CL_ERR_ARG, "cl_conv_create: out is null");
    *out = nullptr;
    if (format != CL_CONV_HICPRO && format != CL_CONV_JUICER && format != CL_CONV_PAIRS) return fail(CL_ERR_ARG, "cl_conv_create: unknown format");
    if (budget < 1 || budget > CL_CONV_BUDGET_MAX) return fail(CL_ERR_ARG, "cl_conv_create: budget outside 1 .. CL_CONV_BUDGET_MAX");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(CL_ERR_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(CL_ERR_ARG, "cl_conv_create: bad device index");
    HIP_TRY(hipSetDevice(device));
    cl_conv* c = new cl_conv();
    c->device = device; c->fmt = format; c->ext = ext; c->budget = budget;
    c->lmax = budget / 16 + K15_T;
    int rc = CL_OK;
    if (stream) c->stream = (hipStream_t)stream;
    else if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) rc = fail(CL_ERR_HIP, "hipStreamCreate");
    else c->own_stream = true;
    for (int i = 0; rc == CL_OK && i < 6; ++i)
        if (hipEventCreate(&c->ev[i]) != hipSuccess) rc = fail(CL_ERR_HIP, "hipEventCreate");
    if (rc == CL_OK) rc = c->err.ensure(16);
    if (rc != CL_OK) { conv_free(c); return rc; }
    *out = c;
    return CL_OK;
}

template <typename T>
static int conv_read(cl_conv* c, T* dst, const void* src)            // one value from device memory, synchronously
{
    HIP_TRY(hipMemcpyAsync(dst, src, sizeof(T), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CL_OK;
}

static int conv_feed(cl_conv* c, const char* bytes, long long cut, long long* consumed, int* bad, long long* L_out)
{
    const bool virt = bytes[cut - 1] != '\n';                          // the input's last line, without its newline
    const long long ne = cut + (virt ? 1 : 0);
    const long long tiles = (ne + K15_TILE - 1) / K15_TILE;
    int rc;
    if ((rc = c->in.ensure((size_t)ne + K15_PAD)) || (rc = c->tcnt.ensure((size_t)(tiles + 1) * 4)) ||
        (rc = c->toff.ensure((size_t)(tiles + 1) * 4)) || (rc = c->ends.ensure((size_t)c->lmax * 4)))
        return rc;
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    HIP_TRY(hipMemcpyAsync(c->in.p, bytes, (size_t)cut, hipMemcpyHostToDevice, c->stream));
    if (virt) HIP_TRY(hipMemsetAsync(c->in.as<char>() + cut, '\n', 1, c->stream));
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(hipMemsetAsync(c->tcnt.as<u32>() + tiles, 0, 4, c->stream));
    HIP_TRY(hipMemsetAsync(c->err.p, 0x7f, 4, c->stream));          // no bad line: 0x7f7f7f7f, above any line index
    hipLaunchKernelGGL(k15_count, dim3((unsigned)tiles), dim3(TPB), 0, c->stream, c->in.as<uint4>(), ne, c->tcnt.as<u32>());
    HIP_TRY(hipGetLastError());
    if ((rc = prim_run(c->tmp, "exclusive_scan(tiles)", [&](void* tmp, size_t& nb) {
            return rocprim::exclusive_scan(tmp, nb, c->tcnt.as<u32>(), c->toff.as<u32>(), 0u, (size_t)tiles + 1, rocprim::plus<u32>(), c->stream);
        })))
        return rc;
    hipLaunchKernelGGL(k15_lines, dim3((unsigned)tiles), dim3(TPB), 0, c->stream, c->in.as<uint4>(), ne, c->toff.as<u32>(), c->lmax,
                       c->ends.as<u32>());
    HIP_TRY(hipGetLastError());
    u32 nl = 0;
    if ((rc = conv_read(c, &nl, c->toff.as<u32>() + tiles))) return rc;
    long long L = nl;
    *consumed = cut;
    if (L > c->lmax) {                                                  // the rest of the chunk waits for the next feed
        L = c->lmax;
        u32 last_end = 0;
        if ((rc = conv_read(c, &last_end, c->ends.as<u32>() + (L - 1)))) return rc;
        *consumed = (long long)last_end + 1;
    }
    if ((rc = c->rec.ensure((size_t)L * sizeof(K15Rec))) || (rc = c->txt.len.ensure((size_t)L * 8)) || (rc = c->txt.end.ensure((size_t)L * 8))) return rc;
    const unsigned grid = (unsigned)((L + K15_T - 1) / K15_T);
    if (c->fmt == CL_CONV_HICPRO)
        hipLaunchKernelGGL(k15_parse<CL_CONV_HICPRO>, dim3(grid), dim3(K15_T), K15_LDS, c->stream, c->in.as<uint4>(), c->ends.as<u32>(), L, c->ext,
                           c->rec.as<K15Rec>(), c->txt.len.as<long long>(), c->err.as<int>());
    else if (c->fmt == CL_CONV_PAIRS)
        hipLaunchKernelGGL(k15_parse<CL_CONV_PAIRS>, dim3(grid), dim3(K15_T), K15_LDS, c->stream, c->in.as<uint4>(), c->ends.as<u32>(), L, c->ext,
                           c->rec.as<K15Rec>(), c->txt.len.as<long long>(), c->err.as<int>());
    else
        hipLaunchKernelGGL(k15_parse<CL_CONV_JUICER>, dim3(grid), dim3(K15_T), K15_LDS, c->stream, c->in.as<uint4>(), c->ends.as<u32>(), L, c->ext,
                           c->rec.as<K15Rec>(), c->txt.len.as<long long>(), c->err.as<int>());
    HIP_TRY(hipGetLastError());
    if ((rc = text_scan(c->txt, c->tmp, L, c->stream))) return rc;
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    if ((rc = conv_read(c, bad, c->err.p))) return rc;
    *L_out = L;
    return CL_OK;
}

extern "C" int cl_conv_feed(cl_conv* c, const char* bytes, int64_t n, int32_t last, int64_t* consumed, int64_t* n_lines, int64_t* n_bytes)
{
    if (!c) return fail(CL_ERR_ARG, "null converter handle");
    if (consumed) *consumed = 0;
    if (n_lines) *n_lines = 0;
    if (n_bytes) *n_bytes = 0;
    if (!consumed || !n_lines || !n_bytes || n < 0 || (n > 0 && !bytes)) return fail(CL_ERR_ARG, "cl_conv_feed: bad arguments");
    if (n > c->budget) return fail(CL_ERR_ARG, "cl_conv_feed: more bytes than the handle's budget");
    c->fed = false; text_reset(c->txt); c->err_line = 0; c->err_kind = 0;
    c->ms_h2d = c->ms_feed = c->ms_render = c->ms_d2h = 0;
    long long cut = n;                                                  // complete lines only, unless the input ends here
    if (!last) {
        const void* nl = n > 0 ? memrchr(bytes, '\n', (size_t)n) : nullptr;
        if (!nl) {
            c->fed = true;                                              // nothing to render
            if (n < c->budget) return CL_OK;                            // no complete line yet
            c->err_line = c->lines + 1;
            c->err_kind = CL_CONV_E_LONG;
            return fail(CL_ERR_PARSE, "cl_conv_feed: a line longer than the chunk budget");
        }
        cut = (const char*)nl - bytes + 1;
    }
    if (cut == 0) { c->fed = true; return CL_OK; }
    HIP_TRY(hipSetDevice(c->device));
    long long used = 0, L = 0;
    int bad = INT_MAX;
    int rc = conv_feed(c, bytes, cut, &used, &bad, &L);
    if (rc != CL_OK) {
        (void)hipStreamSynchronize(c->stream);                          // no copy from `bytes` may still be pending
        return rc;
    }
    const long long R = bad < L ? bad : L;
    if (R > 0 && (rc = text_total(c->txt, R, c->stream))) return rc;                 // (the lines in front of the first bad one)
    const long long total = c->txt.total;
    u32 flags = 0;
    if (bad < L && (rc = conv_read(c, &flags, (const char*)c->rec.p + (size_t)bad * sizeof(K15Rec) + offsetof(K15Rec, flags)))) return rc;
    (void)hipEventElapsedTime(&c->ms_h2d, c->ev[0], c->ev[1]);
    (void)hipEventElapsedTime(&c->ms_feed, c->ev[1], c->ev[2]);
    const long long first = c->lines;
    c->lines += L;
    c->fed = true;
    *consumed = used;
    *n_lines = R;
    *n_bytes = total;
    if (bad < L) {
        c->err_line = first + bad + 1;
        c->err_kind = (int)(flags >> 8);
        return fail(CL_ERR_PARSE, "cl_conv_feed: a line the reference's script would raise on (cl_conv_error)");
    }
    return CL_OK;
}

extern "C" int cl_conv_render(cl_conv* c, char* out, int64_t cap, int64_t* n_bytes)
{
    if (!c) return fail(CL_ERR_ARG, "null converter handle");
    if (n_bytes) *n_bytes = 0;
    TextOut& txt = c->txt;
    if (!n_bytes || (!out && txt.total > 0)) return fail(CL_ERR_ARG, "cl_conv_render: bad arguments");
    if (!c->fed) return fail(CL_ERR_ARG, "cl_conv_render: no feed to render");
    if (cap < txt.total) return fail(CL_ERR_ARG, "cl_conv_render: capacity below the feed's bytes");
    if (txt.R == 0 || txt.total == 0) return CL_OK;                     // no lines, or header lines only
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = text_reserve(txt, txt.total))) return rc;
    const unsigned grid = (unsigned)((txt.R + K15_T - 1) / K15_T);
    HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    if (c->fmt == CL_CONV_HICPRO)
        hipLaunchKernelGGL(k15_render<CL_CONV_HICPRO>, dim3(grid), dim3(K15_T), K15_LDS, c->stream, c->in.as<uint4>(), c->rec.as<K15Rec>(),
                           txt.end.as<long long>(), txt.R, txt.out.as<char>());
    else if (c->fmt == CL_CONV_PAIRS)
        hipLaunchKernelGGL(k15_render<CL_CONV_PAIRS>, dim3(grid), dim3(K15_T), K15_LDS, c->stream, c->in.as<uint4>(), c->rec.as<K15Rec>(),
                           txt.end.as<long long>(), txt.R, txt.out.as<char>());
    else
        hipLaunchKernelGGL(k15_render<CL_CONV_JUICER>, dim3(grid), dim3(K15_T), K15_LDS, c->stream, c->in.as<uint4>(), c->rec.as<K15Rec>(),
                           txt.end.as<long long>(), txt.R, txt.out.as<char>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[4], c->stream));
    if ((rc = text_copy_out(txt, c->stream, out, txt.total, "cl_conv_render", c->ev[5]))) return rc;
    (void)hipEventElapsedTime(&c->ms_render, c->ev[3], c->ev[4]);
    (void)hipEventElapsedTime(&c->ms_d2h, c->ev[4], c->ev[5]);
    *n_bytes = txt.total;
    return CL_OK;
}

extern "C" int cl_conv_error(cl_conv* c, int64_t* line, int32_t* kind)
{
    if (!c) return fail(CL_ERR_ARG, "null converter handle");
    if (!line || !kind) return fail(CL_ERR_ARG, "cl_conv_error: bad arguments");
    *line = c->err_line;
    *kind = c->err_kind;
    return CL_OK;
}

extern "C" int cl_conv_timing(cl_conv* c, float* ms)
{
    if (!c) return fail(CL_ERR_ARG, "null converter handle");
    if (!ms) return fail(CL_ERR_ARG, "cl_conv_timing: bad arguments");
    ms[0] = c->ms_h2d; ms[1] = c->ms_feed; ms[2] = c->ms_render; ms[3] = c->ms_d2h;
    return CL_OK;
}

extern "C" int cl_conv_destroy(cl_conv* c)
{
    if (!c) return CL_OK;
    conv_free(c);
    return CL_OK;
}
