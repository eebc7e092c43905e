// cl_textout.h -- text written on the device, shared by K14 (k_track.hip), K20 (k_cover.hip) and K15 (k_convert.hip).  A text is
// R lines whose byte lengths a unit's own kernel computes; their running sum places line j at [end[j - 1], end[j]).  The text leaves
// the device in chunks of whole lines below a byte budget, each rendered by workgroups of T lines (one per lane) that assemble their
// tile in LDS, placed so that LDS and the output agree modulo 16, and write the tile's byte span with 16-byte stores.
//   device: text_tile (a workgroup's lines and span), text_flush (LDS -> out), k14_bounds (the chunks of a budget)
//   host:   TextOut and text_scan / text_total / text_chunks / text_chunk / text_copy_out; a text is released by assigning TextOut()
// The line formats, and the argument checks and messages of the entry points, stay with the units.
#pragma once
#include "cl_prim.h"

// lines [q0, q1) of workgroup blockIdx.x of a render of lines [r0, r1) with T lines per workgroup; their span [g0, g1) in an output
// that starts at byte b0 of the text; LDS byte i <-> out byte a0 + i
struct TextTile { long long q0, q1, g0, g1, a0; };
__device__ __forceinline__ TextTile text_tile(const long long* __restrict__ end, long long r0, long long r1, long long b0, int T)
{
    TextTile t;
    t.q0 = r0 + (long long)blockIdx.x * T;
    t.q1 = t.q0 + T < r1 ? t.q0 + T : r1;
    t.g0 = (t.q0 > 0 ? end[t.q0 - 1] : 0) - b0; t.g1 = end[t.q1 - 1] - b0;
    t.a0 = t.g0 & ~15ll;
    return t;
}

// the span [g0, g1) as 16-byte words of out: whole words with one store each, the two edge words byte by byte
__device__ __forceinline__ void text_flush(char* __restrict__ out, const uint4* lds, long long g0, long long g1, long long a0)
{
    const char* buf = (const char*)lds;
    const long long w0 = g0 >> 4, w1 = (g1 + 15) >> 4;
    for (long long w = w0 + threadIdx.x; w < w1; w += blockDim.x) {
        const long long b = w << 4;
        if (b >= g0 && b + 16 <= g1) {
            *(uint4*)(out + b) = lds[(b - a0) >> 4];
        } else {
            const long long s = b > g0 ? b : g0, e = b + 16 < g1 ? b + 16 : g1;
            for (long long i = s; i < e; ++i) out[i] = buf[i - a0];
        }
    }
}

// bounds of chunk k: the first line starting at or after k * step (line j starts at end[j - 1]), and its byte offset.  Defined in
// the unit that sets CL_TEXTOUT_KERNELS (k_track.hip), declared in the others
__global__ void __launch_bounds__(TPB)
k14_bounds(const long long* __restrict__ end, long long R, long long step, long long K, long long* __restrict__ brec,
           long long* __restrict__ bbyte)
#ifdef CL_TEXTOUT_KERNELS
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > K) return;
    long long rec = 0;
    if (k > 0) {
        const long long T = k * step;
        long long lo = 0, len = R;                                      // first i with end[i] >= T
        while (len > 0) {
            const long long h = len >> 1;
            if (end[lo + h] < T) { lo += h + 1; len -= h + 1; } else len = h;
        }
        rec = lo + 1 < R ? lo + 1 : R;
    }
    brec[k] = rec;
    bbyte[k] = rec > 0 ? end[rec - 1] : 0;
}
#else
;
#endif

// ---- host side ----------------------------------------------------------------------------------
struct TextOut {
    DevBuf len, end, bnd, out;                    // line lengths, their running sum, chunk bounds, a rendered chunk
    long long R = 0, total = 0;                   // lines and bytes of the whole text (text_total)
    std::vector<long long> crec, cbyte;           // the last text_chunks: line / byte bounds (empty: none made)
};

// the running sum of the n lengths in t.len -> t.end (both allocated by the caller, whose kernel wrote the lengths); enqueued
static inline int text_scan(TextOut& t, DevBuf& tmp, long long n, hipStream_t stream)
{
    return prim_run(tmp, "inclusive_scan(lines)", [&](void* p, size_t& bytes) {
        return rocprim::inclusive_scan(p, bytes, t.len.as<long long>(), t.end.as<long long>(), (size_t)n, rocprim::plus<long long>(), stream);
    });
}

// the text is the first R >= 1 of the scanned lines: its bytes, read from the device; synchronises
static inline int text_total(TextOut& t, long long R, hipStream_t stream)
{
    long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, t.end.as<long long>() + (R - 1), 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    t.R = R; t.total = total;
    return CL_OK;
}

// Chunks: chunk k holds the lines that START in [k S, (k + 1) S), S = budget - lcap + 1, lcap the longest line the format allows, so
// no chunk exceeds the budget and no line is split; empty chunks are dropped.  Kept in t and, if bounds are asked for, copied to
// rec_bounds / byte_bounds (n_chunks + 1 entries each, cap the caller's capacity).  `who`: the entry point, for its messages
static inline int text_chunks(TextOut& t, hipStream_t stream, long long budget, long long lcap, long long cap, int64_t* rec_bounds,
                              int64_t* byte_bounds, int64_t* n_chunks, const char* who)
{
    t.crec.assign(1, 0);
    t.cbyte.assign(1, 0);
    if (t.R > 0) {
        const long long step = budget - lcap + 1;
        const long long K = (t.total + step - 1) / step;
        int rc;
        if ((rc = t.bnd.ensure((size_t)(K + 1) * 16))) return rc;
        long long* brec = t.bnd.as<long long>();
        long long* bbyte = brec + (K + 1);
        hipLaunchKernelGGL(k14_bounds, dim3((unsigned)((K + 1 + TPB - 1) / TPB)), dim3(TPB), 0, stream, t.end.as<long long>(), t.R, step, K, brec,
                           bbyte);
        HIP_TRY(hipGetLastError());
        std::vector<long long> hr((size_t)K + 1), hb((size_t)K + 1);
        hipError_t e = hipMemcpyAsync(hr.data(), brec, (size_t)(K + 1) * 8, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hb.data(), bbyte, (size_t)(K + 1) * 8, hipMemcpyDeviceToHost, stream);
        const hipError_t e2 = hipStreamSynchronize(stream);
        if (e != hipSuccess || e2 != hipSuccess) return fail_at(CL_ERR_HIP, who, "bounds readback", hipGetErrorString(e != hipSuccess ? e : e2));
        for (long long k = 1; k <= K; ++k)
            if (hr[k] != t.crec.back()) { t.crec.push_back(hr[k]); t.cbyte.push_back(hb[k]); }   // empty chunks dropped
        if (t.crec.back() != t.R || t.cbyte.back() != t.total) return fail_at(CL_ERR_HIP, who, "bounds do not cover the text");
    }
    const long long nc = (long long)t.crec.size() - 1;
    *n_chunks = nc;
    if (rec_bounds) {
        if (cap < nc + 1) return fail_at(CL_ERR_ARG, who, "capacity below n_chunks + 1");
        std::copy(t.crec.begin(), t.crec.end(), rec_bounds);
        std::copy(t.cbyte.begin(), t.cbyte.end(), byte_bounds);
    }
    return CL_OK;
}

// chunk k of the last text_chunks: lines [r0, r1), nb bytes from byte b0 of the text
struct TextChunk { long long r0, r1, b0, nb; };
static inline TextChunk text_chunk(const TextOut& t, long long k)
{
    return TextChunk{t.crec[k], t.crec[k + 1], t.cbyte[k], t.cbyte[k + 1] - t.cbyte[k]};
}

// where a render of nb bytes writes: the flush may store the whole 16-byte word that holds the last byte
static inline int text_reserve(TextOut& t, long long nb) { return t.out.ensure((size_t)nb + 16); }

// the nb rendered bytes to the host (and `done` recorded behind the copy, if given); synchronises
static inline int text_copy_out(TextOut& t, hipStream_t stream, char* out, long long nb, const char* who, hipEvent_t done = nullptr)
{
    hipError_t e = hipMemcpyAsync(out, t.out.p, (size_t)nb, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && done) e = hipEventRecord(done, stream);
    const hipError_t e2 = hipStreamSynchronize(stream);
    if (e != hipSuccess || e2 != hipSuccess) return fail_at(CL_ERR_HIP, who, "copy", hipGetErrorString(e != hipSuccess ? e : e2));
    return CL_OK;
}

// no text (the buffers stay: the next text reuses their memory, not their content)
static inline void text_reset(TextOut& t)
{
    t.R = t.total = 0;
    t.crec.clear(); t.cbyte.clear();
}
