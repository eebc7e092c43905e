// cl_pairs.h -- what the readers of tab-separated pairs lines share, K15 (k_convert.hip: HiC-Pro allValidPairs, 4DN pairs) and K18
// (k_ingest.hip: 4DN pairs straight into the reader's records): Python 2's whitespace and int() on bytes, the tokenizer of
// scripts/hicpropairs2bedpe (line.strip().split('\t'), fields 0 .. 6) and the two extended ends of a line.
#pragma once
#include "cl_lines.h"

__device__ __forceinline__ bool k15_ws(u32 c) { return c == 32u || (c >= 9u && c <= 13u); }

// Python 2's int() of the bytes [s, e), bounded to int64 -> 0 and v, or the error kind
__device__ __forceinline__ int k15_int(K15Rd& rd, long long s, long long e, long long& v)
{
    while (s < e && k15_ws(rd.at(s))) ++s;
    while (e > s && k15_ws(rd.at(e - 1))) --e;
    bool neg = false;
    if (s < e) {
        const u32 c = rd.at(s);
        if (c == '+' || c == '-') { neg = c == '-'; ++s; }
    }
    if (s >= e) return CL_CONV_E_INT;
    const u64 lim = neg ? (1ull << 63) : (1ull << 63) - 1;
    u64 m = 0;
    bool over = false;
    for (; s < e; ++s) {
        const u32 d = rd.at(s) - (u32)'0';
        if (d > 9) return CL_CONV_E_INT;                              // ValueError before any overflow
        if (m > (lim - d) / 10) over = true;
        else m = m * 10 + d;
    }
    if (over) return CL_CONV_E_RANGE;
    v = neg ? (long long)(0ull - m) : (long long)m;
    return 0;
}

// scripts/hicpropairs2bedpe:15-16: line.strip().split('\t') of the line [s, e) -> the bounds of fields 0 .. 6; false: fewer than 7
__device__ __forceinline__ bool k15_tabs7(K15Rd& rd, long long s, long long e, long long* fs, long long* fe)
{
    while (e > s && k15_ws(rd.at(e - 1))) --e;
    while (s < e && k15_ws(rd.at(s))) ++s;
    long long q = s;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        if (k > 0) { ok = ok && q < e; ++q; }                        // the '\t' that ended field k - 1
        fs[k] = q;
        if (ok)
            while (q < e && rd.at(q) != '\t') ++q;
        fe[k] = q;
    }
    return ok;
}

// scripts/hicpropairs2bedpe:17-32 with the position and strand of end A in fields P1, S1 and those of end B in P2, S2:
// [p, p + ext] when the strand is exactly "+", else [p - ext, p] -> v = A1 A2 B1 B2 and 0, or the error kind
template <int P1, int S1, int P2, int S2>
__device__ __forceinline__ int k15_ends(K15Rd& rd, const long long* fs, const long long* fe, long long ext, long long* v)
{
    long long p1 = 0, p2 = 0;
    int bad = k15_int(rd, fs[P1], fe[P1], p1);
    if (!bad) bad = k15_int(rd, fs[P2], fe[P2], p2);
    if (bad) return bad;
    const bool plus1 = fe[S1] - fs[S1] == 1 && rd.at(fs[S1]) == '+';
    const bool plus2 = fe[S2] - fs[S2] == 1 && rd.at(fs[S2]) == '+';
    long long a1 = p1, a2 = p1, b1 = p2, b2 = p2;
    bool ovf = plus1 ? __builtin_add_overflow(p1, ext, &a2) : __builtin_sub_overflow(p1, ext, &a1);
    ovf |= plus2 ? __builtin_add_overflow(p2, ext, &b2) : __builtin_sub_overflow(p2, ext, &b1);
    if (ovf) return CL_CONV_E_RANGE;
    v[0] = a1; v[1] = a2; v[2] = b1; v[3] = b2;
    return 0;
}
