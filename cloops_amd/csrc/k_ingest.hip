// k_ingest.hip -- K16: the BEDPE reader of the reference (cLoops/io.py:62-189, parseRawBedpe / parseRawBedpe2, restated by
// cloops_amd/io.py:parse_bedpe) on the device -- kernels and the C entry points of the cl_ingest handle.  K18: the same reader fed
// with 4DN pairs text (cl_ingest_set_format), every data line read as the BEDPE line K15 writes for it.
#include <memory>
#include "cl_chrom.h"
#include "cl_pairs.h"

// ==========================================================================================
// K16: one chunk of complete lines per cl_ingest_feed; its PETs appended by cl_ingest_commit; the chromosomes made by cl_ingest_finish
// ==========================================================================================
// The reference reads one line at a time in Python, splits it, builds a PET object and appends three numbers to a text file per
// chromosome.  Here the host hands over chunks of complete lines (page-locked, up to the handle's byte budget) and keeps only the
// dictionary of chromosome names:
//   feed     k15_count / k15_lines (cl_lines.h)   the line index
//            k16_parse      256 lines per workgroup, one per lane, the tile staged in LDS: fields, the '*' / '-1' rule, four integers,
//                           names and strands compared, swap / floor mid-point / cut -> one record per line; the first exotic line
//            k16_names      the distinct name hashes of the kept lines -> a small table: hash -> first line (per workgroup in LDS first)
//            k16_names_out  the table's entries, compacted, for the host
//   commit   k16_apply      the host's answer (hash -> chromosome id or "drop", with the names' bytes) applied to every record:
//                           the name's bytes are compared with the dictionary's copy (a hash is not proof)
//            radix sort     (id, line) pairs by id: stable, so every chromosome's PETs stay in line order
//            k16_bounds     where every id starts in the sorted order
//            k16_gather     the kept records, grouped by chromosome, into a segment of the handle
//   finish   per chromosome: the segments' pieces copied into one array each; with `unique`, a stable sort of (cA, cB) with the row as
//            payload, the first of every run kept, compaction in row order; the distances of the PETs whose strands differ, ordered by
//            their global line number
// The reading rules are those of cloops_amd/io.py:parse_bedpe under Python 3's text mode; what a kernel should not
// restate of Python's int() and str makes a line EXOTIC, and the host then reads the files itself.
#define K16_T 256                                // lines per parse workgroup (one per lane)
#define K16_LDS (40 * 1024)                      // bytes of a staged tile: 4 workgroups per CU
#define K16_SLOTS (1 << 17)                      // slots of the names table
#define K16_LTAB 1024                            // slots of a workgroup's names table in LDS
#define K16_NAMES_MAX (1 << 16)                  // distinct names of one chunk the table takes (more: the host reads the files)
#define K16_NAME_LEN 255                         // longest chromosome name read on the device
#define K16_KEPT 1u
#define K16_STRANDS 2u
#define K16_EXOTIC 4u
#define K16_HEADER 8u                            // pairs: a '#' line (no PET; it does not count in the lines of the read)

struct K16Rec {                                  // one parsed line
    long long cA, cB;                            // the mid-points, left one first
    u64 hash;                                    // of the chromosome name (never 0)
    u32 off, len;                                // the name in the chunk
    u32 flags, pad;                              // pairs, a line the converter raises on: its CL_CONV_E_* kind << 8
};

struct K16Name { u64 hash; u32 first, off, len, pad; };                // what the host reads per distinct name of a chunk

// the integer of the bytes [s, e): 0 and v for [+-]?[0-9]+ with |v| < 2^62; 1 for a field int() rejects too (all bytes 0x21 .. 0x7e,
// no '_'; the empty field); 2 (exotic) for anything else
__device__ __forceinline__ int k16_int(K15Rd& rd, long long s, long long e, long long& v)
{
    bool plain = true, digits = e > s, big = false, neg = false;
    u64 m = 0;
    for (long long q = s; q < e; ++q) {
        const u32 c = rd.at(q);
        plain = plain && c >= 0x21u && c <= 0x7eu && c != (u32)'_';
        if (q == s && (c == '+' || c == '-')) { neg = c == '-'; digits = e > s + 1; continue; }
        const u32 d = c - (u32)'0';
        if (d > 9) digits = false;
        else if (m >= (1ull << 62) / 10) big = true;                    // stays below 2^62 after the step otherwise
        else m = m * 10 + d;
    }
    if (digits) {
        if (big) return 2;                                              // Python goes on with a long: not restated
        v = neg ? -(long long)m : (long long)m;
        return 0;
    }
    return plain ? 1 : 2;
}

// the last step of a name's hash (FNV-1a over its bytes before): never 0
__device__ __forceinline__ u64 k16_hash_end(u64 h)
{
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
    return h ? h : 1;
}

// one line [s, e) (e: its '\n') -> its record
__device__ __forceinline__ void k16_line(K15Rd& rd, long long s, long long e, long long cut, K16Rec& r)
{
    if (e > s && rd.at(e - 1) == '\r') --e;                             // "\r\n" is one line end
    long long fs[10], fe[10];
    long long q = s;
    bool have = true, star = false, minus1 = false, exotic = false;
    u64 h = 0xcbf29ce484222325ull;
#pragma unroll
    for (int k = 0; k < 10; ++k) {                                      // fields 0 .. 9: bounds in registers
        if (k > 0) { have = have && q < e; if (have) ++q; }             // the '\t' that ended field k - 1
        fs[k] = q;
        u32 b0 = 0, b1 = 0;
        if (have) {
            while (q < e) {
                const u32 c = rd.at(q);
                if (c == '\t') break;
                exotic = exotic || c >= 0x80u || c == '\r';
                if (q == fs[k]) b0 = c;
                if (q == fs[k] + 1) b1 = c;
                if (k == 0) h = (h ^ c) * 0x100000001b3ull;
                ++q;
            }
            star = star || (q - fs[k] == 1 && b0 == '*');
            minus1 = minus1 || (q - fs[k] == 2 && b0 == '-' && b1 == '1');
        }
        fe[k] = q;
    }
    const bool ten = have;
    while (have && q < e) {                                             // the fields past the tenth: only the '*' / '-1' rule reads them
        ++q;
        const long long f0 = q;
        u32 b0 = 0, b1 = 0;
        while (q < e) {
            const u32 c = rd.at(q);
            if (c == '\t') break;
            exotic = exotic || c >= 0x80u || c == '\r';
            if (q == f0) b0 = c;
            if (q == f0 + 1) b1 = c;
            ++q;
        }
        star = star || (q - f0 == 1 && b0 == '*');
        minus1 = minus1 || (q - f0 == 2 && b0 == '-' && b1 == '1');
    }
    r.hash = k16_hash_end(h);
    r.off = (u32)fs[0];
    r.len = (u32)(fe[0] - fs[0]);
    r.cA = r.cB = 0;
    r.pad = 0;
    u32 flags = 0;
    bool keep = ten && !(star && minus1);
    long long v[4] = {0, 0, 0, 0};
    if (ten) {                                                          // the integers of fields 1, 2, 4, 5
        const int k1 = k16_int(rd, fs[1], fe[1], v[0]), k2 = k16_int(rd, fs[2], fe[2], v[1]);
        const int k4 = k16_int(rd, fs[4], fe[4], v[2]), k5 = k16_int(rd, fs[5], fe[5], v[3]);
        exotic = exotic || k1 == 2 || k2 == 2 || k4 == 2 || k5 == 2;
        keep = keep && (k1 | k2 | k4 | k5) == 0;
    }
    if (keep) {                                                         // chromA == chromB, byte for byte
        keep = fe[3] - fs[3] == fe[0] - fs[0];
        for (long long i = 0; keep && i < fe[0] - fs[0]; ++i) keep = rd.at(fs[0] + i) == rd.at(fs[3] + i);
    }
    if (keep && fe[0] - fs[0] > K16_NAME_LEN) exotic = true;
    if (keep) {
        long long sa = v[0] + v[1], sb = v[2] + v[3];                   // |v| < 2^62: no overflow
        if (sa > sb) { const long long t = sa; sa = sb; sb = t; }
        r.cA = sa >> 1;                                                 // floor, also below zero
        r.cB = sb >> 1;
        keep = !(cut > 0 && r.cB - r.cA < cut);
    }
    if (keep) {
        bool diff = fe[8] - fs[8] != fe[9] - fs[9];
        for (long long i = 0; !diff && i < fe[8] - fs[8]; ++i) diff = rd.at(fs[8] + i) != rd.at(fs[9] + i);
        flags |= K16_KEPT | (diff ? K16_STRANDS : 0u);
    }
    r.flags = flags | (exotic ? K16_EXOTIC : 0u);
}

// K18: one line [s, e) of a 4DN pairs file -> the record k16_line makes of the BEDPE line that K15 (CL_CONV_PAIRS, `ext`) writes for
// it, `A0 A1 A2 B0 B1 B2 f0 . f5 f6` -> 0, or the kind of the error the converter raises on it (the record is not kept then)
__device__ __forceinline__ int k18_line(K15Rd& rd, long long s, long long e, long long cut, long long ext, K16Rec& r)
{
    r.cA = r.cB = 0;
    r.hash = 1;
    r.off = r.len = 0;
    r.pad = 0;
    if (s < e && rd.at(s) == '#') { r.flags = K16_HEADER; return 0; }
    long long fs[7], fe[7], v[4];
    int kind = k15_tabs7(rd, s, e, fs, fe) ? 0 : CL_CONV_E_FIELDS;
    if (!kind) kind = k15_ends<2, 5, 4, 6>(rd, fs, fe, ext, v);
    if (kind) { r.flags = (u32)kind << 8; return kind; }
    bool exotic = false;                                                // what Python 3's text mode would change in the copied bytes
    for (long long q = s, qe = e > s && rd.at(e - 1) == '\r' ? e - 1 : e; q < qe; ++q) {
        const u32 c = rd.at(q);
        exotic = exotic || c >= 0x80u || c == '\r';
    }
    const long long big = 1ll << 62;
#pragma unroll
    for (int k = 0; k < 4; ++k) exotic = exotic || v[k] >= big || v[k] <= -big;
    bool star = false, minus1 = v[0] == -1 || v[1] == -1 || v[2] == -1 || v[3] == -1;
    const int copied[5] = {0, 1, 3, 5, 6};                              // the fields of the BEDPE line that are not integers
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const long long f0 = fs[copied[k]], n = fe[copied[k]] - f0;
        star = star || (n == 1 && rd.at(f0) == '*');
        minus1 = minus1 || (n == 2 && rd.at(f0) == '-' && rd.at(f0 + 1) == '1');
    }
    const long long nlen = fe[1] - fs[1];
    bool keep = !(star && minus1) && fe[3] - fs[3] == nlen;
    u64 h = 0xcbf29ce484222325ull;
    for (long long i = 0; keep && i < nlen; ++i) {                      // chr1 == chr2, byte for byte
        const u32 c = rd.at(fs[1] + i);
        keep = c == rd.at(fs[3] + i);
        h = (h ^ c) * 0x100000001b3ull;
    }
    u32 flags = 0;
    if (keep) {
        r.hash = k16_hash_end(h);
        r.off = (u32)fs[1];
        r.len = (u32)nlen;
        if (nlen > K16_NAME_LEN) exotic = true;
    }
    if (keep && !exotic) {
        long long sa = v[0] + v[1], sb = v[2] + v[3];                   // |v| < 2^62: no overflow
        if (sa > sb) { const long long t = sa; sa = sb; sb = t; }
        r.cA = sa >> 1;                                                 // floor, also below zero
        r.cB = sb >> 1;
        keep = !(cut > 0 && r.cB - r.cA < cut);
    }
    if (keep) {
        bool diff = fe[5] - fs[5] != fe[6] - fs[6];
        for (long long i = 0; !diff && i < fe[5] - fs[5]; ++i) diff = rd.at(fs[5] + i) != rd.at(fs[6] + i);
        flags |= K16_KEPT | (diff ? K16_STRANDS : 0u);
    }
    r.flags = flags | (exotic ? K16_EXOTIC : 0u);
    return 0;
}

template <int FMT>
__device__ __forceinline__ void k16_any(K15Rd& rd, long long s, long long e, long long cut, long long ext, K16Rec& r)
{
    if (FMT == CL_INGEST_PAIRS) (void)k18_line(rd, s, e, cut, ext, r);
    else k16_line(rd, s, e, cut, r);
}

// lines [256 b, 256 b + 256) of the chunk -> their records; the first exotic line -> err[0]; pairs: the first line the converter
// raises on -> err[7], the header lines counted in err[10]
template <int FMT>
__global__ void __launch_bounds__(K16_T)
k16_parse(const uint4* __restrict__ in, const u32* __restrict__ ends, long long L, long long cut, long long ext, K16Rec* __restrict__ rec,
          int* __restrict__ err)
{
    extern __shared__ uint4 k16_lds[];
    __shared__ int wmin[2][K16_T / 64];
    const long long q0 = (long long)blockIdx.x * K16_T;
    const long long q1 = q0 + K16_T < L ? q0 + K16_T : L;
    const long long a0 = (q0 > 0 ? (long long)ends[q0 - 1] + 1 : 0) & ~15ll;
    const long long a1 = ((long long)ends[q1 - 1] + 1 + 15) & ~15ll;        // the tile's bytes, its last '\n' included
    const bool fits = a1 - a0 <= K16_LDS;
    if (fits)
        for (long long i = threadIdx.x; i < (a1 - a0) >> 4; i += K16_T) k16_lds[i] = in[(a0 >> 4) + i];
    __syncthreads();
    const long long j = q0 + threadIdx.x;
    int bad = INT_MAX, raised = INT_MAX;
    bool header = false;
    if (j < q1) {
        const long long s = j > 0 ? (long long)ends[j - 1] + 1 : 0, e = ends[j];
        K16Rec r;
        if (fits) {
            K15Rd rd{(const u64*)k16_lds, a0, -1, 0};
            k16_any<FMT>(rd, s, e, cut, ext, r);
        } else {
            K15Rd rd{(const u64*)in, 0, -1, 0};
            k16_any<FMT>(rd, s, e, cut, ext, r);
        }
        if (FMT == CL_INGEST_PAIRS) {
            if (r.flags >> 8) raised = (int)j;
            header = (r.flags & K16_HEADER) != 0;
        }
        if (r.flags & K16_EXOTIC) bad = (int)j;
        rec[j] = r;
    }
    bad = dpp_reduce_wave(bad, OpMin());
    if (FMT == CL_INGEST_PAIRS) {
        raised = dpp_reduce_wave(raised, OpMin());
        const int nh = __popcll(__ballot(header));
        if ((threadIdx.x & 63) == 0 && nh) atomicAdd(&err[10], nh);
    }
    if ((threadIdx.x & 63) == 0) { wmin[0][threadIdx.x >> 6] = bad; wmin[1][threadIdx.x >> 6] = raised; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int m = min(min(wmin[0][0], wmin[0][1]), min(wmin[0][2], wmin[0][3]));
        if (m != INT_MAX) atomicMin(err, m);
        const int m2 = min(min(wmin[1][0], wmin[1][1]), min(wmin[1][2], wmin[1][3]));
        if (FMT == CL_INGEST_PAIRS && m2 != INT_MAX) atomicMin(&err[7], m2);
    }
}

// the names table: key[slot] = hash (0: free), first[slot] = the first line it occurs on; ctr[0] counts the names, ctr[1] is set when
// the table is full.  Both atomics are skipped when a plain read shows nothing to do (a stale read only costs the atomic)
__device__ __forceinline__ void k16_insert(u64* __restrict__ key, u32* __restrict__ first, u32* __restrict__ ctr, u64 h, u32 j)
{
    u32 slot = (u32)h & (K16_SLOTS - 1);
    for (int probe = 0; probe < K16_SLOTS; ++probe) {
        u64 cur = key[slot];
        if (cur == 0) {
            cur = atomicCAS((unsigned long long*)&key[slot], 0ull, (unsigned long long)h);
            if (cur == 0) {
                if (atomicAdd(&ctr[0], 1u) >= K16_NAMES_MAX) ctr[1] = 1u;
                cur = h;
            }
        }
        if (cur == h) {
            if (first[slot] > j) atomicMin(&first[slot], j);
            return;
        }
        if (ctr[1]) return;                                             // full: the host reads the files itself
        slot = (slot + 1) & (K16_SLOTS - 1);
    }
    ctr[1] = 1u;
}

// 256 lines per workgroup: their hashes go through a table in LDS first (1024 slots for at most 256 names: never full), so that the
// global table sees every name once per workgroup, not once per line -- the lines of a file share a few dozen names
__global__ void __launch_bounds__(TPB)
k16_names(const K16Rec* __restrict__ rec, long long L, u64* __restrict__ key, u32* __restrict__ first, u32* __restrict__ ctr)
{
    __shared__ unsigned long long lk[K16_LTAB];
    __shared__ u32 lf[K16_LTAB];
    for (int i = threadIdx.x; i < K16_LTAB; i += TPB) { lk[i] = 0ull; lf[i] = 0xffffffffu; }
    __syncthreads();
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    if (j < L && (rec[j].flags & K16_KEPT)) {
        const unsigned long long h = rec[j].hash;
        u32 slot = (u32)(h >> 32) & (K16_LTAB - 1);
        for (int probe = 0; probe < K16_LTAB; ++probe) {
            unsigned long long cur = lk[slot];
            if (cur == 0ull) {
                cur = atomicCAS(&lk[slot], 0ull, h);
                if (cur == 0ull) cur = h;
            }
            if (cur == h) { atomicMin(&lf[slot], (u32)(j - (long long)blockIdx.x * TPB)); break; }
            slot = (slot + 1) & (K16_LTAB - 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < K16_LTAB; i += TPB)
        if (lk[i] != 0ull) k16_insert(key, first, ctr, lk[i], (u32)((long long)blockIdx.x * TPB + lf[i]));
}

__global__ void __launch_bounds__(TPB)
k16_names_out(const u64* __restrict__ key, const u32* __restrict__ first, const K16Rec* __restrict__ rec, long long L, u32* __restrict__ ctr,
              K16Name* __restrict__ out)
{
    const u32 slot = blockIdx.x * TPB + threadIdx.x;
    if (slot >= K16_SLOTS || key[slot] == 0) return;
    const u32 f = first[slot];
    if ((long long)f >= L) return;
    const u32 p = atomicAdd(&ctr[2], 1u);
    if (p >= K16_NAMES_MAX) return;
    K16Name nm;
    nm.hash = key[slot]; nm.first = f; nm.off = rec[f].off; nm.len = rec[f].len; nm.pad = 0;
    out[p] = nm;
}

// the host's table (hashes ascending) applied to every line: key = chromosome id, n_ids for a line that is not kept or whose
// chromosome is dropped; val = the line.  status[0] != 0: a name whose bytes differ from the dictionary's (1), a hash the table lacks (2)
__global__ void __launch_bounds__(TPB)
k16_apply(const uint4* __restrict__ in, const K16Rec* __restrict__ rec, long long L, const u64* __restrict__ th, const int* __restrict__ tid,
          const u32* __restrict__ toff, const u32* __restrict__ tlen, int nt, const unsigned char* __restrict__ blob, u32 n_ids,
          u32* __restrict__ key, u32* __restrict__ val, int* __restrict__ status)
{
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    if (j >= L) return;
    const K16Rec r = rec[j];
    u32 k = n_ids;
    if (r.flags & K16_KEPT) {
        int lo = 0, hi = nt;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (th[mid] < r.hash) lo = mid + 1; else hi = mid;
        }
        if (lo >= nt || th[lo] != r.hash) {
            atomicMax(status, 2);
        } else {
            bool same = tlen[lo] == r.len;
            K15Rd rd{(const u64*)in, 0, -1, 0};
            for (u32 i = 0; same && i < r.len; ++i) same = rd.at((long long)r.off + i) == blob[toff[lo] + i];
            if (!same) atomicMax(status, 1);
            else if (tid[lo] >= 0) k = (u32)tid[lo];
        }
    }
    key[j] = k;
    val[j] = (u32)j;
}

// start[id] = the first position of the sorted keys that holds id or more (id = 0 .. n_ids: start[n_ids] = the kept lines)
__global__ void __launch_bounds__(TPB)
k16_bounds(const u32* __restrict__ sk, long long L, u32 n_ids, u32* __restrict__ start)
{
    const u32 id = blockIdx.x * TPB + threadIdx.x;
    if (id > n_ids) return;
    long long lo = 0, hi = L;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (sk[mid] < id) lo = mid + 1; else hi = mid;
    }
    start[id] = (u32)lo;
}

__global__ void __launch_bounds__(TPB)
k16_gather(const K16Rec* __restrict__ rec, const u32* __restrict__ sv, long long n, long long line0, long long* __restrict__ a,
           long long* __restrict__ b, long long* __restrict__ gl, unsigned char* __restrict__ sf)
{
    const long long p = (long long)blockIdx.x * TPB + threadIdx.x;
    if (p >= n) return;
    const u32 j = sv[p];
    const K16Rec r = rec[j];
    a[p] = r.cA;
    b[p] = r.cB;
    if (gl) { gl[p] = line0 + j; sf[p] = (r.flags & K16_STRANDS) ? 1 : 0; }
}

// ---- finish: duplicates --------------------------------------------------------------------------
// key = cA << 31 | cB when both are in [0, 2^31) (*wide is set otherwise); val = the row
__global__ void __launch_bounds__(TPB)
k16_pack(const long long* __restrict__ a, const long long* __restrict__ b, long long n, u64* __restrict__ key, u32* __restrict__ val,
         int* __restrict__ wide)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    bool w = false;
    if (i < n) {
        const long long x = a[i], y = b[i];
        w = x < 0 || y < 0 || x >= (1ll << 31) || y >= (1ll << 31);
        key[i] = ((u64)x << 31) | (u64)(y & 0x7fffffffll);
        val[i] = (u32)i;
    }
    if (__any(w) && (threadIdx.x & 63) == 0) atomicOr(wide, 1);
}

__global__ void __launch_bounds__(TPB)
k16_rows(const long long* __restrict__ src, const u32* __restrict__ rows, long long n, long long* __restrict__ dst)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i < n) dst[i] = src[rows[i]];
}

// rows in (cA, cB, row) order -> keep[row] = 1 for the first row of every run of equal (cA, cB)
__global__ void __launch_bounds__(TPB)
k16_mark(const long long* __restrict__ a, const long long* __restrict__ b, const u32* __restrict__ rows, long long n, u32* __restrict__ keep)
{
    const long long p = (long long)blockIdx.x * TPB + threadIdx.x;
    if (p >= n) return;
    const u32 r = rows[p];
    bool k = true;
    if (p > 0) {
        const u32 q = rows[p - 1];
        k = a[r] != a[q] || b[r] != b[q];
    }
    keep[r] = k ? 1u : 0u;
}

__global__ void __launch_bounds__(TPB)
k16_compact(const long long* __restrict__ a, const long long* __restrict__ b, const long long* __restrict__ gl,
            const unsigned char* __restrict__ sf, const u32* __restrict__ keep, const u32* __restrict__ pos, long long n,
            long long* __restrict__ oa, long long* __restrict__ ob, long long* __restrict__ ogl, unsigned char* __restrict__ osf)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const u32 o = pos[i];
    oa[o] = a[i];
    ob[o] = b[i];
    if (gl) { ogl[o] = gl[i]; osf[o] = sf[i]; }
}

// the flagged rows of one chromosome -> (global line, distance) appended at *cnt onwards (any order: the lines are sorted afterwards)
__global__ void __launch_bounds__(TPB)
k16_dist(const long long* __restrict__ a, const long long* __restrict__ b, const long long* __restrict__ gl,
         const unsigned char* __restrict__ sf, long long n, unsigned long long* __restrict__ cnt, long long* __restrict__ dk,
         long long* __restrict__ dv)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n || !sf[i]) return;
    const unsigned long long p = atomicAdd(cnt, 1ull);
    dk[p] = gl[i];
    dv[p] = b[i] - a[i];
}

// int64 mid-points -> the int32 arrays of a cl_chrom; *bad is set when one is outside |v| < 2^29
__global__ void __launch_bounds__(TPB)
k16_xy(const long long* __restrict__ a, const long long* __restrict__ b, long long n, int* __restrict__ x, int* __restrict__ y,
       int* __restrict__ bad)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    bool w = false;
    if (i < n) {
        const long long p = a[i], q = b[i];
        w = p <= -(1ll << 29) || p >= (1ll << 29) || q <= -(1ll << 29) || q >= (1ll << 29);
        x[i] = (int)p;
        y[i] = (int)q;
    }
    if (__any(w) && (threadIdx.x & 63) == 0) atomicOr(bad, 1);
}

// ---- K16 host side ------------------------------------------------------------------------------
struct K16Seg {                                   // the kept PETs of one chunk, grouped by chromosome
    long long chunk = 0, n = 0;
    DevBuf a, b, gl, sf;
    std::vector<u32> start;                       // id -> its first position; start[n_ids of that chunk] = n
};

struct K16Chrom {
    long long n = 0;
    DevBuf a, b, gl, sf, x, y;
    int xy = 0;                                   // 0: not made; 1: made; -1: outside the cl_chrom domain
};

enum { K16_MS_H2D = 0, K16_MS_INDEX, K16_MS_PARSE, K16_MS_NAMES, K16_MS_COMMIT, K16_MS_FINISH, K16_MS_N };

struct cl_ingest {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    long long budget = 0, cut = 0;
    bool want_dist = false;
    int fmt = CL_INGEST_BEDPE;                    // cl_ingest_set_format
    long long ext = 0;
    bool any_feed = false;
    long long err_line = 0, headers = 0;          // of the last feed: cl_ingest_error, cl_ingest_headers
    int err_kind = 0;
    struct Feed { DevBuf in, rec, ends, key, val, skey, sval; } fd;   // what only a feed and its commit need: cl_ingest_finish drops them first
    DevBuf tcnt, toff, tmp, err, nkey, nfirst, nout, th, tid, tof, tln, blob, start;
    long long L = 0;                              // lines of the last feed
    bool fed = false;
    u32 n_names = 0;
    std::vector<std::unique_ptr<K16Seg>> segs;
    std::vector<std::unique_ptr<K16Chrom>> chroms;
    DevBuf dist;                                  // finish: the distances in global line order
    long long n_dist = 0;
    bool finished = false;
    hipEvent_t ev[8] = {};
    float ms[K16_MS_N] = {};
};

// `delete c` frees the buffers, the segments' and chromosomes' included; the events and the stream are noted first and ended
// afterwards (as free_chrom does)
static void ingest_free(cl_ingest* c)
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

static void ingest_ms(cl_ingest* c, int k, int e0, int e1)             // after a synchronisation of the stream
{
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev[e0], c->ev[e1]) == hipSuccess) c->ms[k] += ms;
}

static inline unsigned k16_grid(long long n) { return (unsigned)((n + TPB - 1) / TPB); }

extern "C" int cl_ingest_create(int device, void* stream, int64_t budget, int64_t cut, int32_t want_distances, cl_ingest** out)
{
    if (!out) return fail(CL_ERR_ARG, "cl_ingest_create: out is null");
    *out = nullptr;
    if (budget < 1 || budget > CL_CONV_BUDGET_MAX) return fail(CL_ERR_ARG, "cl_ingest_create: budget outside 1 .. CL_CONV_BUDGET_MAX");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(CL_ERR_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(CL_ERR_ARG, "cl_ingest_create: bad device index");
    HIP_TRY(hipSetDevice(device));
    cl_ingest* c = new cl_ingest();
    c->device = device; c->budget = budget; c->cut = cut; c->want_dist = want_distances != 0;
    int rc = CL_OK;
    if (stream) c->stream = (hipStream_t)stream;
    else if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) rc = fail(CL_ERR_HIP, "hipStreamCreate");
    else c->own_stream = true;
    for (int i = 0; rc == CL_OK && i < 8; ++i)
        if (hipEventCreate(&c->ev[i]) != hipSuccess) rc = fail(CL_ERR_HIP, "hipEventCreate");
    if (rc == CL_OK) rc = c->err.ensure(64);
    if (rc == CL_OK) rc = c->nkey.ensure((size_t)K16_SLOTS * 8);
    if (rc == CL_OK) rc = c->nfirst.ensure((size_t)K16_SLOTS * 4);
    if (rc == CL_OK) rc = c->nout.ensure((size_t)K16_NAMES_MAX * sizeof(K16Name));
    if (rc != CL_OK) { ingest_free(c); return rc; }
    *out = c;
    return CL_OK;
}

template <typename T>
static int ingest_read(cl_ingest* c, T* dst, const void* src, size_t count = 1)   // values from device memory, synchronously
{
    HIP_TRY(hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CL_OK;
}

static int ingest_scan_tmp(cl_ingest* c, size_t need)
{
    return c->tmp.ensure(std::max<size_t>(need, 16));
}

// err words: [0] first exotic line, [1] commit status, [2] wide keys, [3] xy domain; [4 .. 6] names counters; [7] pairs: the first
// line the converter raises on; [8] distance count (u64); [10] pairs: header lines
static int ingest_feed(cl_ingest* c, const char* bytes, long long n, long long* L_out, int* bad, u32* ctr)
{
    const bool virt = bytes[n - 1] != '\n';                             // the input's last line, without its newline
    const long long ne = n + (virt ? 1 : 0);
    const long long tiles = (ne + K15_TILE - 1) / K15_TILE;
    int rc;
    if ((rc = c->fd.in.ensure((size_t)ne + K15_PAD)) || (rc = c->tcnt.ensure((size_t)(tiles + 1) * 4)) || (rc = c->toff.ensure((size_t)(tiles + 1) * 4)))
        return rc;
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    HIP_TRY(hipMemcpyAsync(c->fd.in.p, bytes, (size_t)n, hipMemcpyHostToDevice, c->stream));
    if (virt) HIP_TRY(hipMemsetAsync(c->fd.in.as<char>() + n, '\n', 1, c->stream));
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(hipMemsetAsync(c->tcnt.as<u32>() + tiles, 0, 4, c->stream));
    HIP_TRY(hipMemsetAsync(c->err.p, 0, 64, c->stream));
    HIP_TRY(hipMemsetAsync(c->err.p, 0x7f, 4, c->stream));            // no exotic line: 0x7f7f7f7f, above any line index
    HIP_TRY(hipMemsetAsync(c->err.as<u32>() + 7, 0x7f, 4, c->stream));
    hipLaunchKernelGGL(k15_count, dim3((unsigned)tiles), dim3(TPB), 0, c->stream, c->fd.in.as<uint4>(), ne, c->tcnt.as<u32>());
    HIP_TRY(hipGetLastError());
    if ((rc = prim_run(c->tmp, "exclusive_scan(tiles)", [&](void* tmp, size_t& nb) {
            return rocprim::exclusive_scan(tmp, nb, c->tcnt.as<u32>(), c->toff.as<u32>(), 0u, (size_t)tiles + 1, rocprim::plus<u32>(), c->stream);
        })))
        return rc;
    u32 nl = 0;
    if ((rc = ingest_read(c, &nl, c->toff.as<u32>() + tiles))) return rc;
    const long long L = nl;                                             // >= 1: the chunk ends with a '\n'
    if ((rc = c->fd.ends.ensure((size_t)L * 4)) || (rc = c->fd.rec.ensure((size_t)L * sizeof(K16Rec)))) return rc;
    hipLaunchKernelGGL(k15_lines, dim3((unsigned)tiles), dim3(TPB), 0, c->stream, c->fd.in.as<uint4>(), ne, c->toff.as<u32>(), L, c->fd.ends.as<u32>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    const dim3 pgrid((unsigned)((L + K16_T - 1) / K16_T));
    if (c->fmt == CL_INGEST_PAIRS)
        hipLaunchKernelGGL(k16_parse<CL_INGEST_PAIRS>, pgrid, dim3(K16_T), K16_LDS, c->stream, c->fd.in.as<uint4>(), c->fd.ends.as<u32>(), L, c->cut, c->ext,
                           c->fd.rec.as<K16Rec>(), c->err.as<int>());
    else
        hipLaunchKernelGGL(k16_parse<CL_INGEST_BEDPE>, pgrid, dim3(K16_T), K16_LDS, c->stream, c->fd.in.as<uint4>(), c->fd.ends.as<u32>(), L, c->cut, c->ext,
                           c->fd.rec.as<K16Rec>(), c->err.as<int>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    HIP_TRY(hipMemsetAsync(c->nkey.p, 0, (size_t)K16_SLOTS * 8, c->stream));
    HIP_TRY(hipMemsetAsync(c->nfirst.p, 0xff, (size_t)K16_SLOTS * 4, c->stream));
    u32* dctr = c->err.as<u32>() + 4;
    hipLaunchKernelGGL(k16_names, dim3(k16_grid(L)), dim3(TPB), 0, c->stream, c->fd.rec.as<K16Rec>(), L, c->nkey.as<u64>(), c->nfirst.as<u32>(), dctr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k16_names_out, dim3(k16_grid(K16_SLOTS)), dim3(TPB), 0, c->stream, c->nkey.as<u64>(), c->nfirst.as<u32>(), c->fd.rec.as<K16Rec>(),
                       L, dctr, c->nout.as<K16Name>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[4], c->stream));
    u32 words[12] = {};
    if ((rc = ingest_read(c, words, c->err.p, 12))) return rc;
    *bad = (int)words[0];
    c->headers = words[10];
    if ((long long)words[7] < L) {                                      // pairs: a line the converter raises on
        u32 flags = 0;
        if ((rc = ingest_read(c, &flags, (const char*)c->fd.rec.p + (size_t)words[7] * sizeof(K16Rec) + offsetof(K16Rec, flags)))) return rc;
        c->err_line = (long long)words[7] + 1;
        c->err_kind = (int)(flags >> 8);
    }
    ctr[0] = words[4]; ctr[1] = words[5]; ctr[2] = words[6];
    *L_out = L;
    ingest_ms(c, K16_MS_H2D, 0, 1);
    ingest_ms(c, K16_MS_INDEX, 1, 2);
    ingest_ms(c, K16_MS_PARSE, 2, 3);
    ingest_ms(c, K16_MS_NAMES, 3, 4);
    return CL_OK;
}

extern "C" int cl_ingest_feed(cl_ingest* c, const char* bytes, int64_t n, int64_t* n_lines, int64_t* first_exotic, int64_t* n_names)
{
    if (!c) return fail(CL_ERR_ARG, "null ingest handle");
    if (n_lines) *n_lines = 0;
    if (first_exotic) *first_exotic = -1;
    if (n_names) *n_names = 0;
    if (!n_lines || !first_exotic || !n_names || n < 0 || (n > 0 && !bytes)) return fail(CL_ERR_ARG, "cl_ingest_feed: bad arguments");
    if (n > c->budget) return fail(CL_ERR_ARG, "cl_ingest_feed: more bytes than the handle's budget");
    if (c->finished) return fail(CL_ERR_ARG, "cl_ingest_feed: the handle is finished");
    c->fed = false; c->L = 0; c->n_names = 0;
    c->any_feed = true; c->err_line = 0; c->err_kind = 0; c->headers = 0;
    if (n == 0) { c->fed = true; return CL_OK; }
    HIP_TRY(hipSetDevice(c->device));
    long long L = 0;
    int bad = INT_MAX;
    u32 ctr[3] = {};
    const int rc = ingest_feed(c, bytes, n, &L, &bad, ctr);
    if (rc != CL_OK) {
        (void)hipStreamSynchronize(c->stream);                          // no copy from `bytes` may still be pending
        return rc;
    }
    c->L = L;
    c->fed = true;
    *n_lines = L;
    if (bad < L) *first_exotic = bad;
    if (ctr[1] || ctr[0] > K16_NAMES_MAX) { *n_names = -1; return CL_OK; }   // more distinct names than the table takes
    c->n_names = ctr[2];
    *n_names = ctr[2];
    return CL_OK;
}

extern "C" int cl_ingest_set_format(cl_ingest* c, int32_t format, int64_t ext)
{
    if (!c) return fail(CL_ERR_ARG, "null ingest handle");
    if (format != CL_INGEST_BEDPE && format != CL_INGEST_PAIRS) return fail(CL_ERR_ARG, "cl_ingest_set_format: unknown format");
    if (c->any_feed) return fail(CL_ERR_ARG, "cl_ingest_set_format: allowed only before the first feed");
    c->fmt = format;
    c->ext = ext;
    return CL_OK;
}

extern "C" int cl_ingest_error(cl_ingest* c, int64_t* line, int32_t* kind)
{
    if (!c) return fail(CL_ERR_ARG, "null ingest handle");
    if (!line || !kind) return fail(CL_ERR_ARG, "cl_ingest_error: bad arguments");
    *line = c->err_line;
    *kind = c->err_kind;
    return CL_OK;
}

extern "C" int cl_ingest_headers(cl_ingest* c, int64_t* n)
{
    if (!c) return fail(CL_ERR_ARG, "null ingest handle");
    if (!n) return fail(CL_ERR_ARG, "cl_ingest_headers: bad arguments");
    *n = c->headers;
    return CL_OK;
}

extern "C" int cl_ingest_names(cl_ingest* c, cl_ingest_name* out, int64_t cap, int64_t* n)
{
    if (!c) return fail(CL_ERR_ARG, "null ingest handle");
    if (n) *n = 0;
    if (!n || !c->fed || cap < (int64_t)c->n_names || (c->n_names && !out)) return fail(CL_ERR_ARG, "cl_ingest_names: bad arguments");
    static_assert(sizeof(cl_ingest_name) == sizeof(K16Name), "cl_ingest_name is K16Name");
    if (c->n_names == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    const int rc = ingest_read(c, (K16Name*)out, c->nout.p, c->n_names);
    if (rc != CL_OK) return rc;
    *n = c->n_names;
    return CL_OK;
}

static int ingest_sort_pairs_u32(cl_ingest* c, u32* ki, u32* ko, u32* vi, u32* vo, size_t n, unsigned bits)
{
    return prim_run(c->tmp, "radix_sort_pairs", [&](void* tmp, size_t& nb) {
        return rocprim::radix_sort_pairs(tmp, nb, ki, ko, vi, vo, n, 0, bits, c->stream);
    });
}

extern "C" int cl_ingest_commit(cl_ingest* c, int64_t chunk, int64_t line0, const uint64_t* hashes, const int32_t* ids, const uint32_t* name_off,
                                const uint32_t* name_len, int32_t n_table, const char* names, int64_t names_bytes, int32_t n_ids, int64_t* counts,
                                int32_t* status)
{
    if (!c) return fail(CL_ERR_ARG, "null ingest handle");
    if (status) *status = 0;
    if (!status || !c->fed || n_table < 0 || n_ids < 0 || names_bytes < 0 || (n_ids > 0 && !counts) ||
        (n_table > 0 && (!hashes || !ids || !name_off || !name_len)) || (names_bytes > 0 && !names))
        return fail(CL_ERR_ARG, "cl_ingest_commit: bad arguments");
    for (int i = 0; i < n_ids; ++i) counts[i] = 0;
    for (int i = 0; i < n_table; ++i) {
        if (i > 0 && hashes[i] <= hashes[i - 1]) return fail(CL_ERR_ARG, "cl_ingest_commit: hashes must ascend");
        if ((int64_t)name_off[i] + name_len[i] > names_bytes || ids[i] >= n_ids) return fail(CL_ERR_ARG, "cl_ingest_commit: a table entry out of range");
    }
    const long long L = c->L;
    c->fed = false;
    if (L == 0 || n_ids == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    const size_t nt = (size_t)std::max(n_table, 1);
    if ((rc = c->th.ensure(nt * 8)) || (rc = c->tid.ensure(nt * 4)) || (rc = c->tof.ensure(nt * 4)) || (rc = c->tln.ensure(nt * 4)) ||
        (rc = c->blob.ensure((size_t)std::max<int64_t>(names_bytes, 16))) || (rc = c->fd.key.ensure((size_t)L * 4)) || (rc = c->fd.val.ensure((size_t)L * 4)) ||
        (rc = c->fd.skey.ensure((size_t)L * 4)) || (rc = c->fd.sval.ensure((size_t)L * 4)) || (rc = c->start.ensure(((size_t)n_ids + 1) * 4)))
        return rc;
    HIP_TRY(hipEventRecord(c->ev[5], c->stream));
    if (n_table > 0) {
        HIP_TRY(hipMemcpyAsync(c->th.p, hashes, (size_t)n_table * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->tid.p, ids, (size_t)n_table * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->tof.p, name_off, (size_t)n_table * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->tln.p, name_len, (size_t)n_table * 4, hipMemcpyHostToDevice, c->stream));
        if (names_bytes > 0) HIP_TRY(hipMemcpyAsync(c->blob.p, names, (size_t)names_bytes, hipMemcpyHostToDevice, c->stream));
    }
    int* dstatus = c->err.as<int>() + 1;
    HIP_TRY(hipMemsetAsync(dstatus, 0, 4, c->stream));
    hipLaunchKernelGGL(k16_apply, dim3(k16_grid(L)), dim3(TPB), 0, c->stream, c->fd.in.as<uint4>(), c->fd.rec.as<K16Rec>(), L, c->th.as<u64>(), c->tid.as<int>(),
                       c->tof.as<u32>(), c->tln.as<u32>(), (int)n_table, c->blob.as<unsigned char>(), (u32)n_ids, c->fd.key.as<u32>(), c->fd.val.as<u32>(),
                       dstatus);
    HIP_TRY(hipGetLastError());
    unsigned bits = 1;
    while ((1u << bits) <= (unsigned)n_ids) ++bits;                     // keys 0 .. n_ids
    if ((rc = ingest_sort_pairs_u32(c, c->fd.key.as<u32>(), c->fd.skey.as<u32>(), c->fd.val.as<u32>(), c->fd.sval.as<u32>(), (size_t)L, bits))) return rc;
    hipLaunchKernelGGL(k16_bounds, dim3(k16_grid(n_ids + 1)), dim3(TPB), 0, c->stream, c->fd.skey.as<u32>(), L, (u32)n_ids, c->start.as<u32>());
    HIP_TRY(hipGetLastError());
    std::unique_ptr<K16Seg> s(new K16Seg());
    s->chunk = chunk;
    s->start.resize((size_t)n_ids + 1);
    int st = 0;
    HIP_TRY(hipMemcpyAsync(&st, dstatus, 4, hipMemcpyDeviceToHost, c->stream));
    rc = ingest_read(c, s->start.data(), c->start.p, (size_t)n_ids + 1);
    if (rc != CL_OK || st != 0) {
        *status = st;
        return rc;
    }
    s->n = s->start[n_ids];
    if (s->n > 0) {
        if ((rc = s->a.ensure((size_t)s->n * 8)) || (rc = s->b.ensure((size_t)s->n * 8)) ||
            (c->want_dist && ((rc = s->gl.ensure((size_t)s->n * 8)) || (rc = s->sf.ensure((size_t)s->n))))) return rc;
        hipLaunchKernelGGL(k16_gather, dim3(k16_grid(s->n)), dim3(TPB), 0, c->stream, c->fd.rec.as<K16Rec>(), c->fd.sval.as<u32>(), s->n, (long long)line0,
                           s->a.as<long long>(), s->b.as<long long>(), c->want_dist ? s->gl.as<long long>() : nullptr,
                           c->want_dist ? s->sf.as<unsigned char>() : nullptr);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(c->ev[6], c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(CL_ERR_HIP, "cl_ingest_commit: gather", hipGetErrorString(e));
        ingest_ms(c, K16_MS_COMMIT, 5, 6);
        for (int i = 0; i < n_ids; ++i) counts[i] = (int64_t)s->start[i + 1] - s->start[i];
        c->segs.push_back(std::move(s));
    }
    return CL_OK;
}

// the duplicates of one chromosome removed (the first of every (cA, cB) kept, row order kept)
static int ingest_unique(cl_ingest* c, K16Chrom* h)
{
    const long long n = h->n;
    if (n < 2) return CL_OK;
    if (n >= (1ll << 31)) return fail(CL_ERR_ARG, "cl_ingest_finish: more than 2^31 PETs on one chromosome");
    int rc;
    DevBuf k0, k1, v0, v1, keep, pos;
    if ((rc = k0.ensure((size_t)n * 8)) || (rc = k1.ensure((size_t)n * 8)) || (rc = v0.ensure((size_t)n * 4)) || (rc = v1.ensure((size_t)n * 4)) ||
        (rc = keep.ensure((size_t)n * 4)) || (rc = pos.ensure((size_t)n * 4))) return rc;
    int* dwide = c->err.as<int>() + 2;
    hipError_t e = hipMemsetAsync(dwide, 0, 4, c->stream);
    hipLaunchKernelGGL(k16_pack, dim3(k16_grid(n)), dim3(TPB), 0, c->stream, h->a.as<long long>(), h->b.as<long long>(), n, k0.as<u64>(), v0.as<u32>(), dwide);
    int wide = 0;
    if (e != hipSuccess || (rc = ingest_read(c, &wide, dwide))) return e != hipSuccess ? fail(CL_ERR_HIP, "cl_ingest_finish: memset") : rc;
    size_t bytes_tmp = 0;
    const u32* rows = nullptr;
    if (!wide) {                                                        // one packed key of 62 bits
        rc = prim_run(c->tmp, "cl_ingest_finish: radix_sort_pairs", [&](void* tmp, size_t& nb) {
            return rocprim::radix_sort_pairs(tmp, nb, k0.as<u64>(), k1.as<u64>(), v0.as<u32>(), v1.as<u32>(), (size_t)n, 0, 62, c->stream);
        });
        rows = v1.as<u32>();
    } else {                                                            // any int64: by cB, then (stable) by cA; sized once for the two sorts
        e = rocprim::radix_sort_pairs(nullptr, bytes_tmp, (long long*)nullptr, (long long*)nullptr, (u32*)nullptr, (u32*)nullptr, (size_t)n, 0, 64, c->stream);
        if (e == hipSuccess && (rc = ingest_scan_tmp(c, bytes_tmp)) == CL_OK) {
            bytes_tmp = c->tmp.bytes;
            e = rocprim::radix_sort_pairs(c->tmp.p, bytes_tmp, h->b.as<long long>(), k1.as<long long>(), v0.as<u32>(), v1.as<u32>(), (size_t)n, 0, 64, c->stream);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k16_rows, dim3(k16_grid(n)), dim3(TPB), 0, c->stream, h->a.as<long long>(), v1.as<u32>(), n, k0.as<long long>());
                bytes_tmp = c->tmp.bytes;
                e = rocprim::radix_sort_pairs(c->tmp.p, bytes_tmp, k0.as<long long>(), k1.as<long long>(), v1.as<u32>(), v0.as<u32>(), (size_t)n, 0, 64, c->stream);
            }
        }
        rows = v0.as<u32>();
    }
    if (rc != CL_OK) return rc;
    if (e != hipSuccess) return fail(CL_ERR_HIP, "cl_ingest_finish: radix_sort_pairs", hipGetErrorString(e));
    hipLaunchKernelGGL(k16_mark, dim3(k16_grid(n)), dim3(TPB), 0, c->stream, h->a.as<long long>(), h->b.as<long long>(), rows, n, keep.as<u32>());
    rc = prim_run(c->tmp, "cl_ingest_finish: exclusive_scan", [&](void* tmp, size_t& nb) {
        return rocprim::exclusive_scan(tmp, nb, keep.as<u32>(), pos.as<u32>(), 0u, (size_t)n, rocprim::plus<u32>(), c->stream);
    });
    if (rc != CL_OK) return rc;
    u32 lastp = 0, lastk = 0;
    e = hipMemcpyAsync(&lastk, keep.as<u32>() + (n - 1), 4, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess || (rc = ingest_read(c, &lastp, pos.as<u32>() + (n - 1)))) return e != hipSuccess ? fail(CL_ERR_HIP, "cl_ingest_finish: copy") : rc;
    const long long m = (long long)lastp + lastk;
    if (m < n) {
        DevBuf oa, ob, ogl, osf;
        if ((rc = oa.ensure((size_t)m * 8)) || (rc = ob.ensure((size_t)m * 8)) ||
            (c->want_dist && ((rc = ogl.ensure((size_t)m * 8)) || (rc = osf.ensure((size_t)m))))) return rc;
        hipLaunchKernelGGL(k16_compact, dim3(k16_grid(n)), dim3(TPB), 0, c->stream, h->a.as<long long>(), h->b.as<long long>(),
                           c->want_dist ? h->gl.as<long long>() : nullptr, c->want_dist ? h->sf.as<unsigned char>() : nullptr, keep.as<u32>(),
                           pos.as<u32>(), n, oa.as<long long>(), ob.as<long long>(), ogl.as<long long>(), osf.as<unsigned char>());
        e = hipStreamSynchronize(c->stream);
        h->a = std::move(oa); h->b = std::move(ob); h->gl = std::move(ogl); h->sf = std::move(osf);
        h->n = m;
        if (e != hipSuccess) return fail(CL_ERR_HIP, "cl_ingest_finish: compaction", hipGetErrorString(e));
    }
    return CL_OK;
}

extern "C" int cl_ingest_finish(cl_ingest* c, cl_ingest* other, int32_t n_ids, int32_t unique, int64_t* n_rows, int64_t* n_distances)
{
    if (!c) return fail(CL_ERR_ARG, "null ingest handle");
    if (n_distances) *n_distances = 0;
    if (n_ids < 0 || (n_ids > 0 && !n_rows) || !n_distances || other == c) return fail(CL_ERR_ARG, "cl_ingest_finish: bad arguments");
    if (c->finished || (other && other->finished)) return fail(CL_ERR_ARG, "cl_ingest_finish: finished already");
    if (other && (other->device != c->device || other->want_dist != c->want_dist)) return fail(CL_ERR_ARG, "cl_ingest_finish: handles differ");
    HIP_TRY(hipSetDevice(c->device));
    if (other) {                                                        // its segments move here
        HIP_TRY(hipStreamSynchronize(other->stream));
        c->segs.insert(c->segs.end(), std::make_move_iterator(other->segs.begin()), std::make_move_iterator(other->segs.end()));
        other->segs.clear();
        other->finished = true;
        other->fd = cl_ingest::Feed();
        other->tmp.release();
    }
    c->finished = true;
    c->fd = cl_ingest::Feed();
    std::sort(c->segs.begin(), c->segs.end(), [](const std::unique_ptr<K16Seg>& x, const std::unique_ptr<K16Seg>& y) { return x->chunk < y->chunk; });
    HIP_TRY(hipEventRecord(c->ev[5], c->stream));
    int rc = CL_OK;
    long long total = 0;
    for (int id = 0; id < n_ids && rc == CL_OK; ++id) {
        c->chroms.emplace_back(new K16Chrom());
        K16Chrom* h = c->chroms.back().get();
        for (const auto& s : c->segs)
            if ((size_t)id + 1 < s->start.size()) h->n += (long long)s->start[id + 1] - s->start[id];
        if (h->n == 0) continue;
        if ((rc = h->a.ensure((size_t)h->n * 8)) || (rc = h->b.ensure((size_t)h->n * 8)) ||
            (c->want_dist && ((rc = h->gl.ensure((size_t)h->n * 8)) || (rc = h->sf.ensure((size_t)h->n)))))
            break;
        long long at = 0;
        for (const auto& s : c->segs) {
            if ((size_t)id + 1 >= s->start.size()) continue;
            const long long p = s->start[id], m = (long long)s->start[id + 1] - p;
            if (m == 0) continue;
            HIP_TRY(hipMemcpyAsync(h->a.as<long long>() + at, s->a.as<long long>() + p, (size_t)m * 8, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(h->b.as<long long>() + at, s->b.as<long long>() + p, (size_t)m * 8, hipMemcpyDeviceToDevice, c->stream));
            if (c->want_dist) {
                HIP_TRY(hipMemcpyAsync(h->gl.as<long long>() + at, s->gl.as<long long>() + p, (size_t)m * 8, hipMemcpyDeviceToDevice, c->stream));
                HIP_TRY(hipMemcpyAsync(h->sf.as<unsigned char>() + at, s->sf.as<unsigned char>() + p, (size_t)m, hipMemcpyDeviceToDevice, c->stream));
            }
            at += m;
        }
    }
    if (rc != CL_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->segs.clear();                                                    // (merged: their buffers go now)
    for (int id = 0; id < n_ids; ++id) {
        K16Chrom* h = c->chroms[id].get();
        if (unique && (rc = ingest_unique(c, h))) return rc;
        n_rows[id] = h->n;
        total += h->n;
    }
    if (c->want_dist && total > 0) {
        DevBuf dk, dv, sk;
        unsigned long long* dcnt = (unsigned long long*)(c->err.as<u32>() + 8);
        if ((rc = dk.ensure((size_t)total * 8)) || (rc = dv.ensure((size_t)total * 8))) return rc;
        hipError_t e = hipMemsetAsync(dcnt, 0, 8, c->stream);
        for (const auto& h : c->chroms)
            if (h->n > 0)
                hipLaunchKernelGGL(k16_dist, dim3(k16_grid(h->n)), dim3(TPB), 0, c->stream, h->a.as<long long>(), h->b.as<long long>(),
                                   h->gl.as<long long>(), h->sf.as<unsigned char>(), h->n, dcnt, dk.as<long long>(), dv.as<long long>());
        unsigned long long nd = 0;
        if (e != hipSuccess || (rc = ingest_read(c, &nd, dcnt))) return e != hipSuccess ? fail(CL_ERR_HIP, "cl_ingest_finish: memset") : rc;
        if (nd > 0) {
            if ((rc = sk.ensure((size_t)nd * 8)) || (rc = c->dist.ensure((size_t)nd * 8))) return rc;
            rc = prim_run(c->tmp, "cl_ingest_finish: distances", [&](void* tmp, size_t& nb) {
                return rocprim::radix_sort_pairs(tmp, nb, dk.as<long long>(), sk.as<long long>(), dv.as<long long>(), c->dist.as<long long>(), (size_t)nd, 0,
                                                 64, c->stream);
            });
            if (rc != CL_OK) return rc;
            e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) return fail(CL_ERR_HIP, "cl_ingest_finish: distances", hipGetErrorString(e));
        }
        c->n_dist = (long long)nd;
        for (const auto& h : c->chroms) { h->gl.release(); h->sf.release(); }
    }
    HIP_TRY(hipEventRecord(c->ev[6], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ingest_ms(c, K16_MS_FINISH, 5, 6);
    c->tmp.release();
    *n_distances = c->n_dist;
    return CL_OK;
}

static K16Chrom* ingest_chrom(cl_ingest* c, int32_t id)
{
    if (!c || !c->finished || id < 0 || (size_t)id >= c->chroms.size()) return nullptr;
    return c->chroms[id].get();
}

extern "C" int cl_ingest_rows(cl_ingest* c, int32_t id, int64_t* a, int64_t* b, int64_t cap)
{
    K16Chrom* h = ingest_chrom(c, id);
    if (!h || cap < h->n || (h->n > 0 && (!a || !b))) return fail(CL_ERR_ARG, "cl_ingest_rows: bad arguments");
    if (h->n == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(a, h->a.p, (size_t)h->n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(b, h->b.p, (size_t)h->n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CL_OK;
}

extern "C" int cl_ingest_chrom_arrays(cl_ingest* c, int32_t id, int64_t* n, void** x, void** y)
{
    K16Chrom* h = ingest_chrom(c, id);
    if (!h || !n || !x || !y) return fail(CL_ERR_ARG, "cl_ingest_chrom_arrays: bad arguments");
    *n = h->n; *x = nullptr; *y = nullptr;
    if (h->n == 0) return CL_OK;
    if (h->xy == 0) {
        HIP_TRY(hipSetDevice(c->device));
        int rc;
        if ((rc = h->x.ensure((size_t)h->n * 4)) || (rc = h->y.ensure((size_t)h->n * 4))) return rc;
        int* dbad = c->err.as<int>() + 3;
        HIP_TRY(hipMemsetAsync(dbad, 0, 4, c->stream));
        hipLaunchKernelGGL(k16_xy, dim3(k16_grid(h->n)), dim3(TPB), 0, c->stream, h->a.as<long long>(), h->b.as<long long>(), h->n, h->x.as<int>(),
                           h->y.as<int>(), dbad);
        HIP_TRY(hipGetLastError());
        int bad = 0;
        if ((rc = ingest_read(c, &bad, dbad))) return rc;
        h->xy = bad ? -1 : 1;
    }
    if (h->xy < 0) return fail(CL_ERR_DOMAIN, "coordinates must satisfy |X|,|Y| < 2^29");
    *x = h->x.p;
    *y = h->y.p;
    return CL_OK;
}

extern "C" int cl_ingest_distances(cl_ingest* c, int64_t* out, int64_t cap)
{
    if (!c || !c->finished || cap < c->n_dist || (c->n_dist > 0 && !out)) return fail(CL_ERR_ARG, "cl_ingest_distances: bad arguments");
    if (c->n_dist == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, c->dist.p, (size_t)c->n_dist * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CL_OK;
}

extern "C" int cl_ingest_timing(cl_ingest* c, float* ms)
{
    if (!c) return fail(CL_ERR_ARG, "null ingest handle");
    if (!ms) return fail(CL_ERR_ARG, "cl_ingest_timing: bad arguments");
    for (int i = 0; i < K16_MS_N; ++i) ms[i] = c->ms[i];
    return CL_OK;
}

extern "C" int cl_ingest_destroy(cl_ingest* c)
{
    if (!c) return CL_OK;
    ingest_free(c);
    return CL_OK;
}
