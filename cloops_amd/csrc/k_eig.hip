// k_eig.hip -- K27: compartments -- the leading eigenpairs of the O/E matrix minus one of the folded cells that K24 left on the device,
// K25 weighted and K26 gave expected values -- kernels and C entry points.
#include <cmath>
#include <vector>
#include "cl_chrom.h"

// ==========================================================================================
// K27: M = S - B (S: min(O/E, clip) of the in-band used cells, B: the 0/1 matrix of the in-band valid pairs), never stored densely;
//      subspace iteration on a block of CL_EIG_BLOCK columns
// ==========================================================================================
// Definitions: include/cloops_hip.h, cl_eig_build.  The reference has nothing of the kind; tests/compartments_cases.py restates the
// definitions in numpy.  Input: K24's cells in both orders (c->mx.bx / by as they lie, c->bl.tby / tbx transposed, K25's permutation
// c->bl.vout between the two), K26's effective weights c->ex.w (NaN = invalid bin) and expected values c->ex.exp.
// A block of vectors is laid out [nb][8] fp64: the eight columns of a bin are one 64-byte line.  Its rows at invalid bins and its columns
// from the block's width m = min(8, n_valid) on are zero, always.
//   k27_vals / k27_perm   the value of every cell: min(oe, clip) inside the band (used, ign <= d < dmax), else 0 -- as the cells lie, then
//                   the same values in the transposed order through K25's permutation.  The cells inside the band are counted (integer
//                   atomics, one per workgroup).
//   k27_rows        row pointers of both orders: one lower bound per bin over the sorted run keys (CSR without copying the cells).
//   k27_scan1 / k27_scan2   the band term's prefix sums of a block: inclusive scan inside tiles of K27_SB bins (one bin and its eight
//                   columns per thread: wave shuffles, then the four wave totals in order), then the exclusive sums of the tile totals in
//                   tile order.  P(k) = off[(k - 1) / SB] + pl[k - 1], P(0) = 0.
//   k27_mul         Z = M Q.  One wave per bin, four bins per workgroup: lane = (cell slot 0..7, column 0..7).  The row's cells of the
//                   order as they lie, then those of the transposed order without the diagonal cell, eight cells per step: the eight
//                   lanes of a slot read one cell (one address: one transaction for all eight columns) and one 64-byte line of Q.  The
//                   slots are added in a fixed tree (xor 8, 16, 32), the band term is four look-ups in the prefix sums per column.  No
//                   atomics, no carry between workgroups: the order of the additions depends on the cells alone.
//   k27_gram        the 64 dot products A^T B of two blocks: lane = (a, b), a wave walks bins at stride 4, the four waves are added in
//                   order, one partial per workgroup; the small kernels fold the partials in index order (K25's two levels).
//   k27_ritz        one wave: H = (Q^T Z + its transpose) / 2, cyclic Jacobi (round-robin pairs: 7 steps of 4 disjoint rotations a
//                   sweep, K27_SWEEPS sweeps, lane = (row, column), rotations by wave shuffles), the pairs ordered by |lambda|.
//   k27_rot         Y = Z W, V = Q W (the Ritz vectors: the result), the partial sums of |Y - V lambda|^2 per column.
//   k27_check       one wave: the residuals, the count of the iteration, `stop` in the loop's record when every asked pair meets tol.
//   k27_chol / k27_apply   Gram-Schmidt of a block in the coefficients: R of G = Y^T Y = R^T R column by column, T = R^-1, out = Y T;
//                   twice per orthonormalisation (the second pass removes what the first left of kappa^2 eps).  A column whose
//                   remainder falls to 2^-40 of its own squared norm has vanished under the projections: the first pass replaces it by the
//                   next hash vector, the second orthogonalises that.
//   k27_start / k27_final   the start block: a fixed integer hash of (column, bin); the result: sign rule, NaN on the invalid bins.
// Every kernel of the loop begins by reading `stop`; the host enqueues K27_BLOCK iterations at a time and reads the record after each.
// Only vector stores and integer HIP atomics; every index is checked against its array before a load or store; plain launches in the
// handle's stream, no workgroup waits on another.
#define K27_SB TPB                      // bins per workgroup of the scan: one per thread
#define K27_PARTS 256                   // most workgroups (= partial sums) of k27_gram / k27_rot
#define K27_BLOCK 8                     // iterations enqueued between two reads of the record
#define K27_SWEEPS 10                   // Jacobi sweeps over the 8 x 8 matrix (quadratic convergence: 6 do for fp64)
#define K27_VANISH 9.094947017729282e-13 // 2^-40
static_assert(CL_EIG_BLOCK == 8, "a bin's columns are one 64-byte line; the small kernels are one wave of 8 x 8 lanes");
static_assert(CL_EIG_MAX <= CL_EIG_BLOCK, "the asked pairs are columns of the block");
static_assert(CL_EIG_BINS_MAX == (1 << 20), "the limit of include/cloops_hip.h (the hash key: column 2^20 + bin)");

struct K27Rec {                         // the loop's record
    int iters, converged, stop, nhash;  // nhash: the next hash column
    double lam[8], res[8];
    int repl[8];                        // per column: the hash column that replaces it in k27_apply (-1: none)
};

struct K27M {                           // what k27_mul reads of M
    const int* rp[2]; const int* oth[2]; const double* val[2];                  // per order: row pointers (nb + 1), the other bin, the value
    const double* ew;                                                           // nb effective weights: NaN = invalid
    int b0, nb, ign, dmax, n;
};

__device__ __forceinline__ double k27_hash(int col, long long bin)
{
    u32 h = (u32)col * 1048576u + (u32)bin;
    h = h * 2654435761u + 0x9E3779B9u;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return ((double)(h >> 8) - 8388607.5) / 8388608.0;                          // in (-1, 1), never 0
}

// val[i] = min(oe, clip) of cell i inside the band, else 0; *n_in += the cells inside the band
__global__ void __launch_bounds__(TPB)
k27_vals(const int* __restrict__ bx, const int* __restrict__ by, const u32* __restrict__ cnt, int n, int b0, int nb, int ign, int dmax,
         const double* __restrict__ ew, const double* __restrict__ expected, double clip, double* __restrict__ val, u64* __restrict__ n_in)
{
    __shared__ u32 wu[TPB / 64];
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    u32 in = 0u;
    if (i < n) {
        const long long ix = (long long)bx[i] - b0, d = (long long)by[i] - bx[i], iy = ix + d;
        double v = 0.0;
        if (d >= ign && d < dmax && ix >= 0 && iy < nb) {                       // (d >= 0: ix <= iy; d < dmax <= nb)
            const double wx = ew[ix], wy = ew[iy];
            if (wx == wx && wy == wy) {
                const double oe = ((wx * (double)cnt[i]) * wy) / expected[d];   // (K26's order of operations; the host checked expected[d])
                v = oe < clip ? oe : clip;
                in = 1u;
            }
        }
        val[i] = v;
    }
    for (int o = 32; o > 0; o >>= 1) in += (u32)__shfl_xor((int)in, o);
    if ((threadIdx.x & 63) == 0) wu[threadIdx.x >> 6] = in;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
        for (int q = 0; q < TPB / 64; ++q) s += wu[q];
        if (s) atomicAdd(n_in, s);
    }
}

__global__ void __launch_bounds__(TPB)
k27_perm(const u32* __restrict__ order, const double* __restrict__ val, int n, double* __restrict__ tval)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const u32 j = order[i];
    tval[i] = j < (u32)n ? val[j] : 0.0;
}

// rp[k] = the first cell whose key is at or above b0 + k, k = 0 .. nb
__global__ void __launch_bounds__(TPB)
k27_rows(const int* __restrict__ key, int n, int b0, int nb, int* __restrict__ rp)
{
    const long long k = (long long)blockIdx.x * TPB + threadIdx.x;
    if (k > nb) return;
    const long long want = (long long)b0 + k;
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if ((long long)key[mid] < want) lo = mid + 1; else hi = mid; }
    rp[k] = lo;
}

// q[i][k] = x[k][i] on the valid bins for k < n_vec, else 0
__global__ void __launch_bounds__(TPB)
k27_pack(const double* __restrict__ x, int n_vec, int nb, const double* __restrict__ ew, double* __restrict__ q)
{
    const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
    const long long i = t >> 3; const int k = (int)(t & 7);
    if (i >= nb) return;
    const double w = ew[i];
    q[t] = (k < n_vec && w == w) ? x[(size_t)k * (size_t)nb + (size_t)i] : 0.0;
}

__global__ void __launch_bounds__(TPB)
k27_unpack(const double* __restrict__ z, int n_vec, int nb, double* __restrict__ y)
{
    const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
    const long long i = t >> 3; const int k = (int)(t & 7);
    if (i >= nb || k >= n_vec) return;
    y[(size_t)k * (size_t)nb + (size_t)i] = z[t];
}

__global__ void __launch_bounds__(TPB)
k27_scan1(const double* __restrict__ q, int nb, double* __restrict__ pl, double* __restrict__ tot, const K27Rec* __restrict__ rec)
{
    __shared__ double wt[TPB / 64][8];
    if (rec && rec->stop) return;
    const long long i = (long long)blockIdx.x * K27_SB + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = i < nb ? q[(size_t)i * 8 + k] : 0.0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int k = 0; k < 8; ++k) { const double t = __shfl_up(x[k], (unsigned)d); if (lane >= d) x[k] = t + x[k]; }
    }
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < 8; ++k) wt[wave][k] = x[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        double p = 0.0;
        for (int w = 0; w < wave; ++w) p = w == 0 ? wt[0][k] : p + wt[w][k];
        if (wave > 0) x[k] = p + x[k];
    }
    if (i < nb) {
#pragma unroll
        for (int k = 0; k < 8; ++k) pl[(size_t)i * 8 + k] = x[k];
    }
    if (threadIdx.x == TPB - 1) {
#pragma unroll
        for (int k = 0; k < 8; ++k) tot[(size_t)blockIdx.x * 8 + k] = x[k];       // (the bins behind nb added zeros)
    }
}

// off[T][k] = the totals of the tiles before T, in tile order
__global__ void __launch_bounds__(TPB)
k27_scan2(const double* __restrict__ tot, int ntiles, double* __restrict__ off, const K27Rec* __restrict__ rec)
{
    if (rec && rec->stop) return;
    const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
    const long long T = t >> 3; const int k = (int)(t & 7);
    if (T >= ntiles) return;
    double s = 0.0;
    for (long long u = 0; u < T; ++u) s += tot[(size_t)u * 8 + k];
    off[t] = s;
}

__device__ __forceinline__ double k27_prefix(const double* __restrict__ pl, const double* __restrict__ off, int nb, long long k, int col)
{
    if (k <= 0) return 0.0;
    if (k > nb) k = nb;
    return off[(size_t)((k - 1) / K27_SB) * 8 + col] + pl[(size_t)(k - 1) * 8 + col];
}

__global__ void __launch_bounds__(TPB)
k27_mul(K27M m, const double* __restrict__ q, const double* __restrict__ pl, const double* __restrict__ off, double* __restrict__ z,
        const K27Rec* __restrict__ rec)
{
    if (rec && rec->stop) return;
    const int lane = threadIdx.x & 63, col = lane & 7, slot = lane >> 3;
    const long long i = (long long)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (i >= m.nb) return;                                                      // (the whole wave)
    const double wi = m.ew[i];
    double acc = 0.0;
    if (wi == wi) {                                                             // (the whole wave)
        for (int ph = 0; ph < 2; ++ph) {
            const int lo = m.rp[ph][i], hi = m.rp[ph][i + 1];
            const int* __restrict__ oth = m.oth[ph];
            const double* __restrict__ val = m.val[ph];
#pragma unroll 2
            for (long long j = (long long)lo + slot; j < hi; j += 8) {
                if (j < 0 || j >= m.n) break;
                const double v = val[j];
                const long long o = (long long)oth[j] - m.b0;
                if (v == 0.0 || o < 0 || o >= m.nb || (ph && o == i)) continue; // (outside the band; the diagonal cell counts once)
                acc += v * q[(size_t)o * 8 + col];
            }
        }
    }
    acc += __shfl_xor(acc, 8);
    acc += __shfl_xor(acc, 16);
    acc += __shfl_xor(acc, 32);
    if (slot != 0) return;
    double r = 0.0;
    if (wi == wi) {
        double band = 0.0;
        if (m.dmax > m.ign) {
            const int near = m.ign > 1 ? m.ign : 1;
            const double right = k27_prefix(pl, off, m.nb, i + m.dmax, col) - k27_prefix(pl, off, m.nb, i + m.ign, col);
            const double left = k27_prefix(pl, off, m.nb, i - near + 1, col) - k27_prefix(pl, off, m.nb, i - m.dmax + 1, col);
            band = right + left;
        }
        r = acc - band;
    }
    z[(size_t)i * 8 + col] = r;
}

__global__ void __launch_bounds__(TPB)
k27_gram(const double* __restrict__ A, const double* __restrict__ B, int nb, int per, double* __restrict__ part, const K27Rec* __restrict__ rec)
{
    __shared__ double l[TPB / 64][64];
    if (rec && rec->stop) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, a = lane >> 3, b = lane & 7;
    const long long lo = (long long)blockIdx.x * per, hi = lo + per < nb ? lo + per : nb;
    double acc = 0.0;
    for (long long i = lo + wave; i < hi; i += TPB / 64) acc += A[(size_t)i * 8 + a] * B[(size_t)i * 8 + b];
    l[wave][lane] = acc;
    __syncthreads();
    if (wave == 0) {
        double s = l[0][lane];
        for (int w = 1; w < TPB / 64; ++w) s += l[w][lane];
        part[(size_t)blockIdx.x * 64 + lane] = s;
    }
}

// the partner of index i in step t of the round-robin over 8 indices: i + j == t (mod 7) among 0 .. 6, the one left over meets 7
__device__ __forceinline__ int k27_partner(int i, int t)
{
    if (i == 7) return (4 * t) % 7;
    const int j = (t - i + 7) % 7;
    return j == i ? 7 : j;
}

// the rotation that annihilates a[p][q]: (cs, sn) with col p' = cs col p - sn col q, col q' = sn col p + cs col q
__device__ __forceinline__ void k27_rotation(double app, double aqq, double apq, double& cs, double& sn)
{
    cs = 1.0; sn = 0.0;
    if (apq == 0.0 || apq != apq) return;
    const double th = (aqq - app) / (2.0 * apq);
    if (!(fabs(th) < 1e150)) return;                                            // (the rotation angle has vanished)
    const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
    cs = 1.0 / sqrt(t * t + 1.0);
    sn = t * cs;
}

// one wave.  W[a][k] (sm[a * 8 + k]): the Ritz vectors in the block's coordinates, ordered by |lambda| descending (ties: the lower
// index); rec->lam: their values.  The columns from m on stay unit vectors behind the others
__global__ void __launch_bounds__(64)
k27_ritz(const double* __restrict__ part, int np, int m, double* __restrict__ sm, K27Rec* __restrict__ rec)
{
    if (rec->stop) return;
    const int lane = threadIdx.x & 63, r = lane >> 3, c = lane & 7;
    double h = 0.0;
    for (int g = 0; g < np; ++g) h += part[(size_t)g * 64 + lane];
    h = 0.5 * (h + __shfl(h, c * 8 + r));
    double w = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < K27_SWEEPS; ++sweep) {
        for (int t = 0; t < 7; ++t) {
            const int pc = k27_partner(c, t), pr = k27_partner(r, t);
            const int cp = c < pc ? c : pc, cq = c < pc ? pc : c, rp = r < pr ? r : pr, rq = r < pr ? pr : r;
            double ccs, csn, rcs, rsn;
            k27_rotation(__shfl(h, cp * 8 + cp), __shfl(h, cq * 8 + cq), __shfl(h, cp * 8 + cq), ccs, csn);
            k27_rotation(__shfl(h, rp * 8 + rp), __shfl(h, rq * 8 + rq), __shfl(h, rp * 8 + rq), rcs, rsn);
            const double sc = c == cp ? -csn : csn, sr = r == rp ? -rsn : rsn;
            const double h1 = ccs * h + sc * __shfl(h, r * 8 + pc);             // columns
            w = ccs * w + sc * __shfl(w, r * 8 + pc);
            h = rcs * h1 + sr * __shfl(h1, pr * 8 + c);                         // rows
        }
    }
    const double mine = __shfl(h, c * 8 + c);
    const double kc = c < m ? fabs(mine) : -1.0;
    int rank = 0;
    for (int j = 0; j < 8; ++j) {
        const double lj = __shfl(h, j * 8 + j);
        const double kj = j < m ? fabs(lj) : -1.0;
        rank += (kj > kc || (kj == kc && j < c)) ? 1 : 0;
    }
    if (rank < 0 || rank > 7) return;
    sm[r * 8 + rank] = w;
    if (r == 0) rec->lam[rank] = c < m ? mine : 0.0;
}

// Y = Z W, V = Q W, rpart[g][k] = this workgroup's share of |Y_k - V_k lam_k|^2
__global__ void __launch_bounds__(TPB)
k27_rot(const double* __restrict__ Z, const double* __restrict__ Q, const double* __restrict__ sm, int nb, int per, double* __restrict__ Y,
        double* __restrict__ V, double* __restrict__ rpart, const K27Rec* __restrict__ rec)
{
    __shared__ double l[TPB / 64][8];
    if (rec->stop) return;
    const int k = threadIdx.x & 7, slot = threadIdx.x >> 3, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double wk[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) wk[a] = sm[a * 8 + k];
    const double lam = rec->lam[k];
    const long long lo = (long long)blockIdx.x * per, hi = lo + per < nb ? lo + per : nb;
    double acc = 0.0;
    for (long long i = lo + slot; i < hi; i += TPB / 8) {
        double y = 0.0, v = 0.0;
#pragma unroll
        for (int a = 0; a < 8; ++a) { y += Z[(size_t)i * 8 + a] * wk[a]; v += Q[(size_t)i * 8 + a] * wk[a]; }
        Y[(size_t)i * 8 + k] = y;
        V[(size_t)i * 8 + k] = v;
        const double d = y - v * lam;
        acc += d * d;
    }
    acc += __shfl_xor(acc, 8);
    acc += __shfl_xor(acc, 16);
    acc += __shfl_xor(acc, 32);
    if (lane < 8) l[wave][lane] = acc;
    __syncthreads();
    if (threadIdx.x < 8) {
        double s = l[0][k];
        for (int w = 1; w < TPB / 64; ++w) s += l[w][k];
        rpart[(size_t)blockIdx.x * 8 + k] = s;
    }
}

__global__ void __launch_bounds__(64)
k27_check(const double* __restrict__ rpart, int np, int n_ask, double tol, K27Rec* __restrict__ rec)
{
    if (rec->stop) return;
    const int k = threadIdx.x & 63;
    bool ok = true;
    if (k < 8) {
        double s = 0.0;
        for (int g = 0; g < np; ++g) s += rpart[(size_t)g * 8 + k];
        const double res = sqrt(s);
        rec->res[k] = res;
        ok = k >= n_ask || res <= tol * fabs(rec->lam[0]);
    }
    const u64 all = __ballot(ok);
    if (k == 0) {
        rec->iters += 1;
        if (all == ~0ull) { rec->converged = 1; rec->stop = 1; }
    }
}

// one wave folds G = A^T A; lane 0: R of G = R^T R column by column (Gram-Schmidt in the coefficients), T = R^-1 -> sm[a * 8 + k].
// A column with no remainder is marked for replacement (first pass only) and takes no part in the columns behind it
__global__ void __launch_bounds__(64)
k27_chol(const double* __restrict__ part, int np, int m, int replace, double* __restrict__ sm, K27Rec* __restrict__ rec)
{
    __shared__ double G[8][8], R[8][8], T[8][8];
    __shared__ int gone[8];
    if (rec->stop) return;
    const int lane = threadIdx.x & 63, r = lane >> 3, c = lane & 7;
    double g = 0.0;
    for (int q = 0; q < np; ++q) g += part[(size_t)q * 64 + lane];
    g = 0.5 * (g + __shfl(g, c * 8 + r));
    G[r][c] = g; R[r][c] = 0.0; T[r][c] = 0.0;
    __syncthreads();
    if (lane == 0) {
        int nhash = rec->nhash;
        for (int j = 0; j < 8; ++j) {
            gone[j] = 0;
            rec->repl[j] = -1;
            if (j >= m) { R[j][j] = 1.0; gone[j] = 1; continue; }               // (a zero column: stays zero)
            double d2 = G[j][j];
            for (int k = 0; k < j; ++k) {
                if (gone[k]) continue;
                double s = G[k][j];
                for (int l = 0; l < k; ++l) s -= R[l][k] * R[l][j];
                R[k][j] = s / R[k][k];
                d2 -= R[k][j] * R[k][j];
            }
            if (!(d2 > G[j][j] * K27_VANISH) || !(d2 < 1e300)) {                // vanished (or not a number)
                for (int k = 0; k < j; ++k) R[k][j] = 0.0;
                R[j][j] = 1.0; gone[j] = 1;
                if (replace && nhash < (1 << 11)) rec->repl[j] = nhash++;
            } else R[j][j] = sqrt(d2);
        }
        rec->nhash = nhash;
        for (int j = 0; j < 8; ++j) {                                           // T = R^-1, upper triangular
            T[j][j] = gone[j] ? 0.0 : 1.0 / R[j][j];                               // (vanished, or beyond the block's width)
            for (int i = j - 1; i >= 0; --i) {
                double s = 0.0;
                for (int k = i + 1; k <= j; ++k) s += R[i][k] * T[k][j];
                T[i][j] = gone[i] ? 0.0 : -s / R[i][i];
            }
        }
    }
    __syncthreads();
    sm[lane] = T[r][c];
}

// out[i][k] = sum_a A[i][a] T[a][k], or the hash column rec->repl[k] on the valid bins
__global__ void __launch_bounds__(TPB)
k27_apply(const double* __restrict__ A, const double* __restrict__ sm, const double* __restrict__ ew, int nb, double* __restrict__ out,
          const K27Rec* __restrict__ rec)
{
    if (rec->stop) return;
    const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
    const long long i = t >> 3; const int k = (int)(t & 7);
    if (i >= nb) return;
    const int rp = rec->repl[k];
    double v = 0.0;
    if (rp >= 0) { const double w = ew[i]; v = w == w ? k27_hash(rp, i) : 0.0; }
    else {
#pragma unroll
        for (int a = 0; a < 8; ++a) v += A[(size_t)i * 8 + a] * sm[a * 8 + k];
    }
    out[t] = v;
}

__global__ void __launch_bounds__(TPB)
k27_start(const double* __restrict__ ew, int nb, int m, double nan, double* __restrict__ Y, K27Rec* __restrict__ rec)
{
    const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
    if (t == 0) {
        rec->iters = 0; rec->converged = 0; rec->stop = 0; rec->nhash = 8;
        for (int k = 0; k < 8; ++k) { rec->lam[k] = nan; rec->res[k] = nan; rec->repl[k] = -1; }
    }
    const long long i = t >> 3; const int k = (int)(t & 7);
    if (i >= nb) return;
    const double w = ew[i];
    Y[t] = (k < m && w == w) ? k27_hash(k, i) : 0.0;
}

// workgroup k: out[k][i] = s V[i][k] on the valid bins (s: the entry of largest magnitude positive, the lowest bin on a tie), NaN on the
// others, and everywhere when the column holds no vector
__global__ void __launch_bounds__(TPB)
k27_final(const double* __restrict__ V, const double* __restrict__ ew, int nb, int have, double nan, double* __restrict__ out)
{
    __shared__ double la[TPB]; __shared__ long long li[TPB];
    __shared__ double l_sign;
    const int k = blockIdx.x;
    if (k >= 8) return;
    double best = -1.0; long long at = -1;
    if (k < have)
        for (long long i = threadIdx.x; i < nb; i += TPB) {
            const double w = ew[i], a = fabs(V[(size_t)i * 8 + k]);
            if (w == w && a > best) { best = a; at = i; }                       // (ascending: the lowest bin of a tie stays)
        }
    la[threadIdx.x] = best; li[threadIdx.x] = at;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < TPB; ++t)
            if (li[t] >= 0 && (la[t] > best || (la[t] == best && li[t] < at))) { best = la[t]; at = li[t]; }
        l_sign = (at >= 0 && at < nb && V[(size_t)at * 8 + k] < 0.0) ? -1.0 : 1.0;
    }
    __syncthreads();
    const double s = l_sign;
    for (long long i = threadIdx.x; i < nb; i += TPB) {
        const double w = ew[i];
        out[(size_t)k * (size_t)nb + (size_t)i] = (k < have && w == w) ? s * V[(size_t)i * 8 + k] : nan;
    }
}

// ---- K27 host side ------------------------------------------------------------------------------
// the checks every K27 call shares; -> CL_OK with c usable
static int eig_enter(cl_chrom* c, const char* who, bool need_build)
{
    if (!c) return fail(CL_ERR_ARG, "null chromosome handle");
    if (c->enq != c->deq) return fail(CL_ERR_ARG, who, "asynchronous runs still in flight");
    if (!c->bl.st.ready || !c->ex.st.ready || !c->ex.st.expected) return fail(CL_ERR_ARG, who, "no expected values on this handle (cl_exp_set)");
    if (need_build && !c->eg.st.built) return fail(CL_ERR_ARG, who, "no matrix on this handle (cl_eig_build)");
    return CL_OK;
}

// workgroups of k27_gram / k27_rot over nb bins and the bins of each (a multiple of TPB)
static void k27_parts(long long nb, int& np, int& per)
{
    long long p = (nb + K27_PARTS - 1) / K27_PARTS;
    p = (p + TPB - 1) / TPB * TPB;
    per = (int)std::max<long long>(p, TPB);
    np = (int)std::max<long long>((nb + per - 1) / per, 1);
}

static K27M eig_input(cl_chrom* c)
{
    const cl_chrom::Bal::State& bl = c->bl.st;
    K27M m{};
    const size_t rows = (size_t)bl.nb + 1;
    m.rp[0] = c->eg.rows.as<int>(); m.rp[1] = c->eg.rows.as<int>() + rows;
    m.oth[0] = c->mx.by.as<int>(); m.oth[1] = c->bl.tbx.as<int>();
    m.val[0] = c->eg.val.as<double>(); m.val[1] = c->eg.val.as<double>() + (size_t)bl.n_cells;
    m.ew = c->ex.w.as<double>();
    m.b0 = (int)bl.b0; m.nb = (int)bl.nb; m.ign = bl.ignore_diags; m.dmax = (int)c->eg.st.dmax; m.n = (int)bl.n_cells;
    return m;
}

// z = M q on the stream (q, z: [nb][8]); rec: the loop's record or null
static int eig_mul(cl_chrom* c, const K27M& m, const double* q, double* z, const K27Rec* rec)
{
    const int nb = m.nb, ntiles = (nb + K27_SB - 1) / K27_SB;
    double *pl = c->eg.pl.as<double>(), *tot = c->eg.tot.as<double>(), *off = tot + (size_t)ntiles * 8;
    hipLaunchKernelGGL(k27_scan1, dim3((unsigned)ntiles), dim3(TPB), 0, c->stream, q, nb, pl, tot, rec);
    LAUNCH(k27_scan2, (long long)ntiles * 8, (const double*)tot, ntiles, off, rec);
    hipLaunchKernelGGL(k27_mul, dim3((unsigned)((nb + TPB / 64 - 1) / (TPB / 64))), dim3(TPB), 0, c->stream, m, q, (const double*)pl,
                       (const double*)off, z, rec);
    HIP_TRY(hipGetLastError());
    return CL_OK;
}

static int eig_build(cl_chrom* c, double clip, long long dmax, cl_chrom::Eig::State& st)
{
    const cl_chrom::Bal::State& bl = c->bl.st;
    const int n = (int)bl.n_cells, nb = (int)bl.nb, ntiles = (nb + K27_SB - 1) / K27_SB;
    const size_t sn = (size_t)n, snb = (size_t)nb;
    int rc;
    if ((rc = c->eg.val.ensure(sn * 16)) || (rc = c->eg.rows.ensure((snb + 1) * 8)) || (rc = c->eg.pl.ensure(snb * 64)) ||
        (rc = c->eg.tot.ensure((size_t)ntiles * 128)) || (rc = c->eg.ctr.ensure(64))) return rc;
    HIP_TRY(hipMemsetAsync(c->eg.ctr.p, 0, 64, c->stream));
    double *val = c->eg.val.as<double>(), *tval = val + sn;
    LAUNCH(k27_vals, n, c->mx.bx.as<int>(), c->mx.by.as<int>(), c->mx.cnt.as<u32>(), n, (int)bl.b0, nb, bl.ignore_diags, (int)dmax,
           (const double*)c->ex.w.as<double>(), (const double*)c->ex.exp.as<double>(), clip, val, c->eg.ctr.as<u64>());
    LAUNCH(k27_perm, n, (const u32*)c->bl.vout.as<u32>(), (const double*)val, n, tval);
    LAUNCH(k27_rows, (long long)nb + 1, (const int*)c->mx.bx.as<int>(), n, (int)bl.b0, nb, c->eg.rows.as<int>());
    LAUNCH(k27_rows, (long long)nb + 1, (const int*)c->bl.tby.as<int>(), n, (int)bl.b0, nb, c->eg.rows.as<int>() + snb + 1);
    HIP_TRY(hipGetLastError());
    u64 hin = 0;
    HIP_TRY(hipMemcpyAsync(&hin, c->eg.ctr.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    st.n_in = (long long)hin;
    return CL_OK;
}

extern "C" int cl_eig_build(cl_chrom* c, double clip, int64_t dmax, int64_t* n_valid, int64_t* n_in)
{
    if (n_valid) *n_valid = 0;
    if (n_in) *n_in = 0;
    int rc = eig_enter(c, "cl_eig_build", false);
    if (rc != CL_OK) return rc;
    if (!n_valid || !n_in) return fail(CL_ERR_ARG, "cl_eig_build: bad arguments");
    if (!(clip > 0.0)) return fail(CL_ERR_ARG, "cl_eig_build: clip not above 0 or not a number");
    const cl_chrom::Bal::State& bl = c->bl.st;
    if (bl.nb > CL_EIG_BINS_MAX) return fail(CL_ERR_ARG, "cl_eig_build: more than CL_EIG_BINS_MAX bins (use a coarser res)");
    cl_chrom::Eig::State st;
    st.built = true; st.clip = clip; st.dmax = dmax;
    if (bl.nb == 0) {                                                           // (no bins: no band, no HIP call)
        if (dmax != 0) return fail(CL_ERR_ARG, "cl_eig_build: dmax must be 0 without bins");
        eig_release(c); c->eg.st = st;
        return CL_OK;
    }
    if (dmax < bl.ignore_diags || dmax > bl.nb) return fail(CL_ERR_ARG, "cl_eig_build: dmax outside [ignore_diags, nb]");
    HIP_TRY(hipSetDevice(c->device));
    // the host's look at K26's state: the valid bins, and the expected values of the band's diagonals that hold a valid pair
    const size_t snb = (size_t)bl.nb;
    std::vector<double> ew(snb), ex(snb);
    std::vector<long long> pairs(snb);
    if ((rc = read_back(c, "cl_eig_build", {{ew.data(), c->ex.w.p, snb * 8}, {ex.data(), c->ex.exp.p, snb * 8}, {pairs.data(), c->ex.pairs.p, snb * 8}})))
        return rc;
    for (long long d = bl.ignore_diags; d < dmax; ++d)
        if (pairs[(size_t)d] > 0 && !(ex[(size_t)d] > 0.0 && std::isfinite(ex[(size_t)d])))
            return fail(CL_ERR_ARG, "cl_eig_build: a diagonal of the band has valid pairs and no finite positive expected value (lower dmax)");
    for (size_t i = 0; i < snb; ++i) st.n_valid += ew[i] == ew[i] ? 1 : 0;
    c->eg.st = cl_chrom::Eig::State();                                          // (the earlier state's buffers are written from here on)
    rc = eig_build(c, clip, dmax, st);
    if (rc != CL_OK) {
        (void)hipStreamSynchronize(c->stream);
        eig_release(c);
        return rc;
    }
    c->eg.st = st;
    *n_valid = st.n_valid; *n_in = st.n_in;
    return CL_OK;
}

extern "C" int cl_eig_apply(cl_chrom* c, const double* x, int32_t n_vec, double* y)
{
    int rc = eig_enter(c, "cl_eig_apply", true);
    if (rc != CL_OK) return rc;
    if (n_vec < 1 || n_vec > CL_EIG_BLOCK) return fail(CL_ERR_ARG, "cl_eig_apply: n_vec outside [1, CL_EIG_BLOCK]");
    const size_t snb = (size_t)c->bl.st.nb;
    if (snb == 0) return CL_OK;
    if (!x || !y) return fail(CL_ERR_ARG, "cl_eig_apply: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->eg.io.ensure(snb * 8 * (size_t)n_vec)) || (rc = c->eg.ax.ensure(snb * 128))) return rc;
    double *io = c->eg.io.as<double>(), *ax = c->eg.ax.as<double>(), *az = ax + snb * 8;
    HIP_TRY(hipMemcpyAsync(io, x, snb * 8 * (size_t)n_vec, hipMemcpyHostToDevice, c->stream));
    LAUNCH(k27_pack, (long long)snb * 8, (const double*)io, (int)n_vec, (int)snb, (const double*)c->ex.w.as<double>(), ax);
    const K27M m = eig_input(c);
    if ((rc = eig_mul(c, m, ax, az, nullptr))) { (void)hipStreamSynchronize(c->stream); return rc; }
    LAUNCH(k27_unpack, (long long)snb * 8, (const double*)az, (int)n_vec, (int)snb, io);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); return fail(CL_ERR_HIP, "cl_eig_apply", hipGetErrorString(e)); }
    return read_back(c, "cl_eig_apply", {{y, io, snb * 8 * (size_t)n_vec}});
}

static int eig_iterate(cl_chrom* c, int n_eigs, int max_iters, double tol, int m, K27Rec& h)
{
    const int nb = (int)c->bl.st.nb;
    const size_t snb = (size_t)nb, blk8 = snb * 8;
    int np, per, rc;
    k27_parts(nb, np, per);
    // eg.q: Q, Z, Y, the first pass of an orthonormalisation, V; eg.part: the Gram partials, then the residuals'; eg.sm: W or T, the record
    if ((rc = c->eg.q.ensure(blk8 * 8 * 5)) || (rc = c->eg.part.ensure((size_t)np * 72 * 8)) || (rc = c->eg.sm.ensure(64 * 8 + sizeof(K27Rec) + 64)) ||
        (rc = c->eg.vec.ensure(blk8 * 8))) return rc;
    const double nan = std::nan("");
    double *Q = c->eg.q.as<double>(), *Z = Q + blk8, *Y = Z + blk8, *Q1 = Y + blk8, *V = Q1 + blk8;
    double *part = c->eg.part.as<double>(), *rpart = part + (size_t)np * 64, *sm = c->eg.sm.as<double>();
    K27Rec* rec = (K27Rec*)(sm + 64);
    const double* ew = c->ex.w.as<double>();
    const K27M mm = eig_input(c);
    const int n_ask = std::min(n_eigs, m);
    auto ortho = [&](const double* A, double* out) {                            // out = the orthonormalised A, through Q1
        hipLaunchKernelGGL(k27_gram, dim3((unsigned)np), dim3(TPB), 0, c->stream, A, A, nb, per, part, (const K27Rec*)rec);
        hipLaunchKernelGGL(k27_chol, dim3(1), dim3(64), 0, c->stream, (const double*)part, np, m, 1, sm, rec);
        LAUNCH(k27_apply, (long long)blk8, A, (const double*)sm, ew, nb, Q1, (const K27Rec*)rec);
        hipLaunchKernelGGL(k27_gram, dim3((unsigned)np), dim3(TPB), 0, c->stream, (const double*)Q1, (const double*)Q1, nb, per, part, (const K27Rec*)rec);
        hipLaunchKernelGGL(k27_chol, dim3(1), dim3(64), 0, c->stream, (const double*)part, np, m, 0, sm, rec);
        LAUNCH(k27_apply, (long long)blk8, (const double*)Q1, (const double*)sm, ew, nb, out, (const K27Rec*)rec);
    };
    h = K27Rec{};
    if (m > 0) {
        LAUNCH(k27_start, (long long)blk8, ew, nb, m, nan, Y, rec);
        ortho(Y, Q);
        HIP_TRY(hipGetLastError());
        for (int done = 0; done < max_iters && !h.stop;) {
            const int blk = std::min(K27_BLOCK, max_iters - done);
            for (int k = 0; k < blk; ++k) {
                if ((rc = eig_mul(c, mm, Q, Z, rec))) return rc;
                hipLaunchKernelGGL(k27_gram, dim3((unsigned)np), dim3(TPB), 0, c->stream, (const double*)Q, (const double*)Z, nb, per, part, (const K27Rec*)rec);
                hipLaunchKernelGGL(k27_ritz, dim3(1), dim3(64), 0, c->stream, (const double*)part, np, m, sm, rec);
                hipLaunchKernelGGL(k27_rot, dim3((unsigned)np), dim3(TPB), 0, c->stream, (const double*)Z, (const double*)Q, (const double*)sm, nb, per, Y, V,
                                   rpart, (const K27Rec*)rec);
                hipLaunchKernelGGL(k27_check, dim3(1), dim3(64), 0, c->stream, (const double*)rpart, np, n_ask, tol, rec);
                ortho(Y, Q);
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(hipMemcpyAsync(&h, rec, sizeof(K27Rec), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            done += blk;
            if (h.iters < 0 || h.iters > done) return fail(CL_ERR_HIP, "cl_eig_iterate: the record holds a count no loop can have");
        }
    }
    const int have = h.iters > 0 ? n_ask : 0;
    hipLaunchKernelGGL(k27_final, dim3(8), dim3(TPB), 0, c->stream, (const double*)V, ew, nb, have, nan, c->eg.vec.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CL_OK;
}

extern "C" int cl_eig_iterate(cl_chrom* c, int32_t n_eigs, int32_t max_iters, double tol, int32_t* iters, int32_t* converged, double* eigval,
                              double* resid)
{
    const double nan = std::nan("");
    if (iters) *iters = 0;
    if (converged) *converged = 0;
    int rc = eig_enter(c, "cl_eig_iterate", true);
    if (rc != CL_OK) return rc;
    if (n_eigs < 1 || n_eigs > CL_EIG_MAX) return fail(CL_ERR_ARG, "cl_eig_iterate: n_eigs outside [1, CL_EIG_MAX]");
    if (!iters || !converged || !eigval || !resid) return fail(CL_ERR_ARG, "cl_eig_iterate: bad arguments");
    if (max_iters < 0) return fail(CL_ERR_ARG, "cl_eig_iterate: max_iters below 0");
    if (!(tol >= 0.0)) return fail(CL_ERR_ARG, "cl_eig_iterate: tol below 0 or not a number");
    for (int k = 0; k < n_eigs; ++k) { eigval[k] = nan; resid[k] = nan; }
    c->eg.st.iterated = false; c->eg.st.n_eigs = 0;
    if (c->bl.st.nb == 0) { c->eg.st.iterated = true; c->eg.st.n_eigs = n_eigs; return CL_OK; }
    HIP_TRY(hipSetDevice(c->device));
    const int m = (int)std::min<long long>(CL_EIG_BLOCK, c->eg.st.n_valid);
    K27Rec h{};
    rc = eig_iterate(c, n_eigs, max_iters, tol, m, h);
    if (rc != CL_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    c->eg.st.iterated = true; c->eg.st.n_eigs = n_eigs;
    *iters = h.iters; *converged = h.converged;
    if (h.iters > 0)
        for (int k = 0; k < std::min((int)n_eigs, m); ++k) { eigval[k] = h.lam[k]; resid[k] = h.res[k]; }
    return CL_OK;
}

extern "C" int cl_eig_vectors_get(cl_chrom* c, int32_t which, int64_t first, int64_t count, double* v)
{
    int rc = eig_enter(c, "cl_eig_vectors_get", true);
    if (rc != CL_OK) return rc;
    if (!c->eg.st.iterated) return fail(CL_ERR_ARG, "cl_eig_vectors_get: no vectors on this handle (cl_eig_iterate)");
    if (which < 0 || which >= c->eg.st.n_eigs) return fail(CL_ERR_ARG, "cl_eig_vectors_get: which outside the vectors");
    if (!range_ok(first, count, c->bl.st.nb)) return fail(CL_ERR_ARG, "cl_eig_vectors_get: range outside the bins");
    if (count > 0 && !v) return fail(CL_ERR_ARG, "cl_eig_vectors_get: bad arguments");
    if (count == 0) return CL_OK;
    HIP_TRY(hipSetDevice(c->device));
    return read_back(c, "cl_eig_vectors_get", {{v, c->eg.vec.as<double>() + (size_t)which * (size_t)c->bl.st.nb + first, (size_t)count * 8}});
}

extern "C" int cl_eig_free(cl_chrom* c) { return unit_free(c, "cl_eig_free", eig_release); }
