// cl_segsum.h -- sums over the runs of equal keys of a sorted cell list, in a fixed order: the tile scan and the carry fold that K25
// (k_balance.hip: the marginals over both orders of the cells) and K26 (k_expected.hip: the sums per diagonal) instantiate.
//   k25_marg<V>     blockIdx.y = order (0: as they lie, 1: transposed), one workgroup per K25_TILE consecutive cells, 8 consecutive
//                   cells per thread (two 16-byte loads per array on a full tile; with 4-byte loads an iteration over the 2.77 M
//                   cells of chr1 at 10 kb took 62 instead of 37 us).  Segmented inclusive scan by key: inside the thread, then over the threads (wave shuffles, then
//                   the four wave totals).  A run that lies inside the tile is stored by the thread of its last cell: every key has ONE
//                   run per order, so no atomics.  The run that opens the tile and the run that closes it go to the tile's carry record
//                   (one record when the tile is one run).
//   k25_fold<V>     one thread per tile and order: a piece that starts a chain (the closing piece of a tile, or an opening piece whose
//                   key differs from the key before it) adds the opening pieces of the tiles that follow while their key is its own,
//                   in tile order, and stores the total.  A run over several whole tiles is a walk over their records.
// V: the value of a run (zero / add / up: a wave shuffle / store, and its Out); what a cell adds is k25_term(in, order, key, other bin,
// count, (V*)nullptr), an overload the instantiating unit declares next to its V.
#pragma once
#include "cl_chrom.h"

#define K25_TILE 2048                   // cells per workgroup (K24's tile): 8 per thread, no LDS beyond the wave totals
#define K25_U (K25_TILE / TPB)

struct K25Rec { int iters, converged, stop, pad; double var, scale; };        // the loop's record (32 bytes)
static_assert(sizeof(K25Rec) == 32, "the record is read back as 32 bytes");

template <typename V> struct K25Car { int kf, kl, single, pad; V vf, vl; };     // a tile's opening piece (kf, vf) and closing piece (kl, vl; none when single)

struct K25In {
    const int* key[2]; const int* oth[2]; const u32* cnt[2];                    // per order: the run key, the other bin, the count
    int n, ign, b0, nb;
    int vec;                                                                    // all six arrays start at multiples of 16 bytes
    const double* w;                                                            // fp64 pass: nb weights
};

template <typename V>
__global__ void __launch_bounds__(TPB)
k25_marg(K25In in, typename V::Out out, K25Car<V>* __restrict__ car, int ntiles, u64* __restrict__ n_used, const K25Rec* __restrict__ rec)
{
    __shared__ V wv[TPB / 64];
    __shared__ int wf[TPB / 64];
    __shared__ u32 wu[TPB / 64];
    if (rec && rec->stop) return;                                               // (the whole grid)
    const int ph = blockIdx.y ? 1 : 0;
    const long long t0 = (long long)blockIdx.x * K25_TILE;
    if (t0 >= in.n || (int)blockIdx.x >= ntiles) return;                        // (the whole workgroup)
    const int tn = (int)(in.n - t0 < K25_TILE ? in.n - t0 : K25_TILE);
    const int* __restrict__ key = in.key[ph] + t0;
    const int* __restrict__ oth = in.oth[ph] + t0;
    const u32* __restrict__ cnt = in.cnt[ph] + t0;
    const int base = (int)threadIdx.x * K25_U, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kfirst = key[0], klast = key[tn - 1];
    int k[K25_U], o[K25_U];
    u32 cc[K25_U];
    V v[K25_U];
    u32 used = 0u;
    if (in.vec && tn == K25_TILE) {                                             // (the whole workgroup) a full tile of 16-byte aligned arrays: two
        static_assert(K25_U == 8, "two 16-byte loads per array and thread");   // 16-byte loads per array instead of eight of 4 bytes
        const int4 ka = ((const int4*)(key + base))[0], kb = ((const int4*)(key + base))[1];
        const int4 oa = ((const int4*)(oth + base))[0], ob = ((const int4*)(oth + base))[1];
        const uint4 ca = ((const uint4*)(cnt + base))[0], cb = ((const uint4*)(cnt + base))[1];
        k[0] = ka.x; k[1] = ka.y; k[2] = ka.z; k[3] = ka.w; k[4] = kb.x; k[5] = kb.y; k[6] = kb.z; k[7] = kb.w;
        o[0] = oa.x; o[1] = oa.y; o[2] = oa.z; o[3] = oa.w; o[4] = ob.x; o[5] = ob.y; o[6] = ob.z; o[7] = ob.w;
        cc[0] = ca.x; cc[1] = ca.y; cc[2] = ca.z; cc[3] = ca.w; cc[4] = cb.x; cc[5] = cb.y; cc[6] = cb.z; cc[7] = cb.w;
    } else {
#pragma unroll
        for (int u = 0; u < K25_U; ++u) {
            const int il = base + u;
            if (il < tn) { k[u] = key[il]; o[u] = oth[il]; cc[u] = cnt[il]; }
            else { k[u] = klast; o[u] = klast; cc[u] = 0u; }                    // (behind the tile's end: more of its last run, adding nothing)
        }
    }
#pragma unroll
    for (int u = 0; u < K25_U; ++u) {
        const bool live = base + u < tn;
        v[u] = live ? k25_term(in, ph, k[u], o[u], cc[u], (V*)nullptr) : V::zero();
        if (!ph) used += (live && o[u] - k[u] >= in.ign) ? 1u : 0u;
    }
    const int kprev = base == 0 ? 0 : (base - 1 < tn ? key[base - 1] : klast);
    const int knext = base + K25_U < tn ? key[base + K25_U] : klast;
    // inside the thread: v[u] = the sum of its run's cells from the run's head (or the thread's first cell) to u
    bool h0 = base == 0 || k[0] != kprev, any = h0;
    int first_head = h0 ? 0 : K25_U;                                            // the thread's cells before it belong to a run that began earlier
#pragma unroll
    for (int u = 1; u < K25_U; ++u) {
        const bool h = k[u] != k[u - 1];
        if (!h) v[u] = V::add(v[u - 1], v[u]);
        else if (first_head == K25_U) first_head = u;
        any |= h;
    }
    // over the threads: (f, x) = (a head in the thread, the sum of its last run); inclusive segmented scan in the wave
    int f = any ? 1 : 0;
    V x = v[K25_U - 1];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const V tx = V::up(x, d);
        const int tf = __shfl_up(f, (unsigned)d);
        if (lane >= d) { if (!f) x = V::add(tx, x); f |= tf; }
    }
    if (lane == 63) { wv[wave] = x; wf[wave] = f; }
    V ex = V::up(x, 1);                                                         // exclusive: what the threads before this one leave open
    int ef = __shfl_up(f, 1u);
    if (lane == 0) { ex = V::zero(); ef = 0; }
    __syncthreads();
    V px = V::zero();                                                           // the same of the waves before this one
    for (int q = 0; q < wave; ++q) px = wf[q] ? wv[q] : V::add(px, wv[q]);
    const V cin = ef ? ex : V::add(px, ex);
    // stores: the thread of a run's last cell has its total
    K25Car<V>* my = car + (size_t)ph * (size_t)ntiles + blockIdx.x;
#pragma unroll
    for (int u = 0; u < K25_U; ++u) {
        const int il = base + u;
        if (il >= tn) continue;
        const int kn = u + 1 < K25_U ? k[u + 1] : knext;
        const bool tile_end = il == tn - 1;
        if (!tile_end && kn == k[u]) continue;                                  // not the last cell of its run
        const V tot = u < first_head ? V::add(cin, v[u]) : v[u];
        if (k[u] == kfirst) {                                                   // the run that opens the tile
            my->kf = k[u]; my->vf = tot;
            if (tile_end) { my->kl = k[u]; my->vl = V::zero(); my->single = 1; my->pad = 0; }
        } else if (tile_end) {
            my->kl = k[u]; my->vl = tot; my->single = 0; my->pad = 0;
        } else {
            const long long g = (long long)k[u] - in.b0;
            if (g >= 0 && g < in.nb) V::store(out, (size_t)ph * (size_t)in.nb + (size_t)g, tot);
        }
    }
    if (n_used && !ph) {                                                        // (wave-uniform)
        for (int o = 32; o > 0; o >>= 1) used += (u32)__shfl_xor((int)used, o);
        if (lane == 0) wu[wave] = used;
        __syncthreads();
        if (threadIdx.x == 0) {
            u64 s = 0;
            for (int q = 0; q < TPB / 64; ++q) s += wu[q];
            if (s) atomicAdd(n_used, s);
        }
    }
}

template <typename V>
__global__ void __launch_bounds__(TPB)
k25_fold(const K25Car<V>* __restrict__ car, int ntiles, int b0, int nb, typename V::Out out, const K25Rec* __restrict__ rec)
{
    if (rec && rec->stop) return;
    const int ph = blockIdx.y ? 1 : 0;
    const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
    if (t >= ntiles) return;
    const K25Car<V>* r = car + (size_t)ph * (size_t)ntiles;
    const K25Car<V> me = r[t];
    for (int piece = 0; piece < 2; ++piece) {
        int key; V tot; long long nx = t + 1;
        if (piece == 0) {                                                       // the opening piece: a chain's start unless the tile before ends with its key
            if (t > 0 && r[t - 1].kl == me.kf) continue;
            key = me.kf; tot = me.vf;
            if (!me.single) nx = ntiles;                                        // (its run ends inside this tile)
        } else {
            if (me.single) continue;
            key = me.kl; tot = me.vl;
        }
        for (; nx < ntiles; ++nx) {
            const K25Car<V> o = r[nx];
            if (o.kf != key) break;
            tot = V::add(tot, o.vf);
            if (!o.single) break;
        }
        const long long g = (long long)key - b0;
        if (g >= 0 && g < nb) V::store(out, (size_t)ph * (size_t)nb + (size_t)g, tot);
    }
}
