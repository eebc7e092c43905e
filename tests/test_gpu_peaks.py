"""GPU: kernel K21 (cl_peak_sort / call / get / count / summits) against the numpy oracle of tests/peaks_cases.py, written from the
definitions of include/cloops_hip.h (it does not call cloops_amd.peaks), and on the small cases against a plain sequential DBSCAN.
Degenerate sizes, hand-placed borders and duplicates, every tile edge of k21_core, pile-ups beyond its LDS window, dense and sparse
random sets, counts with bounds beyond the keys and beyond 32 bits, summits (ties, empty intervals, one interval for all, 10^5
intervals of one point), repeatability, the handle's other results (unchanged), argument errors, the chr21 example against pinned
values, jd2peaks against the host functions fed by the oracle, the command line and -peaks on the main command."""
import ctypes
import json
import os

import numpy as np
import pytest

import golden_util as G
import peaks_cases as PC

pytestmark = pytest.mark.gpu

EMPTY = PC.EMPTY
T = 1024             # k_peak.hip K21_TILE: sorted end points per workgroup of k21_core and k21_summit
H = 1024             # k_peak.hip K21_HALO: end points staged in LDS on either side of a tile
IVL = 2048           # k_peak.hip K21_IVL: interval starts that k21_summit stages in LDS


def far(X):
    """a Y for rows whose X alone matters (ends = 1)"""
    return np.asarray(X, np.int64) + 1000000


def chrom(X, Y):
    from cloops_amd import api
    return api.Chromosome(np.asarray(X, np.int64), np.asarray(Y, np.int64))


def points(P, order=None):
    """a handle whose X are the points P (in another order), sorted with ends = 1 -> (handle, S)"""
    P = np.asarray(P, np.int64)
    X = P if order is None else P[order]
    ch = chrom(X, far(X))
    S = np.sort(P)
    assert ch.peaks_sort(0, 1) == ((len(S), int(S[0]), int(S[-1])) if len(S) else (0, 0, 0))
    return ch, S


def check_call(ch, S, eps, minPts, sequential=False):
    """one setting on a sorted handle against the oracle (and the sequential DBSCAN) -> the oracle's (start, end, n_points, n_cores)"""
    want = PC.peaks_oracle(S, eps, minPts)
    if sequential:
        assert [a.tolist() for a in want[:4]] == [list(w) for w in PC.sequential_dbscan(S, eps, minPts)]
    assert ch.peaks_call(eps, minPts) == (len(want[0]), want[4], int(want[2].sum())), (eps, minPts)
    got = ch.peaks_get()
    assert [a.dtype for a in got] == [np.int32, np.int32, np.uint32, np.uint32]
    for g, w in zip(got, want[:4]):
        assert np.array_equal(g, w), (eps, minPts)
    return want[:4]


def check_counts(ch, S, starts, ends):
    got = ch.peaks_count(starts, ends)
    assert got.dtype == np.uint32 and np.array_equal(got, PC.count_oracle(S, starts, ends))
    return got


def check_summits(ch, S, starts, ends, w):
    pos, cnt = ch.peaks_summits(starts, ends, w)
    want = PC.summit_oracle(S, starts, ends, w)
    assert pos.dtype == np.int32 and cnt.dtype == np.uint32
    assert np.array_equal(pos, want[0]) and np.array_equal(cnt, want[1]), w
    return pos, cnt


# ---- degenerate inputs -----------------------------------------------------------------------------
def test_degenerate_sizes():
    ch = chrom(EMPTY, EMPTY)
    assert ch.peaks_sort() == (0, 0, 0) and ch.peaks_call(100, 5) == (0, 0, 0)
    assert all(len(a) == 0 for a in ch.peaks_get())
    assert ch.peaks_count([0, -5], [10, 5]).tolist() == [0, 0]
    assert [a.tolist() for a in ch.peaks_summits([0, 20], [10, 30], 5)] == [[-1, -1], [0, 0]]
    ch.peaks_free()
    ch.close()
    ch = chrom([1000], [5000])
    assert ch.peaks_sort() == (2, 1000, 5000)
    S = np.array([1000, 5000])
    assert [a.tolist() for a in check_call(ch, S, 100, 1, True)] == [[1000, 5000], [1001, 5001], [1, 1], [1, 1]]
    check_call(ch, S, 100, 2, True)                                  # minPts > the points of any window: no peak
    assert [a.tolist() for a in check_call(ch, S, 4000, 2, True)] == [[1000], [5001], [2], [2]]
    check_call(ch, S, 3999, 2, True)
    assert ch.peaks_sort(cut=4001) == (0, 0, 0) and ch.peaks_call(100, 1) == (0, 0, 0)     # the cut removes every row
    assert ch.peaks_count([0], [10000]).tolist() == [0]
    assert ch.peaks_sort(cut=4000) == (2, 1000, 5000)
    ch.close()


def test_minpts_one_and_beyond_m():
    P = np.array([10, 500, 500, 1000, 1050, 3000])
    ch, S = points(P, [3, 0, 5, 1, 4, 2])
    r = check_call(ch, S, 49, 1, True)                               # every point a core; isolated points are peaks of length 1
    assert [a.tolist() for a in r] == [[10, 500, 1000, 1050, 3000], [11, 501, 1001, 1051, 3001], [1, 2, 1, 1, 1], [1, 2, 1, 1, 1]]
    r = check_call(ch, S, 50, 1, True)
    assert r[0].tolist() == [10, 500, 1000, 3000] and r[1].tolist() == [11, 501, 1051, 3001]
    check_call(ch, S, 5000, len(S) + 1, True)                        # minPts > m: no peak
    assert ch.peaks_call(5000, 1 << 40) == (0, 0, 0) and all(len(a) == 0 for a in ch.peaks_get())
    r = check_call(ch, S, 5000, len(S), True)                        # eps larger than the span: one peak
    assert [a.tolist() for a in r] == [[10], [3001], [6], [6]]
    check_call(ch, S, (1 << 29) - 1, 3)
    ch.close()


def test_ends_with_equal_x_and_y():
    X, Y = np.array([100, 400, 400, 900, 901]), np.array([400, 400, 700, 900, 2000])      # rows with X == Y among them
    ch = chrom(X, Y)
    for ends, n in ((1, 5), (2, 5), (3, 10)):
        S = PC.ends_of(X, Y, 0, ends)
        assert ch.peaks_sort(0, ends) == (n, S[0], S[-1])
        for eps, minPts in ((1, 2), (1, 3), (300, 3), (300, 4)):
            check_call(ch, S, eps, minPts, True)
    S = PC.ends_of(X, Y, 300, 3)
    assert ch.peaks_sort(300, 3) == (6, 100, 2000)                   # the rows at or beyond the cut
    check_call(ch, S, 300, 2, True)
    ch.close()


# ---- hand-placed borders and duplicates --------------------------------------------------------------
def test_border_between_two_chains():
    P = [0, 0, 1, 1, 2, 5, 8, 9, 9, 10, 10]                           # eps 3, minPts 5: all but 5 are cores; 5 is within 3 of 2 and 8
    ch, S = points(P, np.random.default_rng(1).permutation(len(P)))
    r = check_call(ch, S, 3, 5, True)
    assert [a.tolist() for a in r] == [[0, 8], [6, 11], [6, 5], [5, 5]]     # it goes left, and the right peak starts after it
    ch.close()
    eps = 10
    for d, minPts, n_points in ((eps, 7, 7), (eps + 1, 5, 5)):        # border points exactly eps and eps + 1 from the cores
        P = [100 - d] + [100] * 5 + [100 + d]                         # (the five at 100 see 7 or 5 points, the two others 6 or 1)
        ch, S = points(P)
        r = check_call(ch, S, eps, minPts, True)
        assert r[2].tolist() == [n_points] and r[3].tolist() == [5]
        ch.close()
    for gap, n_peaks in ((eps, 1), (eps + 1, 2)):                     # cores exactly eps and eps + 1 apart
        P = [0, 0, 0, gap, gap, gap]
        ch, S = points(P)
        r = check_call(ch, S, eps, 3, True)
        assert len(r[0]) == n_peaks and int(r[3].sum()) == 6
        ch.close()


def test_duplicates():
    P = [50, 50, 50, 50, 70, 70, 70, 70]                              # groups of equal positions that are cores only together
    ch, S = points(P)
    assert [a.tolist() for a in check_call(ch, S, 5, 4, True)] == [[50, 70], [51, 71], [4, 4], [4, 4]]
    assert len(check_call(ch, S, 5, 5, True)[0]) == 0
    assert [a.tolist() for a in check_call(ch, S, 20, 8, True)] == [[50], [71], [8], [8]]
    ch.close()
    P = [10, 10, 10, 12, 14, 16, 16, 16, 40, 40, 41, 60]              # equal positions at the head and at the tail of a chain
    ch, S = points(P, np.random.default_rng(2).permutation(len(P)))
    for eps, minPts in ((2, 3), (2, 4), (2, 5), (1, 3), (24, 3), (19, 2), (20, 2)):
        check_call(ch, S, eps, minPts, True)
    ch.close()
    P = np.array([-500, -500, -498, -3, -1, 0, 0, 2, 300])            # negative coordinates
    ch, S = points(P)
    r = check_call(ch, S, 3, 3, True)
    assert [a.tolist() for a in r] == [[-500, -3], [-497, 3], [3, 5], [3, 5]]
    check_counts(ch, S, [-1000, -500, -3, 0], [0, -499, 1, 1000])
    assert check_summits(ch, S, [-600, -10], [-400, 100], 2)[0].tolist() == [-500, -1]
    ch.close()
    rng = np.random.default_rng(3)
    for _ in range(6):                                                 # small random sets with many duplicates, every setting
        P = rng.integers(-40, 41, int(rng.integers(1, 60)))
        ch, S = points(P)
        for eps in (1, 2, 5, 9):
            for minPts in (1, 2, 4):
                check_call(ch, S, eps, minPts, True)
        ch.close()


# ---- tile edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [T - 1, T, T + 1, 2 * T, 2 * T + 1])
def test_tile_edges(m):
    """m points at every tile edge, rows in random order: sparse (windows inside a tile), a chain and a peak across every tile
    boundary, and a value repeated across the boundary"""
    rng = np.random.default_rng(m)
    P = np.sort(rng.integers(0, 40 * m, m))
    for edge in range(T, m, T):                                       # a run of close points across each boundary: one chain over it
        P[edge - 5:edge + 5] = P[edge - 5] + np.arange(len(P[edge - 5:edge + 5]))
    P = np.sort(P)
    ch, S = points(P, rng.permutation(m))
    for eps, minPts in ((10, 3), (40, 2), (200, 8), (40 * m, m)):
        check_call(ch, S, eps, minPts)
    ms, me = PC.peaks_oracle(S, 40, 2)[:2]
    check_counts(ch, S, ms, me)
    check_summits(ch, S, ms, me, 17)
    P[max(0, T - 3):T + 3] = P[max(0, T - 3)]                         # equal positions on both sides of the first boundary
    P[m - 2:] = P[m - 2]
    P = np.sort(P)
    ch.close()
    ch, S = points(P, rng.permutation(m))
    for eps, minPts in ((1, 2), (10, 3), (40, 6)):
        check_call(ch, S, eps, minPts)
    ch.close()


def test_long_peak_and_pile_ups():
    rng = np.random.default_rng(8)
    P = np.concatenate([np.arange(0, 5 * T * 3, 3), [100000, 100001, 200000]])       # a peak several tiles long
    ch, S = points(P, rng.permutation(len(P)))
    r = check_call(ch, S, 3, 3)
    assert r[2].tolist() == [5 * T] and r[0].tolist() == [0]
    check_call(ch, S, 2, 2)                                           # ... and no chain at all but the pair
    check_summits(ch, S, [0, 100000], [15 * T, 200001], 5)
    ch.close()
    m = 3 * (T + 2 * H)                                               # all points equal: every window holds them all
    ch, S = points(np.full(m, 777))
    assert [a.tolist() for a in check_call(ch, S, 1, m)] == [[777], [778], [m], [m]]
    assert ch.peaks_call(1, m + 1) == (0, 0, 0)
    assert check_counts(ch, S, [777, 0, 778], [778, 777, 900]).tolist() == [m, 0, 0]
    assert [a.tolist() for a in check_summits(ch, S, [0, 700], [700, 800], 3)] == [[-1, 777], [0, m]]
    ch.close()
    P = np.concatenate([10000 + rng.integers(0, 300, 4 * (T + 2 * H)), rng.integers(0, 1000000, 3000)])
    ch, S = points(P)                                                 # a dense cluster: an eps window holds more than T + 2 H points
    for eps, minPts in ((200, 50), (400, T + 2 * H + 1), (5, 100), (2000, 4)):
        check_call(ch, S, eps, minPts)
    ms, me = PC.peaks_oracle(S, 2000, 4)[:2]
    check_summits(ch, S, ms, me, 250)
    ch.close()


# ---- random sets --------------------------------------------------------------------------------------
def test_dense_random():
    rng = np.random.default_rng(20)
    a, b = rng.integers(0, 20000, 50000), rng.integers(0, 20000, 50000)
    X, Y = np.minimum(a, b), np.maximum(a, b)
    ch = chrom(X, Y)
    S = PC.ends_of(X, Y)
    assert ch.peaks_sort() == (100000, S[0], S[-1])
    first = None
    for eps, minPts in ((1, 12), (2, 30), (3, 40), (50, 600), (1, 12)):      # several settings after one sort; the first one again
        r = check_call(ch, S, eps, minPts)
        first = first or [a.copy() for a in ch.peaks_get()]
    assert all(np.array_equal(u, v) for u, v in zip(first, ch.peaks_get())) and len(first[0]) > 100
    S1 = PC.ends_of(X, Y, 3000, 1)                                    # a second sort with another cut and ends replaces the first
    assert ch.peaks_sort(3000, 1) == (len(S1), S1[0], S1[-1]) and len(S1) < 50000
    check_call(ch, S1, 3, 8)
    check_counts(ch, S1, [0, 100], [100, 30000])
    ch.close()


def test_sparse_random():
    rng = np.random.default_rng(29)
    a, b = rng.integers(-(1 << 29) + 1, 1 << 29, 100000), rng.integers(-(1 << 29) + 1, 1 << 29, 100000)
    X, Y = np.minimum(a, b), np.maximum(a, b)
    X[0], Y[0] = -(1 << 29) + 1, (1 << 29) - 1                        # the domain's edges
    ch = chrom(X, Y)
    S = PC.ends_of(X, Y)
    assert ch.peaks_sort() == (200000, S[0], S[-1])
    for eps, minPts in ((3000, 3), (20000, 10), ((1 << 29) - 1, 100000), (1, 1)):
        check_call(ch, S, eps, minPts)
    ms, me = PC.peaks_oracle(S, 3000, 3)[:2]
    check_counts(ch, S, ms, me)
    check_summits(ch, S, ms, me, 500)
    ch.close()


# ---- counts ---------------------------------------------------------------------------------------------
def test_counts():
    rng = np.random.default_rng(31)
    P = rng.integers(-5000, 60000, 30000)
    ch, S = points(P)
    s = rng.integers(-8000, 64000, 5000)                              # overlapping, unordered; a third of them empty or reversed
    e = s + rng.integers(-300, 3000, 5000)
    got = check_counts(ch, S, s, e)
    assert (got == 0).sum() > 300 and got.max() > 1000
    big = 1 << 31
    s = np.array([S[0] - 1, S[0], S[0] + 1, S[-1], S[-1] + 1, -big - 5, -(1 << 62), 0, big, big + 7, 100, -(1 << 63)], np.int64)
    e = np.array([S[0], S[0] + 1, S[-1], S[-1] + 1, big, big, 1 << 62, big + 5, big + 9, big + 3, 100, (1 << 63) - 1], np.int64)
    got = check_counts(ch, S, s, e)                                   # bounds below vmin, above vmax, beyond 32 bits
    assert got[0] == 0 and got[5] == got[6] == got[11] == len(S) and got[8] == got[9] == got[10] == 0
    assert len(ch.peaks_count(EMPTY, EMPTY)) == 0
    ch.close()


# ---- summits --------------------------------------------------------------------------------------------
def test_summits():
    P = [100, 100, 103, 103, 110, 200, 201, 202, 300, 400, 400, 401]
    ch, S = points(P)
    pos, cnt = check_summits(ch, S, [90, 120, 195, 250, 300, 390], [120, 190, 250, 300, 301, 500], 1)
    assert pos.tolist() == [100, -1, 201, -1, 300, 400] and cnt.tolist() == [2, 0, 3, 0, 1, 3]      # ties: the smallest position
    pos, cnt = check_summits(ch, S, [0, 101], [101, 1000], 3)
    assert pos.tolist() == [100, 103] and cnt.tolist() == [4, 4]      # n_w counts beyond the interval; 103 ties with nothing later
    check_summits(ch, S, [-(1 << 40), 200, 200, 203], [200, 200, 203, 1 << 40], 2)      # empty intervals sharing a start; far bounds
    assert [len(a) for a in ch.peaks_summits(EMPTY, EMPTY, 5)] == [0, 0]
    ch.close()
    rng = np.random.default_rng(41)
    P = np.concatenate([rng.integers(0, 400000, 150000), 123456 + rng.integers(0, 50, 5000)])
    ch, S = points(P)
    pos, cnt = check_summits(ch, S, [-5], [1 << 35], 25)             # one interval holding every point, a w that is no eps
    assert 123456 <= pos[0] < 123506 and cnt[0] > 5000
    check_summits(ch, S, [0, 200000], [200000, 400000], 1)
    edges = np.sort(rng.choice(400000, IVL + 2, replace=False))      # exactly as many intervals as the LDS stage holds, and one more
    check_summits(ch, S, edges[:-2], edges[1:-1], 7)
    check_summits(ch, S, edges[:-1], edges[1:], 7)
    ch.close()
    n = 100000                                                        # 10^5 intervals of one point each
    P = np.arange(n, dtype=np.int64) * 7
    ch, S = points(P, rng.permutation(n))
    pos, cnt = check_summits(ch, S, P, P + 1, 7)
    assert np.array_equal(pos, P) and cnt[0] == 2 and cnt[1] == 3
    pos, cnt = check_summits(ch, S, P[:-1] + 1, P[1:], 3)            # and 10^5 intervals without one
    assert np.all(pos == -1) and np.all(cnt == 0)
    ch.close()


def test_summit_intervals_are_checked():
    from cloops_amd import _lib
    ch, S = points([10, 20, 30])
    for s, e in (([20, 0], [30, 10]), ([0, 5], [10, 20]), ([0, 10], [10, 9]), ([5], [4])):      # unsorted, overlapping, reversed
        with pytest.raises(_lib.CloopsHipError) as ei:
            ch.peaks_summits(s, e, 5)
        assert ei.value.code == _lib.CL_ERR_ARG
    assert ch.peaks_summits([0, 10, 10], [10, 10, 40], 5)[0].tolist() == [-1, -1, 10]    # abutting and empty intervals are fine
    with pytest.raises(ValueError):
        ch.peaks_summits([0, 1], [5], 5)
    with pytest.raises(ValueError):
        ch.peaks_count([[0, 1]], [[5, 6]])
    ch.close()


# ---- repeatability and isolation ---------------------------------------------------------------------
def test_repeatable_and_isolated():
    X, Y = G.chr21_xy()
    ch = chrom(X, Y)
    lab0 = ch.cluster("v2", 1000, 5).labels.copy()
    agg0 = ch.agg_loops([20000000, 30000000], [20100000, 30200000], 1000, 10, 3, want_mats=True)
    ch.track_build("washu", 0, 75, None, "chr21", "chr21")
    ch.track_chunks(1 << 16)
    trk0 = ch.track_render(3)
    cov0 = ch.coverage_build()
    runs0 = ch.coverage_runs()
    nb0 = ch.coverage_text("chr21")
    ch.coverage_chunks(1 << 18)
    txt0 = ch.coverage_render(2)
    S = PC.ends_of(X, Y)
    assert ch.peaks_sort() == (len(S), S[0], S[-1])
    a = ch.peaks_call(150, 5)
    ra = ch.peaks_get()
    b = ch.peaks_call(150, 5)
    assert a == b and all(np.array_equal(u, v) for u, v in zip(ra, ch.peaks_get()))
    ca = ch.peaks_count(ra[0], ra[1])
    sa = ch.peaks_summits(ra[0], ra[1], 100)
    assert all(np.array_equal(u, v) for u, v in zip(ra, ch.peaks_get()))             # counts and summits leave the called peaks alone
    assert ch.track_render(3) == trk0                                                # the built washU track is still there
    assert ch.coverage_render(2) == txt0 and ch.coverage_text("chr21") == nb0        # ... and the built coverage with its text
    assert all(np.array_equal(u, v) for u, v in zip(runs0, ch.coverage_runs()))
    assert np.array_equal(ch.cluster("v2", 1000, 5).labels, lab0)
    agg1 = ch.agg_loops([20000000, 30000000], [20100000, 30200000], 1000, 10, 3, want_mats=True)
    assert all(np.array_equal(u, v) for u, v in zip(agg0[:3], agg1[:3])) and agg0[3] == agg1[3]
    assert ch.coverage_build() == cov0                                               # a coverage build leaves the sorted ends alone
    assert ch.peaks_call(150, 5) == a and all(np.array_equal(u, v) for u, v in zip(ra, ch.peaks_get()))
    assert np.array_equal(ch.peaks_count(ra[0], ra[1]), ca)
    assert all(np.array_equal(u, v) for u, v in zip(sa, ch.peaks_summits(ra[0], ra[1], 100)))
    s, e, p, c = ch.peaks_get(5, 7)                                                  # a range of peaks
    assert all(np.array_equal(u, v[5:12]) for u, v in zip((s, e, p, c), ra))
    ch.peaks_free()
    ch.coverage_free()
    ch.track_free()
    ch.close()


# ---- argument errors ----------------------------------------------------------------------------------
def test_argument_errors():
    from cloops_amd import api, _lib
    lib = _lib.load()
    E = _lib.CL_ERR_ARG
    X, Y = G.chr21_xy()
    ch = api.Chromosome(X, Y)
    i64 = lambda: ctypes.c_int64(7)
    ne, lo, hi, npk, nc, ncl = i64(), i64(), i64(), i64(), i64(), i64()
    so = (ctypes.byref(ne), ctypes.byref(lo), ctypes.byref(hi))
    co = (ctypes.byref(npk), ctypes.byref(nc), ctypes.byref(ncl))
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    s4, e4, p4, c4 = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    ivs, ive = np.array([0, 20000000], np.int64), np.array([20000000, 50000000], np.int64)
    cnt, pos = np.zeros(2, np.uint32), np.zeros(2, np.int32)
    sort, call, get, count, summits = lib.cl_peak_sort, lib.cl_peak_call, lib.cl_peak_get, lib.cl_peak_count, lib.cl_peak_summits
    # a call, get, count or summit before a sort
    assert call(ch._h, 100, 5, *co) == E and (npk.value, nc.value, ncl.value) == (0, 0, 0)          # (a refused call zeroes its outputs)
    assert get(ch._h, 0, 0, vp(s4), vp(e4), vp(p4), vp(c4)) == E
    assert count(ch._h, vp(ivs), vp(ive), 2, vp(cnt)) == E
    assert summits(ch._h, vp(ivs), vp(ive), 2, 100, vp(pos), vp(cnt)) == E
    # sort: a NULL handle, NULL outputs, ends
    assert sort(None, 0, 3, *so) == E
    for k in range(3):
        assert sort(ch._h, 0, 3, *[None if j == k else o for j, o in enumerate(so)]) == E
    assert sort(ch._h, 0, 0, *so) == E and sort(ch._h, 0, 4, *so) == E and sort(ch._h, 0, -1, *so) == E
    assert b"cl_peak_sort" in lib.cl_last_error()
    assert call(ch._h, 100, 5, *co) == E                                                            # a refused sort sorts nothing
    assert sort(ch._h, 0, 3, *so) == 0 and (ne.value, lo.value, hi.value) == (199348, 5033853, 46688446)
    # get before a call
    assert get(ch._h, 0, 0, vp(s4), vp(e4), vp(p4), vp(c4)) == E
    # call: a NULL handle, NULL outputs, eps, min_pts
    assert call(None, 100, 5, *co) == E
    for k in range(3):
        assert call(ch._h, 100, 5, *[None if j == k else o for j, o in enumerate(co)]) == E
    assert call(ch._h, 0, 5, *co) == E and call(ch._h, -1, 5, *co) == E and call(ch._h, 1 << 29, 5, *co) == E
    assert call(ch._h, 100, 0, *co) == E and call(ch._h, 100, -3, *co) == E
    assert b"cl_peak_call" in lib.cl_last_error()
    assert get(ch._h, 0, 0, vp(s4), vp(e4), vp(p4), vp(c4)) == E                                    # a refused call calls nothing
    assert call(ch._h, (1 << 29) - 1, 5, *co) == 0 and (npk.value, nc.value, ncl.value) == (1, 199348, 199348)
    assert call(ch._h, 100, 5, *co) == 0 and (npk.value, nc.value, ncl.value) == (3421, 59803, 67866)
    # get: the range, NULL outputs
    assert get(None, 0, 1, vp(s4), vp(e4), vp(p4), vp(c4)) == E
    assert get(ch._h, -1, 1, vp(s4), vp(e4), vp(p4), vp(c4)) == E and get(ch._h, 0, -1, vp(s4), vp(e4), vp(p4), vp(c4)) == E
    assert get(ch._h, 3420, 2, vp(s4), vp(e4), vp(p4), vp(c4)) == E and get(ch._h, 3422, 0, vp(s4), vp(e4), vp(p4), vp(c4)) == E
    for k in range(4):
        assert get(ch._h, 0, 1, *[None if j == k else vp(a) for j, a in enumerate((s4, e4, p4, c4))]) == E
    assert get(ch._h, 3421, 0, None, None, None, None) == 0
    assert get(ch._h, 3417, 4, vp(s4), vp(e4), vp(p4), vp(c4)) == 0 and e4[3] > s4[3] > 0 and p4[3] >= c4[3] >= 1
    # count: NULLs, a negative n
    assert count(None, vp(ivs), vp(ive), 2, vp(cnt)) == E and count(ch._h, vp(ivs), vp(ive), -1, vp(cnt)) == E
    assert count(ch._h, None, vp(ive), 2, vp(cnt)) == E and count(ch._h, vp(ivs), None, 2, vp(cnt)) == E
    assert count(ch._h, vp(ivs), vp(ive), 2, None) == E
    assert count(ch._h, None, None, 0, None) == 0
    assert count(ch._h, vp(ivs), vp(ive), 2, vp(cnt)) == 0 and int(cnt.sum()) == 199348
    # summits: NULLs, w, the order of the intervals
    assert summits(None, vp(ivs), vp(ive), 2, 100, vp(pos), vp(cnt)) == E and summits(ch._h, vp(ivs), vp(ive), -1, 100, vp(pos), vp(cnt)) == E
    assert summits(ch._h, None, vp(ive), 2, 100, vp(pos), vp(cnt)) == E and summits(ch._h, vp(ivs), None, 2, 100, vp(pos), vp(cnt)) == E
    assert summits(ch._h, vp(ivs), vp(ive), 2, 100, None, vp(cnt)) == E and summits(ch._h, vp(ivs), vp(ive), 2, 100, vp(pos), None) == E
    assert summits(ch._h, vp(ivs), vp(ive), 2, 0, vp(pos), vp(cnt)) == E and summits(ch._h, vp(ivs), vp(ive), 2, 1 << 29, vp(pos), vp(cnt)) == E
    assert summits(ch._h, vp(ive), vp(ivs), 2, 100, vp(pos), vp(cnt)) == E                          # ends before starts
    bad = np.array([0, 10000000], np.int64)
    assert summits(ch._h, vp(bad), vp(ive), 2, 100, vp(pos), vp(cnt)) == E                          # overlapping
    assert b"cl_peak_summits" in lib.cl_last_error()
    assert summits(ch._h, None, None, 0, 100, None, None) == 0
    assert summits(ch._h, vp(ivs), vp(ive), 2, 100, vp(pos), vp(cnt)) == 0 and pos[0] > 0 and cnt[1] >= 5
    assert get(ch._h, 3417, 4, vp(s4), vp(e4), vp(p4), vp(c4)) == 0                                 # the handle is usable after each
    assert lib.cl_peak_free(None) == E
    # the Python layer
    with pytest.raises(_lib.CloopsHipError):
        ch.peaks_sort(ends=7)
    with pytest.raises(_lib.CloopsHipError):
        ch.peaks_call(0, 5)
    # runs in flight
    assert sort(ch._h, 0, 3, *so) == 0 and call(ch._h, 100, 5, *co) == 0
    ch.cluster_async("v2", 2000, 5)
    assert sort(ch._h, 0, 3, *so) == E and call(ch._h, 100, 5, *co) == E
    assert get(ch._h, 0, 1, vp(s4), vp(e4), vp(p4), vp(c4)) == E
    assert count(ch._h, vp(ivs), vp(ive), 2, vp(cnt)) == E
    assert summits(ch._h, vp(ivs), vp(ive), 2, 100, vp(pos), vp(cnt)) == E
    assert lib.cl_peak_free(ch._h) == E
    ch.wait()
    assert ch.peaks_call(100, 10) == (642, 41236, 45299)                                            # the handle still works
    assert ch.peaks_free() is None
    with pytest.raises(_lib.CloopsHipError):
        ch.peaks_call(100, 10)                                                                      # freed: no sorted ends
    ch.close()


# ---- the chr21 example ----------------------------------------------------------------------------------
PINNED = (((100, 5), 3421, 67866, 59803, 4400),
          ((100, 10), 642, 45299, 41236, 2526),
          ((150, 5), 5137, 86357, 73937, 6028),
          ((200, 10), 937, 58398, 52629, 6217),
          ((200, 20), 327, 43899, 39812, 3377))


@pytest.fixture(scope="module")
def chr21():
    X, Y = G.chr21_xy()
    assert len(X) == 99674
    ch = chrom(X, Y)
    S = PC.ends_of(X, Y)
    assert ch.peaks_sort() == (199348, S[0], S[-1])
    yield ch, X, Y, S
    ch.close()


@pytest.mark.parametrize("setting,n_peaks,n_clustered,n_cores,longest", PINNED)
def test_chr21_pinned(chr21, setting, n_peaks, n_clustered, n_cores, longest):
    ch, X, Y, S = chr21
    r = check_call(ch, S, *setting)
    assert ch.peaks_call(*setting) == (n_peaks, n_cores, n_clustered)
    s, e, p, c = ch.peaks_get()
    assert int((e - s).max()) == longest and int(c.sum()) == n_cores and int(p.sum()) == n_clustered


def test_chr21_left_ends(chr21):
    ch, X, Y, S = chr21
    S1 = PC.ends_of(X, Y, 0, 1)
    assert ch.peaks_sort(0, 1) == (99674, S1[0], S1[-1])
    assert len(check_call(ch, S1, 150, 5)[0]) == 1443
    assert ch.peaks_sort() == (199348, S[0], S[-1])                   # (the fixture's sort for the tests after this one)


# ---- end to end -------------------------------------------------------------------------------------------
def _write_jd(d, name, X, Y):
    import joblib
    os.makedirs(d, exist_ok=True)
    joblib.dump(np.stack([np.arange(len(X)), X, Y], 1).astype(np.int64), os.path.join(d, "%s-%s.jd" % (name, name)))


def _run_module(args, cwd):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "cloops_amd.peaks"] + args, env=env, cwd=cwd, timeout=300, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def _host_texts(data, names, eps, minPts, cut, ends, flank, pcut, escut):
    """the three files from the host functions of cloops_amd.peaks fed by the oracle"""
    from cloops_amd import peaks
    code = peaks.ends_code(ends)
    per = {name: peaks.chrom_peaks(PC.OracleChrom(*data[name]), eps, minPts, cut, code, flank) for name in names}
    return peaks.outputs_of(per, eps, minPts, cut, ends, flank, pcut, escut)[0]


def _files(prefix):
    from cloops_amd import peaks
    out = {}
    for suffix in peaks.SUFFIXES:
        with open(prefix + suffix) as fh:
            out[suffix] = fh.read()
    return out


def test_jd2peaks_and_command_line(tmp_path):
    from cloops_amd import peaks, pipe
    data = PC.seeded_genome()
    d = os.path.join(str(tmp_path), "jd")
    for name, (X, Y) in data.items():                                # creation order chr2, chr10, chrX; string order chr10, chr2, chrX
        _write_jd(d, name, X, Y)
    import joblib
    joblib.dump(np.zeros((3, 3), np.int64), os.path.join(d, "chr2-chr10.jd"))        # a trans file is left out
    pipe.CACHE.clear()
    out = os.path.join(str(tmp_path), "direct")
    js = peaks.jd2peaks(d, out, eps=(60, 120), minPts=(4, 8))
    pipe.CACHE.clear()
    want = _host_texts(data, ["chr10", "chr2", "chrX"], [60, 120], [4, 8], 0, "both", [5, 10], 1e-2, 2.0)
    assert _files(out) == want                                        # all three files byte for byte
    assert list(js["chroms"]) == ["chr10", "chr2", "chrX"] and js["total"]["merged"] > 100 and js["total"]["significant"] > 20
    assert js["total"]["merged"] == want["_peaks.txt"].count("\n") - 1 and js["total"]["significant"] == want["_peaks.bed"].count("\n")
    out = os.path.join(str(tmp_path), "cli")
    _run_module(["-d", d, "-o", out, "-eps", "80", "-minPts", "6,3", "-cut", "1000", "-ends", "left", "-flank", "3", "-pcut", "1e-3",
                 "-escut", "3", "-c", "chr2,chrX"], str(tmp_path))
    want = _host_texts(data, ["chr2", "chrX"], [80], [3, 6], 1000, "left", [3], 1e-3, 3.0)
    assert _files(out) == want
    assert json.loads(want["_peaks.json"])["total"]["significant"] > 5


def test_peaks_flag_of_the_main_command(tmp_path):
    """-peaks on the chr21 BEDPE example writes what the host functions make of the oracle's integers and leaves the loops what they
    were; the module on the .jd files that -s leaves behind gives the pinned totals of the defaults"""
    import gzip
    from cloops_amd import pipe
    X, Y = G.chr21_xy()
    bed = os.path.join(str(tmp_path), "in.bedpe.gz")
    with gzip.open(bed, "wt") as fh:                       # a BEDPE whose mid-points are exactly (X, Y)
        for x, y in zip(X.tolist(), Y.tolist()):
            fh.write("chr21\t%d\t%d\tchr21\t%d\t%d\tid\t1\t+\t-\n" % (x, x, y, y))
    fout = os.path.join(str(tmp_path), "run")
    pipe.CACHE.clear()
    assert pipe.main(["-f", bed, "-o", fout, "-m", "0", "-eps", "500,1000,2000", "-minPts", "5", "-s", "-peaks", "-peakeps", "150",
                      "-peakminPts", "5"]) == 0
    pipe.CACHE.clear()
    assert os.path.isfile(fout + ".loop") and os.path.isfile(os.path.join(fout, "chr21-chr21.jd"))
    assert open(fout + ".loop").read() == open(os.path.join(G.GOLD, "chr21_v2.loop")).read()      # identical with and without the flag
    got = _files(fout)
    js = json.loads(got["_peaks.json"])
    assert js["chroms"]["chr21"]["settings"] == {"150,5": {"n_peaks": 5137, "n_cores": 73937, "n_clustered": 86357}}
    assert js["total"]["n_ends"] == 199348 and js["eps"] == [150] and js["minPts"] == [5] and js["total"]["merged"] == 5137
    assert got == _host_texts({"chr21": (X, Y)}, ["chr21"], [150], [5], 0, "both", [5, 10], 1e-2, 2.0)
    out = os.path.join(str(tmp_path), "again")                        # the module's defaults on the .jd files that -s left behind
    _run_module(["-d", fout, "-o", out], str(tmp_path))
    got = _files(out)
    js = json.loads(got["_peaks.json"])
    assert (js["total"]["candidates"], js["total"]["merged"], js["total"]["significant"]) == (11857, 6849, 403)
    assert js["eps"] == [100, 200] and js["minPts"] == [5, 10]
    assert got == _host_texts({"chr21": (X, Y)}, ["chr21"], [100, 200], [5, 10], 0, "both", [5, 10], 1e-2, 2.0)
