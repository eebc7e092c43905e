"""GPU: kernel K24 (cl_mat_window / cl_mat_cells / cl_mat_cells_get / cl_mat_v4c) against the numpy oracle of tests/matrix_cases.py,
written from the definitions of include/cloops_hip.h (it does not call cloops_amd.matrix): every count equal.  Degenerate inputs, the
bin rule at its edges, tile edges, the LDS and the global path of the window on the same rows, large counts, windows off the data, the
mirror, the cells with their two cross-checks against K12 and the dense window, the virtual 4C with its identity against the two
windows, determinism, the handle's other results (unchanged), argument errors, the three subcommands in a child process and -mat on
the main command."""
import ctypes
import json
import os

import numpy as np
import pytest

import matrix_cases as MC
import golden_util as G

pytestmark = pytest.mark.gpu

EMPTY = MC.EMPTY
TILE = 2048          # k_matrix.hip K24_TILE: table rows per workgroup of k24_window and k24_v4c
CELLS = 8192         # k_matrix.hip K24_CELLS: LDS counters per workgroup (the whole window, or the strip of a tile's X bins)
WMAX = 8192          # include/cloops_hip.h CL_MAT_WMAX
LIM = (1 << 29) - 1  # the largest coordinate of a handle, and the largest res


def chrom(X, Y):
    from cloops_amd import api
    return api.Chromosome(np.asarray(X, np.int64), np.asarray(Y, np.int64))


def check_window(ch, X, Y, res, bx0, by0, nx, ny, cut=0, mirror=False):
    got = ch.mat_window(res, bx0, by0, nx, ny, cut=cut, mirror=mirror)
    want = MC.window_oracle(X, Y, cut, res, bx0, by0, nx, ny, mirror)
    assert got[0].dtype == np.uint32 and got[0].shape == (nx, ny)
    bad = np.argwhere(got[0] != want[0])
    assert len(bad) == 0, (res, bx0, by0, nx, ny, cut, mirror, len(bad), bad[:5], got[0][tuple(bad[:5].T)], want[0][tuple(bad[:5].T)])
    assert got[1:] == want[1:] and got[1] == int(got[0].sum(dtype=np.int64)), (got[1:], want[1:])
    return got


def check_cells(ch, X, Y, res, cut=0, fold=False):
    bx, by, cnt, nk = MC.cells_oracle(X, Y, cut, res, fold)
    got = ch.mat_cells(res, cut=cut, fold=fold)
    assert got == (len(bx), nk, int(cnt.max()) if len(cnt) else 0), (res, cut, fold, got)
    g = ch.mat_cells_get()
    assert [a.dtype for a in g] == [np.int32, np.int32, np.uint32]
    assert np.array_equal(g[0], bx) and np.array_equal(g[1], by) and np.array_equal(g[2], cnt), (res, cut, fold)
    assert int(g[2].sum(dtype=np.int64)) == nk
    return g


def check_v4c(ch, X, Y, res, v0, v1, b0, nb, cut=0):
    got = ch.mat_v4c(res, v0, v1, b0, nb, cut=cut)
    want = MC.v4c_oracle(X, Y, cut, res, v0, v1, b0, nb)
    assert got[0].dtype == np.uint32 and got[0].shape == (nb,)
    bad = np.flatnonzero(got[0] != want[0])
    assert len(bad) == 0, (res, v0, v1, b0, nb, cut, len(bad), bad[:5], got[0][bad[:5]], want[0][bad[:5]])
    assert got[1:] == want[1:], (got[1:], want[1:])
    return got


# ---- degenerate inputs -----------------------------------------------------------------------------
def test_degenerate_inputs():
    for X, Y, cut in ((EMPTY, EMPTY, 0), ([500], [700], 0), ([500, 90], [700, 95], 1 << 20), ([500], [700], 201)):
        ch = chrom(X, Y)
        n = len(MC.kept(X, Y, cut)[0])
        w = check_window(ch, X, Y, 100, 0, 0, 10, 10, cut, True)
        assert w[1:] == (2 * n, n)
        c = check_cells(ch, X, Y, 100, cut)
        assert len(c[0]) == n and ch.mat_cells(100, cut=cut) == (n, n, n)
        assert all(len(a) == 0 for a in ch.mat_cells_get(n, 0))
        v = check_v4c(ch, X, Y, 100, 500, 501, 0, 10, cut)
        assert v[1:] == (n, 0, n)
        ch.mat_free()
        ch.close()


# ---- bins --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [1, 7, 1000, LIM])
def test_bins_of_negative_and_extreme_coordinates(res):
    pts = np.array([-1, 0, -res, -res - 1, res - 1, res, LIM, -LIM, 1, -2], np.int64)
    pts = pts[np.abs(pts) <= LIM]
    X, Y = np.repeat(pts, len(pts)), np.tile(pts, len(pts))
    ch = chrom(X, Y)
    lo = int(np.floor_divide(-LIM, res))
    for bx0, by0, nx, ny in ((-3, -3, 6, 6), (lo, lo, 4, 4), (int(LIM // res) - 2, -2, 4, 4), (-2, lo - 1, 5, 3)):
        check_window(ch, X, Y, res, bx0, by0, nx, ny)
        check_window(ch, X, Y, res, bx0, by0, nx, ny, mirror=True)
    for fold in (False, True):
        g = check_cells(ch, X, Y, res, fold=fold)
    assert g[0][0] == lo                                                    # floor, also below zero
    check_v4c(ch, X, Y, res, -res - 1, 1, -3, 6)
    check_v4c(ch, X, Y, res, -LIM, -LIM + 1, lo, 3)
    check_v4c(ch, X, Y, res, LIM, LIM + 1, lo, 3)
    ch.close()


def test_rows_at_the_edges_of_the_window():
    res, bx0, by0, nx, ny = 250, 37, -5, 9, 11
    ex = np.array([bx0 * res - 1, bx0 * res, (bx0 + nx) * res - 1, (bx0 + nx) * res], np.int64)
    ey = np.array([by0 * res - 1, by0 * res, (by0 + ny) * res - 1, (by0 + ny) * res], np.int64)
    X = np.concatenate([np.repeat(ex, 4), np.repeat(ey, 4)])
    Y = np.concatenate([np.tile(ey, 4), np.tile(ex, 4)])                    # both orientations: the mirrored half meets the same edges
    ch = chrom(X, Y)
    a = check_window(ch, X, Y, res, bx0, by0, nx, ny)
    assert a[1] == 4 and a[0][0, 0] == a[0][0, ny - 1] == a[0][nx - 1, 0] == a[0][nx - 1, ny - 1] == 1
    assert check_window(ch, X, Y, res, bx0, by0, nx, ny, mirror=True)[1] == 8
    v = check_v4c(ch, X, Y, res, bx0 * res, (bx0 + nx) * res, by0, ny)
    assert v[1:3] == (8, 8)
    ch.close()


# ---- tile edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_tile_edges(m):
    rng = np.random.default_rng(m)
    res, bx0, nx = 100, 50, 40
    inside = rng.integers(bx0 * res, (bx0 + nx) * res, m)
    X = np.concatenate([rng.integers(0, bx0 * res, 700), inside, rng.integers((bx0 + nx) * res, 20000, 900)])
    Y = X + rng.integers(0, 3000, len(X))
    ch = chrom(X, Y)
    assert check_window(ch, X, Y, res, bx0, bx0, nx, 60)[1] > m // 2
    check_window(ch, X, Y, res, bx0, bx0, nx, 300)                          # 12 000 cells: the strip of a tile
    check_window(ch, X, Y, res, bx0, bx0, nx, nx, mirror=True)
    v = check_v4c(ch, X, Y, res, bx0 * res, (bx0 + nx) * res, 0, 300)
    assert v[1] == m
    ch.close()


# ---- both paths of the window ----------------------------------------------------------------------------
def test_lds_and_global_paths_on_the_same_rows():
    X, Y = MC.scattered(11, 3 * TILE + 77, 2048, 8192, both=True)
    ch = chrom(X, Y)
    # dense X: 6 000 rows over 21 bins of 100 bp, a tile spans few of them
    check_window(ch, X, Y, 100, 0, 0, 21, 103, mirror=True)                 # 2 163 cells: the whole window in LDS
    check_window(ch, X, Y, 100, 0, 0, 21, 1000)                             # 21 000 cells: the strip of each tile
    # res 1, scattered X and 8192 columns: a tile spans hundreds of X bins, nothing fits, every add is global
    a = check_window(ch, X, Y, 1, 0, 0, 2048, WMAX)
    assert a[1] > TILE
    b = check_window(ch, X, Y, 1, 0, 0, 2048, WMAX, mirror=True)
    assert b[1] > a[1]
    ch.close()


@pytest.mark.parametrize("nx,ny", [(64, 128), (1, CELLS), (CELLS, 1), (3, 2731), (2731, 3), (2, 4097), (4097, 2)])
def test_the_lds_budget_and_one_cell_more(nx, ny):
    assert nx * ny in (CELLS, CELLS + 1, CELLS + 2)
    rng = np.random.default_rng(nx)
    res = 10
    X = rng.integers(0, nx * res, TILE + 300)
    Y = rng.integers(0, ny * res, TILE + 300)
    ch = chrom(X, Y)
    assert check_window(ch, X, Y, res, 0, 0, nx, ny)[1] == TILE + 300
    check_window(ch, X, Y, res, 0, 0, nx, ny, mirror=True)
    ch.close()


def test_large_counts_in_one_cell():
    X = np.concatenate([np.full(70000, 123456), [5, 999999]])
    Y = np.concatenate([np.full(70000, 223456), [7, 1000001]])
    ch = chrom(X, Y)
    a = check_window(ch, X, Y, 1000, 100, 200, 50, 50)
    assert a[0][23, 23] == 70000 and a[1] == 70000                          # above 2^16, from 35 tiles
    assert check_window(ch, X, Y, 1000, 100, 100, 150, 150, mirror=True)[0][123, 23] == 70000
    assert check_window(ch, X, Y, 1, 123000, 223000, 1000, 1000)[0][456, 456] == 70000      # 10^6 cells: the strip path
    assert ch.mat_cells(1000) == (3, 70002, 70000)
    assert check_v4c(ch, X, Y, 1000, 123000, 124000, 0, 1 << 20)[0][223] == 70000
    ch.close()


def test_window_placement():
    X, Y = MC.scattered(2, 5000, 100000, 20000)
    ch = chrom(X, Y)
    assert 0 < check_window(ch, X, Y, 1000, -20, -20, 60, 60)[1] < 5000     # partly below the data
    assert 0 < check_window(ch, X, Y, 1000, 90, 90, 80, 80, mirror=True)[1]   # partly above it
    for bx0, by0 in ((500, 500), (-500, -500), (1 << 30, 1 << 30), (-(1 << 30), -(1 << 30)), (0, 1 << 30), ((1 << 30) - 5, 10)):
        a = check_window(ch, X, Y, 1000, bx0, by0, 40, 40, mirror=True)     # wholly outside
        assert a[1] == 0 and not a[0].any()
    a = check_window(ch, X, Y, LIM, -(1 << 30), -(1 << 30), 1, 1)
    assert a[1] == 0
    ch.close()


# ---- mirror ------------------------------------------------------------------------------------------------
def test_mirror():
    X, Y = MC.scattered(3, 6000, 50000, 12000, both=True)
    assert (Y < X).sum() > 1000
    ch = chrom(X, Y)
    for res, b0, n in ((500, 0, 124), (500, 20, 60), (77, 100, 400)):
        w = check_window(ch, X, Y, res, b0, b0, n, n)[0]
        wm = check_window(ch, X, Y, res, b0, b0, n, n, mirror=True)[0]
        assert np.array_equal(wm, wm.T) and np.array_equal(np.diag(wm), np.diag(w))
        assert np.array_equal(wm.astype(np.int64), w.astype(np.int64) + w.T - np.diag(np.diag(w)))
    # an off-diagonal window whose mirrored range overlaps its own range
    assert check_window(ch, X, Y, 500, 10, 30, 50, 50, mirror=True)[1] > check_window(ch, X, Y, 500, 10, 30, 50, 50)[1]
    ch.close()
    # ... and one no mirrored row reaches: every row has Y >= X, and the window lies above the diagonal
    X, Y = MC.scattered(3, 6000, 50000, 12000)
    ch = chrom(X, Y)
    a, b = check_window(ch, X, Y, 500, 10, 30, 20, 20), check_window(ch, X, Y, 500, 10, 30, 20, 20, mirror=True)
    assert a[1] > 0 and np.array_equal(a[0], b[0]) and a[1] == b[1]
    ch.close()


# ---- cells -------------------------------------------------------------------------------------------------
def test_cells_single_cell_and_order():
    ch = chrom([1001, 1500, 1999], [7000, 7999, 7001])
    g = check_cells(ch, [1001, 1500, 1999], [7000, 7999, 7001], 1000)
    assert (g[0].tolist(), g[1].tolist(), g[2].tolist()) == ([1], [7], [3]) and ch.mat_cells(1000) == (1, 3, 3)
    ch.close()
    X, Y = MC.scattered(4, 4000, 30000, 9000, both=True)
    ch = chrom(X, Y)
    for fold in (False, True):
        bx, by, cnt = check_cells(ch, X, Y, 300, fold=fold)
        key = bx.astype(np.int64) * (1 << 32) + by
        assert (np.diff(key) > 0).all() and (not fold or (bx <= by).all())
    ch.close()


@pytest.mark.parametrize("span", [200000, 200000000])
def test_cells_random_sets(span):
    X, Y = MC.scattered(span % 97, 20000, span, span // 5, both=True)
    ch = chrom(X, Y)
    for res, cut, fold in ((1000, 0, False), (1000, span // 50, True), (1, 0, True), (span // 100, 0, False)):
        check_cells(ch, X, Y, res, cut, fold)
    n = ch.mat_cells(1000, fold=True)[0]
    whole = ch.mat_cells_get()
    parts = [ch.mat_cells_get(f, min(777, n - f)) for f in range(0, n, 777)]
    assert all(np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]) for k in range(3))
    assert all(len(a) == 0 for a in ch.mat_cells_get(n, 0)) and all(len(a) == 1 for a in ch.mat_cells_get(n - 1))
    ch.close()


def test_cells_against_k12_and_the_dense_window():
    rng = np.random.default_rng(6)
    res = 500
    X = np.concatenate([[0], rng.integers(0, 150000, 15000)])
    Y = np.concatenate([[140000], X[1:] + rng.integers(0, 40000, 15000)])    # the smallest coordinate, 0, is a multiple of res at every cut below
    ch = chrom(X, Y)
    for cut in (0, 5000):
        values, mult, nk, minc = ch.contact_hist(res, cut)                  # K12 bins from the data's minimum: the same cells here
        assert minc == 0
        n, nk2, mx = ch.mat_cells(res, cut=cut)
        cnt = ch.mat_cells_get()[2]
        v, c = np.unique(cnt, return_counts=True)
        assert nk2 == nk and np.array_equal(v, values) and np.array_equal(c, mult) and mx == values[-1] and n == mult.sum()
    for fold in (False, True):
        n = ch.mat_cells(res, fold=fold)[0]
        bx, by, cnt = ch.mat_cells_get()
        lo, hi = int(min(bx.min(), by.min())), int(max(bx.max(), by.max()))
        w = hi - lo + 1
        dense, n_in, nk = ch.mat_window(res, lo, lo, w, w)
        assert n_in == nk == len(X)
        if fold:
            dense = np.triu(dense.astype(np.int64)) + np.tril(dense.astype(np.int64), -1).T
        assert np.array_equal(MC.dense_scatter(bx, by, cnt, lo, lo, w, w), dense)
    ch.close()


# ---- virtual 4C ----------------------------------------------------------------------------------------------
def test_v4c():
    X, Y = MC.scattered(7, 3 * TILE + 5, 60000, 15000, both=True)
    X[:3], Y[:3] = [30010, 30020, 30999], [30500, 30020, 30000]             # both ends in the viewpoint [30000, 31000)
    ch = chrom(X, Y)
    v = check_v4c(ch, X, Y, 100, 30000, 31000, 0, 800)                      # nb <= CELLS: LDS
    assert v[0][300:310].sum() >= 6 and v[1] >= 3 and v[2] >= 3
    check_v4c(ch, X, Y, 100, 30000, 31000, 0, 800, cut=2000)
    check_v4c(ch, X, Y, 1, 30000, 31000, -50000, 1 << 20)                   # nb = 2^20: the tile's X bins in LDS, the rest global
    check_v4c(ch, X, Y, 1, 0, 80000, 0, CELLS + 1)                          # one bin above the LDS budget, every row a hit
    assert check_v4c(ch, X, Y, 100, 30000, 30000, 0, 800)[1:3] == (0, 0)    # an empty viewpoint
    assert check_v4c(ch, X, Y, 100, 900000, 990000, 0, 800)[1:3] == (0, 0)  # ... one outside the data
    assert check_v4c(ch, X, Y, 100, -(1 << 40), -5, 0, 800)[1:3] == (0, 0)
    assert check_v4c(ch, X, Y, 100, 30000, 31000, 0, 0)[1] >= 3             # nb = 0: only the counters
    a = check_v4c(ch, X, Y, 100, -(1 << 40), 1 << 40, -10, 900)             # wider than the data: every end counts
    assert a[1:] == (len(X), len(X), len(X)) and int(a[0].sum()) == 2 * len(X)
    assert check_v4c(ch, X, Y, 100, 30000, 31000, 5000, 100)[0].sum() == 0  # the bins off the data, the counters not
    ch.close()


@pytest.mark.parametrize("res,i", [(100, 300), (1000, 7), (250, 0)])
def test_v4c_identity_with_the_windows(res, i):
    X, Y = MC.scattered(8, 9000, 60000, 15000, both=True)
    ch = chrom(X, Y)
    n = 75000 // res + 1
    w = ch.mat_window(res, 0, 0, n, n)[0].astype(np.int64)
    wm = ch.mat_window(res, 0, 0, n, n, mirror=True)[0].astype(np.int64)
    v = check_v4c(ch, X, Y, res, i * res, (i + 1) * res, 0, n)[0].astype(np.int64)
    assert v.sum() > 0 and np.array_equal(v, wm[i] + (np.arange(n) == i) * w[i, i])
    ch.close()


# ---- determinism ---------------------------------------------------------------------------------------------
def test_each_call_twice():
    X, Y = MC.scattered(9, 4 * TILE, 40000, 9000, both=True)
    ch = chrom(X, Y)
    for args in ((100, 0, 0, 400, 400, 0, True), (1, 100, 100, 2048, 4096, 0, False), (500, 0, 0, 50, 50, 3000, True)):
        a, b = ch.mat_window(*args), ch.mat_window(*args)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    for args in ((100, 20000, 21000, 0, 500), (1, 20000, 21000, 0, 1 << 20)):
        a, b = ch.mat_v4c(*args), ch.mat_v4c(*args)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    a = (ch.mat_cells(100, fold=True), ch.mat_cells_get())
    b = (ch.mat_cells(100, fold=True), ch.mat_cells_get())
    assert a[0] == b[0] and all(np.array_equal(u, v) for u, v in zip(a[1], b[1]))
    ch.close()


# ---- the handle's other state ---------------------------------------------------------------------------------
def test_other_results_unchanged():
    from cloops_amd import _lib
    X, Y = G.chr21_xy()
    X, Y = X[:30000], Y[:30000]
    ch = chrom(X, Y)
    cx, cy = [20000000, 30000000], [20100000, 30200000]
    lab0 = ch.cluster("v2", 1000, 5).labels.copy()
    agg0 = ch.agg_loops(cx, cy, 1000, 10, 3, want_mats=True)
    trk0 = ch.domains_tracks(0, 10000, 10)
    dom0 = [a.copy() for a in ch.domains_get()]
    s = np.arange(5000000, 47000000, 1000000)
    cnt0 = ch.domains_count(s, s + 900000)
    assert ch.kdis_build([4], 0) == len(X)
    kd0 = [a.copy() for a in ch.kdis_get()]

    def others_unchanged():
        assert all(np.array_equal(u, v) for u, v in zip(dom0, ch.domains_get()))
        assert all(np.array_equal(u, v) for u, v in zip(cnt0, ch.domains_count(s, s + 900000)))
        assert all(np.array_equal(u, v) for u, v in zip(kd0, ch.kdis_get()))
        agg1 = ch.agg_loops(cx, cy, 1000, 10, 3, want_mats=True)
        assert all(np.array_equal(u, v) for u, v in zip(agg0[:3], agg1[:3])) and agg0[3] == agg1[3]
    b0 = int(X.min()) // 10000
    for cut in (0, 4000):                                                  # the shared table at the same cut, then rebuilt for another
        check_window(ch, X, Y, 10000, b0, b0, 300, 300, cut, True)
        check_v4c(ch, X, Y, 10000, 20000000, 20100000, b0, 4000, cut)
        cells = check_cells(ch, X, Y, 10000, cut, True)
        others_unchanged()
    ch.agg_loops(cx, cy, 1000, 10, 3, cut=9000)                            # the table rebuilt for another cut: the cells are copies
    assert all(np.array_equal(u, v) for u, v in zip(cells, ch.mat_cells_get()))
    assert ch.domains_tracks(0, 10000, 10) == trk0
    assert np.array_equal(ch.cluster("v2", 1000, 5).labels, lab0)
    assert all(np.array_equal(u, v) for u, v in zip(cells, ch.mat_cells_get()))
    assert ch.mat_free() is None
    with pytest.raises(_lib.CloopsHipError):
        ch.mat_cells_get()                                                 # freed: nothing to get
    with pytest.raises(_lib.CloopsHipError):
        ch.mat_cells_get(0, 0)
    others_unchanged()
    check_window(ch, X, Y, 10000, b0, b0, 300, 300)                        # the calls work again behind a free
    ch.close()


# ---- argument errors ----------------------------------------------------------------------------------
def test_argument_errors():
    from cloops_amd import api, _lib
    lib = _lib.load()
    E = _lib.CL_ERR_ARG
    X, Y = MC.scattered(5, 1000, 50000, 9000)
    ch = api.Chromosome(X, Y)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ref = ctypes.byref
    a, b, c = ctypes.c_int64(7), ctypes.c_int64(7), ctypes.c_int64(7)

    def seven():
        a.value = b.value = c.value = 7
    win, cells, get, v4c = lib.cl_mat_window, lib.cl_mat_cells, lib.cl_mat_cells_get, lib.cl_mat_v4c
    out = np.zeros(64, np.uint32)
    t4 = [np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.uint32)]
    # a get before a build
    assert get(ch._h, 0, 0, *map(vp, t4)) == E and b"cl_mat_cells_get" in lib.cl_last_error()
    want = check_cells(ch, X, Y, 500, 0, True)
    nc = len(want[0])

    def still_there():
        return all(np.array_equal(u, v) for u, v in zip(want, ch.mat_cells_get()))
    # window: a NULL handle, NULL outputs, res, the sizes, the origin
    assert win(None, 0, 100, 0, 0, 8, 8, 0, vp(out), ref(a), ref(b)) == E
    for bad in ((0, 0, 0, 0, 8, 8), (0, 1 << 29, 0, 0, 8, 8), (0, -1, 0, 0, 8, 8), (0, 100, 0, 0, 0, 8), (0, 100, 0, 0, 8, 0), (0, 100, 0, 0, -1, 8),
                (0, 100, 0, 0, WMAX + 1, 1), (0, 100, 0, 0, 1, WMAX + 1), (0, 100, 0, 0, 4096, 4097), (0, 100, (1 << 30) + 1, 0, 8, 8),
                (0, 100, 0, -(1 << 30) - 1, 8, 8)):
        seven()
        assert win(ch._h, *bad, 0, vp(out), ref(a), ref(b)) == E and (a.value, b.value) == (0, 0), bad      # (a refused call zeroes its outputs)
        assert b"cl_mat_window" in lib.cl_last_error()
    seven()
    assert win(ch._h, 0, 100, 0, 0, 8, 8, 0, None, ref(a), ref(b)) == E and (a.value, b.value) == (0, 0)
    assert win(ch._h, 0, 100, 0, 0, 8, 8, 0, vp(out), None, ref(b)) == E and win(ch._h, 0, 100, 0, 0, 8, 8, 0, vp(out), ref(a), None) == E
    assert win(ch._h, 0, 100, 0, 0, 8, 8, 0, vp(out), ref(a), ref(b)) == 0 and b.value == 1000
    # cells: NULL outputs, res
    assert cells(None, 0, 100, 0, ref(a), ref(b), ref(c)) == E
    for bad in (0, -5, 1 << 29):
        seven()
        assert cells(ch._h, 0, bad, 0, ref(a), ref(b), ref(c)) == E and (a.value, b.value, c.value) == (0, 0, 0)
        assert b"cl_mat_cells" in lib.cl_last_error()
    seven()
    assert cells(ch._h, 0, 100, 0, None, ref(b), ref(c)) == E and (b.value, c.value) == (0, 0)
    assert cells(ch._h, 0, 100, 0, ref(a), None, ref(c)) == E and cells(ch._h, 0, 100, 0, ref(a), ref(b), None) == E
    assert still_there()                                                    # ... and leaves the earlier cells
    # get: the range, NULL outputs
    assert get(None, 0, 1, *map(vp, t4)) == E
    assert get(ch._h, -1, 1, *map(vp, t4)) == E and get(ch._h, 0, -1, *map(vp, t4)) == E
    assert get(ch._h, nc - 1, 2, *map(vp, t4)) == E and get(ch._h, nc + 1, 0, *map(vp, t4)) == E
    for k in range(3):
        assert get(ch._h, 0, 1, *[None if j == k else vp(x) for j, x in enumerate(t4)]) == E
    assert b"cl_mat_cells_get" in lib.cl_last_error()
    assert get(ch._h, nc, 0, None, None, None) == 0
    assert get(ch._h, nc - 4, 4, *map(vp, t4)) == 0 and all(np.array_equal(t4[k], want[k][nc - 4:]) for k in range(3))
    # v4c: NULL outputs, res, v0 > v1, nb, b0
    assert v4c(None, 0, 100, 0, 10, 0, 8, vp(out), ref(a), ref(b), ref(c)) == E
    for bad in ((0, 0, 0, 10, 0, 8), (0, 1 << 29, 0, 10, 0, 8), (0, 100, 11, 10, 0, 8), (0, 100, 0, 10, 0, -1), (0, 100, 0, 10, 0, (1 << 24) + 1),
                (0, 100, 0, 10, (1 << 30) + 1, 8), (0, 100, 0, 10, -(1 << 30) - 1, 8)):
        seven()
        assert v4c(ch._h, *bad, vp(out), ref(a), ref(b), ref(c)) == E and (a.value, b.value, c.value) == (0, 0, 0), bad
        assert b"cl_mat_v4c" in lib.cl_last_error()
    seven()
    assert v4c(ch._h, 0, 100, 0, 10, 0, 8, None, ref(a), ref(b), ref(c)) == E and (a.value, b.value, c.value) == (0, 0, 0)
    assert v4c(ch._h, 0, 100, 0, 10, 0, 8, vp(out), None, ref(b), ref(c)) == E and v4c(ch._h, 0, 100, 0, 10, 0, 8, vp(out), ref(a), None, ref(c)) == E
    assert v4c(ch._h, 0, 100, 0, 10, 0, 8, vp(out), ref(a), ref(b), None) == E
    assert v4c(ch._h, 0, 100, 0, 60000, 0, 0, None, ref(a), ref(b), ref(c)) == 0 and (a.value, b.value, c.value) == (1000, 1000, 1000)
    assert lib.cl_mat_free(None) == E
    assert still_there()
    # the Python layer
    for f in (lambda: ch.mat_window(100, 0, 0, 0, 8), lambda: ch.mat_window(100, 0, 0, WMAX + 1, 1), lambda: ch.mat_window(100, 0, 0, 4097, 4096),
              lambda: ch.mat_v4c(100, 0, 10, 0, -1), lambda: ch.mat_v4c(100, 0, 10, 0, (1 << 24) + 1), lambda: ch.mat_v4c(100, 11, 10, 0, 8)):
        with pytest.raises(ValueError):
            f()
    for f in (lambda: ch.mat_window(0, 0, 0, 8, 8), lambda: ch.mat_cells(0), lambda: ch.mat_v4c(1 << 29, 0, 10, 0, 8), lambda: ch.mat_cells_get(nc, 1),
              lambda: ch.mat_window(100, 1 << 31, 0, 8, 8)):
        with pytest.raises(_lib.CloopsHipError):
            f()
    assert still_there()
    # runs in flight
    ch.cluster_async("v2", 2000, 5)
    seven()
    assert win(ch._h, 0, 100, 0, 0, 8, 8, 0, vp(out), ref(a), ref(b)) == E and (a.value, b.value) == (0, 0)
    assert cells(ch._h, 0, 100, 0, ref(a), ref(b), ref(c)) == E
    assert get(ch._h, 0, 1, *map(vp, t4)) == E
    assert v4c(ch._h, 0, 100, 0, 10, 0, 8, vp(out), ref(a), ref(b), ref(c)) == E
    assert lib.cl_mat_free(ch._h) == E
    ch.wait()
    assert still_there()                                                    # the handle still works
    ch.mat_free()
    ch.close()


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
    p = subprocess.run([sys.executable, "-m", "cloops_amd.matrix"] + args, env=env, cwd=cwd, timeout=300, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def _files(prefix, suffixes):
    out = {}
    for suffix in suffixes:
        with open(prefix + suffix) as fh:
            out[suffix] = fh.read()
    return out


def _host_cells(data, names, res, cut, fold):
    from cloops_amd import matrix
    per = {n: matrix.chrom_cells(MC.OracleChrom(*data[n]), n, res, cut, fold) for n in names}
    return matrix.cells_outputs(per, res, cut, fold)[0]


def test_the_three_subcommands(tmp_path):
    from cloops_amd import matrix
    data = {name: MC.scattered(seed, 3000, 400000, 90000, both=True) for name, seed in (("chr2", 0), ("chr10", 1), ("chrX", 2))}
    d = os.path.join(str(tmp_path), "jd")
    for name, (X, Y) in data.items():
        _write_jd(d, name, X, Y)
    import joblib
    joblib.dump(np.zeros((3, 3), np.int64), os.path.join(d, "chr2-chr10.jd"))        # a trans file is left out
    S = matrix.SUFFIXES
    out = os.path.join(str(tmp_path), "o")
    _run_module(["window", "-d", d, "-o", out, "-r", "chr10:100000-300000", "-res", "2000", "-plot"], str(tmp_path))
    r = ("chr10", 100000, 300000)
    want = matrix.window_of(MC.OracleChrom(*data["chr10"]), r, r, 2000, 0, True)[0]
    assert _files(out, S[:2]) == want and json.loads(want[S[1]])["n_in"] > 0
    try:
        import matplotlib                                              # noqa: F401
        assert os.path.getsize(out + "_matrix.pdf") > 0
    except ImportError:
        assert not os.path.exists(out + "_matrix.pdf")
    _run_module(["window", "-d", d, "-o", out, "-r", "chrX:0-200000", "-r2", "chrX:100000-490000", "-res", "5000", "-cut", "1000"], str(tmp_path))
    want = matrix.window_of(MC.OracleChrom(*data["chrX"]), ("chrX", 0, 200000), ("chrX", 100000, 490000), 5000, 1000, False)[0]
    assert _files(out, S[:2]) == want
    _run_module(["cells", "-d", d, "-o", out, "-res", "3000"], str(tmp_path))
    assert _files(out, S[2:4]) == _host_cells(data, ["chr10", "chr2", "chrX"], 3000, 0, True)
    _run_module(["cells", "-d", d, "-o", out, "-res", "700", "-cut", "20000", "-c", "chr2,chrX", "-nofold"], str(tmp_path))
    want = _host_cells(data, ["chr2", "chrX"], 700, 20000, False)
    assert _files(out, S[2:4]) == want and 0 < json.loads(want[S[3]])["total"]["n_kept"] < 6000
    _run_module(["v4c", "-d", d, "-o", out, "-v", "chr2:200000-210000"], str(tmp_path))
    want = matrix.v4c_of(MC.OracleChrom(*data["chr2"]), ("chr2", 200000, 210000), None, 1000, 0, "none")[0]
    assert _files(out, S[4:]) == want and json.loads(want[S[5]])["n_x"] > 0
    _run_module(["v4c", "-d", d, "-o", out, "-v", "chr2:200000-210000", "-r", "chr2:150000-260000", "-res", "500", "-cut", "100", "-norm", "cpm"],
                str(tmp_path))
    want = matrix.v4c_of(MC.OracleChrom(*data["chr2"]), ("chr2", 200000, 210000), ("chr2", 150000, 260000), 500, 100, "cpm")[0]
    assert _files(out, S[4:]) == want
    # refused before any file is written
    from cloops_amd import pipe
    pipe.CACHE.clear()
    bad = os.path.join(str(tmp_path), "bad")
    for f in (lambda: matrix.jd2window(d, bad, "chr7:0-1000"), lambda: matrix.jd2window(d, bad, "chr2:0-1000", region2="chr10:0-1000"),
              lambda: matrix.jd2v4c(d, bad, "chr2:1000-10"), lambda: matrix.jd2window(d, bad, "chr2:0-400000", res=10)):
        with pytest.raises(ValueError):
            f()
    pipe.CACHE.clear()
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("bad")]


def test_mat_flag_of_the_main_command(tmp_path):
    """-mat on the chr21 BEDPE example writes what the host functions make of the oracle's integers and leaves the loops what they
    were"""
    import gzip
    from cloops_amd import matrix, pipe
    X, Y = G.chr21_xy()
    bed = os.path.join(str(tmp_path), "in.bedpe.gz")
    with gzip.open(bed, "wt") as fh:                       # a BEDPE whose mid-points are exactly (X, Y)
        for x, y in zip(X.tolist(), Y.tolist()):
            fh.write("chr21\t%d\t%d\tchr21\t%d\t%d\tid\t1\t+\t-\n" % (x, x, y, y))
    fout = os.path.join(str(tmp_path), "run")
    pipe.CACHE.clear()
    assert pipe.main(["-f", bed, "-o", fout, "-m", "0", "-eps", "500,1000,2000", "-minPts", "5", "-mat", "-matres", "20000"]) == 0
    pipe.CACHE.clear()
    assert open(fout + ".loop").read() == open(os.path.join(G.GOLD, "chr21_v2.loop")).read()      # identical with and without the flag
    got = _files(fout, matrix.SUFFIXES[2:4])
    js = json.loads(got["_cells.json"])
    assert js["res"] == 20000 and js["fold"] is True and js["cut"] == 0 and js["total"]["n_kept"] == len(X) == 99674
    assert got == _host_cells({"chr21": (X, Y)}, ["chr21"], 20000, 0, True)
