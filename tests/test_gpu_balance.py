"""GPU: K25 (cl_bal_marginals / cl_bal_iterate / cl_bal_weights_get / cl_bal_cells_get, cloops_amd.balance) against the numpy oracle of
tests/balance_cases.py -- the integer marginals exactly, the weights within bounds that come from the oracle's own spread between two
orders of summation and from the length of the sums, the tile edges of the marginals kernel, masks, lifetimes, refusals, and the
command end to end."""
import ctypes
import json
import os

import numpy as np
import pytest

import balance_cases as BC
import matrix_cases as MC

pytestmark = pytest.mark.gpu

TILE = BC.TILE       # k_balance.hip K25_TILE: cells per workgroup of k25_marg
SCAT = (3, 40000, 200000, 30000)


def chrom(X, Y):
    from cloops_amd import api
    return api.Chromosome(np.asarray(X, np.int64), np.asarray(Y, np.int64))


def cells_of(X, Y, res, cut=0):
    return MC.cells_oracle(X, Y, cut, res, True)[:3]


def check_marginals(ch, X, Y, res, ign, cut=0):
    """mat_cells + bal_marginals against the oracle, array for array -> the cells, (b0, nb, n_used, sum, nnz)"""
    bx, by, cnt = cells_of(X, Y, res, cut)
    assert ch.mat_cells(res, cut=cut, fold=True)[0] == len(bx)
    want = BC.marginals_oracle(bx, by, cnt, ign)
    assert ch.bal_marginals(ign) == want[:3], (res, ign, cut, want[:3])
    s, z = ch.bal_marginals_get()
    assert (s.dtype, z.dtype, len(s), len(z)) == (np.uint64, np.uint32, want[1], want[1])
    bad = np.flatnonzero((s != want[3]) | (z != want[4]))
    assert len(bad) == 0, (res, ign, cut, len(bad), bad[:5], s[bad[:5]], want[3][bad[:5]], z[bad[:5]], want[4][bad[:5]])
    return (bx, by, cnt), want


def check_weights(ch, cells, ign, valid, max_iters, tol, rtol):
    """bal_iterate + bal_weights against the oracle within rtol (relative, NaN at the same bins) -> the oracle's result, the deviation"""
    o = BC.ice_oracle(*cells, ign, valid, max_iters, tol)
    it, cv, var, sc = ch.bal_iterate(valid, max_iters=max_iters, tol=tol)
    w = ch.bal_weights()
    dev = BC.rel_diff(w, o["weight"])
    print("K25 deviation: cells %d iters %d (oracle %d) var %.17g (oracle %.17g) weights %.3g allowed %.3g" %
          (len(cells[0]), it, o["iters"], var, o["var"], dev, rtol))
    assert (it, cv) == (o["iters"], o["converged"])
    if o["iters"] == 0:
        assert np.isnan(var) and np.isnan(sc) and np.isnan(w).all()
    else:
        # var is the mean of (q - 1)^2 with q = s / mean within 2 rtol: it moves by at most 2 sqrt(var) 2 rtol (Cauchy-Schwarz), and by
        # rtol of itself in the mean over the bins
        assert abs(var - o["var"]) <= 4 * rtol * (np.sqrt(o["var"]) + o["var"]) and abs(sc - o["scale"]) <= rtol * o["scale"]
        assert dev <= rtol
    return o, dev


# ---- the integer marginals, exactly ---------------------------------------------------------------------------------
def test_marginals_of_the_twelve_rows():
    X, Y = MC.twelve()
    ch = chrom(X, Y)
    _, w0 = check_marginals(ch, X, Y, 100, 0)
    assert w0[3].tolist() == [4, 5, 2, 4, 5] and w0[4].tolist() == [3, 4, 2, 3, 4]
    _, w2 = check_marginals(ch, X, Y, 100, 2)
    assert w2[3].tolist() == [2, 3, 1, 2, 4] and w2[2] == 4
    check_marginals(ch, X, Y, 100, 1)
    check_marginals(ch, X, Y, 100, 0, cut=100)
    check_marginals(ch, X, Y, 7, 3)
    ch.close()


@pytest.mark.parametrize("ign,cut", [(0, 0), (2, 0), (2, 5000), (0, 12000), (300, 0)])
def test_marginals_of_scattered_rows(ign, cut):
    X, Y = MC.scattered(*SCAT, both=True)
    ch = chrom(X, Y)
    cells, want = check_marginals(ch, X, Y, 1000, ign, cut)
    if (ign, cut) == (0, 0):
        assert (len(cells[0]), want[1]) == (6176, 230)
    if ign == 300:
        assert want[2] == 0 and not want[3].any()
    ch.close()


def test_marginals_with_negative_bins():
    X, Y = MC.scattered(4, 5000, 60000, 9000, both=True)
    X, Y = X - 30000, Y - 30000
    ch = chrom(X, Y)
    for res, ign in ((1000, 0), (1000, 2), (7, 1), (333, 3)):
        _, want = check_marginals(ch, X, Y, res, ign)
        assert want[0] < 0 < want[0] + want[1]
    ch.close()


def test_degenerate_inputs():
    from cloops_amd import _lib
    # one row: nb = 1 on the diagonal, two bins off it
    ch = chrom([500], [700])
    _, want = check_marginals(ch, [500], [700], 1000, 0)
    assert want[:3] == (0, 1, 1)
    assert ch.bal_iterate([True], max_iters=5, tol=0)[:2] == (5, False)
    assert np.array_equal(ch.bal_weights(), [1.0]) and np.array_equal(ch.bal_cells_get(), [1.0])      # s = 1: w stays 1, scale 1
    _, want = check_marginals(ch, [500], [700], 100, 2)
    assert want[:3] == (5, 3, 1) and want[3].tolist() == [1, 0, 1]
    ch.close()
    # rows all on the diagonal with ignore_diags = 2: nothing used, 0 iterations, all NaN, no error
    X = np.arange(0, 50000, 7)
    ch = chrom(X, X + 3)
    cells, want = check_marginals(ch, X, X + 3, 1000, 2)
    assert want[2] == 0 and want[1] == 50
    for valid in (np.zeros(50, bool), np.ones(50, bool)):
        it, cv, var, sc = ch.bal_iterate(valid)
        assert (it, cv) == (0, False) and np.isnan(var) and np.isnan(sc)
        assert np.isnan(ch.bal_weights()).all() and np.isnan(ch.bal_cells_get()).all() and len(ch.bal_cells_get()) == len(cells[0])
    ch.close()
    # a handle without rows, and a cut that keeps none: nb = 0 and no error anywhere
    for X, Y, cut in ((MC.EMPTY, MC.EMPTY, 0), ([500, 90], [700, 95], 1 << 20)):
        ch = chrom(X, Y)
        assert ch.mat_cells(1000, cut=cut, fold=True)[0] == 0
        assert ch.bal_marginals(2) == (0, 0, 0)
        s, z = ch.bal_marginals_get()
        assert len(s) == 0 and len(z) == 0
        it, cv, var, sc = ch.bal_iterate(np.zeros(0, bool))
        assert (it, cv) == (0, False) and np.isnan(var) and np.isnan(sc)
        assert len(ch.bal_weights()) == 0 and len(ch.bal_cells_get()) == 0
        with pytest.raises(_lib.CloopsHipError):
            ch.bal_weights(0, 1)
        assert ch.bal_free() is None
        ch.close()


@pytest.mark.parametrize("n_cells", [TILE, TILE + 1, 2 * TILE, 2 * TILE + 1])
def test_cell_counts_at_the_tile(n_cells):
    X, Y = BC.with_cell_count(n_cells)
    ch = chrom(X, Y)
    for ign in (0, 2):
        cells, want = check_marginals(ch, X, Y, 1000, ign)
        assert len(cells[0]) == n_cells
    check_weights(ch, cells, 2, np.ones(want[1], bool), 1, 0.0, BC.one_step_bound(cells[0], cells[1], 2))
    ch.close()


def test_an_interior_stretch_of_empty_bins():
    X, Y = BC.gapped()
    ch = chrom(X, Y)
    cells, want = check_marginals(ch, X, Y, 1000, 2)
    assert not want[3][85:135].any() and want[3][:80].all() and want[3][140:200].all()
    valid = BC.valid_oracle(want[3], want[4])
    o, _ = check_weights(ch, cells, 2, valid, 200, 1e-5, BC.one_step_bound(cells[0], cells[1], 2))
    assert o["converged"] and np.isnan(ch.bal_weights()[85:135]).all()
    ch.close()


# ---- tile edges: runs of more than two tiles in both orders -----------------------------------------------------------
def test_arrow_runs_across_tiles():
    X, Y = BC.arrow()
    ch = chrom(X, Y)
    cells, want = check_marginals(ch, X, Y, 100, 0)
    row, col = int((cells[0] == cells[0][0]).sum()), int((cells[1] == cells[1].max()).sum())
    assert row > 2 * TILE and col > 2 * TILE and len(cells[0]) > 40000, (row, col, len(cells[0]))
    check_marginals(ch, X, Y, 100, 2)
    cells, want = check_marginals(ch, X, Y, 100, 0)
    valid = np.ones(want[1], bool)
    one = BC.one_step_bound(cells[0], cells[1], 0)
    check_weights(ch, cells, 0, valid, 1, 0.0, one)
    # a FIXED 40 iterations (the case needs far more than 500 to reach 1e-5): the bound is the oracle's own spread between two orders of
    # its cells, times 100, and never below the one-step bound
    a = BC.ice_oracle(*cells, 0, valid, 40, 0.0)
    b = BC.ice_oracle(*cells, 0, valid, 40, 0.0, perm=BC.cell_perm(len(cells[0]), 7))
    spread = BC.rel_diff(a["weight"], b["weight"])
    o, _ = check_weights(ch, cells, 0, valid, 40, 0.0, max(100 * spread, one))
    assert (o["iters"], o["converged"]) == (40, False)
    ch.close()


# ---- one step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ign,cut", [(0, 0), (2, 0), (2, 5000)])
def test_one_step(ign, cut):
    """max_iters = 1, tol = 0: every s is a sum of at most L positive terms (L: the longest row of the full matrix), so two orders of
    summation differ by at most (L - 1) 2^-53 relative in s, the mean over nb of them by as much again plus nb 2^-53, and the division
    and the root add a few roundings: 4 (L + nb) 2^-53 covers the weights"""
    X, Y = MC.scattered(*SCAT, both=True)
    ch = chrom(X, Y)
    cells, want = check_marginals(ch, X, Y, 1000, ign, cut)
    L = BC.longest_row(cells[0], cells[1], ign)
    bound = 4.0 * (L + want[1]) * 2.0 ** -53
    assert bound == BC.one_step_bound(cells[0], cells[1], ign) and 0 < L <= want[1]
    for valid in (np.ones(want[1], bool), BC.valid_oracle(want[3], want[4])):
        o, _ = check_weights(ch, cells, ign, valid, 1, 0.0, bound)
        assert (o["iters"], o["converged"]) == (1, False)
    ch.close()


# ---- converged runs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [1e-5, 1e-10])
@pytest.mark.parametrize("ign,cut", [(0, 0), (2, 0), (2, 5000)])
def test_converged_runs(ign, cut, tol):
    X, Y = MC.scattered(*SCAT, both=True)
    ch = chrom(X, Y)
    cells, want = check_marginals(ch, X, Y, 1000, ign, cut)
    valid = BC.valid_oracle(want[3], want[4])
    a = BC.ice_oracle(*cells, ign, valid, 200, tol)
    b = BC.ice_oracle(*cells, ign, valid, 200, tol, perm=BC.cell_perm(len(cells[0]), 1))
    # the input is far from a tie at the threshold: the last variance lies well below tol and the one before it well above
    before = BC.ice_oracle(*cells, ign, valid, a["iters"] - 1, tol)
    # (the GPU's variance lies within 4 rtol / sqrt(var), some 1e-7, of the oracle's: a margin of a thousandth on either side is ample)
    assert a["converged"] and b["iters"] == a["iters"] and 0.5 < a["var"] / tol < 0.96 and before["var"] / tol > 1.001, (a["var"], before["var"])
    spread = BC.rel_diff(a["weight"], b["weight"])
    assert spread < 1e-14                                                    # (the oracle's own sensitivity to the order: a few ulps)
    rtol = max(100 * spread, BC.one_step_bound(cells[0], cells[1], ign))
    o, dev = check_weights(ch, cells, ign, valid, 200, tol, rtol)
    assert o["converged"] and o["iters"] == a["iters"]
    ch.close()


def test_no_convergence_on_the_twelve_rows():
    """ignore_diags = 2 leaves the bipartite cells (0,4) (1,3) (1,4) (2,4): the iteration oscillates and the variance stays at 0.0727"""
    X, Y = MC.twelve()
    ch = chrom(X, Y)
    cells, want = check_marginals(ch, X, Y, 100, 2)
    # (the weights: nothing contracts here, so the roundings of 50 steps may add up: 50 one-step bounds)
    o, _ = check_weights(ch, cells, 2, np.ones(5, bool), 50, 1e-5, 50 * BC.one_step_bound(cells[0], cells[1], 2))
    assert (o["iters"], o["converged"]) == (50, False) and abs(o["var"] - 0.0726643) < 1e-6
    it, cv, var, _ = ch.bal_iterate(np.ones(5, bool), max_iters=50, tol=1e-5)
    assert (it, cv) == (50, False) and abs(var - o["var"]) <= BC.one_step_bound(cells[0], cells[1], 2) * o["var"]
    for k in (0, 1, 15, 16, 17, 33):                                         # the count across the blocks of enqueued iterations
        assert ch.bal_iterate(np.ones(5, bool), max_iters=k, tol=0)[0] == k
    ch.close()


# ---- determinism ----------------------------------------------------------------------------------------------------------
def test_the_same_bytes_twice():
    X, Y = BC.arrow()
    ch = chrom(X, Y)
    cells, want = check_marginals(ch, X, Y, 100, 1)
    valid = BC.valid_oracle(want[3], want[4], 5, 0, 5)
    r1 = ch.bal_iterate(valid, max_iters=25, tol=1e-7)
    w1, c1 = ch.bal_weights(), ch.bal_cells_get()
    r2 = ch.bal_iterate(valid, max_iters=25, tol=1e-7)
    assert r1[:2] == r2[:2] and np.array([r1[2:]]).tobytes() == np.array([r2[2:]]).tobytes()
    assert ch.bal_weights().tobytes() == w1.tobytes() and ch.bal_cells_get().tobytes() == c1.tobytes()
    # other cells in between, then the same again; and a fresh handle
    ch.mat_cells(1000, fold=True)
    ch.bal_marginals(0)
    ch.bal_iterate(np.ones(ch.bal_marginals(0)[1], bool), max_iters=3)
    check_marginals(ch, X, Y, 100, 1)
    r3 = ch.bal_iterate(valid, max_iters=25, tol=1e-7)
    assert r3[:2] == r1[:2] and ch.bal_weights().tobytes() == w1.tobytes()
    ch.close()
    ch = chrom(X, Y)
    check_marginals(ch, X, Y, 100, 1)
    r4 = ch.bal_iterate(valid, max_iters=25, tol=1e-7)
    assert r4[:2] == r1[:2] and np.array([r4[2:]]).tobytes() == np.array([r1[2:]]).tobytes()
    assert ch.bal_weights().tobytes() == w1.tobytes() and ch.bal_cells_get().tobytes() == c1.tobytes()
    ch.close()


# ---- masks and balanced values ---------------------------------------------------------------------------------------------
def test_masks_and_balanced_values():
    X, Y = MC.scattered(*SCAT, both=True)
    ch = chrom(X, Y)
    cells, want = check_marginals(ch, X, Y, 1000, 1)
    b0, nb = want[0], want[1]
    bound = BC.one_step_bound(cells[0], cells[1], 1)
    valid = BC.valid_oracle(want[3], want[4])
    valid[40:60] = False
    valid[100] = False
    o, _ = check_weights(ch, cells, 1, valid, 200, 1e-6, bound)
    w = ch.bal_weights()
    assert np.isnan(w[~valid]).all() and not np.isnan(w[valid]).any() and o["converged"]
    # the masked bins' cells do not enter the other bins' sums: the same weights as without those cells
    keep = valid[cells[0] - b0] & valid[cells[1] - b0]
    kept = tuple(a[keep] for a in cells)
    kb0, knb = BC.span(kept[0], kept[1])
    off = kb0 - b0
    q = BC.ice_oracle(*kept, 1, valid[off:off + knb], 200, 1e-6)
    assert BC.rel_diff(w[off:off + knb], q["weight"]) <= bound and q["iters"] == o["iters"]
    assert np.isnan(w[:off]).all() and np.isnan(w[off + knb:]).all()
    # balanced = (cnt weight[bx]) weight[by] from the GPU's own weights, exactly, for EVERY cell (also those nearer than ignore_diags)
    bal = ch.bal_cells_get()
    mine = BC.balanced_oracle(*cells, b0, w)
    assert bal.dtype == np.float64 and bal.tobytes() == mine.tobytes()
    diag = cells[0] == cells[1]
    assert diag.any() and not np.isnan(bal[diag & keep]).any() and np.isnan(bal[~keep]).all()
    # pieces of the arrays
    n = len(cells[0])
    assert np.array_equal(ch.bal_cells_get(n - 77, 77), bal[n - 77:], equal_nan=True) and np.array_equal(ch.bal_cells_get(5, 1), bal[5:6], equal_nan=True)
    assert np.array_equal(ch.bal_weights(nb - 9, 9), w[nb - 9:], equal_nan=True) and len(ch.bal_weights(nb, 0)) == 0
    s, z = ch.bal_marginals_get(17, 30)
    assert np.array_equal(s, want[3][17:47]) and np.array_equal(z, want[4][17:47])
    # the balanced rows sum to 1 on the valid bins (within the stop criterion)
    full = np.zeros(nb)
    u = BC.used_cells(cells[0], cells[1], 1) & keep
    np.add.at(full, cells[0][u] - b0, bal[u])
    offd = u & ~diag
    np.add.at(full, cells[1][offd] - b0, bal[offd])
    live = valid & (full > 0)
    assert live.sum() > 100 and np.abs(full[live] - 1).max() < np.sqrt(nb * 1e-6)
    # another mask and tol on the same marginals
    check_weights(ch, cells, 1, np.ones(nb, bool), 30, 1e-3, bound)
    ch.close()


# ---- lifetimes and refusals --------------------------------------------------------------------------------------------------
def test_lifetimes():
    from cloops_amd import _lib
    X, Y = MC.scattered(5, 3000, 50000, 9000)
    ch = chrom(X, Y)
    E = _lib.CloopsHipError
    for f in (lambda: ch.bal_marginals(2), lambda: ch.bal_marginals_get(0, 0), lambda: ch.bal_free() or ch.bal_weights(0, 0)):
        with pytest.raises(E):
            f()                                                              # no cells yet
    ch.mat_cells(500, fold=False)
    with pytest.raises(E):
        ch.bal_marginals(2)                                                  # not folded
    cells, want = check_marginals(ch, X, Y, 500, 2)
    nb = want[1]
    with pytest.raises(E):
        ch.bal_weights()                                                     # no iteration yet
    with pytest.raises(E):
        ch.bal_cells_get()
    for bad in (np.ones(nb - 1, bool), np.ones(nb + 1, bool), np.ones((nb, 1), bool)):
        with pytest.raises(ValueError):
            ch.bal_iterate(bad)
    valid = BC.valid_oracle(want[3], want[4])
    bound = BC.one_step_bound(cells[0], cells[1], 2)
    # agg_loops at another cut rebuilds the shared table between the two calls: the cells and their transposed order are copies
    ch.agg_loops([20000], [25000], 1000, 10, 3, cut=4000)
    o, _ = check_weights(ch, cells, 2, valid, 200, 1e-6, bound)
    w = ch.bal_weights()
    for f in (lambda: ch.bal_weights(-1, 1), lambda: ch.bal_weights(nb, 1), lambda: ch.bal_weights(0, nb + 1), lambda: ch.bal_cells_get(len(cells[0]), 1),
              lambda: ch.bal_cells_get(-1, 1), lambda: ch.bal_marginals_get(nb - 1, 2), lambda: ch.bal_marginals(-1),
              lambda: ch.bal_iterate(valid, max_iters=-1), lambda: ch.bal_iterate(valid, tol=-1e-9), lambda: ch.bal_iterate(valid, tol=float("nan"))):
        with pytest.raises(E):
            f()
    assert np.array_equal(ch.bal_weights(), w, equal_nan=True)               # a refused call leaves the weights
    # bal_free drops the state and keeps the cells
    ch.bal_free()
    assert len(ch.mat_cells_get()[0]) == len(cells[0])
    for f in (lambda: ch.bal_marginals_get(0, 0), lambda: ch.bal_iterate(np.zeros(0, bool)), lambda: ch.bal_weights(0, 0)):
        with pytest.raises((E, ValueError)):
            f()
    check_marginals(ch, X, Y, 500, 2)
    check_weights(ch, cells, 2, valid, 200, 1e-6, bound)
    # mat_cells and mat_free drop it too
    ch.mat_cells(500, fold=True)
    with pytest.raises((E, ValueError)):
        ch.bal_iterate(valid)
    with pytest.raises(E):
        ch.bal_weights(0, 0)
    ch.bal_marginals(2)
    ch.mat_free()
    with pytest.raises(E):
        ch.bal_marginals_get(0, 0)
    with pytest.raises(E):
        ch.bal_marginals(2)
    ch.close()


def test_argument_errors_of_the_c_calls():
    from cloops_amd import api, _lib
    lib = _lib.load()
    assert lib.cl_version() == 105 and _lib.CL_BAL_BINS_MAX == 1 << 24
    E = _lib.CL_ERR_ARG
    X, Y = MC.scattered(5, 1000, 50000, 9000)
    ch = api.Chromosome(X, Y)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ref = ctypes.byref
    a, b, c = ctypes.c_int64(7), ctypes.c_int64(7), ctypes.c_int64(7)
    it, cv, var, sc = ctypes.c_int32(7), ctypes.c_int32(7), ctypes.c_double(7), ctypes.c_double(7)
    marg, mget, iterate, wget, cget = lib.cl_bal_marginals, lib.cl_bal_marginals_get, lib.cl_bal_iterate, lib.cl_bal_weights_get, lib.cl_bal_cells_get
    assert marg(None, 2, ref(a), ref(b), ref(c)) == E and lib.cl_bal_free(None) == E
    assert marg(ch._h, 2, ref(a), ref(b), ref(c)) == E and (a.value, b.value, c.value) == (0, 0, 0) and b"cl_bal_marginals" in lib.cl_last_error()
    nc = ch.mat_cells(500, fold=True)[0]
    assert marg(ch._h, 2, None, ref(b), ref(c)) == E and marg(ch._h, 2, ref(a), None, ref(c)) == E and marg(ch._h, 2, ref(a), ref(b), None) == E
    assert marg(ch._h, -1, ref(a), ref(b), ref(c)) == E
    s8, z4, d8 = np.zeros(4, np.uint64), np.zeros(4, np.uint32), np.zeros(4, np.float64)
    assert mget(ch._h, 0, 1, vp(s8), vp(z4)) == E                            # before cl_bal_marginals
    assert marg(ch._h, 2, ref(a), ref(b), ref(c)) == 0
    nb = b.value
    valid = np.ones(nb, np.uint32)
    assert mget(None, 0, 1, vp(s8), vp(z4)) == E and mget(ch._h, 0, 1, None, vp(z4)) == E and mget(ch._h, 0, 1, vp(s8), None) == E
    assert mget(ch._h, -1, 1, vp(s8), vp(z4)) == E and mget(ch._h, nb - 1, 2, vp(s8), vp(z4)) == E and mget(ch._h, nb + 1, 0, vp(s8), vp(z4)) == E
    assert mget(ch._h, nb, 0, None, None) == 0
    out = (ref(it), ref(cv), ref(var), ref(sc))
    assert wget(ch._h, 0, 1, vp(d8)) == E and cget(ch._h, 0, 1, vp(d8)) == E           # before cl_bal_iterate
    assert iterate(None, vp(valid), 5, 1e-5, *out) == E and iterate(ch._h, None, 5, 1e-5, *out) == E
    for k in range(4):
        assert iterate(ch._h, vp(valid), 5, 1e-5, *[None if j == k else o for j, o in enumerate(out)]) == E
    for mi, tol in ((-1, 1e-5), (5, -1e-5), (5, float("nan"))):
        it.value = cv.value = 7
        assert iterate(ch._h, vp(valid), mi, tol, *out) == E and (it.value, cv.value) == (0, 0) and np.isnan(var.value) and np.isnan(sc.value)
        assert b"cl_bal_iterate" in lib.cl_last_error()
    assert iterate(ch._h, vp(valid), 5, 0.0, *out) == 0 and (it.value, cv.value) == (5, 0)
    assert iterate(ch._h, vp(valid), 5, float("inf"), *out) == 0 and (it.value, cv.value) == (1, 1)
    assert wget(None, 0, 1, vp(d8)) == E and wget(ch._h, 0, 1, None) == E and wget(ch._h, nb - 3, 4, vp(d8)) == E and wget(ch._h, nb - 4, 4, vp(d8)) == 0
    assert cget(None, 0, 1, vp(d8)) == E and cget(ch._h, 0, 1, None) == E and cget(ch._h, nc - 3, 4, vp(d8)) == E and cget(ch._h, nc - 4, 4, vp(d8)) == 0
    assert wget(ch._h, nb, 0, None) == 0 and cget(ch._h, nc, 0, None) == 0
    # runs in flight
    w = ch.bal_weights()
    ch.cluster_async("v2", 2000, 5)
    assert marg(ch._h, 2, ref(a), ref(b), ref(c)) == E and mget(ch._h, 0, 1, vp(s8), vp(z4)) == E and iterate(ch._h, vp(valid), 5, 1e-5, *out) == E
    assert wget(ch._h, 0, 1, vp(d8)) == E and cget(ch._h, 0, 1, vp(d8)) == E and lib.cl_bal_free(ch._h) == E
    ch.wait()
    assert np.array_equal(ch.bal_weights(), w, equal_nan=True)               # the handle still works
    ch.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _write_jd(d, name, X, Y):
    import joblib
    os.makedirs(d, exist_ok=True)
    joblib.dump(np.stack([np.arange(len(X)), X, Y], 1).astype(np.int64), os.path.join(d, "%s-%s.jd" % (name, name)))


def _files(prefix, suffixes):
    out = {}
    for suffix in suffixes:
        with open(prefix + suffix) as fh:
            out[suffix] = fh.read()
    return out


def test_the_command_end_to_end(tmp_path):
    """balance.main on a directory of two chromosomes and a trans file (left out): the four files are EQUAL to those the host
    functions make of the oracle's stand-in -- the ten digits of the texts hide the last few ulps between the two"""
    import joblib
    from cloops_amd import balance, matrix, pipe
    data = {"chr2": MC.scattered(0, 3000, 150000, 40000, both=True), "chr10": MC.scattered(1, 2500, 120000, 30000, both=True)}
    d = os.path.join(str(tmp_path), "jd")
    for name, (X, Y) in data.items():
        _write_jd(d, name, X, Y)
    joblib.dump(np.zeros((3, 3), np.int64), os.path.join(d, "chr2-chr10.jd"))            # a trans file is left out
    out = os.path.join(str(tmp_path), "o")
    pipe.CACHE.clear()
    assert matrix.main(["cells", "-d", d, "-o", out, "-res", "2000"]) == 0
    cells_before = _files(out, ["_cells.txt"])
    args = dict(res=2000, cut=0, ignore_diags=2, min_nnz=10, min_count=0, mad_max=5.0, tol=1e-5, max_iters=200)
    assert balance.main(["-d", d, "-o", out, "-res", "2000", "-r", "chr10:20000-90000"]) == 0
    rg = ("chr10", 20000, 90000)
    per = {n: balance.balance_chrom(BC.OracleChrom(*data[n]), n, 2000, region=rg if n == "chr10" else None) for n in data}
    want, js = balance.balance_outputs(per, dict(args, region="chr10:20000-90000"))
    got = _files(out, balance.SUFFIXES)
    assert json.loads(got["_balance.json"]) == js and all(js["chroms"][n]["converged"] and js["chroms"][n]["n_valid"] > 30 for n in data)
    assert got == want
    assert list(js["chroms"]) == ["chr10", "chr2"] and got["_balance.txt"].startswith("chr10\t")
    assert matrix.main(["cells", "-d", d, "-o", out, "-res", "2000"]) == 0
    assert _files(out, ["_cells.txt"]) == cells_before                       # K24's file is what it was
    # refused before any file is written
    bad = os.path.join(str(tmp_path), "bad")
    for f in (lambda: balance.jd2balance(d, bad, region="chr7:0-1000"), lambda: balance.jd2balance(d, bad, tol=-1.0),
              lambda: balance.jd2balance(d, bad, chroms={"chr2"}, region="chr10:0-1000")):
        with pytest.raises(ValueError):
            f()
    pipe.CACHE.clear()
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("bad")]
