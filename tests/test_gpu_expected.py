"""GPU: K26 (cl_exp_diagonals / cl_exp_diagonals_get / cl_exp_set / cl_exp_cells_get, cloops_amd.expected) against the numpy oracle of
tests/expected_cases.py -- the valid pairs per diagonal and the integer sums exactly, the balanced sums and O/E within bounds that come
from the number of roundings, the edges of the pair kernel's words, diagonal blocks and LDS window and of the sums' tiles, the same
bytes twice, lifetimes, refusals, and the command end to end."""
import ctypes
import json
import os

import numpy as np
import pytest

import balance_cases as BC
import expected_cases as EC
import matrix_cases as MC

pytestmark = pytest.mark.gpu

TILE = EC.TILE                 # cl_segsum.h K25_TILE: cells per workgroup of the sums per diagonal
DIAG_BLOCK = EC.DIAG_BLOCK     # k_expected.hip K26_DB: diagonals per workgroup of k26_pairs
WINDOW = EC.WINDOW             # k_expected.hip K26_WIN: mask words (of 64 bins) per LDS window of k26_pairs
SCAT = (3, 40000, 200000, 30000)
EPS = EC.EPS


def chrom(X, Y):
    from cloops_amd import api
    return api.Chromosome(np.asarray(X, np.int64), np.asarray(Y, np.int64))


def prepare(ch, X, Y, res, ign, cut=0):
    """mat_cells + bal_marginals -> the oracle's cells, (b0, nb)"""
    cells = MC.cells_oracle(X, Y, cut, res, True)[:3]
    assert ch.mat_cells(res, cut=cut, fold=True)[0] == len(cells[0])
    b0, nb = BC.span(cells[0], cells[1])
    assert ch.bal_marginals(ign)[:2] == (b0, nb)
    return cells, b0, nb


def check_raw(ch, cells, b0, nb, ign, valid):
    """exp_diagonals in raw mode against the oracle: the three arrays and n_used exactly, val_sum == cnt_sum -> the oracle's result"""
    v = np.ones(nb, bool) if valid is None else np.asarray(valid, bool)
    want = EC.diagonals_oracle(*cells, b0, nb, ign, v, np.ones(nb))
    assert ch.exp_diagonals(valid=valid, balanced=False) == (nb, want[3]), (nb, ign, want[3])
    p, c, s = ch.exp_diagonals_get()
    assert (p.dtype, c.dtype, s.dtype, len(p), len(c), len(s)) == (np.int64, np.uint64, np.float64, nb, nb, nb)
    bad = np.flatnonzero((p != want[0]) | (c != want[1]))
    assert len(bad) == 0, (nb, ign, len(bad), bad[:5], p[bad[:5]], want[0][bad[:5]], c[bad[:5]], want[1][bad[:5]])
    assert s.tobytes() == c.astype(np.float64).tobytes()                     # raw: the value sum IS the count sum
    return want


# ---- 1. the valid pairs per diagonal, exactly ------------------------------------------------------------------------------
def masks_of(nb, seeds=(1, 2)):
    """name -> (mask or None, closed form or None)"""
    d = np.arange(nb)
    out = {"all": (None, nb - d), "all_given": (np.ones(nb, bool), nb - d), "none": (np.zeros(nb, bool), np.zeros(nb, np.int64))}
    for k in sorted({0, 63, 64, nb - 1}):
        if 0 <= k < nb:
            m = np.ones(nb, bool)
            m[k] = False
            closed = (nb - d) - (k + d < nb) - (k - d >= 0)                  # the pairs (k, k + d) and (k - d, k) go
            closed[0] = nb - 1
            out["without_%d" % k] = (m, closed)
    out["alternating"] = (d % 2 == 0, None)
    for s in seeds:
        out["random_%d" % s] = (np.random.default_rng(s).random(nb) < 0.6, None)
    return out


@pytest.mark.parametrize("nb", [1, 2, 63, 64, 65, 127, 128, 129, DIAG_BLOCK + 1, 4097])
def test_pair_counts(nb):
    X, Y = EC.spanning(nb)
    ch = chrom(X, Y)
    for ign in (0, 2, nb + 3):
        cells, b0, got_nb = prepare(ch, X, Y, 1, ign)
        assert (b0, got_nb) == (0, nb)
        for name, (mask, closed) in masks_of(nb).items():
            want = check_raw(ch, cells, 0, nb, ign, mask)
            if closed is not None:
                c = np.asarray(closed, np.int64).copy()
                c[:min(ign, nb)] = 0
                assert np.array_equal(want[0], c), (name, nb, ign)           # (the oracle against the closed form)
    ch.close()


def test_pair_counts_beyond_one_window():
    """one bin more than an LDS window of the pair kernel holds: the mask's words come in two windows, and the last word has one bit"""
    nb = 64 * WINDOW + 1
    X, Y = EC.spanning(nb)
    ch = chrom(X, Y)
    d = np.arange(nb)
    sparse = np.zeros(nb, bool)
    sparse[np.random.default_rng(5).choice(nb, 400, replace=False)] = True
    sparse[[0, nb - 1, 64 * WINDOW - 1]] = True
    idx = np.flatnonzero(sparse)
    by_differences = np.bincount((idx[None, :] - idx[:, None])[np.triu_indices(len(idx))], minlength=nb)     # every pair i <= j once
    dense = np.random.default_rng(6).random(nb) < 0.5
    for ign in (0, 2):
        cells, b0, got_nb = prepare(ch, X, Y, 1, ign)
        assert (b0, got_nb) == (0, nb)
        for mask, want in ((None, nb - d), (sparse, by_differences)):
            assert ch.exp_diagonals(valid=mask, balanced=False)[0] == nb
            w = np.asarray(want, np.int64).copy()
            w[:ign] = 0
            p = ch.exp_diagonals_get()[0]
            bad = np.flatnonzero(p != w)
            assert len(bad) == 0, (ign, len(bad), bad[:5], p[bad[:5]], w[bad[:5]])
    check_raw(ch, cells, 0, nb, 2, dense)                                    # (np.correlate over 32 769 bins: once)
    ch.close()


# ---- 2. the sums per diagonal, exact integers ------------------------------------------------------------------------------
def test_sums_of_the_twelve_rows():
    X, Y = MC.twelve()
    ch = chrom(X, Y)
    cells, b0, nb = prepare(ch, X, Y, 100, 0)
    w = check_raw(ch, cells, b0, nb, 0, None)
    assert (w[0].tolist(), w[1].tolist(), w[3]) == ([5, 4, 3, 2, 1], [4, 2, 3, 1, 2], 10)
    w = check_raw(ch, cells, b0, nb, 0, [True, True, False, True, True])
    assert (w[0].tolist(), w[1].tolist(), w[3]) == ([4, 2, 1, 2, 1], [3, 2, 2, 1, 2], 8)
    cells, b0, nb = prepare(ch, X, Y, 100, 2)
    w = check_raw(ch, cells, b0, nb, 2, None)
    assert (w[0].tolist(), w[1].tolist(), w[3]) == ([0, 0, 3, 2, 1], [0, 0, 3, 1, 2], 4)
    cells, b0, nb = prepare(ch, X, Y, 7, 3)
    check_raw(ch, cells, b0, nb, 3, None)
    ch.close()


@pytest.mark.parametrize("ign,cut", [(0, 0), (2, 0), (2, 5000), (0, 12000), (300, 0)])
def test_sums_of_scattered_rows(ign, cut):
    X, Y = MC.scattered(*SCAT, both=True)
    ch = chrom(X, Y)
    cells, b0, nb = prepare(ch, X, Y, 1000, ign, cut)
    want = check_raw(ch, cells, b0, nb, ign, None)
    if ign == 300:
        assert want[3] == 0 and not want[1].any() and not want[0].any()
    else:
        assert want[3] > 1000
    mask = np.random.default_rng(4).random(nb) < 0.8
    check_raw(ch, cells, b0, nb, ign, mask)
    check_raw(ch, cells, b0, nb, ign, np.zeros(nb, bool))
    ch.close()


def test_sums_with_a_gap_and_negative_bins():
    X, Y = BC.gapped()
    ch = chrom(X, Y)
    cells, b0, nb = prepare(ch, X, Y, 1000, 2)
    s, z = ch.bal_marginals_get()
    check_raw(ch, cells, b0, nb, 2, BC.valid_oracle(s, z))
    ch.close()
    X, Y = MC.scattered(4, 5000, 60000, 9000, both=True)
    X, Y = X - 30000, Y - 30000
    ch = chrom(X, Y)
    for res, ign in ((1000, 0), (1000, 2), (7, 1), (333, 3)):
        cells, b0, nb = prepare(ch, X, Y, res, ign)
        assert b0 < 0 < b0 + nb
        check_raw(ch, cells, b0, nb, ign, None)
    ch.close()


@pytest.mark.parametrize("n_cells", [TILE, TILE + 1, 2 * TILE + 1])
def test_one_diagonal_over_whole_tiles(n_cells):
    X, Y = EC.one_diagonal(n_cells)
    ch = chrom(X, Y)
    cells, b0, nb = prepare(ch, X, Y, 1, 2)
    assert len(cells[0]) == n_cells and nb == n_cells + 3
    want = check_raw(ch, cells, b0, nb, 2, None)
    assert want[3] == n_cells and np.flatnonzero(want[1]).tolist() == [3] and int(want[1][3]) == len(X)
    mask = np.ones(nb, bool)
    mask[[0, TILE - 1, nb - 1]] = False
    check_raw(ch, cells, b0, nb, 2, mask)
    ch.close()


def test_every_cell_on_its_own_diagonal():
    X, Y = EC.own_diagonals(TILE + 900)
    ch = chrom(X, Y)
    cells, b0, nb = prepare(ch, X, Y, 1, 0)
    want = check_raw(ch, cells, b0, nb, 0, None)
    assert len(cells[0]) == TILE + 900 and want[1][:TILE + 900].tolist() == [1] * (TILE + 900)
    ch.close()


@pytest.mark.parametrize("n_cells", [TILE, TILE + 1])
def test_cell_counts_at_the_tile(n_cells):
    X, Y = BC.with_cell_count(n_cells)
    ch = chrom(X, Y)
    for ign in (0, 2):
        cells, b0, nb = prepare(ch, X, Y, 1000, ign)
        assert len(cells[0]) == n_cells
        check_raw(ch, cells, b0, nb, ign, None)
    ch.close()


# ---- 3. the balanced sums and O/E within derived bounds -----------------------------------------------------------------------
def balanced(ch, X, Y, res, ign, cut=0, tol=1e-5):
    """cells, marginals, the oracle's mask, bal_iterate -> cells, b0, nb, the DEVICE's weights"""
    cells, b0, nb = prepare(ch, X, Y, res, ign, cut)
    s, z = ch.bal_marginals_get()
    it, cv, _, _ = ch.bal_iterate(BC.valid_oracle(s, z), max_iters=200, tol=tol)
    assert cv and it > 0
    return cells, b0, nb, ch.bal_weights()


@pytest.mark.parametrize("ign,cut", [(0, 0), (2, 0), (2, 5000)])
def test_balanced_sums_and_oe(ign, cut):
    """val_sum against the oracle fed the device's own weights (K25's deviation does not enter): every term carries two roundings and a
    diagonal of L positive terms adds at most L - 1 more, so two orders of summation differ by at most (L + 2) 2^-53 relative.  O/E: one
    more division on the term: (3 + 1) 2^-53 relative against the oracle fed the same expected values."""
    X, Y = MC.scattered(*SCAT, both=True)
    ch = chrom(X, Y)
    cells, b0, nb, w = balanced(ch, X, Y, 1000, ign, cut)
    valid = ~np.isnan(w)
    assert 100 < valid.sum() <= nb
    want = EC.diagonals_oracle(*cells, b0, nb, ign, valid, w)
    assert ch.exp_diagonals() == (nb, want[3])
    p, c, s = ch.exp_diagonals_get()
    assert np.array_equal(p, want[0]) and np.array_equal(c, want[1])
    bound, L = EC.sum_bound(cells[0], cells[1], b0, nb, ign, valid)
    assert L.max() > 100 and np.array_equal(L == 0, want[2] == 0) and not s[L == 0].any()
    live = L > 0
    ratio = np.abs(s[live] - want[2][live]) / want[2][live] / bound[live]
    again = EC.diagonals_oracle(*cells, b0, nb, ign, valid, w, perm=BC.cell_perm(len(cells[0]), 2))
    own = np.abs(again[2][live] - want[2][live]) / want[2][live] / bound[live]
    print("K26 val_sum: diagonals %d longest %d, largest deviation over its bound: device %.3g, the oracle under another order %.3g" %
          (live.sum(), L.max(), ratio.max(), own.max()))
    assert own.max() <= 1.0 and np.array_equal(again[1], want[1])            # the bound holds on the CPU
    assert ratio.max() <= 1.0
    # O/E: the average per diagonal as the expected value, with a zero, a NaN and an infinity planted
    e = np.full(nb, np.nan)
    e[p > 0] = s[p > 0] / p[p > 0]
    used_d = np.flatnonzero(live)
    e[used_d[1]], e[used_d[2]], e[used_d[3]] = 0.0, np.nan, np.inf
    ch.exp_set(e)
    oe = ch.exp_cells_get()
    mine = EC.oe_oracle(*cells, b0, nb, ign, valid, w, e)
    assert oe.dtype == np.float64 and len(oe) == len(cells[0]) and np.array_equal(np.isnan(oe), np.isnan(mine))
    d = cells[1].astype(np.int64) - cells[0]
    u = EC.used_of(cells[0], cells[1], b0, ign, valid)
    assert np.isnan(oe[~u]).all() and np.isnan(oe[u & ((d == used_d[1]) | (d == used_d[2]))]).all()
    assert not np.isnan(oe[u & (d == used_d[3])]).any() and not oe[u & (d == used_d[3])].any()          # x / inf = 0
    ok = ~np.isnan(mine) & (mine != 0)
    dev = np.abs(oe[ok] - mine[ok]) / mine[ok]
    print("K26 O/E: cells %d with a value %d, largest relative deviation %.3g allowed %.3g" % (len(oe), ok.sum(), dev.max(), 4 * EPS))
    assert ok.sum() > 1000 and dev.max() <= 4 * EPS
    assert np.isnan(oe[d < ign]).all() and (d < ign).any() == (ign > 0 and cut == 0)     # (a cut of 5000 leaves no cell that near)
    # pieces of the arrays, another exp_set on the same diagonals
    n = len(oe)
    assert np.array_equal(ch.exp_cells_get(n - 77, 77), oe[n - 77:], equal_nan=True) and np.array_equal(ch.exp_cells_get(5, 1), oe[5:6], equal_nan=True)
    p2, c2, s2 = ch.exp_diagonals_get(17, 30)
    assert np.array_equal(p2, p[17:47]) and np.array_equal(c2, c[17:47]) and s2.tobytes() == s[17:47].tobytes()
    ch.exp_set(np.ones(nb))
    assert ch.exp_cells_get().tobytes() == np.where(u, ch.bal_cells_get(), np.nan).tobytes()             # O/E over 1 is the balanced value
    ch.close()


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------
def test_the_same_bytes_twice():
    X, Y = BC.arrow()
    ch = chrom(X, Y)
    cells, b0, nb = prepare(ch, X, Y, 100, 1)
    s, z = ch.bal_marginals_get()
    ch.bal_iterate(BC.valid_oracle(s, z, 5, 0, 5), max_iters=25, tol=1e-7)

    def once():
        r = ch.exp_diagonals()
        p, c, v = ch.exp_diagonals_get()
        e = np.full(nb, np.nan)
        e[p > 0] = v[p > 0] / p[p > 0]
        ch.exp_set(e)
        return r, p.tobytes(), c.tobytes(), v.tobytes(), ch.exp_cells_get().tobytes()
    first = once()
    assert first[0][1] > 2 * TILE and np.frombuffer(first[2], np.uint64).max() > 0
    assert once() == first
    ch.exp_free()
    assert once() == first
    ch.close()


# ---- 5. lifetimes and refusals -------------------------------------------------------------------------------------------------
def test_lifetimes():
    from cloops_amd import _lib
    E = _lib.CloopsHipError
    X, Y = MC.scattered(5, 3000, 50000, 9000)
    ch = chrom(X, Y)

    def refused(*calls):
        for f in calls:
            with pytest.raises(E):
                f()
    getters = (lambda: ch.exp_diagonals_get(0, 0), lambda: ch.exp_set(np.zeros(0)), lambda: ch.exp_cells_get(0, 0))
    refused(lambda: ch.exp_diagonals(balanced=False), *getters)              # no cells, no marginals
    assert ch.exp_free() is None
    ch.mat_cells(500, fold=True)
    refused(lambda: ch.exp_diagonals(balanced=False), *getters)              # no marginals
    cells, b0, nb = prepare(ch, X, Y, 500, 2)
    refused(lambda: ch.exp_diagonals(), *getters)                            # balanced before bal_iterate; gets before exp_diagonals
    for bad in (np.ones(nb - 1, bool), np.ones(nb + 1, bool), np.ones((nb, 1), bool)):
        with pytest.raises(ValueError):
            ch.exp_diagonals(valid=bad, balanced=False)

    def build(raw=False):
        if raw:
            assert ch.exp_diagonals(balanced=False)[0] == nb
        else:
            s, z = ch.bal_marginals_get()
            ch.bal_iterate(BC.valid_oracle(s, z))
            assert ch.exp_diagonals()[0] == nb
        p, c, v = ch.exp_diagonals_get()
        refused(lambda: ch.exp_cells_get(0, 0))                              # before exp_set
        ch.exp_set(np.ones(nb))
        assert len(ch.exp_cells_get()) == len(cells[0])
        return p, c, v
    p, c, v = build(raw=True)
    refused(lambda: ch.exp_diagonals(valid=np.ones(nb, bool), balanced=True), lambda: ch.exp_diagonals(balanced=True))
    assert np.array_equal(ch.exp_diagonals_get()[0], p)                      # a refused call leaves the diagonals
    # the ends of the ranges, count 0, a wrong length
    n = len(cells[0])
    refused(lambda: ch.exp_diagonals_get(-1, 1), lambda: ch.exp_diagonals_get(nb, 1), lambda: ch.exp_diagonals_get(0, nb + 1),
            lambda: ch.exp_diagonals_get(nb + 1, 0), lambda: ch.exp_cells_get(n, 1), lambda: ch.exp_cells_get(-1, 1), lambda: ch.exp_cells_get(0, n + 1),
            lambda: ch.exp_set(np.ones(nb - 1)), lambda: ch.exp_set(np.ones(nb + 1)), lambda: ch.exp_set(np.ones(0)))
    assert len(ch.exp_diagonals_get(nb, 0)[0]) == 0 and len(ch.exp_cells_get(n, 0)) == 0
    assert np.array_equal(ch.exp_diagonals_get(nb - 1, 1)[0], p[nb - 1:]) and len(ch.exp_cells_get(n - 1, 1)) == 1
    assert len(ch.exp_cells_get()) == n                                      # a refused exp_set leaves the expected values
    # agg_loops at another cut rebuilds the shared table: the cells and the diagonal order are copies
    ch.agg_loops([20000], [25000], 1000, 10, 3, cut=4000)
    assert ch.exp_diagonals_get()[1].tobytes() == c.tobytes()
    # the next exp_diagonals drops the expected values; exp_free drops the state and keeps cells, marginals and weights
    build()
    ch.exp_diagonals()
    refused(lambda: ch.exp_cells_get(0, 0))
    ch.exp_set(np.ones(nb))
    ch.exp_free()
    refused(*getters)
    assert len(ch.bal_weights()) == nb and len(ch.mat_cells_get()[0]) == n
    # every call that drops or rebuilds K25's state drops K26's
    build()
    ch.bal_marginals(2)
    refused(*getters)
    build()
    s, z = ch.bal_marginals_get()
    ch.bal_iterate(BC.valid_oracle(s, z), max_iters=3)
    refused(*getters)
    build()
    ch.bal_free()
    refused(*getters)
    prepare(ch, X, Y, 500, 2)
    build()
    ch.mat_cells(500, fold=True)
    refused(*getters)
    prepare(ch, X, Y, 500, 2)
    build(raw=True)
    ch.mat_free()
    refused(lambda: ch.exp_diagonals(balanced=False), *getters)
    ch.close()


def test_no_bins_is_no_error():
    from cloops_amd import _lib
    for X, Y, cut in ((MC.EMPTY, MC.EMPTY, 0), ([500, 90], [700, 95], 1 << 20)):
        ch = chrom(X, Y)
        assert ch.mat_cells(1000, cut=cut, fold=True)[0] == 0 and ch.bal_marginals(2) == (0, 0, 0)
        assert ch.exp_diagonals(balanced=False) == (0, 0) and ch.exp_diagonals(valid=np.zeros(0, bool), balanced=False) == (0, 0)
        assert [len(a) for a in ch.exp_diagonals_get()] == [0, 0, 0]
        ch.exp_set(np.zeros(0))
        assert len(ch.exp_cells_get()) == 0
        ch.bal_iterate(np.zeros(0, bool))
        assert ch.exp_diagonals() == (0, 0)
        with pytest.raises(_lib.CloopsHipError):
            ch.exp_diagonals_get(0, 1)
        lib = _lib.load()
        assert lib.cl_exp_diagonals_get(ch._h, 0, 0, None, None, None) == 0 and lib.cl_exp_set(ch._h, None, 0) == 0
        assert lib.cl_exp_cells_get(ch._h, 0, 0, None) == 0
        assert ch.exp_free() is None
        ch.close()


def test_argument_errors_of_the_c_calls():
    from cloops_amd import api, _lib
    lib = _lib.load()
    E = _lib.CL_ERR_ARG
    X, Y = MC.scattered(5, 1000, 50000, 9000)
    ch = api.Chromosome(X, Y)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ref = ctypes.byref
    a, b, c = ctypes.c_int64(7), ctypes.c_int64(7), ctypes.c_int64(7)
    diag, dget, eset, cget, free = lib.cl_exp_diagonals, lib.cl_exp_diagonals_get, lib.cl_exp_set, lib.cl_exp_cells_get, lib.cl_exp_free
    p8, c8, d8 = np.zeros(4, np.int64), np.zeros(4, np.uint64), np.zeros(4, np.float64)
    assert diag(None, None, 0, ref(a), ref(b)) == E and dget(None, 0, 1, vp(p8), vp(c8), vp(d8)) == E and eset(None, vp(d8), 4) == E
    assert cget(None, 0, 1, vp(d8)) == E and free(None) == E
    # before cl_bal_marginals
    nc = ch.mat_cells(500, fold=True)[0]
    assert diag(ch._h, None, 0, ref(a), ref(b)) == E and (a.value, b.value) == (0, 0) and b"cl_exp_diagonals" in lib.cl_last_error()
    assert dget(ch._h, 0, 0, None, None, None) == E and eset(ch._h, None, 0) == E and cget(ch._h, 0, 0, None) == E and free(ch._h) == 0
    b0, nb, _ = ch.bal_marginals(2)
    valid = np.ones(nb, np.uint32)
    assert diag(ch._h, None, 0, None, ref(b)) == E and diag(ch._h, None, 0, ref(a), None) == E
    for bad in (2, -1, 256):
        a.value = b.value = 7
        assert diag(ch._h, None, bad, ref(a), ref(b)) == E and (a.value, b.value) == (0, 0)
    assert diag(ch._h, None, 1, ref(a), ref(b)) == E                        # balanced before cl_bal_iterate
    assert dget(ch._h, 0, 1, vp(p8), vp(c8), vp(d8)) == E and eset(ch._h, vp(np.ones(nb)), nb) == E and cget(ch._h, 0, 1, vp(d8)) == E   # before cl_exp_diagonals
    ch.bal_iterate(valid)
    assert diag(ch._h, vp(valid), 1, ref(a), ref(b)) == E                   # balanced with a mask
    assert diag(ch._h, vp(valid), 0, ref(a), ref(b)) == 0 and (a.value, b.value > 0) == (nb, True)
    assert diag(ch._h, None, 1, ref(a), ref(b)) == 0 and a.value == nb
    assert dget(ch._h, 0, 1, None, vp(c8), vp(d8)) == E and dget(ch._h, 0, 1, vp(p8), None, vp(d8)) == E and dget(ch._h, 0, 1, vp(p8), vp(c8), None) == E
    assert dget(ch._h, -1, 1, vp(p8), vp(c8), vp(d8)) == E and dget(ch._h, nb - 3, 4, vp(p8), vp(c8), vp(d8)) == E
    assert dget(ch._h, nb + 1, 0, vp(p8), vp(c8), vp(d8)) == E and dget(ch._h, nb - 4, 4, vp(p8), vp(c8), vp(d8)) == 0 and dget(ch._h, nb, 0, None, None, None) == 0
    assert cget(ch._h, 0, 1, vp(d8)) == E                                   # before cl_exp_set
    ones = np.ones(nb + 1)
    assert eset(ch._h, None, nb) == E and eset(ch._h, vp(ones), nb - 1) == E and eset(ch._h, vp(ones), nb + 1) == E and eset(ch._h, vp(ones), 0) == E
    assert cget(ch._h, 0, 1, vp(d8)) == E                                   # ... still: a refused cl_exp_set sets nothing
    assert eset(ch._h, vp(ones), nb) == 0 and eset(ch._h, vp(ones), nb) == 0
    assert cget(ch._h, 0, 1, None) == E and cget(ch._h, nc - 3, 4, vp(d8)) == E and cget(ch._h, -1, 1, vp(d8)) == E and cget(ch._h, nc + 1, 0, vp(d8)) == E
    assert cget(ch._h, nc - 4, 4, vp(d8)) == 0 and cget(ch._h, nc, 0, None) == 0
    # runs in flight
    oe = ch.exp_cells_get()
    ch.cluster_async("v2", 2000, 5)
    assert diag(ch._h, None, 1, ref(a), ref(b)) == E and dget(ch._h, 0, 1, vp(p8), vp(c8), vp(d8)) == E and eset(ch._h, vp(ones), nb) == E
    assert cget(ch._h, 0, 1, vp(d8)) == E and free(ch._h) == E
    ch.wait()
    assert np.array_equal(ch.exp_cells_get(), oe, equal_nan=True)            # the handle still works
    assert free(ch._h) == 0 and cget(ch._h, 0, 1, vp(d8)) == E
    ch.close()


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------
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
    """expected.main on a directory of two chromosomes: the five files are EQUAL to those the host functions make of the oracle's
    stand-in -- the ten digits of the texts hide the last few ulps between the two; -raw and -nosmooth once each"""
    from cloops_amd import expected, pipe
    data = {"chr2": MC.scattered(0, 3000, 150000, 40000, both=True), "chr10": MC.scattered(1, 2500, 120000, 30000, both=True)}
    d = os.path.join(str(tmp_path), "jd")
    for name, (X, Y) in data.items():
        _write_jd(d, name, X, Y)
    out = os.path.join(str(tmp_path), "o")
    rg = ("chr10", 20000, 90000)
    base = dict(res=2000, cut=0, raw=False, per_decade=10, nosmooth=False, ignore_diags=2, min_nnz=10, min_count=0, mad_max=5.0, tol=1e-5,
                max_iters=200, region="chr10:20000-90000")
    for flags, kw in (([], {}), (["-raw"], {"raw": True}), (["-nosmooth", "-perdecade", "3"], {"nosmooth": True, "per_decade": 3})):
        pipe.CACHE.clear()
        assert expected.main(["-d", d, "-o", out, "-res", "2000", "-r", "chr10:20000-90000"] + flags) == 0
        per = {n: expected.expected_chrom(EC.OracleChrom(*data[n]), n, 2000, region=rg if n == "chr10" else None, **kw) for n in data}
        want, js = expected.expected_outputs(per, dict(base, **kw))
        got = _files(out, expected.SUFFIXES)
        assert json.loads(got["_expected.json"]) == js and all(js["chroms"][n]["n_valid"] > 30 and js["chroms"][n]["n_used"] > 500 for n in data)
        assert all(js["chroms"][n]["converged"] != bool(kw.get("raw")) for n in data)
        for suffix in expected.SUFFIXES:
            assert got[suffix] == want[suffix], (flags, suffix)
        assert list(js["chroms"]) == ["chr10", "chr2"] and got["_expected.txt"].startswith("chr10\t2\t4000\t")
    # refused before any file is written
    bad = os.path.join(str(tmp_path), "bad")
    for f in (lambda: expected.jd2expected(d, bad, region="chr7:0-1000"), lambda: expected.jd2expected(d, bad, per_decade=0),
              lambda: expected.jd2expected(d, bad, tol=-1.0), lambda: expected.jd2expected(d, bad, chroms={"chr2"}, region="chr10:0-1000")):
        with pytest.raises(ValueError):
            f()
    pipe.CACHE.clear()
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("bad")]
