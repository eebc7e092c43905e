"""GPU: K27 (cl_eig_build / cl_eig_apply / cl_eig_iterate / cl_eig_vectors_get, cloops_amd.compartments) against the numpy oracle of
tests/compartments_cases.py -- the product M x against the dense matrix within a bound that comes from the number of roundings, at the
edges of the row kernel's cell steps and of the scan's tiles; the eigenpairs against np.linalg.eigh through their own residuals; the
same bytes twice; lifetimes, refusals, and the command end to end."""
import ctypes
import json
import os

import numpy as np
import pytest

import balance_cases as BC
import compartments_cases as CC
import expected_cases as EC
import matrix_cases as MC

pytestmark = pytest.mark.gpu

TILE = CC.TILE                 # cl_segsum.h K25_TILE: the cell counts of the product's cases
SCAN = CC.SCAN_TILE            # k_eig.hip K27_SB: bins per workgroup of the band term's scan
EPS = CC.EPS
INF = float("inf")


def chrom(X, Y):
    from cloops_amd import api
    return api.Chromosome(np.asarray(X, np.int64), np.asarray(Y, np.int64))


def prepare(ch, X, Y, res, ign, raw=False, mask=None, expected=None, nosmooth=False, bal_iters=50):
    """cells, marginals, (weights,) diagonals and expected values on the device -> dict(cells, b0, nb, ign, valid, w, e, p): the DEVICE's
    weights and sums, so that K25's and K26's deviations do not enter"""
    from cloops_amd import expected as X26
    cells = MC.cells_oracle(X, Y, 0, res, True)[:3]
    assert ch.mat_cells(res, fold=True)[0] == len(cells[0])
    b0, nb = BC.span(cells[0], cells[1])
    assert ch.bal_marginals(ign)[:2] == (b0, nb)
    s, z = ch.bal_marginals_get()
    m = BC.valid_oracle(s, z, 1, 0, 0) if mask is None else np.asarray(mask(nb), bool)
    if raw:
        ch.exp_diagonals(valid=m, balanced=False)
        valid, w = m.copy(), np.ones(nb)
    else:
        ch.bal_iterate(m, max_iters=bal_iters)
        w = ch.bal_weights()
        valid = ~np.isnan(w)
        ch.exp_diagonals()
    p, _, vs = ch.exp_diagonals_get()
    e = X26.expected_of(p, vs, ign, nosmooth=nosmooth)[0] if expected is None else expected(nb)
    ch.exp_set(e)
    return dict(cells=cells, b0=b0, nb=nb, ign=ign, valid=valid, w=w, e=e, p=p)


def args_of(st, clip, dmax):
    return (st["cells"], st["b0"], st["nb"], st["ign"], st["valid"], st["w"], st["e"], clip, dmax)


def full_dmax(st):
    from cloops_amd import compartments
    return compartments.pick_dmax(st["p"], st["e"], st["ign"])


def check_apply(ch, st, clip, dmax, seed=0):
    """eig_build + eig_apply with 1 and 8 vectors against dense_M @ x within apply_bound; the oracle's second form stays within the
    same bound on the CPU -> (M, the largest deviation over its bound: device, oracle)"""
    a = args_of(st, clip, dmax)
    nb, valid = st["nb"], st["valid"]
    M = CC.dense_M(*a)
    nv, n_in = ch.eig_build(clip, dmax)
    assert nv == int(valid.sum()) and n_in == int(CC.band_cells(st["cells"][0], st["cells"][1], st["b0"], nb, st["ign"], valid, dmax).sum())
    rng = np.random.default_rng(seed)
    worst = own = 0.0
    for n_vec in (1, 8):
        x = rng.standard_normal((n_vec, nb))
        want = (M @ np.where(valid, x, 0.0).T).T
        bound = CC.apply_bound(*a, x)
        got = ch.eig_apply(x)
        assert got.shape == x.shape and not got[:, ~valid].any()
        mine = CC.apply_sparse(*a, x)
        live = bound > 0
        assert np.array_equal(got[~live], want[~live]) and np.array_equal(mine[~live], want[~live])
        if live.any():
            worst = max(worst, float(np.max(np.abs(got - want)[live] / bound[live])))
            own = max(own, float(np.max(np.abs(mine - want)[live] / bound[live])))
        if n_vec == 1:
            assert np.array_equal(ch.eig_apply(x[0]), got[0])                 # one vector, one-dimensional
    assert own <= 1.0, own                                                    # the bound holds on the CPU
    assert worst <= 1.0, worst
    return M, worst, own


# ---- 1. the product ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 2, 9, 63, 64, 65, SCAN - 1, SCAN, SCAN + 1, 1200])
def test_product_over_the_bins(nb):
    X, Y = EC.spanning(nb, seed=nb, filler=6 * nb)
    ch = chrom(X, Y)
    st = prepare(ch, X, Y, 1, 0, raw=True, mask=lambda n: np.ones(n, bool), expected=lambda n: np.linspace(2.0, 0.5, n))
    assert st["nb"] == nb
    for dmax in sorted({0, nb // 2, nb}):
        for clip in (1.0, INF):
            M, worst, own = check_apply(ch, st, clip, dmax, seed=nb)
            assert M.any() if (dmax > 0 and clip == INF) else (dmax > 0 or not M.any())
    print("K27 product nb %d: largest deviation over its bound: device %.3g, the oracle's second form %.3g" % (nb, worst, own))
    ch.close()


@pytest.mark.parametrize("n_cells", [TILE, TILE + 1, 2 * TILE + 1])
def test_product_cell_counts_at_the_tile(n_cells):
    X, Y = BC.with_cell_count(n_cells)
    ch = chrom(X, Y)
    for ign, raw in ((0, True), (2, False)):
        st = prepare(ch, X, Y, 1000, ign, raw=raw)
        assert len(st["cells"][0]) == n_cells
        check_apply(ch, st, 2.0, full_dmax(st))
    ch.close()


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("nb", [16 * CC.ROWS_PER_WG - 1, 16 * CC.ROWS_PER_WG, 16 * CC.ROWS_PER_WG + 1])
def test_product_rows_at_the_cell_steps(nb, transpose):
    """runs of CELL_STEP - 1, CELL_STEP, CELL_STEP + 1, 2 CELL_STEP - 1, 2 CELL_STEP, 2 CELL_STEP + 1, 1 and 0 cells, in the order as the
    cells lie and in the transposed one; the last workgroup of the product holds 3, 4 and 1 bins"""
    S = CC.CELL_STEP
    X, Y = CC.stepped_rows(nb, transpose=transpose)
    ch = chrom(X, Y)
    st = prepare(ch, X, Y, 1, 1, raw=True, mask=lambda n: np.ones(n, bool), expected=lambda n: np.linspace(2.0, 0.5, n))
    assert st["nb"] == nb
    bx, by = st["cells"][0], st["cells"][1]
    off = bx != by
    runs = np.bincount((by if transpose else bx)[off], minlength=nb)
    runs = runs[::-1] if transpose else runs
    assert runs[:8].tolist() == [S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 1, 0] and runs[8:16].tolist() == runs[:8].tolist()
    for clip in (1.0, INF):
        check_apply(ch, st, clip, nb, seed=nb)
    ch.close()


def test_product_rows_over_several_tiles():
    X, Y = BC.arrow()
    ch = chrom(X, Y)
    st = prepare(ch, X, Y, 100, 1, mask=lambda n: BC.valid_oracle(*ch.bal_marginals_get(), 5, 0, 5))
    L = np.bincount(st["cells"][0] - st["b0"], minlength=st["nb"])
    assert L[0] > TILE and len(st["cells"][0]) > 4 * TILE                     # a row of hundreds of steps of eight cells
    M, worst, own = check_apply(ch, st, 3.0, full_dmax(st))
    print("K27 product, a row of %d cells: largest deviation over its bound: device %.3g, the oracle's second form %.3g" % (L[0], worst, own))
    ch.close()


def test_product_with_a_gap_and_negative_bins():
    X, Y = BC.gapped()
    ch = chrom(X, Y)
    st = prepare(ch, X, Y, 1000, 2, mask=lambda n: BC.valid_oracle(*ch.bal_marginals_get()))
    assert (~st["valid"]).sum() >= 50
    full = full_dmax(st)
    assert st["ign"] < full <= st["nb"]
    check_apply(ch, st, 4.0, full)
    ch.close()
    X, Y = MC.scattered(4, 5000, 60000, 9000, both=True)
    X, Y = X - 30000, Y - 30000
    ch = chrom(X, Y)
    for res, ign in ((1000, 0), (333, 3)):
        st = prepare(ch, X, Y, res, ign, raw=True)
        assert st["b0"] < 0 < st["b0"] + st["nb"]
        check_apply(ch, st, INF, full_dmax(st))
    ch.close()


MASKS = {"ends": lambda n: (np.arange(n) >= 3) & (np.arange(n) < n - 2), "middle": lambda n: np.abs(np.arange(n) - n // 2) > 4,
         "every_second": lambda n: np.arange(n) % 2 == 0, "none": lambda n: np.zeros(n, bool)}


@pytest.mark.parametrize("mask", sorted(MASKS))
@pytest.mark.parametrize("raw", [False, True])
def test_product_masks_bands_and_clips(mask, raw):
    X, Y = MC.scattered(3, 40000, 200000, 30000, both=True)
    ch = chrom(X, Y)
    nb = BC.span(*MC.cells_oracle(X, Y, 0, 1000, True)[:2])[1]
    for ign in (0, 2, nb):                                                    # nb: beyond every cell
        st = prepare(ch, X, Y, 1000, ign, raw=raw, mask=MASKS[mask])
        assert st["nb"] == nb and (not raw or np.array_equal(st["valid"], MASKS[mask](nb)))
        full = full_dmax(st)
        oe = EC.oe_oracle(*st["cells"], st["b0"], nb, ign, st["valid"], st["w"], st["e"])
        bite = float(np.nanpercentile(oe, 80)) if np.isfinite(oe).any() else 1.0
        for dmax in sorted({ign, (ign + full) // 2, full}):
            for clip in (bite, INF):
                M, _, _ = check_apply(ch, st, clip, dmax)
                if dmax > ign and st["valid"].sum() > 10 and np.isfinite(clip):
                    assert M.max() == clip - 1.0                              # the clip bites
    ch.close()


# ---- 2. the eigenpairs ---------------------------------------------------------------------------------------------------
def on_device(ch, c):
    """a planted case on the device with the oracle's mask -> the state of `prepare`, clip and dmax (the case's own)"""
    st = prepare(ch, c["X"], c["Y"], 1000, c["ign"], mask=lambda n: c["mask"], nosmooth=True)
    assert np.array_equal(st["valid"], c["valid"]) and full_dmax(st) == c["dmax"]
    return st, c["clip"], c["dmax"]


def check_pairs(ch, st, M, n_eigs, tol, clip, dmax, it_cv_lam_res):
    """the checks of the issue on the pairs of one eig_iterate -> the device's vectors"""
    it, cv, lam, resid = it_cv_lam_res
    valid, nb = st["valid"], st["nb"]
    have = min(n_eigs, int(valid.sum()))
    ref_lam, ref_vec, ev = CC.eig_oracle(M, valid, n_eigs)
    gaps = CC.gaps_of(ev)
    ref_err = nb * EPS * float(np.abs(ev).max())                              # the reference's own: eigh's backward error, n eps |M|
    assert have >= 1 and cv and it >= 1 and len(lam) == n_eigs and np.isnan(lam[have:]).all() and np.isnan(resid[have:]).all()
    assert np.all(np.abs(lam[:have - 1]) >= np.abs(lam[1:have]))               # ordering
    vecs = []
    for k in range(n_eigs):
        v = ch.eig_vectors(k)
        vecs.append(v)
        if k >= have:
            assert np.isnan(v).all()
            continue
        assert np.array_equal(np.isnan(v), ~valid)                           # NaN exactly on the invalid bins
        v0 = np.where(valid, v, 0.0)
        assert abs(np.linalg.norm(v0) - 1.0) <= 8 * (nb + 8) * EPS            # unit norm: a Gram-Schmidt pass and an 8 x 8 rotation
        assert v0[int(np.argmax(np.abs(v0)))] > 0                             # the sign rule
        slack = float(np.linalg.norm(CC.apply_bound(*args_of(st, clip, dmax), v0)))
        r = float(np.linalg.norm(M @ v0 - lam[k] * v0))
        print("K27 pair %d of %d: lambda %.10g (ref %.10g), residual %.3g (device %.3g), allowed %.3g + %.3g, gap %.3g" %
              (k, n_eigs, lam[k], ref_lam[k], r, resid[k], tol * abs(lam[0]), slack, gaps[k]))
        assert r <= tol * abs(lam[0]) + slack
        # (the theorem is one of exact quantities: r as recomputed here carries the product's rounding, the reference eigh's own error)
        assert abs(lam[k] - ref_lam[k]) <= r + slack + ref_err
        assert gaps[k] > r, (k, gaps[k], r)                                   # Davis-Kahan says something
        assert abs(np.dot(v0, np.where(valid, ref_vec[k], 0.0))) >= np.sqrt(1.0 - (r / gaps[k]) ** 2) - slack / gaps[k] - 8 * nb * EPS
    return vecs


@pytest.mark.parametrize("name", ["small", "large"])
def test_eigenpairs_of_the_planted_data(name):
    c = CC.planted_case(name)
    ch = chrom(c["X"], c["Y"])
    st, clip, dmax = on_device(ch, c)
    M = CC.dense_M(*args_of(st, clip, dmax))
    ch.eig_build(clip, dmax)
    for n_eigs in (1, 3):
        res = ch.eig_iterate(n_eigs)                                          # the defaults: tol 1e-8, 1000 iterations
        vecs = check_pairs(ch, st, M, n_eigs, 1e-8, clip, dmax, res)
        print("K27 planted %s, n_eigs %d: %d iterations" % (name, n_eigs, res[0]))
    from cloops_amd import compartments
    assert abs(compartments.pearson(vecs[0], c["comp"].astype(np.float64))) > 0.8
    with pytest.raises(Exception):
        ch.eig_vectors(3)
    ch.close()


def few_bins(nv, seed):
    """rows at res 1 over 12 bins and a mask of nv valid ones"""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 12, 400)
    Y = rng.integers(0, 12, 400)
    X, Y = np.concatenate([[0], np.minimum(X, Y)]), np.concatenate([[11], np.maximum(X, Y)])
    keep = np.sort(rng.choice(12, nv, replace=False))
    return X.astype(np.int64), Y.astype(np.int64), lambda n: np.isin(np.arange(n), keep)


@pytest.mark.parametrize("nv", [1, 2, 3, 5])
def test_a_block_that_covers_the_space_needs_one_iteration(nv):
    X, Y, mask = few_bins(nv, nv)
    ch = chrom(X, Y)
    st = prepare(ch, X, Y, 1, 0, raw=True, mask=mask, expected=lambda n: np.full(n, 1.5))
    assert st["valid"].sum() == nv
    M, _, _ = check_apply(ch, st, INF, st["nb"])
    it, cv, lam, resid = ch.eig_iterate(6, max_iters=1, tol=1e-12)
    assert it == 1 and cv
    check_pairs(ch, st, M, 6, 1e-12, INF, st["nb"], (it, cv, lam, resid))      # (equal to eigh within the residual and the rounding bound)
    ch.close()


def test_nine_valid_bins_and_a_block_of_eight():
    X, Y, mask = few_bins(9, 9)
    ch = chrom(X, Y)
    st = prepare(ch, X, Y, 1, 0, raw=True, mask=mask, expected=lambda n: np.full(n, 1.5))
    M, _, _ = check_apply(ch, st, INF, st["nb"])
    res = ch.eig_iterate(3, max_iters=1000, tol=1e-10)
    assert res[0] > 1
    check_pairs(ch, st, M, 3, 1e-10, INF, st["nb"], res)
    ch.close()


def test_a_zero_matrix():
    """M = 0 (dmax = ign: an empty band): eigenvalues 0, finite orthonormal vectors, converged"""
    X, Y = MC.scattered(5, 3000, 50000, 9000)
    ch = chrom(X, Y)
    st = prepare(ch, X, Y, 500, 2, raw=True)
    nb, valid = st["nb"], st["valid"]
    assert ch.eig_build(INF, 2) == (int(valid.sum()), 0)
    assert not ch.eig_apply(np.ones(nb)).any()
    it, cv, lam, resid = ch.eig_iterate(6)
    assert (it, cv) == (1, True) and not lam.any() and not resid.any()
    V = np.stack([ch.eig_vectors(k) for k in range(6)])
    assert np.array_equal(np.isnan(V), np.broadcast_to(~valid, V.shape)) and np.isfinite(V[:, valid]).all()
    G = V[:, valid] @ V[:, valid].T
    assert np.abs(G - np.eye(6)).max() <= 8 * (nb + 8) * EPS
    # max_iters = 0: nothing iterated
    it, cv, lam, resid = ch.eig_iterate(2, max_iters=0)
    assert (it, cv) == (0, False) and np.isnan(lam).all() and np.isnan(resid).all() and np.isnan(ch.eig_vectors(0)).all()
    ch.close()


def test_no_valid_bins_and_no_bins():
    from cloops_amd import _lib
    X, Y = MC.scattered(5, 3000, 50000, 9000)
    ch = chrom(X, Y)
    st = prepare(ch, X, Y, 500, 2, raw=True, mask=lambda n: np.zeros(n, bool))
    assert ch.eig_build(INF, st["nb"]) == (0, 0)
    assert not ch.eig_apply(np.ones((8, st["nb"]))).any()
    it, cv, lam, resid = ch.eig_iterate(3)
    assert (it, cv) == (0, False) and np.isnan(lam).all() and np.isnan(resid).all() and np.isnan(ch.eig_vectors(2)).all()
    ch.close()
    for X, Y in ((MC.EMPTY, MC.EMPTY),):
        ch = chrom(X, Y)
        assert ch.mat_cells(1000, fold=True)[0] == 0 and ch.bal_marginals(2) == (0, 0, 0)
        assert ch.exp_diagonals(balanced=False) == (0, 0)
        ch.exp_set(np.zeros(0))
        assert ch.eig_build(INF, 0) == (0, 0) and ch.eig_apply(np.zeros(0)).shape == (0,)
        it, cv, lam, resid = ch.eig_iterate(2)
        assert (it, cv) == (0, False) and np.isnan(lam).all() and len(ch.eig_vectors(0)) == 0
        lib = _lib.load()
        assert lib.cl_eig_vectors_get(ch._h, 0, 0, 0, None) == 0 and lib.cl_eig_apply(ch._h, None, 1, None) == 0
        with pytest.raises(_lib.CloopsHipError):
            ch.eig_vectors(0, 0, 1)
        assert ch.eig_free() is None
        ch.close()


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------
def test_the_same_bytes_twice():
    c = CC.planted_case("small")
    ch = chrom(c["X"], c["Y"])
    st, clip, dmax = on_device(ch, c)
    x = np.random.default_rng(1).standard_normal((8, st["nb"]))

    def once(build=True):
        if build:
            ch.eig_build(clip, dmax)
        y = ch.eig_apply(x)
        it, cv, lam, resid = ch.eig_iterate(3, tol=1e-6)
        return (it, cv, lam.tobytes(), resid.tobytes(), y.tobytes()) + tuple(ch.eig_vectors(k).tobytes() for k in range(3))
    first = once()
    assert first[1] and first[0] > 5
    assert once(build=False) == first                                        # two eig_iterate calls
    ch.eig_free()
    assert once() == first                                                   # after eig_free and a rebuild
    ch.agg_loops([20000], [25000], 1000, 10, 3, cut=4000)                    # rebuilds the shared table: the cells are copies
    assert once(build=False) == first
    ch.close()


# ---- 4. lifetimes and refusals -------------------------------------------------------------------------------------------------
def test_lifetimes():
    from cloops_amd import _lib, expected as X26
    E = _lib.CloopsHipError
    X, Y = MC.scattered(5, 3000, 50000, 9000)
    ch = chrom(X, Y)

    def refused(*calls):
        for f in calls:
            with pytest.raises(E):
                f()
    users = (lambda: ch.eig_apply(np.zeros(getattr(ch, "_bal_bins", 0))), lambda: ch.eig_iterate(1), lambda: ch.eig_vectors(0, 0, 0))
    refused(lambda: ch.eig_build(), *users)                                  # nothing on the handle
    assert ch.eig_free() is None
    ch.mat_cells(500, fold=True)
    refused(lambda: ch.eig_build(), *users)
    b0, nb, _ = ch.bal_marginals(2)
    refused(lambda: ch.eig_build(), *users)
    ch.exp_diagonals(balanced=False)
    refused(lambda: ch.eig_build(), *users)                                  # before exp_set
    n = len(ch.mat_cells_get()[0])

    def build(raw=True, iterate=True):
        if raw:
            ch.exp_diagonals(balanced=False)
        else:
            s, z = ch.bal_marginals_get()
            ch.bal_iterate(BC.valid_oracle(s, z))
            ch.exp_diagonals()
        p, _, vs = ch.exp_diagonals_get()
        e = X26.expected_of(p, vs, 2)[0]
        ch.exp_set(e)
        refused(*users)                                                      # before eig_build
        from cloops_amd import compartments
        dmax = compartments.pick_dmax(p, e, 2)
        assert ch.eig_build(5.0, dmax)[1] > 100
        refused(lambda: ch.eig_vectors(0, 0, 0))                             # before eig_iterate
        if iterate:
            assert ch.eig_iterate(2, tol=1e-6)[1]
            assert len(ch.eig_vectors(1)) == nb
        return e, dmax
    e, dmax = build()
    # the ends of the ranges, count 0, `which`
    v = ch.eig_vectors(0)
    refused(lambda: ch.eig_vectors(0, -1, 1), lambda: ch.eig_vectors(0, nb, 1), lambda: ch.eig_vectors(0, 0, nb + 1), lambda: ch.eig_vectors(0, nb + 1, 0),
            lambda: ch.eig_vectors(2), lambda: ch.eig_vectors(-1), lambda: ch.eig_vectors(6))
    assert len(ch.eig_vectors(0, nb, 0)) == 0 and np.array_equal(ch.eig_vectors(0, nb - 1, 1), v[nb - 1:], equal_nan=True)
    assert np.array_equal(ch.eig_vectors(0, 5, 7), v[5:12], equal_nan=True)
    with pytest.raises(ValueError):
        ch.eig_iterate(0)
    with pytest.raises(ValueError):
        ch.eig_iterate(7)
    for bad in (np.zeros(nb - 1), np.zeros((9, nb)), np.zeros((2, nb + 1)), np.zeros((1, 1, nb))):
        with pytest.raises(ValueError):
            ch.eig_apply(bad)
    # refused builds leave the matrix and the vectors
    refused(lambda: ch.eig_build(0.0), lambda: ch.eig_build(-1.0), lambda: ch.eig_build(float("nan")), lambda: ch.eig_build(5.0, 1),
            lambda: ch.eig_build(5.0, nb + 1), lambda: ch.eig_iterate(1, max_iters=-1), lambda: ch.eig_iterate(1, tol=-1.0),
            lambda: ch.eig_iterate(1, tol=float("nan")))
    assert np.array_equal(ch.eig_vectors(0), v, equal_nan=True)
    # a second eig_iterate replaces the vectors; eig_apply leaves them
    y = ch.eig_apply(np.ones(nb))
    assert np.array_equal(ch.eig_vectors(0), v, equal_nan=True) and y.any()
    ch.eig_iterate(1, tol=1e-6)
    refused(lambda: ch.eig_vectors(1))
    # the rule on the expected values: a diagonal of the band with pairs and no finite positive value
    for badv in (0.0, -1.0, np.nan, np.inf):
        e2 = e.copy()
        e2[7] = badv
        ch.exp_set(e2)                                                       # a second exp_set drops the matrix
        refused(*users)
        refused(lambda: ch.eig_build(5.0, dmax))
        assert ch.eig_build(5.0, 7)[0] == nb                                 # ... below it the band is fine
        refused(lambda: ch.eig_build(5.0, 8))
        assert len(ch.eig_apply(np.ones(nb))) == nb                          # the refused build left the one before
    # eig_free keeps everything below
    build()
    ch.eig_free()
    refused(*users)
    assert len(ch.exp_cells_get()) == n
    # every call that drops or rebuilds K24 .. K26 drops K27
    for drop in (lambda: ch.exp_diagonals(balanced=False), lambda: ch.exp_free(), lambda: ch.bal_marginals(2), lambda: ch.bal_free(),
                 lambda: ch.mat_cells(500, fold=True), lambda: ch.mat_free()):
        if not getattr(ch, "_mat_cells", 0):
            ch.mat_cells(500, fold=True)
        if not getattr(ch, "_bal_bins", 0):
            ch.bal_marginals(2)
        build()
        drop()
        refused(*users)
    ch.mat_cells(500, fold=True)
    ch.bal_marginals(2)
    build(raw=False)
    s, z = ch.bal_marginals_get()
    ch.bal_iterate(BC.valid_oracle(s, z), max_iters=3)
    refused(lambda: ch.eig_build(), *users)
    ch.close()


def test_argument_errors_of_the_c_calls():
    from cloops_amd import api, _lib, expected as X26
    lib = _lib.load()
    E = _lib.CL_ERR_ARG
    X, Y = MC.scattered(5, 1000, 50000, 9000)
    ch = api.Chromosome(X, Y)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ref = ctypes.byref
    a, b = ctypes.c_int64(7), ctypes.c_int64(7)
    it, cv = ctypes.c_int32(7), ctypes.c_int32(7)
    build, apply_, iterate, vget, free = lib.cl_eig_build, lib.cl_eig_apply, lib.cl_eig_iterate, lib.cl_eig_vectors_get, lib.cl_eig_free
    d8, r8 = np.zeros(8, np.float64), np.zeros(8, np.float64)
    assert build(None, 1.0, 0, ref(a), ref(b)) == E and (a.value, b.value) == (0, 0)
    assert apply_(None, vp(d8), 1, vp(r8)) == E and iterate(None, 1, 1, 1e-8, ref(it), ref(cv), vp(d8), vp(r8)) == E and (it.value, cv.value) == (0, 0)
    assert vget(None, 0, 0, 1, vp(d8)) == E and free(None) == E
    ch.mat_cells(500, fold=True)
    b0, nb, _ = ch.bal_marginals(2)
    ch.exp_diagonals(balanced=False)
    a.value = b.value = 7
    assert build(ch._h, 1.0, nb, ref(a), ref(b)) == E and (a.value, b.value) == (0, 0) and b"cl_eig_build" in lib.cl_last_error()   # before cl_exp_set
    assert free(ch._h) == 0
    p, _, vs = ch.exp_diagonals_get()
    e = X26.expected_of(p, vs, 2)[0]
    ch.exp_set(e)
    from cloops_amd import compartments
    full = compartments.pick_dmax(p, e, 2)                                  # (few rows: the far diagonals have pairs and no contacts)
    assert 10 < full < nb
    x, y = np.ones((8, nb)), np.zeros((8, nb))
    assert apply_(ch._h, vp(x), 1, vp(y)) == E and vget(ch._h, 0, 0, 0, None) == E                    # before cl_eig_build
    it.value = cv.value = 7
    assert iterate(ch._h, 1, 1, 1e-8, ref(it), ref(cv), vp(d8), vp(r8)) == E and (it.value, cv.value) == (0, 0)
    assert build(ch._h, 1.0, nb, None, ref(b)) == E and build(ch._h, 1.0, nb, ref(a), None) == E
    for clip, dmax in ((0.0, nb), (-2.0, nb), (float("nan"), nb), (1.0, 1), (1.0, nb + 1), (1.0, -1)):
        a.value = b.value = 7
        assert build(ch._h, clip, dmax, ref(a), ref(b)) == E and (a.value, b.value) == (0, 0)
    assert build(ch._h, float("inf"), nb, ref(a), ref(b)) == E and (a.value, b.value) == (0, 0)       # the rule on the expected values
    assert build(ch._h, float("inf"), full, ref(a), ref(b)) == 0 and a.value == nb and b.value > 0
    assert build(ch._h, 1.0, 2, ref(a), ref(b)) == 0 and (a.value, b.value) == (nb, 0)                # dmax = ign
    assert build(ch._h, 3.0, full, ref(a), ref(b)) == 0
    assert apply_(ch._h, None, 1, vp(y)) == E and apply_(ch._h, vp(x), 1, None) == E and apply_(ch._h, vp(x), 0, vp(y)) == E
    assert apply_(ch._h, vp(x), 9, vp(y)) == E and apply_(ch._h, vp(x), -1, vp(y)) == E and apply_(ch._h, vp(x), 8, vp(y)) == 0
    assert vget(ch._h, 0, 0, 1, vp(d8)) == E                                # before cl_eig_iterate
    for args in ((0, 1, 1e-8), (7, 1, 1e-8), (-1, 1, 1e-8), (1, -1, 1e-8), (1, 1, -1e-8), (1, 1, float("nan"))):
        it.value = cv.value = 7
        assert iterate(ch._h, args[0], args[1], args[2], ref(it), ref(cv), vp(d8), vp(r8)) == E and (it.value, cv.value) == (0, 0)
    assert iterate(ch._h, 1, 1, 1e-8, None, ref(cv), vp(d8), vp(r8)) == E and iterate(ch._h, 1, 1, 1e-8, ref(it), None, vp(d8), vp(r8)) == E
    assert iterate(ch._h, 1, 1, 1e-8, ref(it), ref(cv), None, vp(r8)) == E and iterate(ch._h, 1, 1, 1e-8, ref(it), ref(cv), vp(d8), None) == E
    assert iterate(ch._h, 2, 500, 1e-6, ref(it), ref(cv), vp(d8), vp(r8)) == 0 and it.value > 0 and abs(d8[0]) >= abs(d8[1]) > 0
    assert vget(ch._h, 0, 0, 1, None) == E and vget(ch._h, 2, 0, 1, vp(d8)) == E and vget(ch._h, -1, 0, 1, vp(d8)) == E
    assert vget(ch._h, 0, nb - 3, 4, vp(d8)) == E and vget(ch._h, 0, -1, 1, vp(d8)) == E and vget(ch._h, 0, nb + 1, 0, vp(d8)) == E
    assert vget(ch._h, 1, nb - 4, 4, vp(d8)) == 0 and vget(ch._h, 0, nb, 0, None) == 0
    # runs in flight
    v = ch.eig_vectors(0)
    ch.cluster_async("v2", 2000, 5)
    assert build(ch._h, 1.0, full, ref(a), ref(b)) == E and apply_(ch._h, vp(x), 1, vp(y)) == E and vget(ch._h, 0, 0, 1, vp(d8)) == E
    assert iterate(ch._h, 1, 1, 1e-8, ref(it), ref(cv), vp(d8), vp(r8)) == E and free(ch._h) == E
    ch.wait()
    assert np.array_equal(ch.eig_vectors(0), v, equal_nan=True)               # the handle still works
    assert free(ch._h) == 0 and vget(ch._h, 0, 0, 1, vp(d8)) == E
    ch.close()


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------
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
    """compartments.main -nosmooth -neigs 3 on a directory of two planted chromosomes against the host functions on the oracle's
    stand-in.  The files are, byte for byte, what the host functions make of the device's unformatted vectors.  Those vectors differ from
    the stand-in's by up to 1e-8 |lambda_0| over the gap, which ten digits do not hide: so every float of the files -- all three vector
    columns, the eigenvalues, the residuals, the correlations, the run means -- is compared numerically, within bounds made of measured
    quantities: with M_d the dense matrix of the device's own weights and expected values, M_o the stand-in's, D = |M_d - M_o|_F, r the
    device pair's residual against M_d (itself within tol |lambda_0| + the product's bound), e the reference's own error n eps |M| and
    g the pair's gap in the stand-in's full spectrum less 2 D (Weyl): both vectors are approximate eigenvectors of M_d, so their
    distance is at most sqrt(2) (r + D + 2 e) / g (Davis-Kahan, the chord of the angle), the eigenvalues differ by at most r + D + e.
    Integer columns, run boundaries, flags, and the floats of K25 / K26 at the file's ten digits are compared exactly."""
    from cloops_amd import balance, compartments, pipe
    tol = 1e-8
    cases = {"chr2": CC.planted_case("small"), "chr10": CC.planted_case("second")}
    d = os.path.join(str(tmp_path), "jd")
    for name, c in cases.items():
        _write_jd(d, name, c["X"], c["Y"])
    out = os.path.join(str(tmp_path), "o")
    pipe.CACHE.clear()
    assert compartments.main(["-d", d, "-o", out, "-res", "1000", "-neigs", "3", "-nosmooth"]) == 0
    pipe.CACHE.clear()
    got = _files(out, compartments.SUFFIXES)
    js = json.loads(got["_eigs.json"])
    assert list(js["chroms"]) == ["chr10", "chr2"] and js["args"]["n_eigs"] == 3 and js["args"]["res"] == 1000 and js["args"]["nosmooth"]
    # the files are the host functions' texts of the device's vectors
    dev = {}
    for n, c in cases.items():
        ch = chrom(c["X"], c["Y"])
        dev[n] = compartments.compartments_chrom(ch, n, 1000, n_eigs=3, nosmooth=True)
        ch.close()
    texts, js_dev = compartments.compartments_outputs(dev, js["args"])
    assert js_dev == js and all(got[sfx] == texts[sfx] for sfx in compartments.SUFFIXES)
    per = {n: compartments.compartments_chrom(CC.OracleChrom(c["X"], c["Y"]), n, 1000, n_eigs=3, nosmooth=True) for n, c in cases.items()}
    rows = [line.split("\t") for line in got["_eigs.txt"].splitlines()]
    want_rows = [line.split("\t") for n in sorted(per) for line in per[n]["eigs"].splitlines()]
    assert [r[:4] for r in rows] == [r[:4] for r in want_rows] and all(len(r) == 7 for r in rows)
    runs = [line.split("\t") for line in got["_compartments.bed"].splitlines()]
    want_runs = [line.split("\t") for n in sorted(per) for line in per[n]["runs"].splitlines()]
    assert [r[:4] for r in runs] == [r[:4] for r in want_runs]
    at = 0
    for n in sorted(per):
        c, st, ws = cases[n], js["chroms"][n], per[n]["stats"]
        for key in ("b0", "nb", "n_valid", "n_in", "dmax", "iters", "converged", "flipped", "clip", "var", "scale"):
            assert st[key] == ws[key], (n, key, st[key], ws[key])
        assert st["eig_converged"] and ws["eig_converged"] and st["eig_iters"] >= 1
        nb, valid = c["nb"], c["valid"]
        # the device's own matrix: the same calls as the command's, hence the same weights, expected values and clip
        ch = chrom(c["X"], c["Y"])
        sd = prepare(ch, c["X"], c["Y"], 1000, 2, mask=lambda m: c["mask"], nosmooth=True, bal_iters=200)
        clip_d = compartments.clip_of(ch.exp_cells_get(), 99.9)
        ch.close()
        assert balance._num(clip_d) == st["clip"] and full_dmax(sd) == st["dmax"] and np.array_equal(sd["valid"], valid)
        a = args_of(sd, clip_d, st["dmax"])
        M_d = CC.dense_M(*a)
        D = float(np.linalg.norm(M_d - c["M"]))
        ev = c["eigvals"]
        e_ref = nb * EPS * float(np.abs(ev).max())
        gaps = CC.gaps_of(ev)
        E, W = dev[n]["vectors"], per[n]["vectors"]
        F = np.array([[float(x) for x in r[4:]] for r in rows[at:at + nb]]).T   # the file's columns
        assert E.shape == W.shape == F.shape == (3, nb) and np.array_equal(np.isnan(E), np.isnan(W)) and np.array_equal(np.isnan(F), np.isnan(W))
        lam_d, lam_o = np.array(dev[n]["stats"]["eigvals"]), ev[:3]
        e1_allowed = None
        for k in range(3):
            v = np.where(valid, E[k] / np.sqrt(abs(lam_d[k])), 0.0)
            u = np.where(valid, W[k] / np.sqrt(abs(lam_o[k])), 0.0)
            slack = float(np.linalg.norm(CC.apply_bound(*a, v)))
            r = float(np.linalg.norm(M_d @ v - lam_d[k] * v)) + 1e-9 * abs(lam_d[k])   # (lam_d is the json's: ten digits)
            g = gaps[k] - 2 * D
            assert r <= tol * abs(lam_d[0]) + slack + 1e-9 * abs(lam_d[k]) and st["resid"][k] <= tol * abs(lam_d[0]) and g > r
            assert abs(lam_d[k] - lam_o[k]) <= r + D + e_ref
            dist = np.sqrt(2.0) * (r + D + 2 * e_ref) / g
            allowed = np.sqrt(abs(lam_o[k])) * dist + (r + D + e_ref) / np.sqrt(abs(lam_o[k])) * np.abs(v).max()
            devn = float(np.abs(E[k][valid] - W[k][valid]).max())
            text = 1e-9 * float(np.abs(W[k][valid]).max())                   # ten digits, the file's
            print("K27 end to end %s E%d: lambda %.10g, gap %.3g, |M_d - M_o| %.3g, residual %.3g, deviation %.3g allowed %.3g" %
                  (n, k + 1, lam_d[k], g, D, r, devn, allowed))
            assert devn <= allowed and float(np.abs(F[k][valid] - W[k][valid]).max()) <= allowed + text
            # Pearson's r of a unit vector with a track moves by at most twice the vector's move over its centred norm
            cu = float(np.linalg.norm(u[valid] - u[valid].mean()))
            assert abs(st["phase_corr"][k] - ws["phase_corr"][k]) <= 2 * dist / cu + 1e-9
            if k == 0:
                e1_allowed = allowed + text
        assert abs(compartments.pearson(F[0], c["comp"].astype(np.float64))) > 0.8
        mine = [(float(r[4]), float(q[4])) for r, q in zip(runs, want_runs) if r[0] == n]
        assert len(mine) > 2 and all(abs(x - y) <= e1_allowed + 1e-9 * abs(y) for x, y in mine)    # a run's mean moves no more than its entries
        at += nb
    bg = [line.split("\t") for line in got["_E1.bedGraph"].splitlines()]
    assert [b[:3] for b in bg] == [[r[0], r[1], r[2]] for r in rows if r[3] == "1"] and [b[3] for b in bg] == [r[4] for r in rows if r[3] == "1"]
    # refused before any file is written
    bad = os.path.join(str(tmp_path), "bad")
    for f in (lambda: compartments.jd2compartments(d, bad, n_eigs=0), lambda: compartments.jd2compartments(d, bad, clip=0.0),
              lambda: compartments.jd2compartments(d, bad, eig_tol=-1.0), lambda: compartments.jd2compartments(d, bad, phase=bad + ".none")):
        with pytest.raises(ValueError):
            f()
    pipe.CACHE.clear()
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("bad")]
