"""GPU: K30 (cl_sad_sums / cl_sad_get, cloops_amd.saddle) against the numpy oracle of tests/saddle_cases.py fed the device's own weights
and expected values -- `pairs` and `cells` for equality, `sum` within (2 L + 4) 2^-53 per entry -- at the edges of the sums kernel's
tiles and wave steps, of the band and of the pair counts' scan tile; the same bytes twice; lifetimes, refusals, and the command end to
end."""
import ctypes
import json
import os

import numpy as np
import pytest

import balance_cases as BC
import compartments_cases as CC
import expected_cases as EC
import matrix_cases as MC
import saddle_cases as SC

pytestmark = pytest.mark.gpu

T = SC.TILE                    # k_saddle.hip K30_TILE: cells per step of a workgroup of the sums (a chunk is one tile up to 1024 tiles)
SCAN = SC.SCAN_TILE            # k_saddle.hip K30_PT: bins per workgroup of the pair counts


def chrom(X, Y):
    from cloops_amd import api
    return api.Chromosome(np.asarray(X, np.int64), np.asarray(Y, np.int64))


def prepare(ch, X, Y, res, ign, raw=False, mask=None, expected=None, nosmooth=False, cut=0, bal_iters=50):
    """cells, marginals, (weights,) diagonals and expected values on the device -> dict(cells, b0, nb, ign, valid, w, e, p): the DEVICE's
    weights and sums, so that K25's and K26's deviations do not enter"""
    from cloops_amd import expected as X26
    cells = MC.cells_oracle(X, Y, cut, res, True)[:3]
    assert ch.mat_cells(res, cut=cut, fold=True)[0] == len(cells[0])
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


def plain(ch, X, Y, res=1, ign=1):
    """raw, every bin valid, a falling positive expected value on every diagonal"""
    return prepare(ch, X, Y, res, ign, raw=True, mask=lambda n: np.ones(n, bool), expected=lambda n: np.linspace(2.0, 0.5, n))


def full_hi(st, lo=None):
    """the first diagonal from lo (ignore_diags) on that the rule on the expected values refuses, or nb"""
    from cloops_amd import compartments
    return min(compartments.pick_dmax(st["p"], st["e"], st["ign"] if lo is None else lo), st["nb"])


def check(ch, st, cls, n_cls, lo, hi):
    """sad_sums + sad_get against the oracle -> (sum, pairs, cells, the largest deviation of a sum over its bound)"""
    want = SC.tables_oracle(st["cells"], st["b0"], st["nb"], st["ign"], st["valid"], st["w"], st["e"], cls, n_cls, lo, hi)
    nbin, npair, nin = ch.sad_sums(cls, n_cls, lo, hi)
    s, p, c = ch.sad_get()
    assert s.shape == p.shape == c.shape == (n_cls, n_cls) and (s.dtype, p.dtype, c.dtype) == (np.float64, np.int64, np.int64)
    assert np.array_equal(p, want[1]) and np.array_equal(c, want[2])
    assert (nbin, npair, nin) == (int(np.count_nonzero(SC.effective(st["valid"], cls) >= 0)), int(want[1].sum()), int(want[2].sum()))
    ok, worst = SC.within(s, want[0], want[2])
    assert ok, worst
    assert not s[want[2] == 0].any()
    return s, p, c, worst


def cycling(nb, n_cls, shift=0):
    return ((np.arange(nb) + shift) % n_cls).astype(np.int32)


# ---- 1. small and scattered data ---------------------------------------------------------------------------------------------------
def test_the_twelve_rows():
    X, Y = MC.twelve()
    ch = chrom(X, Y)
    for ign in (0, 1, 2):
        st = plain(ch, X, Y, 100, ign)
        nb = st["nb"]
        assert nb == 5
        for cls in (np.zeros(nb, np.int32), np.array([0, 1, 0, 1, 2], np.int32), np.array([2, -1, 0, 1, 2], np.int32)):
            for lo in range(max(ign, 1), nb + 1):
                for hi in range(lo, nb + 1):
                    s, p, c, _ = check(ch, st, cls, 3, lo, hi)
                    assert np.array_equal(p, SC.pairs_by_loop(st["valid"], cls, 3, lo, hi)) and (hi > lo or not (p.any() or c.any() or s.any()))
    ch.close()


@pytest.mark.parametrize("ign,cut", [(0, 0), (2, 0), (0, 3000), (2, 3000)])
def test_scattered_rows(ign, cut):
    X, Y = MC.scattered(11, 30000, 200000, 30000, both=True)
    ch = chrom(X, Y)
    worst = 0.0
    for raw in (True, False):
        st = prepare(ch, X, Y, 1000, ign, raw=raw, mask=(lambda n: np.arange(n) % 9 != 4) if raw else None, cut=cut)
        near = max(ign, 1, -(-cut // 1000) + 1)                                 # (below a cut the diagonals have pairs and no contacts)
        nb, hi = st["nb"], full_hi(st, near)
        assert hi > 10 and (raw or np.isnan(st["w"]).sum() < nb // 2) and (not raw or (~st["valid"]).sum() > 10)
        rng = np.random.default_rng(ign + cut)
        for n_cls in (1, 12, 64):
            cls = rng.integers(-1, n_cls, nb).astype(np.int32)
            for lo, h in ((near, hi), (near + 3, hi // 2 + 3)):
                worst = max(worst, check(ch, st, cls, n_cls, lo, h)[3])
        smooth = np.minimum((np.arange(nb) * 12) // nb, 11).astype(np.int32)     # a smooth track: few keys a wave step
        _, p, c, w2 = check(ch, st, smooth, 12, near, hi)
        assert c.sum() > 1000
        worst = max(worst, w2)
    print("K30 scattered ign %d cut %d: largest deviation of a sum over its bound %.3g" % (ign, cut, worst))
    ch.close()


# ---- 2. the sums kernel's tiles and wave steps ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cells", [T - 1, T, T + 1, 2 * T + 1])
def test_cell_counts_at_the_tile_one_row_across_the_boundary(n_cells):
    """every cell in the row of bin 0: the row straddles every tile and wave boundary.  One key for all 64 cells of a wave step (n_cls = 1,
    and one class), 64 distinct keys a step (n_cls = 64, the classes cycling along by), and both mixed"""
    X, Y = SC.row_of_cells(n_cells)
    ch = chrom(X, Y)
    st = plain(ch, X, Y)
    nb = st["nb"]
    assert len(st["cells"][0]) == n_cells and nb == n_cells + 3 and np.all(st["cells"][0] == 0)
    _, p, c, _ = check(ch, st, np.zeros(nb, np.int32), 1, 1, nb)
    assert c[0][0] == n_cells and p[0][0] == nb * (nb - 1) // 2
    s, p, c, _ = check(ch, st, cycling(nb, 64), 64, 1, nb)
    assert not c[1:].any() and c[0].min() >= n_cells // 64 - 1 and c[0].sum() == n_cells
    check(ch, st, np.full(nb, 5, np.int32), 64, 1, nb)                       # one key of a large table
    check(ch, st, (np.arange(nb) // 40 % 3).astype(np.int32), 3, 2, nb - 1)  # runs of one key across the waves
    ch.close()


@pytest.mark.parametrize("n_cells", [T, T + 1, 2 * T + 1])
def test_cell_counts_at_the_tile_balanced(n_cells):
    X, Y = BC.with_cell_count(n_cells)
    ch = chrom(X, Y)
    for ign, raw in ((0, True), (2, False)):
        st = prepare(ch, X, Y, 1000, ign, raw=raw)
        assert len(st["cells"][0]) == n_cells
        check(ch, st, cycling(st["nb"], 7), 7, max(ign, 1), full_hi(st))
    ch.close()


def test_rows_of_every_length_around_the_wave():
    """rows of 63, 64, 65, 1, 0, 127, 128, 129 cells: a wave step begins and ends in every position of a row"""
    X, Y = SC.rows_of([63, 64, 65, 1, 0, 127, 128, 129] * 3)
    ch = chrom(X, Y)
    st = plain(ch, X, Y)
    nb = st["nb"]
    for n_cls in (2, 64):
        check(ch, st, cycling(nb, n_cls), n_cls, 1, nb)
        check(ch, st, cycling(nb, n_cls, 5), n_cls, 3, 100)
    ch.close()


def test_more_cells_than_chunks_times_the_tile():
    """more than K30_CHUNKS tiles: a chunk is two tiles, the last chunk one"""
    n = SC.CHUNKS * T + 300
    rng = np.random.default_rng(4)
    nb = 1500
    i = rng.integers(0, nb - 1, 3 * n)
    j = np.minimum(i + 1 + rng.integers(0, 400, 3 * n), nb - 1)
    u = np.unique(np.stack([i, j], 1), axis=0)
    assert len(u) >= n
    u = u[np.sort(rng.choice(len(u), n, replace=False))]
    X, Y = np.concatenate([u[:, 0], [0]]), np.concatenate([u[:, 1], [nb - 1]])
    ch = chrom(X, Y)
    st = plain(ch, X, Y)
    assert SC.CHUNKS * T < len(st["cells"][0]) <= SC.CHUNKS * T + 301
    _, p, c, worst = check(ch, st, (np.arange(st["nb"]) * 20 // st["nb"]).astype(np.int32), 20, 1, 300)
    print("K30 %d cells: largest deviation of a sum over its bound %.3g" % (len(st["cells"][0]), worst))
    ch.close()


# ---- 3. classes of -1, the band, the scan tile ---------------------------------------------------------------------------------------
def test_classes_of_minus_one_and_the_band():
    X, Y = SC.rows_of([70] * 90)
    ch = chrom(X, Y)
    st = plain(ch, X, Y, ign=2)
    nb = st["nb"]
    base = cycling(nb, 5)
    first_last = base.copy()
    first_last[[0, nb - 1]] = -1
    own = base.copy()
    own[10:30] = -1                                                          # whole rows: the lower bin of all their cells
    partner = base.copy()
    partner[np.arange(nb) % 3 == 1] = -1
    for cls in (base, first_last, own, partner, np.full(nb, -1, np.int32)):
        for lo, hi in ((2, nb), (2, 71), (5, 6), (7, 7), (nb, nb), (nb - 1, nb), (3, 40)):
            s, p, c, _ = check(ch, st, cls, 5, lo, hi)
    # d == lo is taken and d == hi is left out: the cells of every row lie on d = 1 .. 70
    one = np.zeros(nb, np.int32)
    assert check(ch, st, one, 1, 5, 6)[2][0][0] == 90 and check(ch, st, one, 1, 5, 5)[2][0][0] == 0
    assert check(ch, st, one, 1, 70, 71)[2][0][0] == 90 and check(ch, st, one, 1, 71, 72)[2][0][0] == 0
    assert check(ch, st, one, 1, 69, 70)[2][0][0] == 90 and check(ch, st, one, 1, 2, nb)[2][0][0] == 90 * 69
    ch.close()


@pytest.mark.parametrize("nb", [1, 2, 63, 64, 65, SCAN - 1, SCAN, SCAN + 1, 2 * SCAN + 1, 1200])
def test_bins_at_the_scan_tile(nb):
    X, Y = EC.spanning(nb, seed=nb, filler=6 * nb)
    ch = chrom(X, Y)
    st = plain(ch, X, Y, ign=0)
    assert st["nb"] == nb
    rng = np.random.default_rng(nb)
    for n_cls in (1, 3, 64):
        cls = rng.integers(-1, n_cls, nb).astype(np.int32)
        for lo, hi in sorted({(1, nb), (1, max(1, nb // 2)), (min(2, nb), nb), (nb, nb), (min(nb, SCAN - 1), nb), (1, min(nb, SCAN + 1))}):
            if 1 <= lo <= hi:
                s, p, c, _ = check(ch, st, cls, n_cls, lo, hi)
                if nb <= 65:
                    assert np.array_equal(p, SC.pairs_by_loop(st["valid"], cls, n_cls, lo, hi))
    ch.close()


# ---- 4. the same bytes, lifetimes, refusals -------------------------------------------------------------------------------------------
def test_the_same_bytes_twice():
    c = CC.planted_case("small")
    ch = chrom(c["X"], c["Y"])
    st = prepare(ch, c["X"], c["Y"], 1000, 2, mask=lambda m: c["mask"], nosmooth=True)
    rng = np.random.default_rng(0)
    cls = rng.integers(-1, 52, st["nb"]).astype(np.int32)
    hi = full_hi(st)
    a = check(ch, st, cls, 52, 2, hi)
    b = check(ch, st, cls, 52, 2, hi)
    ch.sad_free()
    d = check(ch, st, cls, 52, 2, hi)
    ch.close()
    ch2 = chrom(c["X"], c["Y"])
    st2 = prepare(ch2, c["X"], c["Y"], 1000, 2, mask=lambda m: c["mask"], nosmooth=True)
    e = check(ch2, st2, cls, 52, 2, hi)
    ch2.close()
    for other in (b, d, e):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], other[:3]))
    assert a[2].sum() > 10000


def test_lifetimes():
    from cloops_amd import _lib
    E = _lib.CloopsHipError
    X, Y = MC.scattered(5, 3000, 50000, 9000)
    ch = chrom(X, Y)

    def refused(*calls):
        for f in calls:
            with pytest.raises(E):
                f()
    refused(lambda: ch.sad_sums(np.zeros(0, np.int32), 1, 0, 0), ch.sad_get)   # nothing on the handle
    assert ch.sad_free() is None
    st = prepare(ch, X, Y, 500, 2, raw=True)
    nb = st["nb"]
    cls = cycling(nb, 4)
    hi = full_hi(st)
    refused(ch.sad_get)
    want = check(ch, st, cls, 4, 2, hi)[:3]
    same = lambda: all(np.array_equal(x, y) for x, y in zip(ch.sad_get(), want))
    assert same()
    # K27's and K29's state and K30's do not touch each other
    ch.eig_build(5.0, hi)
    ch.eig_iterate(1, max_iters=5)
    v = ch.eig_vectors(0)
    assert same()
    ch.dot_lambdas(1, 3, 4, min(hi, 30))
    assert same()
    ch.eig_free()
    ch.dot_free()
    assert same()
    ch.eig_build(5.0, hi)
    ch.eig_iterate(1, max_iters=5)
    assert np.array_equal(ch.eig_vectors(0), v, equal_nan=True)
    ch.dot_lambdas(1, 3, 4, min(hi, 30))
    la = ch.dot_lambdas_get(0)
    check(ch, st, cycling(nb, 6), 6, 3, hi)
    ch.sad_free()
    refused(ch.sad_get)
    assert np.array_equal(ch.eig_vectors(0), v, equal_nan=True) and np.array_equal(ch.dot_lambdas_get(0), la, equal_nan=True)
    assert len(ch.exp_cells_get()) == len(st["cells"][0])                    # sad_free keeps everything below
    # a refused call leaves the tables
    want = check(ch, st, cls, 4, 2, hi)[:3]
    refused(lambda: ch.sad_sums(cls, 4, 1, hi), lambda: ch.sad_sums(cls, 4, 2, nb + 1), lambda: ch.sad_sums(cls, 4, hi + 1, hi),
            lambda: ch.sad_sums(cls, 4, 2, nb))                              # (the last: the rule on the expected values -- few rows, far diagonals without contacts)
    assert hi < nb and same()
    for bad in (lambda: ch.sad_sums(cls[:-1], 4, 2, hi), lambda: ch.sad_sums(cls, 0, 2, hi), lambda: ch.sad_sums(cls, 65, 2, hi),
                lambda: ch.sad_sums(cls, 3, 2, hi), lambda: ch.sad_sums(cls - 2, 4, 2, hi), lambda: ch.sad_sums(cls.astype(np.float64), 4, 2, hi)):
        with pytest.raises(ValueError):
            bad()
    assert same()
    # every call that drops or rebuilds K24 .. K26 drops K30
    for drop in (lambda: ch.exp_set(st["e"]), lambda: ch.exp_diagonals(balanced=False), lambda: ch.exp_free(), lambda: ch.bal_marginals(2),
                 lambda: ch.bal_free(), lambda: ch.mat_cells(500, fold=True), lambda: ch.mat_free()):
        st = prepare(ch, X, Y, 500, 2, raw=True)
        check(ch, st, cls, 4, 2, hi)
        drop()
        refused(ch.sad_get)
    st = prepare(ch, X, Y, 500, 2, raw=False)
    check(ch, st, cls, 4, 2, full_hi(st))
    s, z = ch.bal_marginals_get()
    ch.bal_iterate(BC.valid_oracle(s, z), max_iters=3)
    refused(ch.sad_get, lambda: ch.sad_sums(cls, 4, 2, hi))
    ch.close()


def test_argument_errors_of_the_c_calls_and_no_bins():
    from cloops_amd import api, _lib, expected as X26, compartments
    lib = _lib.load()
    E = _lib.CL_ERR_ARG
    X, Y = MC.scattered(5, 1000, 50000, 9000)
    ch = api.Chromosome(X, Y)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ref = ctypes.byref
    a, b, c = ctypes.c_int64(7), ctypes.c_int64(7), ctypes.c_int64(7)
    sums, get, free = lib.cl_sad_sums, lib.cl_sad_get, lib.cl_sad_free

    def call(h, cls, count, n_cls, lo, hi, pa=True, pb=True, pc=True):
        a.value = b.value = c.value = 7
        rc = sums(h, None if cls is None else vp(cls), count, n_cls, lo, hi, ref(a) if pa else None, ref(b) if pb else None, ref(c) if pc else None)
        return rc, (a.value if pa else 0, b.value if pb else 0, c.value if pc else 0)
    S, P, C = np.zeros((4, 4)), np.zeros((4, 4), np.int64), np.zeros((4, 4), np.int64)
    k0 = np.zeros(8, np.int32)
    assert call(None, k0, 8, 4, 2, 3) == (E, (0, 0, 0)) and get(None, vp(S), vp(P), vp(C)) == E and free(None) == E
    ch.mat_cells(500, fold=True)
    b0, nb, _ = ch.bal_marginals(2)
    ch.exp_diagonals(balanced=False)
    cls = cycling(nb, 4)
    assert call(ch._h, cls, nb, 4, 2, 3) == (E, (0, 0, 0)) and b"cl_sad_sums" in lib.cl_last_error()          # before cl_exp_set
    assert free(ch._h) == 0
    p, _, vs = ch.exp_diagonals_get()
    e = X26.expected_of(p, vs, 2)[0]
    ch.exp_set(e)
    full = compartments.pick_dmax(p, e, 2)
    assert 10 < full < nb
    assert get(ch._h, vp(S), vp(P), vp(C)) == E                                                               # before cl_sad_sums
    assert call(ch._h, cls, nb, 4, 2, full)[0] == 0 and a.value == nb and b.value > c.value > 0
    assert get(ch._h, vp(S), vp(P), vp(C)) == 0 and P.sum() == b.value and C.sum() == c.value and S.sum() > 0
    keep = (S.copy(), P.copy(), C.copy())
    for pa, pb, pc in ((False, True, True), (True, False, True), (True, True, False)):
        assert call(ch._h, cls, nb, 4, 2, full, pa, pb, pc) == (E, (0, 0, 0))
    bad_hi, bad_lo = cls.copy(), cls.copy()
    bad_hi[nb // 2], bad_lo[nb - 1] = 4, -2
    for args in ((None, nb, 4, 2, full), (cls, nb - 1, 4, 2, full), (cls, nb + 1, 4, 2, full), (cls, nb, 0, 2, full), (cls, nb, 65, 2, full),
                 (cls, nb, -1, 2, full), (cls, nb, 3, 2, full), (bad_hi, nb, 4, 2, full), (bad_lo, nb, 4, 2, full), (cls, nb, 4, 1, full),
                 (cls, nb, 4, 0, full), (cls, nb, 4, -1, full), (cls, nb, 4, 5, 4), (cls, nb, 4, 2, nb + 1), (cls, nb, 4, nb + 1, nb + 1),
                 (cls, nb, 4, 2, nb), (cls, nb, 4, 2, full + 1)):                                             # (the last two: the rule on the expected values)
        assert call(ch._h, *args) == (E, (0, 0, 0)), args[1:]
    assert get(ch._h, None, vp(P), vp(C)) == E and get(ch._h, vp(S), None, vp(C)) == E and get(ch._h, vp(S), vp(P), None) == E
    assert get(ch._h, vp(S), vp(P), vp(C)) == 0 and all(np.array_equal(x, y) for x, y in zip((S, P, C), keep))   # the state is still usable
    for badv in (0.0, -1.0, np.nan, np.inf):
        e2 = e.copy()
        e2[7] = badv
        ch.exp_set(e2)                                                                                        # a second exp_set drops the tables
        assert get(ch._h, vp(S), vp(P), vp(C)) == E
        assert call(ch._h, cls, nb, 4, 2, full) == (E, (0, 0, 0)) and call(ch._h, cls, nb, 4, 2, 8) == (E, (0, 0, 0))
        assert call(ch._h, cls, nb, 4, 2, 7)[0] == 0 and call(ch._h, cls, nb, 4, 8, full)[0] == 0             # beside it the band is fine
    ch.exp_set(e)
    assert call(ch._h, cls, nb, 4, full, full) == (0, (nb, 0, 0)) and get(ch._h, vp(S), vp(P), vp(C)) == 0 and not (S.any() or P.any() or C.any())
    # runs in flight
    assert call(ch._h, cls, nb, 4, 2, full)[0] == 0
    ch.cluster_async("v2", 2000, 5)
    assert call(ch._h, cls, nb, 4, 2, full) == (E, (0, 0, 0)) and get(ch._h, vp(S), vp(P), vp(C)) == E and free(ch._h) == E
    ch.wait()
    assert get(ch._h, vp(S), vp(P), vp(C)) == 0 and all(np.array_equal(x, y) for x, y in zip((S, P, C), keep))
    assert free(ch._h) == 0 and get(ch._h, vp(S), vp(P), vp(C)) == E
    ch.close()
    # no bins
    ch = api.Chromosome(MC.EMPTY, MC.EMPTY)
    assert ch.mat_cells(1000, fold=True)[0] == 0 and ch.bal_marginals(2) == (0, 0, 0) and ch.exp_diagonals(balanced=False) == (0, 0)
    ch.exp_set(np.zeros(0))
    assert ch.sad_sums(np.zeros(0, np.int32), 3, 0, 0) == (0, 0, 0)
    s, p, c2 = ch.sad_get()
    assert s.shape == (3, 3) and not (s.any() or p.any() or c2.any())
    assert call(ch._h, None, 0, 3, 0, 0) == (0, (0, 0, 0)) and call(ch._h, None, 0, 3, 0, 1) == (E, (0, 0, 0)) and call(ch._h, None, 0, 3, 2, 2) == (E, (0, 0, 0))
    ch.close()


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------
def _write_jd(d, name, X, Y, other=None):
    import joblib
    os.makedirs(d, exist_ok=True)
    joblib.dump(np.stack([np.arange(len(X)), X, Y], 1).astype(np.int64), os.path.join(d, "%s-%s.jd" % (name, other or name)))


def _files(prefix, suffixes):
    out = {}
    for suffix in suffixes:
        with open(prefix + suffix) as fh:
            out[suffix] = fh.read()
    return out


def test_the_command_end_to_end(tmp_path):
    """saddle.main -nosmooth -q 10 on a directory of two planted chromosomes and a trans .jd that is left out, the track written from
    the oracle's oriented first vectors, against the host functions on the oracle's stand-in: integer fields and the layout are equal, the sums
    lie within the entries' bounds plus what K25's weights and K26's expected values differ between device and stand-in (both enter a
    term once or twice: measured on the device's own state), the strengths within the sum of those"""
    from cloops_amd import compartments, pipe, saddle
    cases = {"chr2": CC.planted_case("small"), "chr10": CC.planted_case("second")}
    d = os.path.join(str(tmp_path), "jd")
    for name, c in cases.items():
        _write_jd(d, name, c["X"], c["Y"])
    _write_jd(d, "chr2", cases["chr2"]["X"][:500], cases["chr10"]["Y"][:500], other="chr10")
    track = os.path.join(str(tmp_path), "e1.bedGraph")
    with open(track, "w") as fh:
        for n in sorted(cases):
            c = cases[n]
            e1 = c["vectors"][0] * np.sqrt(abs(c["eigvals"][0]))              # scaled as compartments writes it, oriented by the plant
            e1 = -e1 if compartments.pearson(e1, c["comp"].astype(np.float64)) < 0 else e1
            for i in np.flatnonzero(c["valid"]).tolist():
                fh.write("%s\t%d\t%d\t%r\n" % (n, (c["b0"] + i) * 1000, (c["b0"] + i + 1) * 1000, float(e1[i])))
    out = os.path.join(str(tmp_path), "o")
    pipe.CACHE.clear()
    assert saddle.main(["-d", d, "-o", out, "-track", track, "-res", "1000", "-q", "10", "-nosmooth"]) == 0
    pipe.CACHE.clear()
    got = _files(out, saddle.SUFFIXES)
    js = json.loads(got["_saddle.json"])
    assert list(js["chroms"]) == ["chr10", "chr2"] and js["args"]["q"] == 10 and js["args"]["nosmooth"] and js["args"]["track"] == track
    per = saddle.genome_tracks(saddle.read_bedgraph(track), sorted(cases), 1000)
    edges = saddle.edges_of(np.concatenate([per[n] for n in sorted(cases)]), 10)
    want = {n: saddle.saddle_chrom(SC.OracleChrom(c["X"], c["Y"]), n, 1000, per[n], edges, nosmooth=True) for n, c in cases.items()}
    texts, js_want, _ = saddle.saddle_outputs(want, js["args"], edges, 0.2)
    assert js["edges"] == js_want["edges"] and got["_saddle_bins.txt"] == texts["_saddle_bins.txt"]
    rows = [line.split("\t") for line in got["_saddle_sums.txt"].splitlines()]
    want_rows = [line.split("\t") for line in texts["_saddle_sums.txt"].splitlines()]
    assert [r[:3] + r[4:] for r in rows] == [r[:3] + r[4:] for r in want_rows] and len(rows) == 3 * 144
    slack = {}
    for n in sorted(cases):
        c, st, ws = cases[n], js["chroms"][n], js_want["chroms"][n]
        for key in ("b0", "nb", "n_binned", "n_pairs", "n_in", "lo", "hi", "iters", "converged", "var", "scale"):
            assert st[key] == ws[key], (n, key, st[key], ws[key])
        # the device's own weights and expected values: the same calls as the command's
        ch = chrom(c["X"], c["Y"])
        sd = prepare(ch, c["X"], c["Y"], 1000, 2, mask=lambda m: c["mask"], nosmooth=True, bal_iters=200)
        ch.close()
        wd, ed, p = sd["w"], sd["e"], sd["p"]
        ok = c["valid"]
        assert np.array_equal(sd["valid"], ok) and full_hi(sd) == st["hi"]
        mine = per[n][c["b0"]:c["b0"] + c["nb"]]
        cls = saddle.classes_of(np.concatenate([mine, np.full(c["nb"] - len(mine), np.nan)]), ok, edges)
        fed = SC.tables_oracle(sd["cells"], sd["b0"], sd["nb"], 2, ok, wd, ed, cls, 12, st["lo"], st["hi"])
        # how far they lie from the stand-in's: a term holds two weights and one expected value
        band = slice(st["lo"], st["hi"])
        has = np.asarray(p)[band] > 0
        slack[n] = 2 * float(np.max(np.abs(wd[ok] - c["w"][ok]) / c["w"][ok])) + float(np.max(np.abs(ed[band][has] - c["expected"][band][has]) / c["expected"][band][has]))
        mine = [r for r in rows if r[0] == n]
        theirs = want[n]["tables"]
        s = np.array([float(r[3]) for r in mine]).reshape(12, 12)
        allowed = (SC.sum_bound(theirs[2]) + 1.5 * slack[n] + 1e-9) * theirs[0]
        print("K30 end to end %s: strength %s (stand-in %s), weights and expected values within %.3g, largest deviation of a sum over its allowance %.3g"
              % (n, st["strength"], ws["strength"], slack[n], float(np.max(np.abs(s - theirs[0]) / np.maximum(allowed, 1e-300)))))
        assert np.all(np.abs(s - theirs[0]) <= allowed)
        assert np.array_equal(fed[1], theirs[1]) and np.array_equal(fed[2], theirs[2])
        assert np.all(np.abs(s - fed[0]) <= (SC.sum_bound(fed[2]) + 1e-9) * fed[0])      # the oracle fed the device's own state: the bound, and the file's ten digits
        for key in ("strength", "aa_ab", "bb_ab"):
            assert abs(st[key] - ws[key]) <= (4 * (float(SC.sum_bound(theirs[2]).max()) + 1.5 * slack[n]) + 2e-9) * ws[key]
        assert 2.5 < st["strength"] < 3.1
    worst = max(slack.values())
    for key in ("strength", "aa_ab", "bb_ab"):
        assert abs(js["all"][key] - js_want["all"][key]) <= (4 * (float(SC.sum_bound(sum(w["tables"][2] for w in want.values())).max()) + 1.5 * worst) + 2e-9) * js_want["all"][key]
    mat, want_mat = ([line.split("\t") for line in t["_saddle.txt"].splitlines()] for t in (got, texts))
    assert mat[0] == want_mat[0] and [r[0] for r in mat] == [r[0] for r in want_mat]
    a, b = (np.array([[float(x) for x in r[1:]] for r in m[1:]]) for m in (mat, want_mat))
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.allclose(a[~np.isnan(a)], b[~np.isnan(b)], rtol=4 * 1.5 * worst + 1e-8, atol=0)
    # refused before any file is written
    bad = os.path.join(str(tmp_path), "bad")
    for f in (lambda: saddle.jd2saddle(d, bad, track, q=0), lambda: saddle.jd2saddle(d, bad, track, corner=0.0),
              lambda: saddle.jd2saddle(d, bad, bad + ".none"), lambda: saddle.jd2saddle(d, bad, track, chroms={"chr7"})):
        with pytest.raises(ValueError):
            f()
    pipe.CACHE.clear()
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("bad")]
