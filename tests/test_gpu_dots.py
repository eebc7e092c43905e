"""GPU: K29 (cl_dot_lambdas / cl_dot_hist / cl_dot_call and their gets, cloops_amd.dots) against the numpy restatement of
tests/dots_cases.py -- the four la of every pixel within a bound that comes from the number of additions, at the edges of the tiles,
the window, the mask and the diagonal; the histogram and the call exactly, from the device's own la; the same bytes twice; lifetimes,
refusals, and the command end to end."""
import ctypes
import json
import os

import numpy as np
import pytest

import balance_cases as BC
import dots_cases as DC
import matrix_cases as MC

pytestmark = pytest.mark.gpu

CMAX = DC.CMAX


def chrom(X, Y):
    from cloops_amd import api
    return api.Chromosome(np.asarray(X, np.int64), np.asarray(Y, np.int64))


def prepare(ch, X, Y, res, ign, raw=True, mask=None, expected=None, bal_iters=50):
    """cells, marginals, (weights,) diagonals and expected values on the device -> dict(cells, b0, nb, ign, valid, w, e): the DEVICE's
    weights and sums, so that K25's and K26's deviations do not enter"""
    from cloops_amd import expected as X26
    cells = MC.cells_oracle(X, Y, 0, res, True)[:3]
    assert ch.mat_cells(res, fold=True)[0] == len(cells[0])
    b0, nb = BC.span(cells[0], cells[1])
    assert ch.bal_marginals(ign)[:2] == (b0, nb)
    m = np.ones(nb, bool) if mask is None else np.asarray(mask(nb), bool)
    if raw:
        ch.exp_diagonals(valid=m, balanced=False)
        valid, w = m.copy(), np.ones(nb)
    else:
        ch.bal_iterate(m, max_iters=bal_iters)
        w = ch.bal_weights()
        valid = ~np.isnan(w)
        ch.exp_diagonals()
    p, _, vs = ch.exp_diagonals_get()
    e = X26.expected_of(p, vs, ign)[0] if expected is None else expected(nb)
    ch.exp_set(e)
    return dict(cells=cells, b0=b0, nb=nb, ign=ign, valid=valid, w=w, e=e)


def on_device(name):
    c = DC.LA_CASES[name]
    X, Y = DC.case_rows(name)
    ch = chrom(X, Y)
    st = prepare(ch, X, Y, 1, c["ign"], raw=c["raw"], mask=c["mask"], expected=c["expected"])
    assert st["nb"] == c["nb"] and st["b0"] == c.get("shift", 0)
    return ch, st, c


def device_la(ch):
    return np.stack([ch.dot_lambdas_get(k) for k in range(4)])


def want_la(st, p, w, dmin, dmax):
    return DC.lambdas_oracle(st["cells"], st["b0"], st["nb"], st["ign"], st["valid"], st["w"], st["e"], p, w, dmin, dmax)


def close(got, want, w):
    """NaN at the same places, and the numbers within the bound of the additions"""
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    dev = np.abs(got[ok] - want[ok])
    lim = DC.rtol(w) * np.abs(want[ok])
    worst = float(np.max(dev[lim > 0] / lim[lim > 0])) if (lim > 0).any() else 0.0
    assert np.all(dev <= lim), worst
    return worst


# ---- 1. la ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DC.LA_CASES))
def test_la_against_the_restatement(name):
    ch, st, c = on_device(name)
    p, w, dmin, dmax = c["p"], c["w"], c["dmin"], c["dmin"] + c["nd"]
    n_cand, n_full = ch.dot_lambdas(p, w, dmin, dmax)
    want, wc, wf = want_la(st, p, w, dmin, dmax)
    got = device_la(ch)
    worst = close(got, want, w)
    print("K29 la %s: largest deviation over its bound %.3g; %d candidates, %d full" % (name, worst, n_cand, n_full))
    assert (n_cand, n_full) == (wc, wf)
    if c["nb"] > 2:
        assert wf > 0
    # a range of bins, and the gather of the cells
    lo, n = c["nb"] // 3, max(1, c["nb"] // 2)
    assert np.array_equal(ch.dot_lambdas_get(2, lo, n), got[2, lo:lo + n], equal_nan=True)
    cells = st["cells"]
    g = ch.dot_cells()
    assert g.shape == (len(cells[0]), 4) and np.array_equal(g, DC.cells_la(cells, st["b0"], st["nb"], dmin, dmax, got), equal_nan=True)
    k = len(cells[0]) // 2
    m = min(5, len(cells[0]) - k)
    assert np.array_equal(ch.dot_cells(k, m), g[k:k + m], equal_nan=True)
    # the same bytes twice
    assert ch.dot_lambdas(p, w, dmin, dmax) == (n_cand, n_full) and device_la(ch).tobytes() == got.tobytes()
    ch.close()


def test_every_pair_of_p_and_w_on_one_sample():
    ch, st, c = on_device("nd31_neg")
    for p, w in ((0, 1), (1, 3), (2, 5), (4, 7), (0, 16), (15, 16)):
        dmin, dmax = max(st["ign"], 1), 40
        ch.dot_lambdas(p, w, dmin, dmax)
        close(device_la(ch), want_la(st, p, w, dmin, dmax)[0], w)
    ch.close()


def test_an_empty_sample():
    ch = chrom(np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert ch.mat_cells(1000, fold=True)[0] == 0 and ch.bal_marginals(2)[:2] == (0, 0)
    assert ch.exp_diagonals(balanced=False) == (0, 0)
    ch.exp_set(np.zeros(0))
    assert ch.dot_lambdas(2, 5, 0, 0) == (0, 0)
    assert ch.dot_lambdas_get(0).shape == (0, 0) and ch.dot_cells().shape == (0, 4)
    hist, nbey = ch.dot_hist([1.0, 2.0])
    assert hist.shape == (4, 2, CMAX + 1) and not hist.any() and nbey == 0
    assert ch.dot_call(np.zeros((4, 2), np.uint32)) == 0 and len(ch.dot_sig()) == 0
    ch.dot_free()
    ch.close()


# ---- 2. histogram and call, exactly, from the device's own la ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def heavy():
    """the case nd31_neg with one cell of more than CMAX rows, on the device with its la -> (ch, st, la, counts, dmin, dmax)"""
    c = DC.LA_CASES["nd31_neg"]
    X, Y = DC.case_rows("nd31_neg")
    X, Y = np.concatenate([X, np.full(CMAX + 905, 11 - 40)]), np.concatenate([Y, np.full(CMAX + 905, 23 - 40)])
    ch = chrom(X, Y)
    st = prepare(ch, X, Y, 1, c["ign"], mask=DC.sparse_mask)
    dmin, dmax = 4, 4 + 31
    ch.dot_lambdas(c["p"], c["w"], dmin, dmax)
    la = device_la(ch)
    counts = DC.count_plane(st["cells"], st["b0"], st["nb"], dmin, dmax)
    assert counts.max() > CMAX
    yield ch, st, la, counts, dmin, dmax
    ch.close()


def edges_of(la, kind):
    v = np.unique(la[~np.isnan(la)])
    v = v[v > 0]
    if kind == "coincide":                                                  # values that occur are edges; the largest la lies inside
        return np.unique(np.concatenate([v[::max(1, len(v) // 20)][:20], v[-1:]]))
    if kind == "single":
        return v[len(v) // 2: len(v) // 2 + 1]
    if kind == "64":
        return np.unique(np.quantile(v, np.linspace(0.01, 0.9, 64)))
    return np.array([2.0 ** (l / 3.0) for l in range(6)])                   # "default": a few of the command's edges


@pytest.mark.parametrize("kind", ["coincide", "single", "64", "default"])
def test_histogram_is_numpys_binning_of_the_devices_la(heavy, kind):
    ch, st, la, counts, dmin, dmax = heavy
    edges = edges_of(la, kind)
    assert {"single": 1, "64": 64}.get(kind, len(edges)) == len(edges)
    hist, nbey = ch.dot_hist(edges)
    want, wbey = DC.hist_oracle(la, counts, edges)
    assert np.array_equal(hist, want) and nbey == wbey
    full = int((~np.isnan(la).any(axis=0)).sum())
    assert all(int(hist[k].sum()) == full - nbey for k in range(4))         # no pixel is left out but the beyond ones
    assert hist[:, :, 0].sum() > 0 and hist[:, :, 1:].sum() > 0
    if kind == "coincide":
        assert nbey == 0 and hist[:, :, CMAX].sum() == 4                    # the heavy cell, once per kernel
    else:
        assert nbey > 0
    hist2, nbey2 = ch.dot_hist(edges)
    assert hist2.tobytes() == hist.tobytes() and nbey2 == nbey


def test_histogram_over_several_workgroups():
    """24 000 pixels: more than the 16 384 of one workgroup of the histogram pass, most of them with a cell"""
    X, Y = DC.band_rows(600, 50, 40000, 12)
    X, Y = np.concatenate([X, np.full(20, 100), np.full(30, 300)]), np.concatenate([Y, np.full(20, 110), np.full(30, 305)])
    ch = chrom(X, Y)
    st = prepare(ch, X, Y, 1, 2)
    dmin, dmax = 2, 42
    assert st["nb"] * (dmax - dmin) > 16384
    ch.dot_lambdas(1, 3, dmin, dmax)
    la = device_la(ch)
    counts = DC.count_plane(st["cells"], st["b0"], st["nb"], dmin, dmax)
    edges = np.array([2.0 ** (l / 3.0) for l in range(4)])
    hist, nbey = ch.dot_hist(edges)
    want, wbey = DC.hist_oracle(la, counts, edges)
    assert np.array_equal(hist, want) and nbey == wbey and nbey > 0
    assert hist[:, :, 0].sum() > 0 and hist[:, :, 1:16].sum() > 0 and hist[:, :, 16:].sum() > 0    # counts on both sides of the LDS counters' reach
    ch.close()


@pytest.mark.parametrize("kind", ["coincide", "64", "default"])
def test_call_is_numpys_from_the_devices_la(heavy, kind):
    ch, st, la, counts, dmin, dmax = heavy
    edges = edges_of(la, kind)
    ch.dot_hist(edges)
    la4 = ch.dot_cells()
    n = len(st["cells"][0])
    rng = np.random.default_rng(7)
    some = None
    for thr in (np.zeros((4, len(edges))), np.full((4, len(edges)), DC.NO_THRESHOLD), rng.integers(0, 4, (4, len(edges))),
                rng.integers(0, 3, (4, len(edges))) * 2):
        thr = thr.astype(np.uint32)
        n_sig = ch.dot_call(thr)
        sig = ch.dot_sig()
        want = DC.call_oracle(st["cells"], la4, edges, thr)
        assert n_sig == len(want) and np.array_equal(sig, want) and np.all(np.diff(sig) > 0)
        if n_sig > 3:
            assert np.array_equal(ch.dot_sig(1, 2), sig[1:3])
        if thr.max() == DC.NO_THRESHOLD:
            assert n_sig == 0
        elif thr.max() == 0:
            some = n_sig
            assert 0 < n_sig < n                                            # (masked bins, cells outside the diagonals)
        else:
            assert 0 < n_sig <= some
    assert ch.dot_call(thr) == n_sig and np.array_equal(ch.dot_sig(), sig)   # the same list twice


def test_call_takes_every_cell():
    """all bins valid, every diagonal tested, every la inside the edges, thresholds of 0: every cell is significant"""
    rng = np.random.default_rng(3)
    X = np.concatenate([[0], rng.integers(0, 64, 1500)])
    Y = np.concatenate([[64], np.minimum(X[1:] + 1 + rng.integers(0, 64, 1500), 64)])       # no cell on the main diagonal
    ch = chrom(X, Y)
    st = prepare(ch, X, Y, 1, 0, expected=DC.line_expected)
    assert ch.dot_lambdas(0, 1, 1, 65) == (65 * 64 // 2, 65 * 64 // 2)
    la = device_la(ch)
    edges = np.array([float(np.nanmax(la))])
    hist, nbey = ch.dot_hist(edges)
    assert nbey == 0 and int(hist[0].sum()) == 65 * 64 // 2
    n = len(st["cells"][0])
    assert ch.dot_call(np.zeros((4, 1), np.uint32)) == n and np.array_equal(ch.dot_sig(), np.arange(n))
    ch.close()


# ---- 3. lifetimes and refusals ----------------------------------------------------------------------------------------------------
def test_lifetimes():
    from cloops_amd import _lib
    X, Y = DC.case_rows("nd1")
    ch = chrom(X, Y)
    st = prepare(ch, X, Y, 1, 2)
    edges, thr = np.array([1.0, 4.0, 64.0]), np.ones((4, 3), np.uint32)

    def build():
        ch.dot_lambdas(2, 5, 4, 40)
        ch.dot_hist(edges)
        return ch.dot_call(thr)

    def refused(*calls):
        for f in calls:
            with pytest.raises(_lib.CloopsHipError) as ei:
                f()
            assert ei.value.code == _lib.CL_ERR_ARG

    users = (lambda: ch.dot_lambdas_get(0), lambda: ch.dot_cells(0, 1), lambda: ch.dot_hist(edges), lambda: ch.dot_call(thr),
             lambda: ch.dot_sig(0, 0))
    n_sig = build()
    assert n_sig > 0
    # K27's state survives cl_dot_free, and K29's survives cl_eig_free
    ch.eig_build(2.0, 10)
    y = ch.eig_apply(np.ones(st["nb"]))
    ch.dot_free()
    refused(*users)
    assert np.array_equal(ch.eig_apply(np.ones(st["nb"])), y)
    assert build() == n_sig
    ch.eig_free()
    assert len(ch.dot_sig()) == n_sig
    # a new histogram drops the call, new lambdas drop the histogram
    ch.dot_hist(edges)
    refused(lambda: ch.dot_sig(0, 0))
    ch.dot_lambdas(2, 5, 4, 40)
    refused(lambda: ch.dot_call(thr), lambda: ch.dot_sig(0, 0))
    # every call that drops or rebuilds K26's state drops K29's
    for drop in (lambda: ch.exp_set(st["e"]), lambda: ch.exp_diagonals(balanced=False), lambda: ch.exp_free(), lambda: ch.bal_marginals(2),
                 lambda: ch.bal_free(), lambda: ch.mat_cells(1, fold=True), lambda: ch.mat_free()):
        if not getattr(ch, "_mat_cells", 0):
            ch.mat_cells(1, fold=True)
        if not getattr(ch, "_bal_bins", 0):
            ch.bal_marginals(2)
        if not getattr(ch, "_exp_diags", 0):
            ch.exp_diagonals(balanced=False)
        ch.exp_set(st["e"])
        assert build() == n_sig
        drop()
        refused(*users)
    ch.close()


def test_argument_errors_of_the_c_calls():
    from cloops_amd import api, _lib
    lib = _lib.load()
    E = _lib.CL_ERR_ARG
    X, Y = DC.case_rows("nd1")
    ch = api.Chromosome(X, Y)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ref = ctypes.byref
    a, b = ctypes.c_int64(7), ctypes.c_int64(7)
    u = ctypes.c_uint64(7)
    lam, lget, cget, hist, call, sget, free = (lib.cl_dot_lambdas, lib.cl_dot_lambdas_get, lib.cl_dot_cells_get, lib.cl_dot_hist, lib.cl_dot_call,
                                               lib.cl_dot_sig_get, lib.cl_dot_free)
    edges, thr = np.array([1.0, 4.0, 64.0]), np.ones((4, 3), np.uint32)
    H, d8, i8 = np.zeros((4, 3, CMAX + 1), np.uint64), np.zeros(4096, np.float64), np.zeros(8, np.int64)
    # a NULL handle
    assert lam(None, 2, 5, 4, 40, ref(a), ref(b)) == E and (a.value, b.value) == (0, 0)
    assert lget(None, 0, 0, 1, vp(d8)) == E and cget(None, 0, 1, vp(d8)) == E and hist(None, vp(edges), 3, vp(H), ref(u)) == E and u.value == 0
    assert call(None, vp(thr), ref(a)) == E and sget(None, 0, 0, vp(i8)) == E and free(None) == E
    # before cl_exp_set
    ch.mat_cells(1, fold=True)
    b0, nb, _ = ch.bal_marginals(2)
    ch.exp_diagonals(balanced=False)
    a.value = b.value = 7
    assert lam(ch._h, 2, 5, 4, 40, ref(a), ref(b)) == E and (a.value, b.value) == (0, 0) and b"cl_dot_lambdas" in lib.cl_last_error()
    assert free(ch._h) == 0
    e = np.linspace(2.0, 0.5, nb)
    ch.exp_set(e)
    # before cl_dot_lambdas
    u.value = 7
    assert lget(ch._h, 0, 0, 1, vp(d8)) == E and cget(ch._h, 0, 1, vp(d8)) == E and hist(ch._h, vp(edges), 3, vp(H), ref(u)) == E and u.value == 0
    assert call(ch._h, vp(thr), ref(a)) == E and sget(ch._h, 0, 0, vp(i8)) == E
    # p, w, dmin, dmax, NULL outputs, the band limit
    assert lam(ch._h, 2, 5, 4, 40, None, ref(b)) == E and lam(ch._h, 2, 5, 4, 40, ref(a), None) == E
    for p, w, dmin, dmax in ((-1, 5, 4, 40), (5, 5, 4, 40), (6, 5, 4, 40), (2, 17, 4, 40), (16, 17, 4, 40), (2, 5, 1, 40), (2, 5, -1, 40),
                             (2, 5, 40, 40), (2, 5, 41, 40), (2, 5, 4, nb + 1), (2, 5, 0, 0)):
        a.value = b.value = 7
        assert lam(ch._h, p, w, dmin, dmax, ref(a), ref(b)) == E and (a.value, b.value) == (0, 0), (p, w, dmin, dmax)
    # the rule on the expected values: NaN, infinite or negative on a diagonal of the band with valid pairs; zero is allowed, and so is
    # anything below ign or at and beyond dmax + 2w
    for at, bad in ((4, np.nan), (30, np.inf), (49, -1.0)):
        f = e.copy()
        f[at] = bad
        ch.exp_set(f)
        assert lam(ch._h, 2, 5, 4, 40, ref(a), ref(b)) == E and (a.value, b.value) == (0, 0) and b"expected" in lib.cl_last_error()
    f = e.copy()
    f[:2] = np.nan
    f[50:] = np.nan
    f[7] = 0.0
    ch.exp_set(f)
    assert lam(ch._h, 2, 5, 4, 40, ref(a), ref(b)) == 0 and a.value > 0 and 0 < b.value <= a.value
    n_cand = a.value
    # a refused call leaves the earlier state usable
    assert lam(ch._h, 5, 5, 4, 40, ref(a), ref(b)) == E and lget(ch._h, 0, 0, 1, vp(d8)) == 0
    # the gets: kernel index, ranges, NULL arrays
    n = ch._mat_cells
    assert lget(ch._h, 4, 0, 1, vp(d8)) == E and lget(ch._h, -1, 0, 1, vp(d8)) == E and lget(ch._h, 0, nb - 1, 2, vp(d8)) == E
    assert lget(ch._h, 0, -1, 1, vp(d8)) == E and lget(ch._h, 0, 0, 1, None) == E and lget(ch._h, 3, nb, 0, None) == 0
    assert cget(ch._h, n - 1, 2, vp(d8)) == E and cget(ch._h, -1, 1, vp(d8)) == E and cget(ch._h, 0, 1, None) == E and cget(ch._h, n, 0, None) == 0
    # cl_dot_call before cl_dot_hist; the edges
    assert call(ch._h, vp(thr), ref(a)) == E
    for bad in ([1.0, 1.0, 2.0], [2.0, 1.0, 3.0], [0.0, 1.0, 2.0], [-1.0, 1.0, 2.0], [1.0, np.nan, 2.0], [1.0, 2.0, np.inf]):
        u.value = 7
        assert hist(ch._h, vp(np.array(bad)), 3, vp(H), ref(u)) == E and u.value == 0, bad
    assert hist(ch._h, vp(edges), 0, vp(H), ref(u)) == E and hist(ch._h, vp(np.arange(1.0, 66.0)), 65, vp(H), ref(u)) == E
    assert hist(ch._h, None, 3, vp(H), ref(u)) == E and hist(ch._h, vp(edges), 3, None, ref(u)) == E and hist(ch._h, vp(edges), 3, vp(H), None) == E
    assert hist(ch._h, vp(edges), 3, vp(H), ref(u)) == 0 and H.sum() > 0
    # cl_dot_sig_get before cl_dot_call; NULL arguments; ranges
    assert sget(ch._h, 0, 0, vp(i8)) == E
    assert call(ch._h, None, ref(a)) == E and call(ch._h, vp(thr), None) == E
    a.value = 7
    assert call(ch._h, vp(thr), ref(a)) == 0 and a.value > 2
    ns = a.value
    assert sget(ch._h, ns - 1, 2, vp(i8)) == E and sget(ch._h, -1, 1, vp(i8)) == E and sget(ch._h, 0, 1, None) == E
    assert sget(ch._h, ns - 2, 2, vp(i8)) == 0 and sget(ch._h, ns, 0, None) == 0
    # runs in flight
    sig = ch.dot_sig()
    ch.cluster_async("v2", 20, 5)
    assert lam(ch._h, 2, 5, 4, 40, ref(a), ref(b)) == E and lget(ch._h, 0, 0, 1, vp(d8)) == E and cget(ch._h, 0, 1, vp(d8)) == E
    assert hist(ch._h, vp(edges), 3, vp(H), ref(u)) == E and call(ch._h, vp(thr), ref(a)) == E and sget(ch._h, 0, 1, vp(i8)) == E and free(ch._h) == E
    ch.wait()
    assert np.array_equal(ch.dot_sig(), sig)                                # the handle still works
    assert lam(ch._h, 2, 5, 4, 40, ref(a), ref(b)) == 0 and a.value == n_cand
    assert free(ch._h) == 0 and lget(ch._h, 0, 0, 1, vp(d8)) == E
    ch.close()


def test_the_band_limit():
    """three million bins: nb (dmax + 4 w) passes CL_DOT_BAND_MAX at dmax = 40, w = 5, and the call is refused before any allocation"""
    from cloops_amd import _lib
    lib = _lib.load()
    ch = chrom(np.array([0, 5, 3000000]), np.array([3, 9, 3000000]))
    ch.mat_cells(1, fold=True)
    b0, nb, _ = ch.bal_marginals(2)
    assert nb == 3000001 and nb * (40 + 20) > _lib.CL_DOT_BAND_MAX
    ch.exp_diagonals(balanced=False)
    ch.exp_set(np.ones(nb))
    a, b = ctypes.c_int64(7), ctypes.c_int64(7)
    assert lib.cl_dot_lambdas(ch._h, 2, 5, 4, 40, ctypes.byref(a), ctypes.byref(b)) == _lib.CL_ERR_ARG and (a.value, b.value) == (0, 0)
    assert b"band" in lib.cl_last_error()
    with pytest.raises(ValueError):
        ch.dot_lambdas(2, 5, 4, 40)
    ch.close()


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------
def _write_jd(d, name, X, Y):
    import joblib
    os.makedirs(d, exist_ok=True)
    joblib.dump(np.stack([np.arange(len(X)), X, Y], 1).astype(np.int64), os.path.join(d, "%s-%s.jd" % (name, name)))


RECOVERY = ["-res", "1000", "-raw", "-nosmooth", "-ignorediags", "2", "-p", "2", "-w", "5", "-maxdist", "199000", "-fdr", "0.1", "-mad", "0"]


def test_the_command_end_to_end_recovers_the_planted_loops(tmp_path):
    """dots.main on a directory with the recovery sample and its null twin: every planted pair is called at its bins, nothing else is,
    the null sample yields none; the files are what the host functions make of the restatement's stand-in (raw mode: the terms are
    integers and the expected values their quotients, the la of a significant pixel differs in its last bits at most, so the texts are
    compared field by field: integers exactly, la within the bound of the additions)"""
    from cloops_amd import dots, pipe
    d = os.path.join(str(tmp_path), "jd")
    rows = {"chr1": DC.recovery_rows(DC.RECOVERY_SEED, True), "chr2": DC.recovery_rows(DC.RECOVERY_SEED, False)}
    for name, (X, Y) in rows.items():
        _write_jd(d, name, X, Y)
    out = os.path.join(str(tmp_path), "o")
    pipe.CACHE.clear()
    assert dots.main(["-d", d, "-o", out] + RECOVERY) == 0
    pipe.CACHE.clear()
    got = {}
    for sfx in dots.SUFFIXES:
        with open(out + sfx) as fh:
            got[sfx] = fh.read()
    js = json.loads(got["_dots.json"])
    assert list(js["chroms"]) == ["chr1", "chr2"] and js["args"]["w"] == 5 and js["args"]["raw"] and js["warnings"] == []
    loops = [line.split("\t") for line in got["_dots.bedpe"].splitlines()]
    assert sorted((int(r[1]) // 1000, int(r[4]) // 1000) for r in loops) == sorted(DC.PLANTED) and all(r[0] == "chr1" for r in loops)
    assert js["chroms"]["chr1"]["n_loops"] == len(DC.PLANTED) and js["chroms"]["chr2"]["n_sig"] == 0 and js["chroms"]["chr2"]["n_loops"] == 0
    per = {n: dots.dots_chrom(DC.OracleChrom(X, Y), n, 1000, p=2, w=5, maxdist=199000, fdr=0.1, raw=True, nosmooth=True, ignore_diags=2, mad_max=0)
           for n, (X, Y) in rows.items()}
    texts, js_o = dots.dots_outputs(per, js["args"])
    assert js_o == js and got["_dots_thresholds.txt"] == texts["_dots_thresholds.txt"]
    for sfx, first, last in (("_dots.bedpe", 7, 11), ("_dots_pixels.txt", 7, 11)):
        mine, want = [l.split("\t") for l in got[sfx].splitlines()], [l.split("\t") for l in texts[sfx].splitlines()]
        assert len(mine) == len(want) > 0
        for r, q in zip(mine, want):
            assert r[:first] == q[:first] and r[last:] == q[last:]
            assert all(abs(float(x) - float(y)) <= DC.rtol(5) * abs(float(y)) for x, y in zip(r[first:last], q[first:last]))
    # refused before any file is written
    bad = os.path.join(str(tmp_path), "bad")
    for f in (lambda: dots.jd2dots(d, bad, p=5, w=5), lambda: dots.jd2dots(d, bad, w=17), lambda: dots.jd2dots(d, bad, fdr=0.0),
              lambda: dots.jd2dots(d, bad, chunks=65), lambda: dots.jd2dots(d, bad, enrich="1,2,3")):
        with pytest.raises(ValueError):
            f()
    pipe.CACHE.clear()
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("bad")]
