"""GPU: K28 (cl_scc_moments / cl_scc_free, cloops_amd.similarity) against the numpy restatement of tests/similarity_cases.py -- every
moment array EQUAL (the device computes integers only), at the edges of the kernel's tiles in both directions and of the box, on windows
that cut the data, negative bins, gaps, squares beyond 2^32, empty samples and a sample against itself; the same bytes twice; the
scratch's lifetime; every refusal of the C call; and the command end to end."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import balance_cases as BC
import matrix_cases as MC
import similarity_cases as SC

pytestmark = pytest.mark.gpu

NAMES = ("n", "sx", "sy", "sxx", "syy", "sxy")


def chrom(X, Y):
    from cloops_amd import api
    return api.Chromosome(np.asarray(X, np.int64), np.asarray(Y, np.int64))


def with_cells(X, Y, res, cut=0):
    """a handle with its folded cells, and the oracle's cells"""
    ch = chrom(X, Y)
    cells = MC.cells_oracle(X, Y, cut, res, True)
    assert ch.mat_cells(res, cut=cut, fold=True)[:2] == (len(cells[0]), cells[3])
    return ch, cells


def check(cha, chb, ca, cb, b0, nb, h, D):
    """scc_moments == the restatement, array by array -> the device's arrays"""
    got = cha.scc_moments(chb, b0, nb, h=h, n_diags=D)
    want = SC.as_arrays(SC.moments_oracle(ca, cb, b0, nb, h, D))
    assert [a.dtype for a in got] == [np.int64] + [np.uint64] * 5 and all(len(a) == D for a in got)
    for name, g, w in zip(NAMES, got, want):
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (name, b0, nb, h, D, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])
    return got


# ---- 1. every moment equal to the restatement's -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", SC.SIZES)
def test_moments_at_the_tile_edges(nb):
    """windows of 1 .. three tiles + 1 bins, 1 .. nb diagonals (the same edges in the tiles' other direction), every class of h
    including h >= nb and 2h >= D; the rows reach beyond the window on both sides"""
    Xa, Ya = SC.sized(nb, nb)
    Xb, Yb = SC.sized(nb, nb + 100)
    cha, ca = with_cells(Xa, Ya, 1)
    chb, cb = with_cells(Xb, Yb, 1)
    some = False
    for D in sorted({d for d in (1,) + SC.SIZES + (nb,) if d <= nb}):
        for h in SC.HS:
            got = check(cha, chb, ca, cb, 0, nb, h, D)
            some = some or bool(got[5].any())
    assert some or nb == 1
    cha.close()
    chb.close()


def test_a_window_that_cuts_through_the_data():
    Xa, Ya, Xb, Yb, res, b0, nb = SC.cut_window()
    cha, ca = with_cells(Xa, Ya, res)
    chb, cb = with_cells(Xb, Yb, res)
    for h, D in ((0, nb), (1, 40), (3, nb), (20, 33)):
        got = check(cha, chb, ca, cb, b0, nb, h, D)
        assert got[0][0] > 10 and got[5].any()
    check(cha, chb, ca, cb, b0 - 40, nb + 80, 2, 50)                          # ... and one that holds all of it, from a negative bin on
    cha.close()
    chb.close()


def test_negative_bins():
    Xa, Ya = MC.scattered(4, 3000, 60000, 9000, both=True)
    Xb, Yb = MC.scattered(5, 3000, 60000, 9000, both=True)
    cha, ca = with_cells(Xa - 30000, Ya - 30000, 333)
    chb, cb = with_cells(Xb - 30000, Yb - 30000, 333)
    b0, nb = SC.span_of(ca, cb)
    assert b0 < 0 < b0 + nb
    for h, D in ((0, 30), (2, nb), (5, 64)):
        assert check(cha, chb, ca, cb, b0, nb, h, D)[5].any()
    cha.close()
    chb.close()


def test_a_gap_wider_than_a_tile():
    X, Y = SC.gapped()
    cha, ca = with_cells(X, Y, 1)
    chb, cb = with_cells(X[::2], Y[::2] + 1, 1)
    b0, nb = SC.span_of(ca, cb)
    for h in (0, 1, 4, 20):
        got = check(cha, chb, ca, cb, b0, nb, h, nb)
        if h <= 4:
            # rows inside a cluster span at most 6 bins, the bridging ones at least 2 TILE_I + 1: with the boxes' 2h the strata between are empty
            assert got[0][:7].all() and not got[0][16:2 * SC.TILE_I - 8].any() and got[0][2 * SC.TILE_I:].any()
    cha.close()
    chb.close()


def test_squares_beyond_32_bits():
    cha, ca = with_cells(*SC.heavy(1), 1)
    chb, cb = with_cells(*SC.heavy(2), 1)
    for h in (0, 1, 3):
        got = check(cha, chb, ca, cb, 0, 40, h, 10)
        assert int(got[3].max()) > 1 << 32 and int(got[5].max()) > 1 << 32
    cha.close()
    chb.close()


def test_empty_samples_and_a_sample_against_itself():
    (Xa, Ya), _ = SC.general()
    cha, ca = with_cells(Xa, Ya, 1000)
    b0, nb = SC.span_of(ca)
    empty = MC.cells_oracle(MC.EMPTY, MC.EMPTY, 0, 1000, True)
    for X, Y, cut in ((MC.EMPTY, MC.EMPTY, 0), ([500, 90], [700, 95], 1 << 20)):            # no rows; a cut that removes every row
        che = chrom(X, Y)
        assert che.mat_cells(1000, cut=cut, fold=True)[0] == 0
        got = check(cha, che, ca, empty, b0, nb, 1, 40)
        assert got[0][0] > 0 and not got[2].any() and not got[4].any() and not got[5].any() and got[1].any()
        got = check(che, cha, empty, ca, b0, nb, 1, 40)
        assert not got[1].any() and got[2].any()
        got = check(che, che, empty, empty, b0, nb, 2, 40)
        assert not any(a.any() for a in got)
        che2 = chrom(MC.EMPTY, MC.EMPTY)
        che2.mat_cells(1000, fold=True)
        assert not any(a.any() for a in check(che, che2, empty, empty, 0, 5, 0, 5))
        che2.close()
        che.close()
    for h in (0, 3):
        got = check(cha, cha, ca, ca, b0, nb, h, 40)                         # a is b
        assert np.array_equal(got[1], got[2]) and np.array_equal(got[3], got[4]) and np.array_equal(got[3], got[5])
    cha.close()


def test_different_cuts_and_the_general_case():
    (Xa, Ya), (Xb, Yb) = SC.general()
    cha, ca = with_cells(Xa, Ya, 1000)
    chb, cb = with_cells(Xb, Yb, 1000, cut=9000)
    assert len(cb[0]) < len(MC.cells_oracle(Xb, Yb, 0, 1000, True)[0])
    b0, nb = SC.span_of(ca, cb)
    assert nb > 9 * SC.TILE_I
    for h, D in ((0, 50), (1, 50), (3, 50), (20, 45), (2, nb)):
        got = check(cha, chb, ca, cb, b0, nb, h, D)
        assert got[5].any() and (h > 0 or not got[2][:9].any())              # b has no cell nearer than its cut
    from cloops_amd import similarity
    dev = similarity.combine(cha.scc_moments(chb, b0, nb, h=1, n_diags=50))
    want = SC.scc_oracle(SC.moments_oracle(ca, cb, b0, nb, 1, 50))
    assert abs(dev["scc"] - want["scc"]) <= 1e-12 and abs(dev["pcc"] - want["pcc"]) <= 1e-12 and dev["pixels"] == want["pixels"]
    cha.close()
    chb.close()


# ---- 2. determinism --------------------------------------------------------------------------------------------------------------
def test_the_same_bytes_twice():
    (Xa, Ya), (Xb, Yb) = SC.general()
    cha, ca = with_cells(Xa, Ya, 1000)
    chb, cb = with_cells(Xb, Yb, 1000)
    b0, nb = SC.span_of(ca, cb)

    def once():
        return tuple(a.tobytes() for a in cha.scc_moments(chb, b0, nb, h=3, n_diags=60))
    first = once()
    assert np.frombuffer(first[5], np.uint64).any() and once() == first
    cha.scc_free()
    assert once() == first
    cha.agg_loops([20000], [25000], 1000, 10, 3, cut=4000)                   # rebuilds the shared table at another cut: the cells are copies
    chb.agg_loops([20000], [25000], 1000, 10, 3, cut=7000)
    assert once() == first
    assert cha.mat_cells(1000, fold=True)[0] == len(ca[0]) and chb.mat_cells(1000, fold=True)[0] == len(cb[0])      # a rebuild
    assert once() == first
    cha.close()
    chb.close()


# ---- 3. lifetimes ------------------------------------------------------------------------------------------------------------------
def device_free_bytes():
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_the_scratch_is_reused_and_released():
    """a smaller and a larger window after the first; the four releasing calls give the device its memory back: two band arrays of
    256 MiB each are held after a call with 8192 bins x 8192 diagonals, far more than anything else the handles own"""
    (Xa, Ya), (Xb, Yb) = SC.general()
    cha, ca = with_cells(Xa, Ya, 1000)
    chb, cb = with_cells(Xb, Yb, 1000)
    b0, nb = SC.span_of(ca, cb)
    first = check(cha, chb, ca, cb, b0, nb, 2, 50)
    check(cha, chb, ca, cb, b0 + 40, 70, 1, 20)                              # smaller: the scratch of the first call, partly stale, is reused
    check(cha, chb, ca, cb, b0 - 50, nb + 100, 4, 90)                        # larger
    again = check(cha, chb, ca, cb, b0, nb, 2, 50)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    BIG, HALF = 8192, 1 << 28                                                # the scratch is two arrays of BIG * BIG * 4 = HALF bytes

    def big():
        before = device_free_bytes()
        got = cha.scc_moments(chb, b0, BIG, h=0, n_diags=BIG)
        assert before - device_free_bytes() >= HALF
        return got

    def released(call):
        before = device_free_bytes()
        call()
        assert device_free_bytes() - before >= HALF
    want = SC.as_arrays(SC.moments_oracle(ca, cb, b0, nb, 0, nb))
    got = big()
    assert all(np.array_equal(g[:nb], w) and not g[nb:].any() for g, w in zip(got, want))
    released(cha.scc_free)
    cha.scc_free()                                                           # twice is no error
    big()
    released(lambda: cha.mat_cells(1000, fold=True))
    big()
    released(cha.mat_free)
    cha.mat_cells(1000, fold=True)
    big()
    before = device_free_bytes()
    cha.close()
    assert device_free_bytes() - before >= HALF
    # nothing was kept on b: its scc_free and mat_free give back less than a band array
    before = device_free_bytes()
    chb.scc_free()
    assert abs(device_free_bytes() - before) < HALF
    chb.close()


def test_k25_to_k27_results_survive_a_call():
    (Xa, Ya), (Xb, Yb) = SC.general()
    cha, ca = with_cells(Xa, Ya, 1000)
    chb, cb = with_cells(Xb, Yb, 1000)

    def chain(ch):
        b0, nb, _ = ch.bal_marginals(2)
        s, z = ch.bal_marginals_get()
        ch.bal_iterate(BC.valid_oracle(s, z), max_iters=50)
        ch.exp_diagonals()
        p, c, v = ch.exp_diagonals_get()
        e = np.full(nb, np.nan)
        e[p > 0] = v[p > 0] / p[p > 0]
        e[e == 0] = np.nan
        ch.exp_set(e)
        from cloops_amd.compartments import pick_dmax
        ch.eig_build(float("inf"), pick_dmax(p, e, 2))
        ch.eig_iterate(2, max_iters=20)

    def state(ch):
        return (tuple(a.tobytes() for a in ch.mat_cells_get()), ch.bal_weights().tobytes(), tuple(a.tobytes() for a in ch.bal_marginals_get()),
                tuple(a.tobytes() for a in ch.exp_diagonals_get()), ch.exp_cells_get().tobytes(), ch.eig_vectors(0).tobytes(), ch.eig_vectors(1).tobytes())
    chain(cha)
    chain(chb)
    sa, sb = state(cha), state(chb)
    b0, nb = SC.span_of(ca, cb)
    check(cha, chb, ca, cb, b0, nb, 3, 50)
    assert state(cha) == sa and state(chb) == sb
    check(chb, cha, cb, ca, b0, nb, 1, 50)
    cha.scc_free()
    assert state(cha) == sa and state(chb) == sb
    cha.close()
    chb.close()


# ---- 4. every refusal of the C call ----------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_c_calls():
    from cloops_amd import api, _lib
    lib = _lib.load()
    E = _lib.CL_ERR_ARG
    (Xa, Ya), (Xb, Yb) = MC.scattered(5, 1000, 50000, 9000), MC.scattered(6, 1000, 50000, 9000)      # (X <= Y: a clustering run is started below)
    cha, chb = api.Chromosome(Xa, Ya), api.Chromosome(Xb, Yb)
    D, ROOM = 8, 32                                                          # the arrays hold more than any n_diags tried that a call may zero
    arrs = [np.full(ROOM, 7, np.int64)] + [np.full(ROOM, 7, np.uint64) for _ in range(5)]
    ptr = [a.ctypes.data_as(t) for a, t in zip(arrs, lib.cl_scc_moments.argtypes[6:])]
    call = lambda a, b, b0, nb, h, d, p=None: lib.cl_scc_moments(a, b, b0, nb, h, d, *(p or ptr))

    def refused(*args, **kw):
        for a in arrs:
            a[:] = 7
        assert call(*args, **kw) == E
        return lib.cl_last_error()

    def zeroed(d=D):
        return not any(a[:d].any() for a in arrs) and all((a[d:] == 7).all() for a in arrs)
    assert lib.cl_scc_free(None) == E
    assert refused(None, chb._h, 0, 20, 0, D) and zeroed() and refused(cha._h, None, 0, 20, 0, D) and zeroed()
    # no cells, unfolded cells, different res
    assert b"no cells" in refused(cha._h, chb._h, 0, 20, 0, D) and zeroed()
    cha.mat_cells(1000, fold=True)
    assert b"no cells" in refused(cha._h, chb._h, 0, 20, 0, D) and b"no cells" in refused(chb._h, cha._h, 0, 20, 0, D)
    chb.mat_cells(1000, fold=False)
    assert b"not folded" in refused(cha._h, chb._h, 0, 20, 0, D) and b"not folded" in refused(chb._h, cha._h, 0, 20, 0, D) and zeroed()
    chb.mat_cells(2000, fold=True)
    assert b"different res" in refused(cha._h, chb._h, 0, 20, 0, D) and zeroed()
    chb.mat_cells(1000, fold=True)
    good = lambda: call(cha._h, chb._h, 0, 20, 1, D)
    assert good() == 0 and arrs[0][:D].all() and arrs[5][:D].any() and all((a[D:] == 7).all() for a in arrs)
    kept = [a.copy() for a in arrs]
    # the scalars
    for b0, nb, h, d in ((0, 20, -1, D), (0, 20, 21, D), (0, 20, 0, 0), (0, 20, 0, -1), (0, 20, 0, 21), (0, -1, 0, 0), (0, 0, 0, 1), (0, 7, 0, D),
                         ((1 << 30) + 1, 20, 0, D), (-(1 << 30) - 1, 20, 0, D), (0, (1 << 28) + 1, 0, 1), (0, 1 << 40, 0, 1)):
        assert refused(cha._h, chb._h, b0, nb, h, d), (b0, nb, h, d)
        assert zeroed(d if 1 <= d <= ROOM else 0), (b0, nb, h, d)
    # NULL outputs
    for k in range(6):
        p = list(ptr)
        p[k] = None
        assert refused(cha._h, chb._h, 0, 20, 0, D, p=p)
        assert not any(a[:D].any() for j, a in enumerate(arrs) if j != k)
    assert lib.cl_scc_moments(cha._h, chb._h, 5, 0, 0, 0, None, None, None, None, None, None) == 0      # nb == 0: nothing to do, NULL arrays
    assert call(cha._h, chb._h, 5, 0, 3, 0) == 0
    # the band limit: nb (D + 4h) beyond 2^28 with nb, D and h each in range
    assert b"band" in refused(cha._h, chb._h, 0, 1 << 26, 0, 5) and zeroed(5) and b"band" in refused(cha._h, chb._h, 0, 1 << 22, 16, 1) and zeroed(1)
    assert good() == 0 and all(np.array_equal(a, b) for a, b in zip(arrs, kept))          # the earlier state is usable, the scratch too
    # runs in flight, on either handle
    cha.cluster_async("v2", 2000, 5)
    assert b"in flight" in refused(cha._h, chb._h, 0, 20, 1, D) and b"in flight" in refused(chb._h, cha._h, 0, 20, 1, D) and zeroed()
    assert lib.cl_scc_free(cha._h) == E
    cha.wait()
    assert good() == 0 and all(np.array_equal(a, b) for a, b in zip(arrs, kept))
    assert lib.cl_scc_free(cha._h) == 0 and lib.cl_scc_free(chb._h) == 0 and good() == 0
    # the Python binding refuses what it can before the call
    for f in (lambda: cha.scc_moments(None, 0, 5), lambda: cha.scc_moments(chb, 0, 5, h=21), lambda: cha.scc_moments(chb, 0, 5, n_diags=6),
              lambda: cha.scc_moments(chb, 0, 5, n_diags=0), lambda: cha.scc_moments(chb, 0, -1), lambda: cha.scc_moments(chb, 0, 1 << 26, n_diags=5)):
        with pytest.raises(ValueError):
            f()
    with pytest.raises(_lib.CloopsHipError):
        cha.scc_moments(chb, 1 << 31, 5)
    assert [len(a) for a in cha.scc_moments(chb, 0, 0)] == [0] * 6
    cha.close()
    chb.close()


def test_the_overflow_rule_refuses_on_the_host():
    """2^20 rows in one cell of each sample and a row 2^24 bins away: 2^40 (2^24 + 1) >= 2^64.  Nothing is launched: no scratch is
    allocated for the 64 MiB band, and the handles go on working"""
    from cloops_amd import _lib
    X, Y = SC.overflowing()
    cha, ca = with_cells(X, Y, 1)
    chb, cb = with_cells(X, Y, 1)
    b0, nb = SC.span_of(ca, cb)
    assert (b0, nb) == (5, (1 << 24) + 1)
    before = device_free_bytes()
    for a, b in ((cha, chb), (cha, cha)):
        with pytest.raises(_lib.CloopsHipError) as ei:
            a.scc_moments(b, b0, nb, h=0, n_diags=1)
        assert ei.value.code == _lib.CL_ERR_ARG and "overflow rule" in str(ei.value)
    assert before - device_free_bytes() < 1 << 25
    got = check(cha, chb, ca, cb, b0, 1 << 10, 0, 1)                        # one step inside: 2^40 2^10 < 2^64
    assert got[0].tolist() == [1] and int(got[3][0]) == 1 << 40
    got = cha.scc_moments(chb, b0, (1 << 24) - 1, h=0, n_diags=1)            # the largest window the rule lets through: the far row lies outside
    assert [int(a[0]) for a in got] == [1, 1 << 20, 1 << 20, 1 << 40, 1 << 40, 1 << 40]
    with pytest.raises(_lib.CloopsHipError):
        cha.scc_moments(chb, b0, 1 << 24, h=0, n_diags=1)
    cha.close()
    chb.close()


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------
def _write_jd(d, name, X, Y):
    import joblib
    os.makedirs(d, exist_ok=True)
    joblib.dump(np.stack([np.arange(len(X)), X, Y], 1).astype(np.int64), os.path.join(d, "%s-%s.jd" % (name, name)))


def same(got, want):
    """a float of a file against the restatement's: within 1e-12, NaN for NaN"""
    return (math.isnan(got) and math.isnan(want)) or abs(got - want) <= 1e-12


def test_the_command_end_to_end(tmp_path):
    """similarity.main on two directories, one chromosome missing from the second: every number of the four files against the
    restatement -- integers exactly, floats within 1e-12"""
    from cloops_amd import pipe, similarity
    (Xa, Ya), (Xb, Yb) = SC.general()
    data = {"one": {"chr2": (Xa, Ya), "chr10": (Xb[:1500], Yb[:1500]), "chr5": (Xa[:700], Ya[:700])},
            "two": {"chr2": (Xb, Yb), "chr10": (Xa[:1400] + 5000, Ya[:1400] + 5000)}}
    for s, chroms in data.items():
        for name, (X, Y) in chroms.items():
            _write_jd(os.path.join(str(tmp_path), s), name, X, Y)
    out = os.path.join(str(tmp_path), "o")
    res, h, dmax, ign = 2000, 2, 60000, 1
    pipe.CACHE.clear()
    assert similarity.main(["-d", "%s,%s" % (os.path.join(str(tmp_path), "one"), os.path.join(str(tmp_path), "two")), "-o", out, "-res", str(res),
                            "-h", str(h), "-dmax", str(dmax), "-ignorediags", str(ign)]) == 0
    pipe.CACHE.clear()
    want = {}
    for c in ("chr10", "chr2"):
        ca, cb = MC.cells_oracle(*data["one"][c], 0, res, True), MC.cells_oracle(*data["two"][c], 0, res, True)
        b0, nb = SC.span_of(ca, cb)
        D = min(nb, dmax // res + 1)
        m = SC.moments_oracle(ca, cb, b0, nb, h, D)
        want[c] = dict(SC.scc_oracle(m, ign), n=m[0], bins=nb, diags=D, keptA=ca[3], keptB=cb[3])
        assert D == 31 and want[c]["pixels"] > 1000 and -1 < want[c]["scc"] < 1
    rows = [r.split("\t") for r in open(out + "_scc.txt").read().splitlines()[2:]]
    assert [r[:3] for r in rows] == [["one", "two", "chr10"], ["one", "two", "chr2"], ["one", "two", "genome"]]
    for r in rows[:2]:
        w = want[r[2]]
        assert [int(v) for v in r[3:7]] == [w["bins"], w["diags"], h, w["pixels"]] and [int(v) for v in r[9:]] == [w["keptA"], w["keptB"]]
        assert same(float(r[7]), w["scc"]) and same(float(r[8]), w["pcc"])
    genome = (want["chr10"]["scc"] + want["chr2"]["scc"]) / 2
    assert same(float(rows[2][7]), genome) and same(float(rows[2][8]), (want["chr10"]["pcc"] + want["chr2"]["pcc"]) / 2)
    assert int(rows[2][3]) == sum(w["bins"] for w in want.values()) and int(rows[2][6]) == sum(w["pixels"] for w in want.values())
    strata = [r.split("\t") for r in open(out + "_scc_strata.txt").read().splitlines()[1:]]
    assert len(strata) == 62
    for k, r in enumerate(strata):
        c, d = ("chr10", k) if k < 31 else ("chr2", k - 31)
        w = want[c]
        assert r[:4] == ["one", "two", c, str(d)] and int(r[4]) == w["n"][d] and same(float(r[5]), w["rho"][d]) and same(float(r[6]), w["weight"][d])
    assert float(strata[0][6]) == 0.0 and float(strata[1][6]) > 0            # ignorediags 1
    mat = [r.split("\t") for r in open(out + "_scc_matrix.txt").read().splitlines()]
    assert mat[0] == ["", "one", "two"] and mat[1][0] == "one" and mat[1][1] == mat[2][2] == "1" and mat[1][2] == mat[2][1] and same(float(mat[1][2]), genome)
    js = json.load(open(out + "_scc.json"))
    assert js["pairs"][0]["skipped"] == ["chr5"] and js["samples"] == ["one", "two"] and js["warnings"] == []
    assert js["args"]["res"] == res and js["args"]["h"] == h and js["args"]["dmax"] == dmax and js["args"]["ignore_diags"] == ign
    for c, w in want.items():
        r = js["pairs"][0]["chroms"][c]
        assert (r["bins"], r["diags"], r["pixels"], r["keptA"], r["keptB"]) == (w["bins"], w["diags"], w["pixels"], w["keptA"], w["keptB"])
        assert same(r["scc"], w["scc"]) and same(r["pcc"], w["pcc"])
    assert same(js["pairs"][0]["genome"]["scc"], genome)
    # a sample against itself, its directory spelled two ways: one resident, its lock taken once; every stratum with variance is 1
    one = os.path.join(str(tmp_path), "one")
    js = similarity.jds2similarity([one, os.path.join(one, ".")], out + "_self", res=res, h=h, dmax=dmax)
    pipe.CACHE.clear()
    assert js["samples"] == ["s1", "s2"] and js["pairs"][0]["skipped"] == [] and sorted(js["pairs"][0]["chroms"]) == ["chr10", "chr2", "chr5"]
    for r in js["pairs"][0]["chroms"].values():
        assert abs(r["scc"] - 1.0) <= 100 * 2.0 ** -53 and abs(r["pcc"] - 1.0) <= 5 * 2.0 ** -53 and r["keptA"] == r["keptB"] > 0 and r["pixels"] > 500
    assert abs(js["pairs"][0]["genome"]["scc"] - 1.0) <= 100 * 2.0 ** -53 and js["warnings"] == []
    # refused before any GPU work or file
    bad = os.path.join(str(tmp_path), "bad")
    for f in (lambda: similarity.jds2similarity([one], bad), lambda: similarity.jds2similarity([one, one], bad, h=21),
              lambda: similarity.jds2similarity([one, one], bad, res=0), lambda: similarity.jds2similarity([one, one], bad, names=["x"])):
        with pytest.raises(ValueError):
            f()
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("bad")]
