"""GPU: kernel K23 (cl_kdis_build / get / hist) against the numpy oracle of tests/kdis_cases.py, written from the definitions of
include/cloops_hip.h (it does not call cloops_amd.esteps): every value, X, Y and the order equal, not close.  Degenerate sizes,
duplicates, tile and wave edges, the traps of the early stop, the coordinate range, every list capacity, dense and sparse random
sets with and without a cut, the histogram at its bin edges, the core rule against K2's neighbour counts, the handle's other
results (unchanged), argument errors, jd2esteps and the command line against the host functions fed by the oracle, and -kdis on the
main command."""
import ctypes
import json
import os

import numpy as np
import pytest

import kdis_cases as KC
import golden_util as G
from cloops_amd.ests import logbin

pytestmark = pytest.mark.gpu

EMPTY = KC.EMPTY
TILE = 256           # k_kdis.hip K23_TILE: table rows per workgroup of k23_walk, one per lane
LIM = (1 << 29) - 1  # the largest coordinate of a handle


def chrom(X, Y):
    from cloops_amd import api
    return api.Chromosome(np.asarray(X, np.int64), np.asarray(Y, np.int64))


def check(ch, X, Y, cut, ks, form="auto"):
    """one build against the oracle: the rows in table order, every d, every histogram -> the oracle's (xs, ys, {k: d}, rows)"""
    want = KC.kdis_oracle(X, Y, cut, ks, form)
    xs, ys, d, _ = want
    assert ch.kdis_build(ks, cut) == len(xs), (cut, ks)
    for w, k in enumerate(ks):
        got = ch.kdis_get(w)
        assert [a.dtype for a in got] == [np.int32] * 3 and [len(a) for a in got] == [len(xs)] * 3
        assert np.array_equal(got[0], xs) and np.array_equal(got[1], ys), (cut, k)
        bad = np.flatnonzero(got[2] != d[k])
        assert len(bad) == 0, (cut, k, len(bad), bad[:5], got[2][bad[:5]], d[k][bad[:5]])
        hist, nz, nn = ch.kdis_hist(w)
        h, z, n = KC.hist_oracle(d[k])
        assert hist.dtype == np.uint64 and hist.shape == (KC.BINS,) and np.array_equal(hist.astype(np.int64), h) and (nz, nn) == (z, n), (cut, k)
    return want


def scattered(seed, m, span=100000, width=30000):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, span, m)
    return X, X + rng.integers(0, width, m)


# ---- degenerate inputs -----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5])
def test_degenerate_sizes(k):
    ch = chrom(EMPTY, EMPTY)
    assert ch.kdis_build([k]) == 0 and all(len(a) == 0 for a in ch.kdis_get())
    hist, nz, nn = ch.kdis_hist()
    assert not hist.any() and (nz, nn) == (0, 0)
    ch.kdis_free()
    ch.close()
    for m in (1, k, k + 1, k + 2):
        X, Y = scattered(m, m)
        ch = chrom(X, Y)
        d = check(ch, X, Y, 0, [k])[2][k]
        assert ((d == -1).all() and ch.kdis_hist()[2] == m) if m <= k else ((d >= 0).all() and ch.kdis_hist()[2] == 0)      # m = k + 1 is the first with a k-th neighbour
        assert ch.kdis_build([k], 1 << 20) == 0 and all(len(a) == 0 for a in ch.kdis_get())      # the cut removes every row
        assert not ch.kdis_hist()[0].any() and ch.kdis_hist()[1:] == (0, 0)
        ch.close()


def test_duplicates():
    for k in (1, 7):
        X, Y = np.full(k + 1, 4242), np.full(k + 1, 9000)
        ch = chrom(X, Y)
        d = check(ch, X, Y, 0, [k])[2][k]
        assert (d == 0).all() and ch.kdis_hist()[1:] == (k + 1, 0)
        ch.close()
    # a pile of 300 identical rows at table positions 100 .. 399, across the edge of the first tile
    rng = np.random.default_rng(3)
    X = np.concatenate([rng.integers(0, 5000, 100), np.full(300, 6000), rng.integers(7000, 12000, 100)])
    Y = np.concatenate([X[:100] + rng.integers(0, 900, 100), np.full(300, 6500), X[400:] + rng.integers(0, 900, 100)])
    o = rng.permutation(500)
    X, Y = X[o], Y[o]
    ch = chrom(X, Y)
    xs, _, d, _ = check(ch, X, Y, 0, [4, 64])
    assert 100 < TILE < 400 and (xs[100:400] == 6000).all() and (d[64][100:400] == 0).all() and ch.kdis_hist(1)[1] == 300
    ch.close()


# ---- tile and wave edges ----------------------------------------------------------------------------
@pytest.mark.parametrize("m", [63, 64, 65, 255, 256, 257, 511, 513])
def test_tile_and_wave_edges(m):
    """evenly spaced rows: the nearest of the first row all lie to its right, those of the last row to its left, and those of rows
    255 / 256 on both sides of the workgroup boundary"""
    rng = np.random.default_rng(m)
    X = np.arange(m) * 10
    Y = 500 + rng.integers(0, 3, m)
    o = rng.permutation(m)
    ch = chrom(X[o], Y[o])
    xs, _, d, rows = check(ch, X[o], Y[o], 0, [3, 8], "brute")
    assert np.array_equal(xs, X) and np.array_equal(o[rows], np.arange(m))
    assert 30 <= d[3][0] <= 32 and 30 <= d[3][m - 1] <= 32 and 20 <= d[3][m // 2] <= 22        # three to one side; two and one
    ch.close()


def test_equal_x_keep_input_order():
    X = np.array([5, 3, 5, 3, 5, 4, 3])
    Y = np.array([70, 60, 50, 40, 30, 20, 10])
    ch = chrom(X, Y)
    xs, ys, _, rows = check(ch, X, Y, 0, [2], "brute")
    assert rows.tolist() == [1, 3, 6, 5, 0, 2, 4] and ys.tolist() == [60, 40, 10, 20, 70, 50, 30]
    ch.close()


# ---- the traps of the early stop ---------------------------------------------------------------------
def test_all_x_equal_and_all_y_equal():
    rng = np.random.default_rng(11)
    v = rng.integers(0, 40000, 3000)
    for X, Y in ((np.full(3000, 777), v), (v - 50000, np.full(3000, 777))):
        ch = chrom(X, Y)
        d = check(ch, X, Y, 0, [5, 20], "brute")[2]
        assert (d[5] >= 0).all() and d[20].max() > 0
        ch.close()


def test_comb():
    """500 rows share the query's X but lie 10^6 away in Y; 2000 rows follow in X order that lie 2 10^6 away in Y; only then come the
    query's true nearest.  The walk must neither stop at the comb nor take it"""
    k = 6
    x0, y0 = 100000, 150000
    X = np.concatenate([[x0], np.full(500, x0), x0 + 1 + np.arange(2000), x0 + 2001 + np.arange(k), x0 - 1 - np.arange(1000)])
    Y = np.concatenate([[y0], y0 + 1000000 + np.arange(500), np.full(2000, y0 + 2000000), np.full(k, y0), np.full(1000, y0 - 3000000)])
    ch = chrom(X, Y)
    xs, ys, d, rows = check(ch, X, Y, 0, [k], "brute")
    q = int(np.flatnonzero(rows == 0)[0])
    assert d[k][q] == 2001 + k - 1                                    # the last of the k true neighbours, 2000 table positions away
    ch.close()


def test_neighbour_at_the_threshold():
    """the k-th neighbour differs in X alone, so |dx| equals the threshold it sets; ties beyond it on either side"""
    k = 4
    X = np.array([0, 1, -2, 3, 50, -50, 50, -50, 49, 51, 200])
    Y = np.array([0, 1, 0, -2, 0, 0, 0, 1, 1, 0, 0])
    ch = chrom(X, Y)
    xs, _, d, rows = check(ch, X, Y, 0, [k, k + 1, k + 2], "brute")
    q = int(np.flatnonzero(rows == 0)[0])
    assert (d[k][q], d[k + 1][q], d[k + 2][q]) == (50, 50, 50)        # (3, -2) at 5 is the third; then four rows at exactly 50
    ch.close()


# ---- the range of the coordinates ---------------------------------------------------------------------
def test_coordinate_limits():
    k = 5
    X = np.concatenate([np.full(k, -LIM), np.full(k, LIM)])
    ch = chrom(X, X)
    d = check(ch, X, X, 0, [k - 1, k])[2]
    assert (d[k - 1] == 0).all() and (d[k] == (1 << 31) - 4).all()    # the k-th neighbour lies in the other corner
    hist, nz, nn = ch.kdis_hist(1)
    assert hist[KC.BINS - 1] == 2 * k and hist.sum() == 2 * k
    ch.close()
    rng = np.random.default_rng(17)
    X = rng.integers(-LIM, -LIM + 60000, 900)
    Y = X + rng.integers(-20000, 20000, 900).clip(-LIM - X, None)
    ch = chrom(X, Y)
    check(ch, X, Y, 0, [3, 12], "brute")
    check(ch, X, Y, 5000, [3, 12], "brute")
    ch.close()


# ---- k handling -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """700 rows with their 64 nearest, made once"""
    X, Y = scattered(29, 700)
    return X, Y, KC.kdis_oracle(X, Y, 0, range(1, 65), "brute")


@pytest.mark.parametrize("k", [1, 8, 9, 16, 17, 32, 33, 64])
def test_every_capacity(small, k):
    X, Y, (xs, ys, d, _) = small
    ch = chrom(X, Y)
    assert ch.kdis_build([k]) == 700
    gx, gy, gd = ch.kdis_get()
    assert np.array_equal(gx, xs) and np.array_equal(gy, ys) and np.array_equal(gd, d[k])
    ch.close()


def test_several_k_in_one_build(small):
    X, Y, (xs, ys, d, _) = small
    ch = chrom(X, Y)
    ch.kdis_build([5, 10, 20])
    three = [ch.kdis_get(w)[2].copy() for w in range(3)]
    hists = [ch.kdis_hist(w) for w in range(3)]
    for w, k in enumerate((5, 10, 20)):
        ch.kdis_build([k])                                            # a second build replaces the first
        assert np.array_equal(ch.kdis_get()[2], three[w]) and np.array_equal(three[w], d[k])
        h = ch.kdis_hist()
        assert np.array_equal(h[0], hists[w][0]) and h[1:] == hists[w][1:]
        from cloops_amd import _lib
        with pytest.raises(_lib.CloopsHipError):
            ch.kdis_get(1)
    ks = [1, 8, 9, 16, 17, 32, 33, 64]                                # eight at once, over every capacity
    ch.kdis_build(ks)
    assert all(np.array_equal(ch.kdis_get(w)[2], d[k]) for w, k in enumerate(ks))
    assert np.array_equal(ch.kdis_get(3, 690, 10)[2], d[16][690:]) and np.array_equal(ch.kdis_get(7, 255, 2)[0], xs[255:257])
    ch.close()


# ---- random sets ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", [200000, 200000000])
def test_random_sets(span):
    rng = np.random.default_rng(span % 1000 + 1)
    X = rng.integers(0, span, 20000)
    Y = X + rng.integers(-span // 100, span // 4, 20000)
    ch = chrom(X, Y)
    a = check(ch, X, Y, 0, [4, 9, 19])
    cut = span // 10
    b = check(ch, X, Y, cut, [4, 9, 19])                               # rows under the cut are neither queries nor neighbours
    assert 0 < len(b[0]) < len(a[0]) == 20000 and ((b[1] - b[0]) >= cut).all()
    ch.close()


# ---- the histogram at its bin edges -------------------------------------------------------------------------
def test_histogram_bin_edges():
    small = [1, 2, 127, 128, 129, 255, 256]
    X = np.concatenate([[1000000 * j, 1000000 * j + v] for j, v in enumerate(small)])
    Y = np.repeat(1000000 * np.arange(len(small)) + 500, 2)
    ch = chrom(X, Y)
    d = check(ch, X, Y, 0, [1], "brute")[2][1]
    assert sorted(d.tolist()) == sorted(small * 2)
    hist = ch.kdis_hist()[0]
    assert all(hist[logbin(v)] == 2 for v in small) and hist.sum() == 2 * len(small)
    ch.close()
    for v in ((1 << 30) - 1, 1 << 30, (1 << 31) - 4):                # two rows that far apart, alone on a handle
        a = v // 4
        X, Y = np.array([-a, v // 2 - a]), np.array([-a, v - v // 2 - a])
        ch = chrom(X, Y)
        d = check(ch, X, Y, 0, [1], "brute")[2][1]
        assert d.tolist() == [v, v] and ch.kdis_hist()[0][logbin(v)] == 2
        ch.close()


# ---- the core rule, against K2 ------------------------------------------------------------------------------
def test_core_rule_against_neighbor_counts():
    """row by row: neighbor_counts(eps, cut) >= k + 1 iff d_k <= eps -- K23 against K2, the oracle takes no part beyond the order"""
    rng = np.random.default_rng(41)
    X = rng.integers(0, 400000, 6000)
    Y = X + rng.integers(0, 60000, 6000)
    X[:200], Y[:200] = X[0] + rng.integers(-150, 150, 200), Y[0] + rng.integers(-150, 150, 200)      # a dense spot
    ch = chrom(X, Y)
    for cut in (0, 20000):
        _, _, rows = KC.table_order(X, Y, cut)
        ks = [1, 4, 9, 19, 40]
        assert ch.kdis_build(ks, cut) == len(rows)
        d = [ch.kdis_get(w)[2] for w in range(len(ks))]
        for eps in (100, 750, 2000, 9000):
            cnt = ch.neighbor_counts(eps, cut)
            assert (cnt[rows] >= 1).all() and (np.delete(cnt, rows) == -1).all()
            for w, k in enumerate(ks):
                core = cnt[rows] >= k + 1
                assert np.array_equal(core, d[w] <= eps), (cut, eps, k)
            assert 0 < (d[1] <= eps).sum() < len(rows)                    # both answers occur
    ch.close()


# ---- the handle's other state ---------------------------------------------------------------------------------
def test_other_results_unchanged():
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
    a = check(ch, X, Y, 0, [4, 9])                                     # the shared table, at the same cut
    assert all(np.array_equal(u, v) for u, v in zip(dom0, ch.domains_get()))
    assert all(np.array_equal(u, v) for u, v in zip(cnt0, ch.domains_count(s, s + 900000)))
    agg1 = ch.agg_loops(cx, cy, 1000, 10, 3, want_mats=True)
    assert all(np.array_equal(u, v) for u, v in zip(agg0[:3], agg1[:3])) and agg0[3] == agg1[3]
    b = check(ch, X, Y, 4000, [4, 9])                                  # another cut: the table is rebuilt for it
    assert len(b[0]) < len(a[0])
    assert all(np.array_equal(u, v) for u, v in zip(dom0, ch.domains_get()))
    assert all(np.array_equal(u, v) for u, v in zip(cnt0, ch.domains_count(s, s + 900000)))      # the rows of the tracks' cut again
    agg1 = ch.agg_loops(cx, cy, 1000, 10, 3, want_mats=True)           # ... and the aggregate builds its own
    assert all(np.array_equal(u, v) for u, v in zip(agg0[:3], agg1[:3])) and agg0[3] == agg1[3]
    got = ch.kdis_get(1)                                               # the k-distances of cut 4000 outlive the table of cut 0
    assert np.array_equal(got[0], b[0]) and np.array_equal(got[1], b[1]) and np.array_equal(got[2], b[2][9])
    assert ch.domains_tracks(0, 10000, 10) == trk0
    assert np.array_equal(ch.cluster("v2", 1000, 5).labels, lab0)
    assert np.array_equal(ch.kdis_get(0)[2], b[2][4])
    assert ch.kdis_free() is None
    from cloops_amd import _lib
    with pytest.raises(_lib.CloopsHipError):
        ch.kdis_get()                                                  # freed: nothing to get
    with pytest.raises(_lib.CloopsHipError):
        ch.kdis_hist()
    assert all(np.array_equal(u, v) for u, v in zip(dom0, ch.domains_get()))
    ch.domains_free()
    ch.close()


# ---- argument errors ----------------------------------------------------------------------------------
def test_argument_errors():
    from cloops_amd import api, _lib
    lib = _lib.load()
    E = _lib.CL_ERR_ARG
    X, Y = scattered(5, 1000)
    ch = api.Chromosome(X, Y)
    nk = ctypes.c_int64(7)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    i32 = lambda *v: np.array(v, np.int32)
    build, get, hist = lib.cl_kdis_build, lib.cl_kdis_get, lib.cl_kdis_hist
    t4 = [np.zeros(4, np.int32) for _ in range(3)]
    hh, nz, nn = np.zeros(KC.BINS, np.uint64), ctypes.c_uint64(7), ctypes.c_uint64(7)
    # a get or hist before a build
    assert get(ch._h, 0, 0, 0, *map(vp, t4)) == E
    assert hist(ch._h, 0, vp(hh), ctypes.byref(nz), ctypes.byref(nn)) == E and (nz.value, nn.value) == (0, 0)
    want = check(ch, X, Y, 0, [4, 9], "brute")

    def still_there():
        got = ch.kdis_get(1)
        return np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2][9]) and np.array_equal(ch.kdis_get(0)[2], want[2][4])
    # build: a NULL handle, NULL ks / output, n_k, the range and order of ks
    ks = i32(4, 9)
    assert build(None, 0, vp(ks), 2, ctypes.byref(nk)) == E
    assert build(ch._h, 0, None, 2, ctypes.byref(nk)) == E and nk.value == 0
    assert build(ch._h, 0, vp(ks), 2, None) == E
    nine = i32(*range(1, 10))
    for bad, n in ((ks, 0), (ks, -1), (nine, 9), (i32(0, 4), 2), (i32(-1), 1), (i32(65), 1), (i32(4, 65), 2), (i32(9, 4), 2), (i32(4, 4), 2),
                   (i32(4, 9, 9), 3)):
        nk.value = 7
        assert build(ch._h, 0, vp(bad), n, ctypes.byref(nk)) == E and nk.value == 0, (bad, n)       # (a refused call zeroes its output)
        assert b"cl_kdis_build" in lib.cl_last_error()
    assert still_there()                                                                             # ... and leaves the earlier build
    assert build(ch._h, 0, vp(nine), 8, ctypes.byref(nk)) == 0 and nk.value == 1000                  # eight are fine
    want = check(ch, X, Y, 0, [4, 9], "brute")
    # get: which, the range, NULL outputs
    assert get(None, 0, 0, 1, *map(vp, t4)) == E
    assert get(ch._h, -1, 0, 1, *map(vp, t4)) == E and get(ch._h, 2, 0, 1, *map(vp, t4)) == E
    assert get(ch._h, 0, -1, 1, *map(vp, t4)) == E and get(ch._h, 0, 0, -1, *map(vp, t4)) == E
    assert get(ch._h, 0, 999, 2, *map(vp, t4)) == E and get(ch._h, 0, 1001, 0, *map(vp, t4)) == E
    for k in range(3):
        assert get(ch._h, 0, 0, 1, *[None if j == k else vp(a) for j, a in enumerate(t4)]) == E
    assert b"cl_kdis_get" in lib.cl_last_error()
    assert get(ch._h, 1, 1000, 0, None, None, None) == 0
    assert get(ch._h, 1, 996, 4, *map(vp, t4)) == 0 and np.array_equal(t4[2], want[2][9][996:]) and np.array_equal(t4[0], want[0][996:])
    # hist: which, NULL outputs
    assert hist(None, 0, vp(hh), ctypes.byref(nz), ctypes.byref(nn)) == E
    assert hist(ch._h, 2, vp(hh), ctypes.byref(nz), ctypes.byref(nn)) == E and hist(ch._h, -1, vp(hh), ctypes.byref(nz), ctypes.byref(nn)) == E
    assert hist(ch._h, 0, None, ctypes.byref(nz), ctypes.byref(nn)) == E
    assert hist(ch._h, 0, vp(hh), None, ctypes.byref(nn)) == E and hist(ch._h, 0, vp(hh), ctypes.byref(nz), None) == E
    assert b"cl_kdis_hist" in lib.cl_last_error()
    assert hist(ch._h, 0, vp(hh), ctypes.byref(nz), ctypes.byref(nn)) == 0 and int(hh.sum()) + nz.value == 1000 and nn.value == 0
    assert lib.cl_kdis_free(None) == E
    assert still_there()
    # the Python layer
    with pytest.raises(_lib.CloopsHipError):
        ch.kdis_build([])
    with pytest.raises(_lib.CloopsHipError):
        ch.kdis_build([9, 4])
    with pytest.raises(ValueError):
        ch.kdis_build([[4, 9]])
    assert still_there()
    # runs in flight
    ch.cluster_async("v2", 2000, 5)
    nk.value = 7
    assert build(ch._h, 0, vp(ks), 2, ctypes.byref(nk)) == E and nk.value == 0
    assert get(ch._h, 0, 0, 1, *map(vp, t4)) == E
    assert hist(ch._h, 0, vp(hh), ctypes.byref(nz), ctypes.byref(nn)) == E
    assert lib.cl_kdis_free(ch._h) == E
    ch.wait()
    assert still_there()                                                                             # the handle still works
    assert ch.kdis_build(7) == 1000                                                                  # (one k as a number)
    ch.kdis_free()
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
    p = subprocess.run([sys.executable, "-m", "cloops_amd.esteps"] + args, env=env, cwd=cwd, timeout=300, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def _host_texts(data, names, ks, cut):
    """the files from the host functions of cloops_amd.esteps fed by the oracle"""
    from cloops_amd import esteps
    per = {name: esteps.chrom_kdis(KC.OracleChrom(*data[name]), ks, cut) for name in names}
    return esteps.outputs_of(per, ks, cut)[0]


def _files(prefix):
    from cloops_amd import esteps
    out = {}
    for suffix in esteps.SUFFIXES:
        with open(prefix + suffix) as fh:
            out[suffix] = fh.read()
    return out


def test_jd2esteps_and_command_line(tmp_path):
    from cloops_amd import esteps, pipe
    data = {name: KC.mixture(seed, 1500, 15, 30, 300)[:2] for name, seed in (("chr2", 0), ("chr10", 1), ("chrX", 2))}
    data["chrM"] = (np.arange(6) * 100, np.arange(6) * 100 + 50)          # fewer rows than k: counted in n_none
    d = os.path.join(str(tmp_path), "jd")
    for name, (X, Y) in data.items():
        _write_jd(d, name, X, Y)
    import joblib
    joblib.dump(np.zeros((3, 3), np.int64), os.path.join(d, "chr2-chr10.jd"))        # a trans file is left out
    pipe.CACHE.clear()
    out = os.path.join(str(tmp_path), "direct")
    js = esteps.jd2esteps(d, out)
    pipe.CACHE.clear()
    want = _host_texts(data, ["chr10", "chr2", "chrM", "chrX"], [4, 9, 19], 0)
    assert _files(out) == want                                        # both files byte for byte
    assert list(js["chroms"]) == ["chr10", "chr2", "chrM", "chrX"] and js["total"]["n"] == 3 * 1950 + 6
    assert [js["estimates"][k]["n_none"] for k in ("4", "9", "19")] == [0, 6, 6]
    assert all(js["estimates"][k]["eps"] is not None for k in ("4", "9", "19")) and not os.path.exists(out + "_kdis.pdf")
    out = os.path.join(str(tmp_path), "cli")
    _run_module(["-d", d, "-o", out, "-k", "12,3", "-cut", "30000", "-c", "chr2,chrX", "-plot"], str(tmp_path))
    want = _host_texts(data, ["chr2", "chrX"], [3, 12], 30000)
    assert _files(out) == want
    js = json.loads(want["_kdis.json"])
    assert js["k"] == [3, 12] and js["cut"] == 30000 and 0 < js["total"]["n"] < 2 * 1950
    try:
        import matplotlib                                              # noqa: F401
        assert os.path.getsize(out + "_kdis.pdf") > 0
    except ImportError:
        assert not os.path.exists(out + "_kdis.pdf")


def test_kdis_flag_of_the_main_command(tmp_path):
    """-kdis on the chr21 BEDPE example writes what the host functions make of the oracle's integers, with n the PETs of the run, and
    leaves the loops what they were"""
    import gzip
    from cloops_amd import pipe
    X, Y = G.chr21_xy()
    bed = os.path.join(str(tmp_path), "in.bedpe.gz")
    with gzip.open(bed, "wt") as fh:                       # a BEDPE whose mid-points are exactly (X, Y)
        for x, y in zip(X.tolist(), Y.tolist()):
            fh.write("chr21\t%d\t%d\tchr21\t%d\t%d\tid\t1\t+\t-\n" % (x, x, y, y))
    fout = os.path.join(str(tmp_path), "run")
    pipe.CACHE.clear()
    assert pipe.main(["-f", bed, "-o", fout, "-m", "0", "-eps", "500,1000,2000", "-minPts", "5", "-kdis", "-kdisk", "9,4"]) == 0
    pipe.CACHE.clear()
    assert open(fout + ".loop").read() == open(os.path.join(G.GOLD, "chr21_v2.loop")).read()      # identical with and without the flag
    got = _files(fout)
    js = json.loads(got["_kdis.json"])
    assert js["k"] == [4, 9] and js["chroms"] == {"chr21": {"n": len(X)}} and js["total"]["n"] == len(X) == 99674
    assert [int(line.split("\t")[2]) for line in got["_kdis.txt"].splitlines()[1:]] == [len(X)] * 2
    assert got == _host_texts({"chr21": (X, Y)}, ["chr21"], [4, 9], 0)
