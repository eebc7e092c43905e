"""GPU: kernel K22 (cl_dom_tracks / get / count) against the numpy oracle of tests/domains_cases.py, written from the definitions of
include/cloops_hip.h (it does not call cloops_amd.domains), and on the small cases against the brute-force count of the definition.
Degenerate sizes, hand-placed rows at every edge of the three intervals, every tile edge of k22_tracks, tiles at and one bin beyond
its LDS window, pile-ups, dense and sparse random sets, several w on one sort, counts (random, empty and abutting domains, bounds
beyond the keys and beyond 32 bits, one domain for all, the LDS stage's capacity and one more, 10^5 domains of one bin), the handle's
other results (unchanged), argument errors, the chr21 example against pinned values, jd2domains and the command line against the host
functions fed by the oracle, and -domains on the main command."""
import ctypes
import json
import os

import numpy as np
import pytest

import domains_cases as DC
import golden_util as G

pytestmark = pytest.mark.gpu

EMPTY = DC.EMPTY
T = 2048             # k_domain.hip K22_TILE: sorted rows per workgroup of k22_tracks and k22_count
BW = 3072            # k_domain.hip K22_BW: bins per LDS window of k22_tracks; a tile needs bx_last - bx_first + 2 w + 1 of them
DL = 2048            # k_domain.hip K22_DL: domain starts that k22_count stages in LDS
DW = 1024            # k_domain.hip K22_DW: domains whose counters k22_count keeps in LDS, from the domain of a tile's first X on
LIM = (1 << 29) - 1  # the largest coordinate of a handle


def chrom(X, Y):
    from cloops_amd import api
    return api.Chromosome(np.asarray(X, np.int64), np.asarray(Y, np.int64))


def check_tracks(ch, X, Y, cut, res, w, brute=False):
    """one tracks call against the oracle (and the brute-force form) -> the oracle's (cross, up, down, n_bins, bin0, n_kept)"""
    want = DC.tracks_oracle(X, Y, cut, res, w)
    if brute:
        b = DC.tracks_oracle(X, Y, cut, res, w, "brute")
        assert all(np.array_equal(p, q) for p, q in zip(want[:3], b[:3])) and want[3:] == b[3:]
    assert ch.domains_tracks(cut, res, w) == want[3:], (cut, res, w)
    got = ch.domains_get()
    assert [a.dtype for a in got] == [np.uint32] * 3 and [len(a) for a in got] == [want[3]] * 3
    for name, g, v in zip(("cross", "up", "down"), got, want[:3]):
        assert np.array_equal(g, v), (name, cut, res, w)
    return want


def check_counts(ch, X, Y, cut, starts, ends):
    got = ch.domains_count(starts, ends)
    want = DC.count_oracle(X, Y, cut, starts, ends)
    assert [a.dtype for a in got] == [np.uint32] * 3
    for name, g, v in zip(("intra", "nx", "ny"), got, want):
        assert np.array_equal(g, v), name
    return want


# ---- degenerate inputs -----------------------------------------------------------------------------
def test_degenerate_sizes():
    ch = chrom(EMPTY, EMPTY)
    assert ch.domains_tracks() == (0, 0, 0) and all(len(a) == 0 for a in ch.domains_get())
    assert [a.tolist() for a in ch.domains_count([0, 20], [10, 30])] == [[0, 0]] * 3
    ch.domains_free()
    ch.close()
    X, Y = np.array([12345]), np.array([67890])
    ch = chrom(X, Y)
    for res, w in ((10000, 10), (10000, 1), (1000, 5), (1, 1)):
        r = check_tracks(ch, X, Y, 0, res, w, res > 1)
    assert r[3:] == (67890 - 12345 + 2, 12345, 1)
    assert check_tracks(ch, X, Y, 100000, 10000, 10)[3:] == (0, 0, 0)        # the cut removes every row
    assert all(len(a) == 0 for a in ch.domains_get())
    assert [a.tolist() for a in ch.domains_count([0], [100000])] == [[0]] * 3
    check_tracks(ch, X, Y, 55545, 10000, 10, True)                           # Y - X == cut stays
    assert [a.tolist() for a in check_counts(ch, X, Y, 55545, [0, 12345, 12346], [12345, 12346, 67891])] == [[0, 0, 0], [0, 1, 0], [0, 0, 1]]
    ch.close()
    X, Y = np.array([500, 900, 700, 900]), np.array([100, 200, 300, 899])    # all rows with Y < X: no counts, but kept and spanned
    ch = chrom(X, Y)
    r = check_tracks(ch, X, Y, 0, 100, 2, True)
    assert r[3:] == (10, 1, 4) and not any(a.any() for a in r[:3])
    assert [a.tolist() for a in check_counts(ch, X, Y, 0, [0, 450], [450, 1000])] == [[0, 1], [0, 4], [3, 1]]
    ch.close()


# ---- hand-placed rows --------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 10])
def test_interval_edges(w):
    res = 7
    X, Y = [], []
    for k, d in enumerate((0, w - 1, w, 2 * w - 1, 2 * w, 2 * w + 1)):       # by - bx at every edge of the three intervals
        for x0 in (-500 + 40 * k, 3 + 40 * k):                               # below zero, where floor is not trunc, and above
            for xo, yo in ((0, 0), (res - 1, 0), (0, res - 1), (res - 1, res - 1)):
                bx = x0 // res
                X.append(bx * res + xo)
                Y.append((bx + d) * res + yo)
    X, Y = np.array(X), np.array(Y)
    ch = chrom(X, Y)
    check_tracks(ch, X, Y, 0, res, w, True)
    check_tracks(ch, X, Y, 0, 1, w, True)                                    # res 1: a bin per position
    check_tracks(ch, X, Y, 3 * w, res, w, True)
    ch.close()


def test_coordinate_limits():
    X = np.array([-LIM, -LIM, -LIM + 5, 0, LIM - 300, LIM, -5, -1])
    Y = np.array([-LIM, -LIM + 200, -LIM + 700, 100, LIM, LIM, 3, 0])
    ch = chrom(X, Y)
    r = check_tracks(ch, X, Y, 0, 128, 3)
    assert r[3:] == ((1 << 23) + 1, -(1 << 22), 8)                           # 2^23 bins and the entry behind them
    r = check_tracks(ch, X, Y, 0, 128, 1024)
    from cloops_amd import _lib
    with pytest.raises(_lib.CloopsHipError):
        ch.domains_tracks(0, 32, 3)                                          # 2^25 bins
    with pytest.raises(_lib.CloopsHipError):
        ch.domains_tracks(500, 32, 3)                                        # the span of ALL rows counts, whatever the cut
    assert all(np.array_equal(a, b) for a, b in zip(ch.domains_get(), r[:3]))            # a refused call leaves the tracks
    with pytest.raises(_lib.CloopsHipError):
        ch.domains_tracks(0, 64, 3)                                          # 2^24 + 1 bins: one too many
    assert ch.domains_tracks(0, 65, 3) == (LIM // 65 - (-LIM // 65) + 2, -LIM // 65, 8)
    check_tracks(ch, X, Y, 0, 128, 3)
    check_counts(ch, X, Y, 0, [-LIM, -5, 1], [-LIM + 1, 1, LIM + 1])
    ch.close()


# ---- tile edges ----------------------------------------------------------------------------------------
def dense_rows(rng, n, span, reach):
    X = rng.integers(0, span, n)
    return X, X + rng.integers(-reach // 8, reach, n)


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T, 2 * T + 1])
def test_tile_edges(n):
    rng = np.random.default_rng(n)
    X, Y = dense_rows(rng, n, 40000, 3000)                                   # rows shuffled: the sort is the kernel's
    ch = chrom(X, Y)
    check_tracks(ch, X, Y, 0, 100, 5)
    check_tracks(ch, X, Y, 0, 100, 1)
    cuts = np.sort(rng.integers(-500, 44000, 41))
    check_counts(ch, X, Y, 0, cuts[:-1], cuts[1:])
    ch.close()


def test_equal_x_across_a_tile_boundary():
    rng = np.random.default_rng(5)
    X = np.concatenate([rng.integers(0, 5000, T - 700), np.full(1500, 5000), rng.integers(5001, 9000, 900)])   # 1500 rows at one X from row T - 700 on
    Y = X + rng.integers(0, 2500, len(X))
    o = rng.permutation(len(X))
    X, Y = X[o], Y[o]
    ch = chrom(X, Y)
    for res, w in ((100, 10), (1, 40), (1000, 2)):
        check_tracks(ch, X, Y, 0, res, w)
    check_counts(ch, X, Y, 0, [0, 5000, 5001, 7000], [5000, 5001, 7000, 12000])
    ch.close()


def test_window_exactly_full_and_one_bin_more():
    rng = np.random.default_rng(6)
    w = 4

    def tile(x0, span, n):                                                   # n rows whose bins (res 1) span x0 .. x0 + span exactly
        X = np.concatenate([[x0, x0 + span], rng.integers(x0, x0 + span + 1, n - 2)])
        return X, X + rng.integers(0, 3 * w, n)

    a = tile(0, BW - 2 * w - 1, T)                                           # needs exactly BW counters: LDS
    b = tile(100000, BW - 2 * w, T)                                          # one bin more: global atomics
    c = tile(200000, 50, 5)
    X, Y = np.concatenate([a[0], b[0], c[0]]), np.concatenate([a[1], b[1], c[1]])
    o = rng.permutation(len(X))
    X, Y = X[o], Y[o]
    ch = chrom(X, Y)
    check_tracks(ch, X, Y, 0, 1, w)
    check_tracks(ch, X, Y, 0, 1, w + 1)                                      # now the first tile does not fit either
    check_tracks(ch, X, Y, 0, 1, w - 1)                                      # and now both do
    ch.close()


def test_sparse_rows_fall_back():
    rng = np.random.default_rng(7)
    n = 3 * T + 77
    X = rng.integers(-LIM, LIM - 4000000, n)                                 # every tile spans millions of bins
    Y = X + rng.integers(-1000, 4000000, n)
    ch = chrom(X, Y)
    check_tracks(ch, X, Y, 0, 100, 1000)
    check_tracks(ch, X, Y, 1000000, 4096, 7)
    cuts = np.sort(rng.integers(-LIM, LIM, 3001))
    check_counts(ch, X, Y, 1000000, cuts[:-1], cuts[1:])                     # more domains than the LDS stage, far apart
    ch.close()


def test_one_bin_holds_every_count():
    X, Y = np.full(3 * T, 777777), np.full(3 * T, 779999)                    # three tiles of identical rows
    ch = chrom(X, Y)
    r = check_tracks(ch, X, Y, 0, 1000, 10, True)
    assert int(r[0].max()) == 3 * T
    r = check_tracks(ch, X, Y, 0, 10000, 10)
    assert int(r[1].max()) == int(r[2].max()) == 3 * T and not r[0].any()
    assert [a.tolist() for a in check_counts(ch, X, Y, 0, [0, 777777, 777778], [777777, 777778, 780000])] == [[0, 0, 0], [0, 3 * T, 0], [0, 0, 3 * T]]
    ch.close()


def test_widest_window():
    rng = np.random.default_rng(8)
    X, Y = dense_rows(rng, 3000, 30000, 25000)
    ch = chrom(X, Y)
    check_tracks(ch, X, Y, 0, 100, 1024)                                     # 300 bins and 2049 around them: in LDS
    check_tracks(ch, X, Y, 0, 100, 1023)
    check_tracks(ch, X, Y, 0, 3, 1024)                                       # 10 000 bins over two tiles: neither fits
    ch.close()


# ---- random sets -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense():
    rng = np.random.default_rng(2022)
    X, Y = dense_rows(rng, 100000, 20000, 9000)
    ch = chrom(X, Y)
    yield ch, X, Y
    ch.close()


@pytest.mark.parametrize("w", [1, 5, 50])
def test_dense_random(dense, w):
    ch, X, Y = dense
    r = check_tracks(ch, X, Y, 0, 100, w)
    assert r[5] == 100000 and r[0].any() and r[1].any() and r[2].any()
    check_tracks(ch, X, Y, 2000, 100, w)


def test_several_w_on_one_sort(dense):
    ch, X, Y = dense
    first = check_tracks(ch, X, Y, 500, 100, 3)
    for w in (7, 1, 200, 1024):
        check_tracks(ch, X, Y, 500, 100, w)
    check_tracks(ch, X, Y, 500, 37, 3)                                       # another res on the same rows
    again = check_tracks(ch, X, Y, 500, 100, 3)
    assert all(np.array_equal(a, b) for a, b in zip(first[:3], again[:3]))
    a, b, c = ch.domains_get(5, 11)                                          # a range of entries
    assert all(np.array_equal(u, v[5:16]) for u, v in zip((a, b, c), again[:3]))
    assert all(len(u) == 0 for u in ch.domains_get(again[3], 0))


def test_counts(dense):
    ch, X, Y = dense
    rng = np.random.default_rng(9)
    check_tracks(ch, X, Y, 0, 100, 5)
    cuts = np.sort(rng.integers(-2000, 31000, 301))
    s, e = cuts[:-1].copy(), cuts[1:].copy()
    e[::4] -= np.minimum(e[::4] - s[::4], rng.integers(0, 60, len(e[::4])))  # abutting, apart, and empty ones among them
    r = check_counts(ch, X, Y, 0, s, e)
    assert int(r[0].sum()) > 1000 and (e == s).any() and (s[1:] == e[:-1]).any()
    big = 1 << 40
    r = check_counts(ch, X, Y, 0, [-big, -big + 5, 3000, 1 << 33], [-big + 5, 3000, 1 << 33, big])     # bounds beyond the keys and 32 bits
    assert r[1].tolist()[0] == 0 and int(r[1].sum()) == 100000
    r = check_counts(ch, X, Y, 0, [-big], [big])                             # one domain over everything
    assert [a.tolist() for a in r] == [[100000]] * 3
    assert all(len(a) == 0 for a in ch.domains_count(EMPTY, EMPTY))          # no domains
    for n in (DL, DL + 1):                                                   # the LDS stage's capacity and one more
        cuts = np.sort(rng.integers(-100, 30000, n + 1))
        check_counts(ch, X, Y, 0, cuts[:-1], cuts[1:])
    check_tracks(ch, X, Y, 3000, 100, 5)                                     # under a cut the counts are those of the kept rows
    r = check_counts(ch, X, Y, 3000, s, e)
    assert 0 < int(r[1].sum()) < 100000
    from cloops_amd import _lib
    for bs, be in (([0, 500, 100], [100, 600, 200]), ([0, 50], [100, 200]), ([100], [50])):           # unordered, overlapping, reversed
        with pytest.raises(_lib.CloopsHipError):
            ch.domains_count(bs, be)
    check_counts(ch, X, Y, 3000, s, e)                                       # the handle works after a refusal


def test_many_domains_of_one_bin():
    rng = np.random.default_rng(10)
    res = 100
    X = rng.integers(0, 10000000, 100000)
    Y = X + rng.integers(0, 300, 100000)
    ch = chrom(X, Y)
    check_tracks(ch, X, Y, 0, res, 2)
    s = np.arange(100000, dtype=np.int64) * res
    r = check_counts(ch, X, Y, 0, s, s + res)
    assert int(r[1].sum()) == 100000 and int(r[0].sum()) > 10000
    ch.close()


# ---- the handle's other results --------------------------------------------------------------------------------
def test_repeatable_and_isolated():
    X, Y = G.chr21_xy()
    ch = chrom(X, Y)
    cx, cy = [20000000, 30000000], [20100000, 30200000]
    lab0 = ch.cluster("v2", 1000, 5).labels.copy()
    agg0 = ch.agg_loops(cx, cy, 1000, 10, 3, want_mats=True)
    ch.track_build("washu", 0, 75, None, "chr21", "chr21")
    ch.track_chunks(1 << 16)
    trk0 = ch.track_render(3)
    cov0 = ch.coverage_build()
    runs0 = ch.coverage_runs()
    nb0 = ch.coverage_text("chr21")
    ch.coverage_chunks(1 << 18)
    txt0 = ch.coverage_render(2)
    ch.peaks_sort()
    pk0 = ch.peaks_call(150, 5)
    pks0 = ch.peaks_get()
    a = check_tracks(ch, X, Y, 0, 10000, 10)
    b = check_tracks(ch, X, Y, 0, 10000, 10)
    assert all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3]))
    s = np.arange(5000000, 47000000, 1000000)
    ca = check_counts(ch, X, Y, 0, s, s + 900000)
    assert all(np.array_equal(u, v) for u, v in zip(a[:3], ch.domains_get()))            # a count leaves the tracks alone
    assert ch.track_render(3) == trk0                                                    # the built washU track is still there
    assert ch.coverage_render(2) == txt0 and ch.coverage_text("chr21") == nb0            # ... and the built coverage with its text
    assert all(np.array_equal(u, v) for u, v in zip(runs0, ch.coverage_runs()))
    assert all(np.array_equal(u, v) for u, v in zip(pks0, ch.peaks_get())) and ch.peaks_call(150, 5) == pk0
    assert np.array_equal(ch.cluster("v2", 1000, 5).labels, lab0)
    agg1 = ch.agg_loops(cx, cy, 1000, 10, 3, want_mats=True)                             # the shared table, at the same cut
    assert all(np.array_equal(u, v) for u, v in zip(agg0[:3], agg1[:3])) and agg0[3] == agg1[3]
    check_tracks(ch, X, Y, 3000, 5000, 20)
    fresh = chrom(X, Y)
    for cut in (3000, 7000, 0):                                                          # the tracks' cut, another one, and back
        got, want = ch.agg_loops(cx, cy, 1000, 10, 3, cut=cut, want_mats=True), fresh.agg_loops(cx, cy, 1000, 10, 3, cut=cut, want_mats=True)
        assert all(np.array_equal(u, v) for u, v in zip(got[:3], want[:3])) and got[3] == want[3]
    fresh.close()
    cb = check_counts(ch, X, Y, 3000, s, s + 900000)                                     # the rows of the tracks' cut again, not the aggregate's
    assert int(cb[1].sum()) < int(ca[1].sum())
    assert all(np.array_equal(u, v) for u, v in zip(ch.domains_get(), DC.tracks_oracle(X, Y, 3000, 5000, 20)[:3]))
    assert ch.coverage_build() == cov0
    ch.domains_free()
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
    nb, b0, nk = i64(), i64(), i64()
    to = (ctypes.byref(nb), ctypes.byref(b0), ctypes.byref(nk))
    vals = lambda: (nb.value, b0.value, nk.value)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    t4 = [np.zeros(4, np.uint32) for _ in range(3)]
    ivs, ive = np.array([0, 20000000], np.int64), np.array([20000000, 50000000], np.int64)
    c2 = [np.zeros(2, np.uint32) for _ in range(3)]
    tracks, get, count = lib.cl_dom_tracks, lib.cl_dom_get, lib.cl_dom_count
    # a get or count before tracks
    assert get(ch._h, 0, 0, *map(vp, t4)) == E
    assert count(ch._h, vp(ivs), vp(ive), 2, *map(vp, c2)) == E
    # tracks: a NULL handle, NULL outputs, res, w, w res, the bins
    assert tracks(None, 0, 10000, 10, *to) == E
    for k in range(3):
        assert tracks(ch._h, 0, 10000, 10, *[None if j == k else o for j, o in enumerate(to)]) == E
    nb.value = b0.value = nk.value = 7
    assert tracks(ch._h, 0, 0, 10, *to) == E and vals() == (0, 0, 0)                               # (a refused call zeroes its outputs)
    assert tracks(ch._h, 0, -5, 10, *to) == E and tracks(ch._h, 0, 1 << 29, 1, *to) == E
    assert tracks(ch._h, 0, 10000, 0, *to) == E and tracks(ch._h, 0, 10000, -1, *to) == E and tracks(ch._h, 0, 10000, 1025, *to) == E
    assert tracks(ch._h, 0, 1 << 19, 1024, *to) == E and tracks(ch._h, 0, (1 << 19) - 1, 1024, *to) == 0      # w res below 2^29
    assert tracks(ch._h, 0, 2, 10, *to) == E                                                        # 20.8 M bins
    assert b"cl_dom_tracks" in lib.cl_last_error()
    assert tracks(ch._h, 0, 10000, 10, *to) == 0 and vals() == (4167, 503, 99674)
    keep = [a.copy() for a in ch.domains_get(0, 4167)]
    assert int(keep[0].sum()) == 110425
    nb.value = 7
    assert tracks(ch._h, 0, 10000, 2000, *to) == E and nb.value == 0                                # a refused call leaves the earlier tracks
    assert all(np.array_equal(u, v) for u, v in zip(keep, ch.domains_get(0, 4167)))
    # get: the range, NULL outputs
    assert get(None, 0, 1, *map(vp, t4)) == E
    assert get(ch._h, -1, 1, *map(vp, t4)) == E and get(ch._h, 0, -1, *map(vp, t4)) == E
    assert get(ch._h, 4166, 2, *map(vp, t4)) == E and get(ch._h, 4168, 0, *map(vp, t4)) == E
    for k in range(3):
        assert get(ch._h, 0, 1, *[None if j == k else vp(a) for j, a in enumerate(t4)]) == E
    assert get(ch._h, 4167, 0, None, None, None) == 0
    assert get(ch._h, 4163, 4, *map(vp, t4)) == 0 and all(np.array_equal(a, k[4163:]) for a, k in zip(t4, keep))
    # count: NULLs, n, the order of the intervals
    assert count(None, vp(ivs), vp(ive), 2, *map(vp, c2)) == E and count(ch._h, vp(ivs), vp(ive), -1, *map(vp, c2)) == E
    assert count(ch._h, None, vp(ive), 2, *map(vp, c2)) == E and count(ch._h, vp(ivs), None, 2, *map(vp, c2)) == E
    for k in range(3):
        assert count(ch._h, vp(ivs), vp(ive), 2, *[None if j == k else vp(a) for j, a in enumerate(c2)]) == E
    assert count(ch._h, vp(ivs), vp(ive), (1 << 31) - 4095, *map(vp, c2)) == E
    assert count(ch._h, vp(ive), vp(ivs), 2, *map(vp, c2)) == E                                     # ends before starts
    bad = np.array([0, 10000000], np.int64)
    assert count(ch._h, vp(bad), vp(ive), 2, *map(vp, c2)) == E                                     # overlapping
    assert b"cl_dom_count" in lib.cl_last_error()
    assert count(ch._h, None, None, 0, None, None, None) == 0
    assert count(ch._h, vp(ivs), vp(ive), 2, *map(vp, c2)) == 0 and int(c2[1].sum()) == 99674 and int(c2[0].sum()) < 99674
    assert get(ch._h, 4163, 4, *map(vp, t4)) == 0                                                   # the handle is usable after each
    assert lib.cl_dom_free(None) == E
    # the Python layer
    with pytest.raises(_lib.CloopsHipError):
        ch.domains_tracks(0, 0, 10)
    with pytest.raises(ValueError):
        ch.domains_count([0, 1], [1])
    # runs in flight
    ch.cluster_async("v2", 2000, 5)
    assert tracks(ch._h, 0, 10000, 10, *to) == E and vals() == (0, 0, 0)
    assert get(ch._h, 0, 1, *map(vp, t4)) == E
    assert count(ch._h, vp(ivs), vp(ive), 2, *map(vp, c2)) == E
    assert lib.cl_dom_free(ch._h) == E
    ch.wait()
    assert ch.domains_tracks(0, 10000, 10) == (4167, 503, 99674)                                    # the handle still works
    assert ch.domains_free() is None
    with pytest.raises(_lib.CloopsHipError):
        ch.domains_get(0, 0)                                                                        # freed: no tracks
    ch.close()


# ---- the chr21 example ----------------------------------------------------------------------------------
# (res, w) -> bins, sum(cross), max(cross), boundaries, domains, sum(intra), domains with ES >= 1 at mincov 20, delta 0.05, maxbins 500
CHR21_PINNED = {(10000, 10): (4167, 110425, 395, 55, 50, 80328, 40),
                (5000, 20): (8333, 220078, 395, 65, 59, 73565, 40)}


@pytest.mark.parametrize("res,w", sorted(CHR21_PINNED))
def test_chr21_pinned(res, w):
    from cloops_amd import domains
    X, Y = G.chr21_xy()
    ch = chrom(X, Y)
    r = domains.chrom_domains(ch, res, [w], 0)[w]
    ES, _ = domains.enrichment(r["intra"], r["nx"], r["ny"], r["start"], r["end"])
    got = (r["n_bins"], int(r["cross"].sum()), int(r["cross"].max()), len(r["boundary"]), len(r["start"]), int(r["intra"].sum()),
           int((ES >= 1.0).sum()))
    assert got == CHR21_PINNED[(res, w)]
    want = DC.tracks_oracle(X, Y, 0, res, w)
    assert all(np.array_equal(r[k], v) for k, v in zip(("cross", "up", "down"), want[:3]))
    assert all(np.array_equal(r[k], v) for k, v in zip(("intra", "nx", "ny"), DC.count_oracle(X, Y, 0, r["start"], r["end"])))
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
    p = subprocess.run([sys.executable, "-m", "cloops_amd.domains"] + args, env=env, cwd=cwd, timeout=300, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def _host_texts(data, names, res, ws, cut, mincov, delta, maxbins, escut):
    """the files from the host functions of cloops_amd.domains fed by the oracle"""
    from cloops_amd import domains
    per = {name: domains.chrom_domains(DC.OracleChrom(*data[name]), res, ws, cut, mincov, delta, maxbins) for name in names}
    return domains.outputs_of(per, res, ws, cut, mincov, delta, maxbins, escut)[0]


def _files(prefix, ws):
    from cloops_amd import domains
    out = {}
    for suffix in domains.suffixes_of(ws):
        with open(prefix + suffix) as fh:
            out[suffix] = fh.read()
    return out


def test_jd2domains_and_command_line(tmp_path):
    from cloops_amd import domains, pipe
    data = {name: DC.planted_genome(seed)[:2] for name, seed in (("chr2", 0), ("chr10", 1), ("chrX", 2))}
    d = os.path.join(str(tmp_path), "jd")
    for name, (X, Y) in data.items():                                # creation order chr2, chr10, chrX; string order chr10, chr2, chrX
        _write_jd(d, name, X, Y)
    import joblib
    joblib.dump(np.zeros((3, 3), np.int64), os.path.join(d, "chr2-chr10.jd"))        # a trans file is left out
    pipe.CACHE.clear()
    out = os.path.join(str(tmp_path), "direct")
    js = domains.jd2domains(d, out)
    pipe.CACHE.clear()
    want = _host_texts(data, ["chr10", "chr2", "chrX"], 10000, [10], 0, 20, 0.05, 500, 1.0)
    assert _files(out, [10]) == want                                  # every file byte for byte
    assert list(js["chroms"]) == ["chr10", "chr2", "chrX"] and js["total"]["domains"] == 36 and js["total"]["significant"] == 36
    assert js["total"]["domains"] == want["_domains.txt"].count("\n") - 1 == want["_domains.bed"].count("\n")
    out = os.path.join(str(tmp_path), "cli")
    _run_module(["-d", d, "-o", out, "-res", "5000", "-w", "20,8", "-cut", "2000", "-mincov", "50", "-delta", "0.1", "-maxbins", "100",
                 "-escut", "6", "-c", "chr2,chrX"], str(tmp_path))
    want = _host_texts(data, ["chr2", "chrX"], 5000, [8, 20], 2000, 50, 0.1, 100, 6.0)
    assert _files(out, [8, 20]) == want
    js = json.loads(want["_domains.json"])
    assert js["w"] == [8, 20] and 0 < js["total"]["significant"] < js["total"]["domains"]


def test_domains_flag_of_the_main_command(tmp_path):
    """-domains on the chr21 BEDPE example writes what the host functions make of the oracle's integers and leaves the loops what
    they were"""
    import gzip
    from cloops_amd import pipe
    X, Y = G.chr21_xy()
    bed = os.path.join(str(tmp_path), "in.bedpe.gz")
    with gzip.open(bed, "wt") as fh:                       # a BEDPE whose mid-points are exactly (X, Y)
        for x, y in zip(X.tolist(), Y.tolist()):
            fh.write("chr21\t%d\t%d\tchr21\t%d\t%d\tid\t1\t+\t-\n" % (x, x, y, y))
    fout = os.path.join(str(tmp_path), "run")
    pipe.CACHE.clear()
    assert pipe.main(["-f", bed, "-o", fout, "-m", "0", "-eps", "500,1000,2000", "-minPts", "5", "-domains", "-domres", "5000",
                      "-domw", "20,10"]) == 0
    pipe.CACHE.clear()
    assert open(fout + ".loop").read() == open(os.path.join(G.GOLD, "chr21_v2.loop")).read()      # identical with and without the flag
    got = _files(fout, [10, 20])
    js = json.loads(got["_domains.json"])
    assert js["chroms"]["chr21"]["20"] == {"n_kept": 99674, "bins": 8333, "bin0": 1006, "valid": js["chroms"]["chr21"]["20"]["valid"],
                                           "boundaries": 65, "domains": 59, "significant": 40}
    assert js["res"] == 5000 and js["w"] == [10, 20]
    assert got == _host_texts({"chr21": (X, Y)}, ["chr21"], 5000, [10, 20], 0, 20, 0.05, 500, 1.0)
