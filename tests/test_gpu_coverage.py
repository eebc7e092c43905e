"""GPU: kernel K20 (cl_cov_build / runs / text / chunks / render) against two numpy oracles written from the definitions of
include/cloops_hip.h (neither calls cloops_amd.coverage): an events oracle that works at any coordinate and a per-base difference
array for the small cases; in every case the area is also compared with the sum of the interval lengths, which needs neither.
Degenerate sizes, hand-placed intervals, clamped starts, bins, pile-ups beyond any LDS tile, dense and sparse random sets, every tile
size of the kernels, cuts, the exact bytes of the text, repeatability, the handle's other results (unchanged), argument errors, the
chr21 example against pinned values, the command line and -bdg on the main command."""
import ctypes
import json
import os

import numpy as np
import pytest

import golden_util as G

pytestmark = pytest.mark.gpu

EMPTY = np.zeros(0, np.int64)


# ---- the oracles ---------------------------------------------------------------------------------
def intervals(X, Y, cut, ends, ext, res):
    """-> (start, end) int64 of the non-empty intervals, and the number of end points (empty intervals included)"""
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    if cut > 0:
        keep = (Y - X) >= cut
        X, Y = X[keep], Y[keep]
    p = np.concatenate(([X] if ends & 1 else []) + ([Y] if ends & 2 else []) + [EMPTY])
    if res == 0:
        s, e = np.maximum(0, p - ext), p + ext
    else:
        b = (p // res) * res                                           # numpy's // floors, also for negative p
        s, e = np.maximum(0, b), b + res
    ok = e > s
    return s[ok], e[ok], len(p)


def merge_runs(st, en, dp):
    """stretches in ascending order -> zero depth dropped, abutting stretches of equal depth merged"""
    k = dp > 0
    st, en, dp = st[k], en[k], dp[k]
    if len(st) == 0:
        return EMPTY, EMPTY, EMPTY
    first = np.ones(len(st), bool)
    first[1:] = (st[1:] != en[:-1]) | (dp[1:] != dp[:-1])
    idx = np.flatnonzero(first)
    last = np.append(idx[1:] - 1, len(st) - 1)
    return st[idx], en[last], dp[idx]


def events_oracle(s, e):
    """unique positions, summed +-1, cumsum, drop zero depth, merge abutting equal depths"""
    if len(s) == 0:
        return EMPTY, EMPTY, EMPTY
    pos = np.concatenate([s, e])
    delta = np.concatenate([np.ones(len(s), np.int64), -np.ones(len(e), np.int64)])
    u, inv = np.unique(pos, return_inverse=True)
    d = np.zeros(len(u), np.int64)
    np.add.at(d, inv, delta)
    depth = np.cumsum(d)
    return merge_runs(u[:-1], u[1:], depth[:-1])


def per_base_oracle(s, e):
    """a difference array over every base, then one stretch per base, merged"""
    if len(s) == 0:
        return EMPTY, EMPTY, EMPTY
    L = int(e.max())
    d = np.zeros(L + 1, np.int64)
    np.add.at(d, s, 1)
    np.add.at(d, e, -1)
    depth = np.cumsum(d)[:L]
    t = np.arange(L, dtype=np.int64)
    return merge_runs(t, t + 1, depth)


def check(ch, X, Y, cut=0, ends=3, ext=75, res=0, per_base=False):
    """build on the handle, compare runs and totals with the oracle(s) -> (start, end, depth) int64"""
    s, e, n_ends = intervals(X, Y, cut, ends, ext, res)
    want = events_oracle(s, e)
    if per_base:
        pb = per_base_oracle(s, e)
        assert all(np.array_equal(a, b) for a, b in zip(want, pb))     # the two oracles agree
    nr, md, ne, area = ch.coverage_build(cut, ends, ext, res)
    gs, ge, gd = ch.coverage_runs()
    assert gs.dtype == np.int32 and ge.dtype == np.int32 and gd.dtype == np.uint32
    assert ne == n_ends
    assert nr == len(want[0]) == len(gs)
    assert np.array_equal(gs, want[0]) and np.array_equal(ge, want[1]) and np.array_equal(gd, want[2])
    assert md == (int(want[2].max()) if len(want[2]) else 0)
    assert area == int((e - s).sum())                                  # independent of both oracles
    assert area == int((want[2] * (want[1] - want[0])).sum())
    return want


def fmt_value(depth, scale):
    if scale is None:
        return str(int(depth))
    q = (int(depth) * scale[0] + scale[1] // 2) // scale[1]
    return "%d.%03d" % (q // 1000, q % 1000)


def fmt_runs(name, runs, scale=None):
    return "".join("%s\t%d\t%d\t%s\n" % (name, s, e, fmt_value(d, scale)) for s, e, d in zip(*[a.tolist() for a in runs])).encode()


def far(X):
    """a Y for rows whose X alone matters (ends = 1)"""
    return np.asarray(X, np.int64) + 1000000


def chrom(X, Y):
    from cloops_amd import api
    return api.Chromosome(np.asarray(X, np.int64), np.asarray(Y, np.int64))


# ---- degenerate sizes ------------------------------------------------------------------------------
def test_degenerate_sizes():
    ch = chrom(EMPTY, EMPTY)
    assert ch.coverage_build() == (0, 0, 0, 0)
    assert all(len(a) == 0 for a in ch.coverage_runs())
    assert ch.coverage_text("chr1") == 0 and list(ch.coverage_iter(4096)) == []
    assert ch.coverage_build(res=10) == (0, 0, 0, 0)
    ch.coverage_free()
    ch.close()
    ch = chrom([1000], [5000])
    r = check(ch, [1000], [5000], per_base=True)
    assert [a.tolist() for a in r] == [[925, 4925], [1075, 5075], [1, 1]]
    check(ch, [1000], [5000], res=100, per_base=True)
    assert ch.coverage_build(cut=4001) == (0, 0, 0, 0)                 # the cut removes every row
    assert ch.coverage_text("chr1") == 0 and list(ch.coverage_iter(4096)) == []
    check(ch, [1000], [5000], cut=4000, per_base=True)
    ch.close()
    X, Y = np.array([100, 400, 400, 900, 901]), np.array([400, 400, 700, 900, 2000])      # rows with X == Y among them
    ch = chrom(X, Y)
    for ends in (1, 2, 3):
        for ext, res in ((75, 0), (1, 0), (0, 50)):
            check(ch, X, Y, ends=ends, ext=ext, res=res, per_base=True)
    assert ch.coverage_build(ends=3)[2] == 10 and ch.coverage_build(ends=1)[2] == 5
    ch.close()


# ---- hand-placed intervals, window mode -------------------------------------------------------------
@pytest.mark.parametrize("ext", [1, 2, 75])
def test_hand_placed_windows(ext):
    p1, k = 1000, 5

    def runs_of(P):
        ch = chrom(P, far(P))
        r = check(ch, P, far(P), ends=1, ext=ext, per_base=True)
        ch.close()
        return [a.tolist() for a in r]

    assert runs_of([p1, p1 + 2 * ext]) == [[p1 - ext], [p1 + 3 * ext], [1]]                        # abutting, equal depth: one run
    assert runs_of([p1, p1 + 2 * ext + 1])[0] == [p1 - ext, p1 + ext + 1]                          # a gap of one base: two runs
    r = runs_of([p1, p1 + 2 * ext - 1])                                                            # one base of overlap: three runs
    assert r == [[p1 - ext, p1 + ext - 1, p1 + ext], [p1 + ext - 1, p1 + ext, p1 + 3 * ext - 1], [1, 2, 1]]
    assert runs_of([p1] * k + [p1 + 2 * ext] * k) == [[p1 - ext], [p1 + 3 * ext], [k]]             # +k and -k cancel: one run
    r = runs_of([p1] * k + [p1 + 2 * ext] * (k + 1))                                               # k end where k + 1 begin
    assert r == [[p1 - ext, p1 + ext], [p1 + ext, p1 + 3 * ext], [k, k + 1]]
    r = runs_of([p1 + 2 * ext] * k + [p1] * (k + 1) + [p1 + 4 * ext] * k)                          # both at once, rows in another order
    assert r == [[p1 - ext, p1 + ext], [p1 + ext, p1 + 5 * ext], [k + 1, k]]                        # ... and the two stretches of k are one run


def test_clamped_starts():
    ext = 75
    P = np.array([0, 3, 10, 74, 75, 76, -75, -80, -74, -1, 200, 0])
    ch = chrom(P, far(P))
    r = check(ch, P, far(P), ends=1, ext=ext, per_base=True)
    assert r[0][0] == 0 and ch.coverage_build(ends=1, ext=ext)[2] == len(P)     # p + ext <= 0 is dropped, and still counted
    ch.close()
    for P in ([-75], [-74], [-75, -76, -1000], [75], [0], [-74, -74, 0, 75]):
        ch = chrom(P, far(P))
        r = check(ch, P, far(P), ends=1, ext=ext, per_base=True)
        ch.close()
        if P == [-74]:
            assert [a.tolist() for a in r] == [[0], [1], [1]]
        if P == [-75, -76, -1000]:
            assert len(r[0]) == 0


# ---- bin mode ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [1, 7, 1000])
def test_bins(res):
    k = 5
    P = [k * res - 1, k * res, k * res + res - 1,                       # last base of bin k - 1, first and last base of bin k
         (k + 1) * res, (k + 1) * res + res // 2,                       # bin k + 1 holds two as bin k does: they merge
         (k + 2) * res, (k + 2) * res, (k + 2) * res + res - 1,         # bin k + 2 holds three: it does not
         (k + 4) * res,                                                 # a bin left empty in between
         0, res - 1, -1, -res, -res - 1, -3 * res]                      # bin 0, and negative p: bins -1, -1, -2, -3, all empty
    ch = chrom(P, far(P))
    r = check(ch, P, far(P), ends=1, ext=0, res=res, per_base=True)
    assert [a.tolist() for a in r] == [[0, (k - 1) * res, k * res, (k + 2) * res, (k + 4) * res],
                                       [res, k * res, (k + 2) * res, (k + 3) * res, (k + 5) * res], [2, 1, 2, 3, 1]]
    assert ch.coverage_build(ends=1, ext=0, res=res)[2] == len(P)
    check(ch, P, far(P), ends=3, res=res)
    ch.close()
    rng = np.random.default_rng(res)
    X = rng.integers(-3 * res, 40 * res + 5, 3000)
    Y = X + rng.integers(0, 7 * res, 3000)
    ch = chrom(X, Y)
    check(ch, X, Y, res=res, per_base=True)
    check(ch, X, Y, cut=2 * res, ends=2, res=res, per_base=True)
    ch.close()


# ---- pile-ups: more points in a window than any tile holds ------------------------------------------
def test_all_points_equal():
    n, p = 70000, 123456
    X = np.full(n, p)
    ch = chrom(X, X)
    r = check(ch, X, X)
    assert [a.tolist() for a in r] == [[p - 75], [p + 75], [2 * n]]                  # beyond a 16-bit counter
    check(ch, X, X, res=1000)
    ch.close()
    rng = np.random.default_rng(5)
    X = p + rng.integers(0, 100, n)                                                  # spread over fewer than 2 ext bases
    Y = X + rng.integers(0, 40, n)
    ch = chrom(X, Y)
    r = check(ch, X, Y, per_base=True)
    assert int(r[2].max()) == 2 * n
    check(ch, X, Y, ext=3, per_base=True)
    ch.close()


def test_dense_random():
    rng = np.random.default_rng(20)
    a, b = rng.integers(0, 20000, 50000), rng.integers(0, 20000, 50000)
    X, Y = np.minimum(a, b), np.maximum(a, b)
    ch = chrom(X, Y)
    check(ch, X, Y, ext=5000, per_base=True)                                         # a window holds tens of thousands of points
    check(ch, X, Y, ext=1, per_base=True)
    ch.close()


@pytest.mark.parametrize("ext", [1, (1 << 29) - 1])
def test_sparse_random(ext):
    rng = np.random.default_rng(29)
    a, b = rng.integers(0, 1 << 29, 5000), rng.integers(0, 1 << 29, 5000)
    X, Y = np.minimum(a, b), np.maximum(a, b)
    X[0], Y[0], Y[1] = 0, (1 << 29) - 1, (1 << 29) - 1
    ch = chrom(X, Y)
    check(ch, X, Y, ext=ext)
    check(ch, X, Y, ends=2, ext=ext)
    ch.close()


# ---- tile edges -------------------------------------------------------------------------------------
TPB = 256            # cl_common.h TPB: threads of a workgroup; elements per pass of a thread's loop in k20_breaks
K20_T = 256          # k_cover.hip K20_T: lines per render tile
K20_TILE = 1024      # k_cover.hip K20_TILE: sorted end points per workgroup of k20_breaks
K20_HALO = 1024      # k_cover.hip K20_HALO: end points staged in LDS on either side of a tile
K20_ROWS = 2048      # k_cover.hip K20_ROWS: rows per workgroup of the key pass (TPB * K20_ITEMS)
EDGES = sorted({TPB, K20_T, K20_TILE, K20_HALO, K20_ROWS, K20_TILE + K20_HALO, 2 * K20_TILE, K20_TILE + 2 * K20_HALO, 2 * K20_ROWS})


@pytest.mark.parametrize("size", EDGES)
def test_tile_edges(size):
    """n_ends one below, at and one above `size`, rows in random order; then with one value repeated across sorted positions
    size - 3 .. size + 2 (and across every multiple of K20_TILE), so that a group of equal break points starts in one tile and ends
    in the next; a narrow window (searches stay in LDS) and a wide one (they leave it)"""
    rng = np.random.default_rng(size)
    for n in (size - 1, size, size + 1):
        P = np.sort(rng.integers(0, 4 * n, n))
        for straddle in (False, True):
            if straddle:
                for edge in sorted(set(list(range(K20_TILE, n, K20_TILE)) + [size])):
                    lo, hi = max(0, edge - 3), min(n, edge + 3)
                    P[lo:hi] = P[lo]
                assert np.all(np.diff(P) >= 0)
            X = P[rng.permutation(n)]
            ch = chrom(X, far(X))
            for ext in (2, n):
                check(ch, X, far(X), ends=1, ext=ext, per_base=True)
            check(ch, X, far(X), ends=1, res=3, per_base=True)
            ch.close()
    n = size // 2                                                                    # both ends: n_ends = size exactly, from size / 2 rows
    X = rng.integers(0, 4 * size, n)
    Y = X + rng.integers(0, 50, n)
    ch = chrom(X, Y)
    assert check(ch, X, Y, ext=10, per_base=True) is not None and ch.coverage_build(ext=10)[2] == 2 * n
    ch.close()


# ---- cut --------------------------------------------------------------------------------------------
def test_cut_and_rebuild():
    rng = np.random.default_rng(7)
    X = rng.integers(0, 50000, 4000)
    Y = X + rng.integers(0, 3000, 4000)
    Y[:10] = X[:10] + 1500                                                           # rows exactly at the cut stay
    Y[10:20] = X[10:20] + 1499
    ch = chrom(X, Y)
    a = check(ch, X, Y, cut=1500, per_base=True)
    b = check(ch, X, Y, cut=0, per_base=True)                                        # the scratch is rebuilt, not reused
    c = check(ch, X, Y, cut=2900, ends=1, per_base=True)
    a2 = check(ch, X, Y, cut=1500, per_base=True)
    assert len(a[0]) != len(b[0]) and len(c[0]) != len(a[0]) and all(np.array_equal(u, v) for u, v in zip(a, a2))
    assert ch.coverage_build(cut=1500)[2] == 2 * int((Y - X >= 1500).sum())
    ch.close()


# ---- text, exact bytes ------------------------------------------------------------------------------
def text_of(ch, budget):
    chunks = [bytes(mv) for mv in ch.coverage_iter(budget)]
    return b"".join(chunks), chunks


def test_text_chunks():
    from cloops_amd import api
    rng = np.random.default_rng(14)
    X = rng.integers(0, 3000000, 3000)
    Y = X + rng.integers(0, 20000, 3000)
    ch = chrom(X, Y)
    runs = check(ch, X, Y, ext=40)
    name = "chr21"
    want = fmt_runs(name, runs)
    assert ch.coverage_text(name) == len(want)
    got, chunks = text_of(ch, 1 << 20)
    assert got == want and len(chunks) == 1
    budget = 2000
    run_b, byte_b = ch.coverage_chunks(budget)
    K = len(run_b) - 1
    assert K >= 24                                                                   # dozens of chunks
    assert run_b[0] == 0 and byte_b[0] == 0 and run_b[-1] == len(runs[0]) and byte_b[-1] == len(want)
    assert np.all(np.diff(run_b) > 0) and np.all(np.diff(byte_b) > 0) and np.all(np.diff(byte_b) <= budget)      # no chunk is empty
    lines = want.split(b"\n")[:-1]
    ends = np.cumsum([len(l) + 1 for l in lines])
    assert np.array_equal(byte_b[1:], ends[run_b[1:] - 1])                           # a bound is never inside a line
    parts = [ch.coverage_render(k) for k in range(K)]
    assert all(p.endswith(b"\n") for p in parts) and b"".join(parts) == want
    assert [len(p) for p in parts] == np.diff(byte_b).tolist()
    got, chunks = text_of(ch, budget)
    assert got == want and len(chunks) == K
    long_name = "c" * api.Chromosome.TRACK_NAME_MAX                                  # a name of CL_TRACK_NAME_MAX bytes
    want = fmt_runs(long_name, runs)
    assert ch.coverage_text(long_name) == len(want)
    assert text_of(ch, 5000)[0] == want
    ch.close()
    ch = chrom(X[:100], Y[:100])                                                     # the smallest budget allowed: a line per chunk
    runs = check(ch, X[:100], Y[:100], ext=40)
    want = fmt_runs(long_name, runs)
    assert ch.coverage_text(long_name) == len(want)
    got, chunks = text_of(ch, api.Chromosome.TRACK_NAME_MAX + 44)
    assert got == want and len(chunks) == len(runs[0])
    ch.close()


DIGIT_COUNTS = (1, 9, 10, 99999, 100000)
SCALES = ((1, 2),                    # even den, remainder exactly den / 2 at odd depths: rounds up; q < 1000 and q % 1000 < 10
          (1000, 3),                 # odd den
          (10 ** 9, 200019),         # counts per million of this set
          (1 << 30, 1),              # the largest numerator
          (1000, 1),                 # the depth itself with ".000"
          (7, 1000),                 # q = 0 for small depths: "0.000"
          (5, 10))                   # remainder exactly den / 2 at every odd depth


def test_text_digits_and_fixed_point():
    X = np.concatenate([np.full(c, 10000 * (k + 1)) for k, c in enumerate(DIGIT_COUNTS)])
    ch = chrom(X, far(X))
    runs = check(ch, X, far(X), ends=1, ext=75)
    assert runs[2].tolist() == list(DIGIT_COUNTS) and len(X) == SCALES[2][1]
    want = fmt_runs("chrX", runs)
    assert ch.coverage_text("chrX") == len(want) and text_of(ch, 4096)[0] == want
    assert want.split(b"\n")[3] == b"chrX\t39925\t40075\t99999"
    for scale in SCALES:
        want = fmt_runs("chrX", runs, scale)
        assert ch.coverage_text("chrX", scale) == len(want)
        assert text_of(ch, 4096)[0] == want, scale
    assert fmt_runs("chrX", runs, (1, 2)).split(b"\n")[0] == b"chrX\t9925\t10075\t0.001"
    assert fmt_runs("chrX", runs, (1000, 3)).split(b"\n")[2].endswith(b"\t3.333")
    ch.close()
    rng = np.random.default_rng(3)                                                   # many depths under an odd and an even scale
    X = rng.integers(0, 3000, 20000)
    ch = chrom(X, far(X))
    runs = check(ch, X, far(X), ends=1, ext=30, per_base=True)
    for scale in ((10 ** 9, 20000), (999, 7), (1, 2)):
        want = fmt_runs("chr1", runs, scale)
        assert ch.coverage_text("chr1", scale) == len(want) and text_of(ch, 3000)[0] == want, scale
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
    a = ch.coverage_build()
    ra = ch.coverage_runs()
    ta = (ch.coverage_text("chr21"), text_of(ch, 1 << 18)[0])
    b = ch.coverage_build()
    rb = ch.coverage_runs()
    tb = (ch.coverage_text("chr21"), text_of(ch, 1 << 18)[0])
    assert a == b and ta == tb and all(np.array_equal(u, v) for u, v in zip(ra, rb))
    ch.coverage_build(cut=4601, ends=1, res=5000)
    assert ch.track_render(3) == trk0                                                # the built washU track is still there
    assert np.array_equal(ch.cluster("v2", 1000, 5).labels, lab0)
    agg1 = ch.agg_loops([20000000, 30000000], [20100000, 30200000], 1000, 10, 3, want_mats=True)
    assert all(np.array_equal(u, v) for u, v in zip(agg0[:3], agg1[:3])) and agg0[3] == agg1[3]
    c = ch.coverage_build()                                                          # and the coverage after them
    assert c == a and all(np.array_equal(u, v) for u, v in zip(ra, ch.coverage_runs()))
    s, e, d = ch.coverage_runs(5, 7)                                                 # a range of runs
    assert np.array_equal(s, ra[0][5:12]) and np.array_equal(e, ra[1][5:12]) and np.array_equal(d, ra[2][5:12])
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
    nr, md, ne, ar, nb, nc = (ctypes.c_int64(0), ctypes.c_uint32(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0),
                              ctypes.c_int64(0))
    outs = (ctypes.byref(nr), ctypes.byref(md), ctypes.byref(ne), ctypes.byref(ar))
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    s3, e3, d3 = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.uint32)
    buf = np.zeros(1 << 16, np.uint8)
    rb, bb = np.zeros(8, np.int64), np.zeros(8, np.int64)
    # text / chunks / render / runs without a build
    assert lib.cl_cov_text(ch._h, b"chr21", 0, 0, ctypes.byref(nb)) == E
    assert lib.cl_cov_chunks(ch._h, 4096, 0, None, None, ctypes.byref(nc)) == E
    assert lib.cl_cov_render(ch._h, 0, vp(buf), len(buf), ctypes.byref(nb)) == E
    assert lib.cl_cov_runs(ch._h, 0, 1, vp(s3), vp(e3), vp(d3)) == E
    # build: a NULL handle, NULL outputs, ends, ext, res
    build = lib.cl_cov_build
    assert build(None, 0, 3, 75, 0, *outs) == E
    for k in range(4):
        assert build(ch._h, 0, 3, 75, 0, *[None if j == k else o for j, o in enumerate(outs)]) == E
    assert build(ch._h, 0, 0, 75, 0, *outs) == E and build(ch._h, 0, 4, 75, 0, *outs) == E          # ends outside 1..3
    assert build(ch._h, 0, 3, 0, 0, *outs) == E and build(ch._h, 0, 3, -1, 0, *outs) == E           # ext < 1 in window mode
    assert build(ch._h, 0, 3, 1 << 29, 0, *outs) == E                                               # ext >= 2^29
    assert build(ch._h, 0, 3, 0, -1, *outs) == E and build(ch._h, 0, 3, 0, 1 << 29, *outs) == E     # res < 0, res >= 2^29
    assert build(ch._h, 0, 3, 75, 1000, *outs) == E                                                 # res > 0 with ext != 0
    assert b"cl_cov_build" in lib.cl_last_error()
    assert lib.cl_cov_runs(ch._h, 0, 1, vp(s3), vp(e3), vp(d3)) == E                                # a refused build builds nothing
    assert build(ch._h, 0, 3, (1 << 29) - 1, 0, *outs) == 0 and md.value == 199348                  # the largest ext: every start at 0
    assert build(ch._h, 0, 3, 0, (1 << 29) - 1, *outs) == 0 and (nr.value, md.value) == (1, 199348) # the largest res: one bin
    assert build(ch._h, 0, 3, 75, 0, *outs) == 0 and nr.value == 305609
    # runs: a range outside them, NULL outputs
    assert lib.cl_cov_runs(None, 0, 1, vp(s3), vp(e3), vp(d3)) == E
    assert lib.cl_cov_runs(ch._h, -1, 1, vp(s3), vp(e3), vp(d3)) == E
    assert lib.cl_cov_runs(ch._h, 0, -1, vp(s3), vp(e3), vp(d3)) == E
    assert lib.cl_cov_runs(ch._h, 305608, 2, vp(s3), vp(e3), vp(d3)) == E
    assert lib.cl_cov_runs(ch._h, 305610, 0, vp(s3), vp(e3), vp(d3)) == E
    assert lib.cl_cov_runs(ch._h, 0, 1, None, vp(e3), vp(d3)) == E
    assert lib.cl_cov_runs(ch._h, 305609, 0, None, None, None) == 0
    assert lib.cl_cov_runs(ch._h, 305605, 4, vp(s3), vp(e3), vp(d3)) == 0 and (s3[3], e3[3], d3[3]) == (46688371, 46688521, 1)
    # chunks before the text
    assert lib.cl_cov_chunks(ch._h, 4096, 0, None, None, ctypes.byref(nc)) == E
    # text: NULLs, a name too long, the scale
    text = lib.cl_cov_text
    assert text(None, b"chr21", 0, 0, ctypes.byref(nb)) == E
    assert text(ch._h, None, 0, 0, ctypes.byref(nb)) == E and text(ch._h, b"chr21", 0, 0, None) == E
    assert text(ch._h, b"c" * (_lib.CL_TRACK_NAME_MAX + 1), 0, 0, ctypes.byref(nb)) == E
    assert text(ch._h, b"chr21", (1 << 30) + 1, 5, ctypes.byref(nb)) == E                           # scale_num out of range
    assert text(ch._h, b"chr21", -1, 5, ctypes.byref(nb)) == E and text(ch._h, b"chr21", 0, 5, ctypes.byref(nb)) == E
    assert text(ch._h, b"chr21", 5, -1, ctypes.byref(nb)) == E
    assert b"cl_cov_text" in lib.cl_last_error()
    assert lib.cl_cov_render(ch._h, 0, vp(buf), len(buf), ctypes.byref(nb)) == E                    # a refused text leaves no chunks
    assert text(ch._h, b"chr21", 0, 0, ctypes.byref(nb)) == 0 and nb.value > 0
    total = nb.value                                                                                # (a refused call zeroes its outputs)
    # chunks: the budget, the capacity; render: the index, the capacity
    chunks = lib.cl_cov_chunks
    assert chunks(None, 4096, 0, None, None, ctypes.byref(nc)) == E
    assert chunks(ch._h, 4096, 0, None, None, None) == E
    assert chunks(ch._h, 4096, 8, vp(rb), None, ctypes.byref(nc)) == E
    assert chunks(ch._h, len(b"chr21") + 43, 0, None, None, ctypes.byref(nc)) == E                  # below the longest possible line
    assert lib.cl_cov_render(ch._h, 0, vp(buf), len(buf), ctypes.byref(nb)) == E                    # no chunks made yet
    assert chunks(ch._h, total // 3 + 4096, 0, None, None, ctypes.byref(nc)) == 0 and 3 <= nc.value <= 4
    assert chunks(ch._h, total // 3 + 4096, nc.value, vp(rb), vp(bb), ctypes.byref(nc)) == E     # capacity below n_chunks + 1
    assert chunks(ch._h, 1 << 15, 0, None, None, ctypes.byref(nc)) == 0 and nc.value > 8
    render = lib.cl_cov_render
    assert render(None, 0, vp(buf), len(buf), ctypes.byref(nb)) == E
    assert render(ch._h, 0, None, len(buf), ctypes.byref(nb)) == E and render(ch._h, 0, vp(buf), len(buf), None) == E
    assert render(ch._h, -1, vp(buf), len(buf), ctypes.byref(nb)) == E
    assert render(ch._h, nc.value, vp(buf), len(buf), ctypes.byref(nb)) == E
    assert render(ch._h, 0, vp(buf), 100, ctypes.byref(nb)) == E                                    # capacity below the chunk's bytes
    assert render(ch._h, 0, vp(buf), len(buf), ctypes.byref(nb)) == 0 and bytes(buf[:nb.value]).endswith(b"\n")
    assert bytes(buf[:nb.value]).startswith(b"chr21\t5033778\t5033928\t1\n")
    assert lib.cl_cov_free(None) == E
    # the Python layer
    with pytest.raises(ValueError):
        ch.coverage_text("chr21", (5, 0))
    with pytest.raises(_lib.CloopsHipError):
        ch.coverage_build(ends=7)
    # runs in flight
    assert build(ch._h, 0, 3, 75, 0, *outs) == 0
    ch.cluster_async("v2", 2000, 5)
    assert build(ch._h, 0, 3, 75, 0, *outs) == E
    assert lib.cl_cov_runs(ch._h, 0, 1, vp(s3), vp(e3), vp(d3)) == E
    assert text(ch._h, b"chr21", 0, 0, ctypes.byref(nb)) == E
    assert chunks(ch._h, 4096, 0, None, None, ctypes.byref(nc)) == E
    assert render(ch._h, 0, vp(buf), len(buf), ctypes.byref(nb)) == E
    assert lib.cl_cov_free(ch._h) == E
    ch.wait()
    assert ch.coverage_build() == (305609, 326, 199348, 29902200)                    # the handle still works
    ch.close()


# ---- the chr21 example ----------------------------------------------------------------------------------
PINNED = (((0, 3, 75, 0), 199348, 305609, 326, 29902200),
          ((4601, 3, 75, 0), 106694, 152472, 149, 16004100),
          ((0, 1, 500, 0), 99674, 184672, 455, 99674000),
          ((0, 2, 1, 0), 99674, 97032, 12, 199348),
          ((0, 3, 0, 1000), 199348, 26718, 749, 199348000),
          ((4601, 3, 0, 5000), 106694, 6030, 448, 533470000))


@pytest.fixture(scope="module")
def chr21():
    X, Y = G.chr21_xy()
    assert len(X) == 99674
    ch = chrom(X, Y)
    yield ch, X, Y
    ch.close()


@pytest.mark.parametrize("args,n_ends,n_runs,max_depth,area", PINNED)
def test_chr21_pinned(chr21, args, n_ends, n_runs, max_depth, area):
    ch, X, Y = chr21
    cut, ends, ext, res = args
    runs = check(ch, X, Y, cut, ends, ext, res)
    assert ch.coverage_build(cut, ends, ext, res) == (n_runs, max_depth, n_ends, area)
    if args == (0, 3, 75, 0):
        assert tuple(int(a[0]) for a in runs) == (5033778, 5033928, 1) and tuple(int(a[-1]) for a in runs) == (46688371, 46688521, 1)


# ---- the command line ------------------------------------------------------------------------------------
def _write_jd(d, name, X, Y):
    import joblib
    os.makedirs(d, exist_ok=True)
    joblib.dump(np.stack([np.arange(len(X)), X, Y], 1).astype(np.int64), os.path.join(d, "%s-%s.jd" % (name, name)))


def _run_module(args, cwd):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "cloops_amd.coverage"] + args, env=env, cwd=cwd, timeout=300, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_command_line(tmp_path):
    rng = np.random.default_rng(11)
    d = os.path.join(str(tmp_path), "jd")
    data = {}
    for name, n in (("chr2", 3000), ("chr10", 2000), ("chrX", 500)):                 # creation order; string order: chr10, chr2, chrX
        X = rng.integers(0, 400000, n)
        data[name] = (X, X + rng.integers(0, 30000, n))
        _write_jd(d, name, *data[name])
    import joblib
    joblib.dump(np.zeros((3, 3), np.int64), os.path.join(d, "chr2-chr10.jd"))        # a trans file is left out
    for norm, extra, names in (("none", [], ["chr10", "chr2", "chrX"]),
                               ("cpm", ["-norm", "cpm", "-c", "chr2,chr10", "-ext", "40", "-cut", "1000", "-ends", "left"], ["chr10", "chr2"])):
        out = os.path.join(str(tmp_path), "cli_" + norm + str(len(extra)))
        _run_module(["-d", d, "-o", out] + extra, str(tmp_path))
        cut = 1000 if "-cut" in extra else 0
        ends = 1 if "left" in extra else 2 if "right" in extra else 3
        res = 500 if "-res" in extra else 0
        ext = 40 if "-ext" in extra else 75
        runs, stats = {}, {}
        for name in names:
            s, e, n_ends = intervals(*data[name], cut, ends, ext, res)
            runs[name] = events_oracle(s, e)
            stats[name] = {"n_runs": len(runs[name][0]), "max_depth": int(runs[name][2].max()), "n_ends": n_ends, "area": int((e - s).sum())}
        scale = (10 ** 9, sum(st["n_ends"] for st in stats.values())) if norm == "cpm" else None
        want = b"".join(fmt_runs(name, runs[name], scale) for name in names)
        assert open(out + ".bedGraph", "rb").read() == want
        with open(out + "_bedGraph.json") as fh:
            js = json.load(fh)
        assert js["chroms"] == stats and list(js["chroms"]) == sorted(names)
        assert (js["ext"], js["res"], js["cut"], js["ends"], js["norm"]) == (ext, res, cut, ends, norm)
        assert js["total"] == {"n_runs": sum(st["n_runs"] for st in stats.values()), "max_depth": max(st["max_depth"] for st in stats.values()),
                               "n_ends": sum(st["n_ends"] for st in stats.values()), "area": sum(st["area"] for st in stats.values())}


def test_bdg_flag_of_the_main_command(tmp_path):
    """-bdg on the chr21 BEDPE example writes the bytes the module writes from the .jd files that -s leaves behind"""
    import gzip
    from cloops_amd import pipe
    X, Y = G.chr21_xy()
    bed = os.path.join(str(tmp_path), "in.bedpe.gz")
    with gzip.open(bed, "wt") as fh:                       # a BEDPE whose mid-points are exactly (X, Y)
        for x, y in zip(X.tolist(), Y.tolist()):
            fh.write("chr21\t%d\t%d\tchr21\t%d\t%d\tid\t1\t+\t-\n" % (x, x, y, y))
    fout = os.path.join(str(tmp_path), "run")
    pipe.CACHE.clear()
    assert pipe.main(["-f", bed, "-o", fout, "-m", "0", "-eps", "500,1000,2000", "-minPts", "5", "-s", "-bdg", "-bdgext", "60"]) == 0
    pipe.CACHE.clear()
    assert os.path.isfile(fout + ".loop") and os.path.isfile(os.path.join(fout, "chr21-chr21.jd"))
    out = os.path.join(str(tmp_path), "again")
    _run_module(["-d", fout, "-o", out, "-ext", "60"], str(tmp_path))
    got = open(fout + ".bedGraph", "rb").read()
    assert got == open(out + ".bedGraph", "rb").read()
    s, e, n_ends = intervals(X, Y, 0, 3, 60, 0)
    assert got == fmt_runs("chr21", events_oracle(s, e))
    with open(fout + "_bedGraph.json") as fh:
        js = json.load(fh)
    assert js["chroms"]["chr21"]["n_ends"] == n_ends == 199348 and js["ext"] == 60 and js["norm"] == "none"
    assert open(fout + ".loop").read() == open(os.path.join(G.GOLD, "chr21_v2.loop")).read()      # the loops are what they were
