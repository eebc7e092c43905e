"""GPU: kernel K19 (cl_agg_loops) against a numpy brute force written from the definitions of include/cloops_hip.h (it does not call
cloops_amd.agg): random sets, hand-placed PETs at every window and bin boundary, pile-ups, many loops, edge cases, argument errors,
repeatability, its effect on the handle's other results (none), the chr21 loops against pinned values, the command line and -agg on
the main command."""
import ctypes
import json
import os

import numpy as np
import pytest

import golden_util as G

pytestmark = pytest.mark.gpu

LOOPS = os.path.join(G.GOLD, "chr21_v2.loop")


def brute(X, Y, cx, cy, res, w, corner, cut=0, want_mats=True):
    """-> (S int64 [W, W], stats int32 [n, 6], mats int32 [n, W, W] or None): per loop a mask over the PETs, then np.add.at (a few
    loops at a time, so that the masks of a chunk fit in memory)"""
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    if cut > 0:
        keep = (Y - X) >= cut
        X, Y = X[keep], Y[keep]
    cx, cy = np.asarray(cx, np.int64), np.asarray(cy, np.int64)
    W = 2 * w + 1
    n = len(cx)
    S = np.zeros((W, W), np.int64)
    stats = np.zeros((n, 6), np.int64)
    mats = np.zeros((n, W, W), np.int64) if want_mats else None
    ox = cx - w * res - res // 2
    oy = cy - w * res - res // 2
    chunk = max(1, 4000000 // max(len(X), 1))
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        dx = X[None, :] - ox[a:b, None]
        dy = Y[None, :] - oy[a:b, None]
        inside = (dx >= 0) & (dx < W * res) & (dy >= 0) & (dy < W * res)
        loop, pet = np.nonzero(inside)
        M = np.zeros((b - a, W, W), np.int64)
        np.add.at(M, (loop, dx[loop, pet] // res, dy[loop, pet] // res), 1)
        S += M.sum(0)
        stats[a:b, 0] = M.sum((1, 2))
        stats[a:b, 1] = M[:, w, w]
        stats[a:b, 2] = M[:, W - corner:, :corner].sum((1, 2))
        stats[a:b, 3] = M[:, :corner, :corner].sum((1, 2))
        stats[a:b, 4] = M[:, :corner, W - corner:].sum((1, 2))
        stats[a:b, 5] = M[:, W - corner:, W - corner:].sum((1, 2))
        if want_mats:
            mats[a:b] = M
    return S, stats.astype(np.int32), (mats.astype(np.int32) if want_mats else None)


def _check(ch, X, Y, cx, cy, res, w, corner, cut=0):
    S, stats, mats, kept = ch.agg_loops(cx, cy, res, w, corner, cut, want_stats=True, want_mats=True)
    wS, wstats, wmats = brute(X, Y, cx, cy, res, w, corner, cut)
    W = 2 * w + 1
    assert S.dtype == np.int64 and S.shape == (W, W) and stats.dtype == np.int32 and stats.shape == (len(cx), 6)
    assert mats.dtype == np.int32 and mats.shape == (len(cx), W, W)
    assert np.array_equal(mats, wmats)
    assert np.array_equal(stats, wstats)
    assert np.array_equal(S, wS)
    assert kept == (int(((np.asarray(Y, np.int64) - np.asarray(X, np.int64)) >= cut).sum()) if cut > 0 else len(X))
    return S, stats, mats


@pytest.fixture(scope="module")
def rnd():
    from cloops_amd import api
    rng = np.random.default_rng(19)
    n = 5000
    X = rng.integers(0, 200000, n)
    Y = X + rng.integers(0, 150000, n)
    cx = rng.integers(-30000, 260000, 64)                              # some outside the data
    cy = cx + rng.integers(-5000, 160000, 64)
    k = rng.integers(0, n, 16)
    cx[:16], cy[:16] = X[k], Y[k]                                      # some on a PET
    ch = api.Chromosome(X, Y)
    yield ch, X, Y, cx, cy
    ch.close()


@pytest.mark.parametrize("cut", [0, 3000])
@pytest.mark.parametrize("res,w,corner", [(1, 1, 1), (7, 5, 2), (1000, 10, 3), (5000, 20, 20)])
def test_random(rnd, res, w, corner, cut):
    ch, X, Y, cx, cy = rnd
    S, stats, _ = _check(ch, X, Y, cx, cy, res, w, corner, cut)
    if res >= 1000:
        assert S.sum() > 0 and (stats[:, 0] > 0).sum() > 8             # the case is not vacuous


@pytest.mark.parametrize("res", [1, 2, 7, 10, 1000, 1001])
@pytest.mark.parametrize("centre", [(3, 5), (50000, 90000), (10 ** 8, 10 ** 8 + 777)])
def test_boundaries(res, centre):
    """PETs by hand at X or Y = o - 1, o, o + res - 1, o + res, o + W res - 1, o + W res for both axes; a centre whose window reaches
    below 0; a centre beyond the largest coordinate"""
    from cloops_amd import api
    cx, cy = centre
    for w, corner in ((1, 1), (3, 2)):
        W = 2 * w + 1
        ox, oy = cx - w * res - res // 2, cy - w * res - res // 2
        ex = [ox - 1, ox, ox + res - 1, ox + res, ox + W * res - 1, ox + W * res, cx]
        ey = [oy - 1, oy, oy + res - 1, oy + res, oy + W * res - 1, oy + W * res, cy]
        X = np.array([a for a in ex for _ in ey] + [0, 7], np.int64)   # every X edge with every Y edge
        Y = np.array([b for _ in ex for b in ey] + [1, 7], np.int64)
        ch = api.Chromosome(X, Y)
        far = int(max(X.max(), Y.max())) + 5 * W * res + 11
        _check(ch, X, Y, [cx], [cy], res, w, corner)
        _check(ch, X, Y, [cx, far, cx, -far, 3], [cy, far, far, cy, 5], res, w, corner)
        S, stats, mats, _ = ch.agg_loops([cx], [cy], res, w, corner, want_mats=True)
        assert mats[0, 0, 0] >= 1 and mats[0, W - 1, W - 1] >= 1 and stats[0, 1] >= 1      # (ox, oy), the last cell's last PET, the centre
        ch.close()


def test_extreme_centres():
    """centres anywhere in int32 are clamped without changing a count; coordinates at the handle's limit"""
    from cloops_amd import api
    LIM = (1 << 29) - 1
    X = np.array([-LIM, -LIM, 0, LIM - 1, -LIM + 1, LIM], np.int64)
    Y = np.array([-LIM, LIM, LIM, LIM, LIM - 1, LIM], np.int64)
    ch = api.Chromosome(X, Y)
    I = np.iinfo(np.int32)
    cs = [I.min, I.min + 1, -(1 << 30) - 1, -(1 << 30), -(1 << 30) + 1, -LIM - 5, -LIM, 0, LIM, LIM + 5, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, I.max]
    cx = np.array([a for a in cs for _ in cs], np.int64)
    cy = np.array([b for _ in cs for b in cs], np.int64)
    for res, w, corner in ((1, 20, 3), (1000, 10, 3), (((1 << 29) - 1) // 41, 20, 20), (((1 << 29) - 1) // 3, 1, 1)):
        _check(ch, X, Y, cx, cy, res, w, corner)
    ch.close()


def test_pile_up():
    """70 000 PETs at one coordinate in one cell + 1000 scattered: counters of 32 bits, LDS contention, a window longer than a stride"""
    from cloops_amd import api
    rng = np.random.default_rng(5)
    X = np.r_[np.full(70000, 100200), rng.integers(90000, 112000, 1000)]
    Y = np.r_[np.full(70000, 300700), rng.integers(290000, 312000, 1000)]
    p = rng.permutation(len(X))
    X, Y = X[p], Y[p]
    ch = api.Chromosome(X, Y)
    S, stats, mats = _check(ch, X, Y, [100000, 100000, 95000], [300000, 300000, 305000], 1000, 10, 3)
    assert mats[0, 10, 11] >= 70000 and S[10, 11] >= 140000 and stats[0, 0] >= 70000
    S2, stats2, _ = _check(ch, X, Y, [100200], [300700], 1, 1, 1)      # all of them in the centre cell
    assert stats2[0, 1] >= 70000
    ch.close()


def test_many_loops():
    """70 000 loops (more workgroups than a grid dimension of 65 535 would take), half of them on one centre (contended adds)"""
    from cloops_amd import api
    rng = np.random.default_rng(23)
    n = 2000
    X = rng.integers(0, 100000, n)
    Y = X + rng.integers(0, 60000, n)
    L = 70000
    cx = rng.integers(-5000, 110000, L)
    cy = cx + rng.integers(0, 60000, L)
    cx[::2], cy[::2] = 40000, 60000
    ch = api.Chromosome(X, Y)
    res, w, corner = 1000, 3, 2
    S, stats, mats, kept = ch.agg_loops(cx, cy, res, w, corner)
    assert mats is None and kept == n
    uniq, inv, mult = np.unique(np.stack([cx, cy], 1), axis=0, return_inverse=True, return_counts=True)
    _, ustats, umats = brute(X, Y, uniq[:, 0], uniq[:, 1], res, w, corner)
    wS = (umats.astype(np.int64) * mult[:, None, None]).sum(0)
    assert mult.max() >= 35000 and np.array_equal(S, wS) and S.sum() > 35000
    sample = np.r_[0, 1, 2, 3, rng.integers(0, L, 500), L - 2, L - 1]
    assert np.array_equal(stats[sample], ustats[inv.ravel()[sample]])
    assert int(stats[:, 0].astype(np.int64).sum()) == int(S.sum())
    ch.close()


def test_edge_cases():
    from cloops_amd import api
    rng = np.random.default_rng(2)
    X = rng.integers(0, 50000, 300)
    Y = X + rng.integers(0, 30000, 300)
    ch = api.Chromosome(X, Y)
    # no loops
    S, stats, mats, kept = ch.agg_loops([], [], 1000, 10, 3, want_mats=True)
    assert S.shape == (21, 21) and not S.any() and stats.shape == (0, 6) and mats.shape == (0, 21, 21) and kept == 300
    # a cut that removes every row
    S, stats, mats, kept = ch.agg_loops([20000, 30000], [30000, 40000], 1000, 10, 3, cut=10 ** 6, want_mats=True)
    assert not S.any() and not stats.any() and not mats.any() and kept == 0 and stats.shape == (2, 6)
    # stats without mats and the reverse
    cx, cy = rng.integers(0, 50000, 20), rng.integers(0, 80000, 20)
    wS, wstats, wmats = brute(X, Y, cx, cy, 1000, 10, 3)
    S, stats, mats, _ = ch.agg_loops(cx, cy, 1000, 10, 3, want_stats=True, want_mats=False)
    assert mats is None and np.array_equal(S, wS) and np.array_equal(stats, wstats)
    S, stats, mats, _ = ch.agg_loops(cx, cy, 1000, 10, 3, want_stats=False, want_mats=True)
    assert stats is None and np.array_equal(S, wS) and np.array_equal(mats, wmats)
    S, stats, mats, _ = ch.agg_loops(cx, cy, 1000, 10, 3, want_stats=False, want_mats=False)
    assert stats is None and mats is None and np.array_equal(S, wS)
    ch.close()
    # an empty chromosome
    ch = api.Chromosome(np.zeros(0, np.int64), np.zeros(0, np.int64))
    S, stats, mats, kept = ch.agg_loops([5, 6], [7, 8], 10, 2, 1, want_mats=True)
    assert S.shape == (5, 5) and not S.any() and not stats.any() and not mats.any() and kept == 0
    ch.close()
    # one row
    ch = api.Chromosome(np.array([5]), np.array([9]))
    _check(ch, [5], [9], [5, 4, 6, 100], [9, 9, 8, 100], 1, 1, 1)
    ch.close()


def test_argument_errors():
    from cloops_amd import api, _lib
    lib = _lib.load()
    X, Y = G.chr21_xy()
    ch = api.Chromosome(X, Y)
    for kw in (dict(res=0), dict(res=-5), dict(w=0), dict(w=21), dict(corner=0), dict(corner=4, w=3), dict(res=(1 << 29) // 21 + 1, w=10)):
        args = dict(res=1000, w=10, corner=3)
        args.update(kw)
        with pytest.raises(ValueError):
            ch.agg_loops([1000], [50000], **args)
    with pytest.raises(ValueError):
        ch.agg_loops([1, 2], [3], 1000)
    with pytest.raises(ValueError):
        ch.agg_loops([1 << 31], [3], 1000)
    # the C entry itself
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    cx, cy = np.array([1000, 2000], np.int32), np.array([50000, 60000], np.int32)
    S = np.zeros(21 * 21, np.int64)
    nk = ctypes.c_int64(0)
    r = lambda *a: lib.cl_agg_loops(*a)
    E = _lib.CL_ERR_ARG
    assert r(None, 0, 1000, 10, 3, 2, vp(cx), vp(cy), vp(S), None, None, ctypes.byref(nk)) == E
    assert r(ch._h, 0, 1000, 10, 3, 2, vp(cx), vp(cy), None, None, None, ctypes.byref(nk)) == E
    assert r(ch._h, 0, 0, 10, 3, 2, vp(cx), vp(cy), vp(S), None, None, None) == E
    assert r(ch._h, 0, 1000, 0, 1, 2, vp(cx), vp(cy), vp(S), None, None, None) == E
    assert r(ch._h, 0, 1000, 21, 3, 2, vp(cx), vp(cy), vp(S), None, None, None) == E
    assert r(ch._h, 0, 1000, 10, 0, 2, vp(cx), vp(cy), vp(S), None, None, None) == E
    assert r(ch._h, 0, 1000, 10, 11, 2, vp(cx), vp(cy), vp(S), None, None, None) == E
    assert r(ch._h, 0, (1 << 29) // 21 + 1, 10, 3, 2, vp(cx), vp(cy), vp(S), None, None, None) == E
    assert r(ch._h, 0, 1000, 10, 3, -1, vp(cx), vp(cy), vp(S), None, None, None) == E
    assert r(ch._h, 0, 1000, 10, 3, 2, None, vp(cy), vp(S), None, None, None) == E
    assert r(ch._h, 0, 1000, 10, 3, 2, vp(cx), None, vp(S), None, None, None) == E
    assert b"cl_agg_loops" in lib.cl_last_error()
    assert r(ch._h, 0, 1000, 10, 3, 0, None, None, vp(S), None, None, None) == 0           # no loops, no centres, no n_kept
    # runs in flight
    ch.cluster_async("v2", 2000, 5)
    assert r(ch._h, 0, 1000, 10, 3, 2, vp(cx), vp(cy), vp(S), None, None, ctypes.byref(nk)) == E
    ch.wait()
    _check(ch, X, Y, cx, cy, 1000, 10, 3)                              # the handle still works
    ch.close()


def _chr21_loops(sig):
    """the centres of the chr21 loops, read here (not by cloops_amd.agg): anchors in the columns iva / ivb, significance last"""
    cx, cy = [], []
    with open(LOOPS) as fh:
        head = fh.readline().rstrip("\n").split("\t")
        ia, ib = head.index("iva"), head.index("ivb")
        for line in fh:
            f = line.rstrip("\n").split("\t")
            if sig and float(f[-1]) < 1:
                continue
            (x1, x2), (y1, y2) = ([int(v) for v in f[k].split(":")[1].split("-")] for k in (ia, ib))
            cx.append((x1 + x2) // 2)
            cy.append((y1 + y2) // 2)
    return np.array(cx, np.int64), np.array(cy, np.int64)


def test_repeatable_and_isolated():
    """the same call twice, another cut and back; neighbour counts and labels of the handle -- and of a subsample of it -- are the same
    before and after"""
    from cloops_amd import api
    X, Y = G.chr21_xy()
    cx, cy = _chr21_loops(False)
    ch = api.Chromosome(X, Y)
    nc0 = ch.neighbor_counts(1000)
    lab0 = ch.cluster("v2", 1000, 5).labels.copy()
    a = ch.agg_loops(cx, cy, 1000, 10, 3, want_mats=True)
    b = ch.agg_loops(cx, cy, 1000, 10, 3, want_mats=True)
    c = ch.agg_loops(cx, cy, 1000, 10, 3, cut=4601, want_mats=True)
    d = ch.agg_loops(cx, cy, 1000, 10, 3, want_mats=True)
    e = ch.agg_loops(cx[::-1].copy(), cy[::-1].copy(), 1000, 10, 3, want_mats=True)      # the loops in another order
    for r in (b, d):
        assert all(np.array_equal(u, v) for u, v in zip(a[:3], r[:3])) and r[3] == a[3] == len(X)
    assert np.array_equal(e[0], a[0]) and np.array_equal(e[1][::-1], a[1]) and np.array_equal(e[2][::-1], a[2])
    wc = brute(X, Y, cx, cy, 1000, 10, 3, 4601)
    assert all(np.array_equal(u, v) for u, v in zip(c[:3], wc)) and c[3] == int((Y - X >= 4601).sum()) and c[0].sum() < a[0].sum()
    assert np.array_equal(ch.neighbor_counts(1000), nc0)
    assert np.array_equal(ch.cluster("v2", 1000, 5).labels, lab0)
    fresh = api.Chromosome(X, Y)
    assert np.array_equal(ch.cluster("v2", 2000, 5, 4601).labels, fresh.cluster("v2", 2000, 5, 4601).labels)
    fresh.close()
    rows = np.random.default_rng(4).choice(len(X), len(X) // 2, replace=False)
    sub = ch.subsample(rows)
    ref = api.Chromosome(X[rows], Y[rows])
    snc, slab = ref.neighbor_counts(1000), ref.cluster("v2", 1000, 5).labels.copy()
    ref.close()
    _check(sub, X[rows], Y[rows], cx, cy, 1000, 10, 3)
    assert np.array_equal(sub.neighbor_counts(1000), snc) and np.array_equal(sub.cluster("v2", 1000, 5).labels, slab)
    _check(sub, X[rows], Y[rows], cx, cy, 1000, 10, 3, 4601)
    assert np.array_equal(ch.agg_loops(cx, cy, 1000, 10, 3)[0], a[0])  # the parent's table is its own
    sub.close()
    ch.close()


PINNED = ((1000, 10, False, 343, 312, 2441, 11708), (1000, 10, True, 202, 193, 2095, 8158), (5000, 5, False, 343, 270, 5700, 17919))


@pytest.mark.parametrize("res,w,sig,n_loops,used,centre,total", PINNED)
def test_chr21_pinned(res, w, sig, n_loops, used, centre, total):
    """the chr21 loops at the default distance, corner 3: equal to the brute force AND to values computed once on the CPU"""
    from cloops_amd import api
    X, Y = G.chr21_xy()
    cx, cy = _chr21_loops(sig)
    assert len(cx) == n_loops
    keep = (cy - cx) >= (2 * w + 2) * res
    assert int(keep.sum()) == used
    wS = brute(X, Y, cx[keep], cy[keep], res, w, 3, want_mats=False)[0]
    assert (int(wS[w, w]), int(wS.sum())) == (centre, total)           # the brute force re-derives the pinned values
    ch = api.Chromosome(X, Y)
    S = _check(ch, X, Y, cx[keep], cy[keep], res, w, 3)[0]
    ch.close()
    assert (int(S[w, w]), int(S.sum())) == (centre, total)


def _write_jd(d, X, Y):
    import joblib
    os.makedirs(d, exist_ok=True)
    joblib.dump(np.stack([np.arange(len(X)), X, Y], 1).astype(np.int64), os.path.join(d, "chr21-chr21.jd"))


def test_module_and_mem_names(tmp_path):
    """aggLoops on a 'mem://' chromosome (no .jd file) and on a directory give the same; a chromosome without PETs is reported"""
    from cloops_amd import agg, pipe
    X, Y = G.chr21_xy()
    pipe.CACHE.clear()
    f = pipe.CACHE.put_arrays("chr21-chr21", X, Y)
    out = os.path.join(str(tmp_path), "m")
    r = agg.aggLoops(LOOPS, [f], out, sig=False)
    assert (int(r["S"][10, 10]), int(r["S"].sum())) == (2441, 11708)
    s = r["summary"]
    assert (s["loops_read"], s["loops_used"], s["loops_skipped_near_diagonal"], s["loops_without_pets"]) == (343, 312, 31, 0)
    assert s["scores"] == agg.scores(r["S"], 3) and s["pets"] == len(X)
    assert len(r["rows"]) == 312 and sum(row[3] for row in r["rows"]) == 11708
    d = os.path.join(str(tmp_path), "jd")
    _write_jd(d, X, Y)
    r2 = agg.aggLoops(LOOPS, d, None, sig=False)
    assert np.array_equal(r2["S"], r["S"]) and [row[:9] for row in r2["rows"]] == [row[:9] for row in r["rows"]]
    assert np.array_equal([row[9] for row in r2["rows"]], [row[9] for row in r["rows"]], equal_nan=True)      # P2LL: 0 / 0 is nan
    r3 = agg.aggLoops(LOOPS, os.path.join(str(tmp_path), "nothing_here"), None)
    assert r3["summary"]["loops_without_pets"] == 202 and r3["summary"]["loops_used"] == 0 and not r3["S"].any()
    r4 = agg.aggLoops(LOOPS, [f], None, res=5000, w=5, min_dist=0, sig=False)
    assert r4["summary"]["loops_used"] == 343 and r4["summary"]["loops_skipped_near_diagonal"] == 0
    pipe.CACHE.clear()


def test_command_line(tmp_path):
    import subprocess
    import sys
    X, Y = G.chr21_xy()
    d = os.path.join(str(tmp_path), "jd")
    _write_jd(d, X, Y)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = os.path.join(str(tmp_path), "cli")
    p = subprocess.run([sys.executable, "-m", "cloops_amd.agg", "-d", d, "-f", LOOPS, "-o", out, "-plot"], env=env, cwd=str(tmp_path),
                       timeout=300, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    for suffix in ("_agg.txt", "_agg_loops.txt", "_agg.json"):
        assert os.path.isfile(out + suffix), suffix
    cx, cy = _chr21_loops(True)
    keep = (cy - cx) >= 22000
    wS, wstats, _ = brute(X, Y, cx[keep], cy[keep], 1000, 10, 3, want_mats=False)
    S = np.loadtxt(out + "_agg.txt", dtype=np.int64, delimiter="\t")
    assert np.array_equal(S, wS) and (int(S[10, 10]), int(S.sum())) == (2095, 8158)
    with open(out + "_agg.json") as fh:
        s = json.load(fh)
    assert (s["loops_in_file"], s["loops_read"], s["loops_used"], s["loops_skipped_near_diagonal"], s["loops_without_pets"]) == (343, 202, 193, 9, 0)
    assert (s["res"], s["w"], s["corner"], s["cut"], s["min_dist"]) == (1000, 10, 3, 0, 22000)
    assert s["scores"]["APA"] == float(wS[10, 10]) / (float(wS[18:, :3].sum()) / 9.0) and set(s["scores"]) == {"APA", "P2UL", "P2UR", "P2LR", "ZscoreLL"}
    lines = open(out + "_agg_loops.txt").read().split("\n")
    assert lines[0].split("\t") == ["loopId", "cx", "cy", "total", "centre", "ll", "ul", "ur", "lr", "P2LL"] and len(lines) == 193 + 2
    got = np.array([[int(v) for v in l.split("\t")[1:9]] for l in lines[1:-1]], np.int64)
    assert np.array_equal(got[:, 0], cx[keep]) and np.array_equal(got[:, 1], cy[keep]) and np.array_equal(got[:, 2:], wstats)
    try:
        import matplotlib  # noqa: F401
        assert os.path.isfile(out + "_agg.pdf")
    except ImportError:
        assert "no heat map drawn" in p.stderr                         # nothing worse than a warning


def test_agg_flag_of_the_main_command(tmp_path):
    """-agg on the chr21 BEDPE example: `<out>_agg.txt` equals aggLoops run afterwards on the written `.loop`"""
    import gzip
    from cloops_amd import agg, pipe
    X, Y = G.chr21_xy()
    bed = os.path.join(str(tmp_path), "in.bedpe.gz")
    with gzip.open(bed, "wt") as fh:                       # a BEDPE whose mid-points are exactly (X, Y)
        for x, y in zip(X.tolist(), Y.tolist()):
            fh.write("chr21\t%d\t%d\tchr21\t%d\t%d\tid\t1\t+\t-\n" % (x, x, y, y))
    fout = os.path.join(str(tmp_path), "run")
    pipe.CACHE.clear()
    assert pipe.main(["-f", bed, "-o", fout, "-m", "0", "-eps", "500,1000,2000", "-minPts", "5", "-agg"]) == 0
    assert open(fout + ".loop").read() == open(LOOPS).read()
    for suffix in ("_agg.txt", "_agg_loops.txt", "_agg.json"):
        assert os.path.isfile(fout + suffix), suffix
    f = pipe.CACHE.put_arrays("chr21-chr21", X, Y)
    r = agg.aggLoops(fout + ".loop", [f], None, res=2000)              # -res defaults to the largest eps of the run
    assert np.array_equal(np.loadtxt(fout + "_agg.txt", dtype=np.int64, delimiter="\t"), r["S"]) and r["S"].sum() > 0
    with open(fout + "_agg.json") as fh:
        s = json.load(fh)
    assert s["res"] == 2000 and s["loops_read"] == 202 and s["loops_used"] == r["summary"]["loops_used"]
    pipe.CACHE.clear()
