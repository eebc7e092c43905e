"""Seeded inputs for the region-query routes that the goldens and the genome chains do not reach (no GPU needed).

A run picks its region-query kernel on the host (cl_launch_region, run_sort_and_count): minPts 2 .. 128 goes to the clustering
kernels with the count cache, minPts 1, minPts >= 129 and the exact counts of cl_neighbor_counts go to k_region_count.  The data
sets here keep the mean strip population n // S far from the shape thresholds (40 and 400) and hold clusters that are still
clusters at minPts in the hundreds, so that the second class has something to find.

Every data set is a `Case`: X, Y (0 <= X <= Y, shuffled rows), eps, the minPts values and the two cuts its GPU tests use.
tests/test_route_cases.py checks on the CPU oracle that no setting is empty; tests/test_gpu_routes.py runs them on the GPU."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name X Y eps min_pts cut")


def grid_strips(X, Y, eps, variant="v2"):
    """the number of strips S of a run's grid (make_grid): strips are eps wide in p = X + Y, counted from 0 for variant 2 and
    from the smallest p for the others"""
    p = np.asarray(X, np.int64) + np.asarray(Y, np.int64)
    a0 = 0 if variant == "v2" else int(p.min())
    return int((int(p.max()) - a0) // eps - (int(p.min()) - a0) // eps + 1)


def _finish(rng, X, Y):
    X = np.abs(np.asarray(X, np.int64))
    Y = np.abs(np.asarray(Y, np.int64))
    X, Y = np.minimum(X, Y), np.maximum(X, Y)
    p = rng.permutation(len(X))
    return X[p], Y[p]


def _blob(rng, n, eps, width, cluster_sizes, dmax, spanmax, x0=20000):
    """half background with log-uniform distances up to dmax, half clusters (normal, sigma eps / 10) of the given relative sizes
    whose distances reach spanmax, on about `width` strips of X (the style of _dense_blob in tests/test_gpu_edges.py)"""
    L = width * eps // 2
    ncl = len(cluster_sizes)
    n1 = n // 2
    bx = x0 + rng.integers(0, L, n - n1)
    by = bx + np.exp(rng.uniform(np.log(10), np.log(dmax), n - n1)).astype(np.int64)
    ax = x0 + rng.integers(0, L, ncl)
    span = rng.integers(0, spanmax, ncl)
    w = np.asarray(cluster_sizes, np.float64)
    which = rng.choice(ncl, n1, p=w / w.sum())
    cx = ax[which] + rng.normal(0, 0.1 * eps, n1)
    cy = ax[which] + span[which] + rng.normal(0, 0.1 * eps, n1)
    return _finish(rng, np.concatenate([bx, cx.astype(np.int64)]), np.concatenate([by, cy.astype(np.int64)]))


#: sparse: (PETs, half width in bp, distance) of every pile-up.  Two PETs of a pile-up are at most 4 * half width apart: up to
#: 50 bp every PET of it has exactly its size as neighbour count at eps 200.  The cut 19950 removes some pile-ups, halves others.
SPARSE_PILEUPS = ((128, 40, 20100), (129, 50, 20300), (135, 45, 19700), (180, 70, 19950), (260, 60, 19960), (400, 50, 20500),
                  (330, 70, 20050))


def sparse():
    """n // S < 5: 6000 background PETs over 2 Mbp and pile-ups of 128 .. 400 PETs at one distance each, near 20000"""
    rng = np.random.default_rng(20260)
    eps = 200
    bx = rng.integers(0, 2000000, 6000)
    by = bx + rng.integers(0, 40000, 6000)
    xs, ys = [bx], [by]
    for k, (m, hw, d) in enumerate(SPARSE_PILEUPS):
        c = 150000 + 250000 * k
        xs.append(c + rng.integers(-hw, hw + 1, m))
        ys.append(c + d + rng.integers(-hw, hw + 1, m))
    X, Y = _finish(rng, np.concatenate(xs), np.concatenate(ys))
    return Case("sparse", X, Y, eps, (1, 2, 127, 128, 129, 130, 200, 300), 19950)


def mid():
    """n // S in 80 .. 250: 30000 PETs at eps 2000, clusters of 100 .. 700 PETs (about 400)"""
    rng = np.random.default_rng(20261)
    X, Y = _blob(rng, 30000, 2000, 160, rng.integers(100, 701, 38), 40 * 2000, 30 * 2000)
    return Case("mid", X, Y, 2000, (2, 128, 129, 160, 250), 20000)


def long():
    """n // S >= 450: 30000 PETs at eps 5000, clusters of 350 .. 1100 PETs (about 700)"""
    rng = np.random.default_rng(20262)
    X, Y = _blob(rng, 30000, 5000, 36, rng.integers(350, 1101, 21), 20 * 5000, 15 * 5000)
    return Case("long", X, Y, 5000, (128, 129, 300, 600), 30000)


def sparse_grid():
    """S > 8 n: 4000 PETs at eps 8 over 400 kbp, 60 clumps of 20 PETs; the cuts of its test fall inside the clumps' distances"""
    rng = np.random.default_rng(20263)
    bx = rng.integers(0, 400000, 2800)
    by = bx + rng.integers(0, 3000, 2800)
    c = rng.integers(0, 400000, 60)
    d = rng.integers(100, 3000, 60)
    which = np.repeat(np.arange(60), 20)
    cx = c[which] + rng.integers(-2, 3, len(which))
    cy = c[which] + d[which] + rng.integers(-2, 3, len(which))
    X, Y = _finish(rng, np.concatenate([bx, cx]), np.concatenate([by, cy]))
    return Case("sparse_grid", X, Y, 8, (3, 5), 500)


#: the cuts of the sparse grid's run on one handle: the band re-map is declined every time, only the last run finds its own words
SPARSE_GRID_CUTS = (0, 500, 1500, 500, 500)

#: the cuts of the large-cut set: the distance histogram of the upload ends at 65536, the host does not know how many PETs pass
LARGE_CUTS = (65535, 65536, 100000)


def large_cut():
    """a mid-style blob at eps 5000 whose distances reach 200000: thousands of PETs pass a cut of 65536 and more"""
    rng = np.random.default_rng(20264)
    X, Y = _blob(rng, 30000, 5000, 120, rng.integers(100, 701, 38), 200000, 200000)
    Y[:8] = X[:8] + 65535                                  # (the first two cuts differ in these rows)
    return Case("large_cut", X, Y, 5000, (20, 129), 65536)


#: one handle across the minPts classes (mid): every minPts at cut 0, under the data set's cut, then two of them under a third cut
ONE_HANDLE_MIN_PTS = (200, 129, 128, 50)
ONE_HANDLE_CUT2 = 35000


def one_handle_runs():
    """(minPts, cut) in the order the runs are made"""
    c1 = get("mid").cut
    return [(m, 0) for m in ONE_HANDLE_MIN_PTS] + [(m, c1) for m in ONE_HANDLE_MIN_PTS] + [(129, ONE_HANDLE_CUT2), (50, ONE_HANDLE_CUT2)]


#: minPts of the level / switch runs and of the sweep steps (mid and long), and of the sweep on mid
LEVEL_MIN_PTS = (129, 300)
SWEEP_MIN_PTS = (160, 129, 100)

DENSE = ("mid", "long")
MAKERS = {"sparse": sparse, "mid": mid, "long": long, "sparse_grid": sparse_grid, "large_cut": large_cut}
_made = {}


def get(name):
    """the data set `name`, made once per process"""
    if name not in _made:
        _made[name] = MAKERS[name]()
    return _made[name]


def settings(name):
    """(minPts, cut) of every run that tests/test_gpu_routes.py checks against the oracle on data set `name`"""
    c = get(name)
    if name == "sparse_grid":
        return [(m, cut) for m in c.min_pts for cut in sorted(set(SPARSE_GRID_CUTS))]
    if name == "large_cut":
        return [(m, cut) for m in c.min_pts for cut in LARGE_CUTS]
    out = [(m, cut) for m in c.min_pts for cut in (0, c.cut)]
    if name in DENSE:
        out += [(m, cut) for m in LEVEL_MIN_PTS for cut in (0, c.cut) if (m, cut) not in out]
    if name == "mid":
        out += [s for s in one_handle_runs() if s not in out]
    return out
