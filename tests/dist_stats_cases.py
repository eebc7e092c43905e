"""Inputs where the sweep's distance statistics are fragile (shared by test_dist_stats_host.py and
test_gpu_dist_stats.py): groups of (nearly) equal distances, whose one-pass squared deviation
sum x^2 - (sum x)^2 / n cancels to rounding noise, and genomes written as .jd files."""
import os

import joblib
import numpy as np

#: every case: one cut, eps 500, minPts 5 -- the PETs below the cut all go to the self group (pipe.py:63)
CUT = 40000


def _blobs(rng, n_blobs, per, dist, x0, jitter=300, exact=False):
    """n_blobs inter-ligation clusters of `per` PETs, ~`dist` apart (exact: every PET exactly `dist`)"""
    X, Y = [], []
    for b in range(n_blobs):
        base = x0 + b * 10 ** 7
        for k in range(per):
            x = base + (k * 29 if exact else int(rng.randint(0, jitter)))
            X.append(x)
            Y.append(x + dist + (0 if exact else int(rng.randint(0, jitter))))
    return X, Y


def _short(n, dists, x0=10 ** 8, step=100000):
    """n PETs below the cut, far apart (they never meet the clustering: the cut removes them first)"""
    X = [x0 + k * step for k in range(n)]
    return X, [x + int(dists[k % len(dists)]) for k, x in enumerate(X)]


def case(name, seed=1):
    """-> (X, Y) int64 of one chromosome.  Names:
      self_equal       1001 PETs at 33333 (self group degenerate), 40 jittered inter blobs at ~2e6
      inter_equal      varied short PETs, 40 inter blobs of exactly 2e6
      both_equal       self group at 33333, inter blobs of exactly 2e6
      self_2 / self_3 / self_100k   the self group degenerate with 2, 3 and 100000 PETs
      self_two         the self group of two distances only (17000 and 33333)"""
    rng = np.random.RandomState(seed)
    if name == "self_equal":
        a, b = _short(1001, [33333]), _blobs(rng, 40, 10, 2 * 10 ** 6, 10 ** 6)
    elif name == "inter_equal":
        a, b = _short(1001, rng.randint(200, 30000, 1001)), _blobs(rng, 40, 10, 2 * 10 ** 6, 10 ** 6, exact=True)
    elif name == "both_equal":
        a, b = _short(1001, [33333]), _blobs(rng, 40, 10, 2 * 10 ** 6, 10 ** 6, exact=True)
    elif name in ("self_2", "self_3", "self_100k"):
        n = {"self_2": 2, "self_3": 3, "self_100k": 100000}[name]
        a, b = _short(n, [33333], step=100000 if n < 1000 else 50), _blobs(rng, 40, 10, 2 * 10 ** 6, 10 ** 6)
    elif name == "self_two":
        a, b = _short(1000, [17000, 33333]), _blobs(rng, 40, 10, 2 * 10 ** 6, 10 ** 6)
    else:
        raise KeyError(name)
    X = np.asarray(a[0] + b[0], np.int64)
    Y = np.asarray(a[1] + b[1], np.int64)
    o = np.argsort(X, kind="stable")
    return X[o], Y[o]


NAMES = ["self_equal", "inter_equal", "both_equal", "self_2", "self_3", "self_100k", "self_two"]


def write_jd(tmpdir, chrom, X, Y):
    f = os.path.join(str(tmpdir), "%s-%s.jd" % (chrom, chrom))
    joblib.dump(np.stack([np.arange(len(X)), X, Y], 1).astype(np.int64), f)
    return f


def grid_sum(t, blocks, threads):
    """float64 sum of the terms t in the order of a K7 reduction (k_sweep.hip: k7_summary, k7_reduce_parts): block b takes
    the contiguous range [b per, (b + 1) per), its thread i adds elements i, i + threads, ... in order; a 64-lane
    shuffle tree per wave, the waves of a block in order, then thread j of the reducing workgroup adds partials j,
    j + 256, ... in order and an 8-level tree closes"""
    t = np.asarray(t, np.float64)
    n = len(t)
    per = -(-n // blocks) if n else 0
    rows = np.zeros((blocks, -(-per // threads) * threads if per else threads))
    for b in range(blocks):
        seg = t[b * per:min(n, (b + 1) * per)]
        rows[b, :len(seg)] = seg
    acc = np.zeros((blocks, threads))
    for k in range(0, rows.shape[1], threads):          # (adding the zero padding changes no partial sum)
        acc = acc + rows[:, k:k + threads]
    w = acc.reshape(blocks, threads // 64, 64)
    o = 32
    while o:
        w = w.copy()
        w[:, :, :o] = w[:, :, :o] + w[:, :, o:2 * o]
        o >>= 1
    parts = np.zeros(blocks)
    for v in range(threads // 64):
        parts = parts + w[:, v, 0]
    red = np.zeros(256)
    for j in range(0, blocks, 256):
        chunk = parts[j:j + 256]
        red[:len(chunk)] = red[:len(chunk)] + chunk
    o = 128
    while o:
        red = red.copy()
        red[:o] = red[:o] + red[o:2 * o]
        o >>= 1
    return float(red[0])
