"""The numpy oracle of kernel K23, written from the definitions of include/cloops_hip.h (cl_kdis_build) -- it does not import
cloops_amd.esteps --: the kept rows in table order, the k-distances by brute force (the full distance matrix, np.partition; up to
BRUTE_MAX rows) and by scipy's cKDTree with p = 1 on float64 copies (exact: every value is an integer far below 2^53), the log-binned
histogram, a host stand-in for the kdis_* methods of api.Chromosome that answers from the oracle, and seeded mixtures of uniform
background and tight loops.  Shared by tests/test_kdis_host.py and tests/test_gpu_kdis.py; `self_test` holds the two forms against each
other."""
import numpy as np

EMPTY = np.zeros(0, np.int64)
KMAX = 64                   # CL_KDIS_KMAX
BINS = 31 * 128             # CL_KDIS_BINS
BRUTE_MAX = 4000


def table_order(X, Y, cut=0):
    """-> (xs, ys, rows): the kept rows ascending by X, equal X in input order, and their input row numbers"""
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    keep = np.flatnonzero((Y - X) >= cut) if cut > 0 else np.arange(len(X))
    o = np.argsort(X[keep], kind="stable")
    rows = keep[o]
    return X[rows], Y[rows], rows


def nearest_brute(xs, ys, kmax):
    """-> int64[m, kmax]: per row the ascending distances to its kmax nearest other rows, -1 where there are fewer"""
    m = len(xs)
    out = np.full((m, kmax), -1, np.int64)
    if m < 2:
        return out
    D = np.abs(xs[:, None] - xs[None, :]) + np.abs(ys[:, None] - ys[None, :])
    D[np.arange(m), np.arange(m)] = np.int64(1) << 62           # q != p (a duplicate of p stays, at distance 0)
    have = min(kmax, m - 1)
    part = np.partition(D, have - 1, axis=1)[:, :have] if have < m - 1 else D
    out[:, :have] = np.sort(part, axis=1)[:, :have]
    return out


def nearest_tree(xs, ys, kmax):
    """the same from cKDTree(p = 1): the kmax + 1 nearest of a row hold the row itself or a duplicate of it at distance 0 in front"""
    from scipy.spatial import cKDTree
    m = len(xs)
    out = np.full((m, kmax), -1, np.int64)
    if m < 2:
        return out
    pts = np.stack([xs, ys], 1).astype(np.float64)
    d, _ = cKDTree(pts).query(pts, k=kmax + 1, p=1)
    d = d[:, 1:]
    ok = np.isfinite(d)                                          # (missing neighbours come back as inf)
    out[ok] = d[ok].astype(np.int64)
    return out


def kdis_oracle(X, Y, cut, ks, form="auto"):
    """-> (xs, ys, {k: d int64 in table order}, rows)"""
    xs, ys, rows = table_order(X, Y, cut)
    ks = [int(k) for k in ks]
    assert all(1 <= k <= KMAX for k in ks)
    if form == "auto":
        form = "brute" if len(xs) <= BRUTE_MAX else "tree"
    near = (nearest_brute if form == "brute" else nearest_tree)(xs, ys, max(ks))
    return xs, ys, {k: near[:, k - 1].copy() for k in ks}, rows


def logbin(d):
    """the log bin of integers d >= 1, vectorised: floor(log2 d) * 128 + the 7 bits below the leading one"""
    d = np.asarray(d, np.int64)
    assert d.size == 0 or (d.min() >= 1 and d.max() < (1 << 52))
    e = np.frexp(d.astype(np.float64))[1].astype(np.int64) - 1   # exact: d < 2^53
    m = np.where(e >= 7, d >> np.maximum(e - 7, 0), d << np.maximum(7 - e, 0)) & 127
    return e * 128 + m


def hist_oracle(d):
    """-> (hist int64[BINS], n_zero, n_none) of k-distances d"""
    d = np.asarray(d, np.int64)
    return np.bincount(logbin(d[d >= 1]), minlength=BINS).astype(np.int64), int((d == 0).sum()), int((d < 0).sum())


class OracleChrom:
    """answers the kdis_* methods of api.Chromosome from the oracle"""

    def __init__(self, X, Y):
        self.X, self.Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
        self.res = None

    def kdis_build(self, ks, cut=0):
        self.res = (list(ks),) + kdis_oracle(self.X, self.Y, cut, ks)[:3]
        return len(self.res[1])

    def kdis_get(self, which=0, first=0, count=None):
        ks, xs, ys, d = self.res
        sl = slice(first, None if count is None else first + count)
        return xs[sl].astype(np.int32), ys[sl].astype(np.int32), d[ks[which]][sl].astype(np.int32)

    def kdis_hist(self, which=0):
        h, nz, nn = hist_oracle(self.res[3][self.res[0][which]])
        return h.astype(np.uint64), nz, nn

    def kdis_free(self):
        self.res = None


# the three mixtures of the estimate's test: (background PETs, loops, PETs per loop, jitter in bp), and the seed of each
MIXTURES = ((6000, 60, 40, 400), (20000, 30, 30, 300), (3000, 100, 60, 800))
MIXTURE_SEEDS = (2301, 2302, 2303)


def mixture(seed, n_bg, n_loops, per_loop, jitter, span=2000000):
    """uniform background (X in the span, Y - X in 1 .. 400 kb) and tight loops (anchors in the span, 20 .. 400 kb apart, every PET
    within +-jitter of them on both ends), shuffled -> (X, Y, is_loop)"""
    rng = np.random.default_rng(seed)
    bx = rng.integers(0, span, n_bg)
    by = bx + rng.integers(1000, 400001, n_bg)
    ax = rng.integers(0, span - 400000, n_loops)
    ay = ax + rng.integers(20000, 400001, n_loops)
    lx = np.repeat(ax, per_loop) + rng.integers(-jitter, jitter + 1, n_loops * per_loop)
    ly = np.repeat(ay, per_loop) + rng.integers(-jitter, jitter + 1, n_loops * per_loop)
    X, Y = np.concatenate([bx, lx]), np.concatenate([by, ly])
    loop = np.concatenate([np.zeros(n_bg, bool), np.ones(n_loops * per_loop, bool)])
    o = rng.permutation(len(X))
    return X[o], Y[o], loop[o]


def self_test():
    """the two forms agree on a 3000-point set with duplicates, for every k at once; the vectorised log bin is ests.logbin's rule"""
    rng = np.random.default_rng(23)
    X = rng.integers(0, 300000, 3000)
    Y = X + rng.integers(0, 50000, 3000)
    X[100:140], Y[100:140] = X[100], Y[100]                      # a pile of duplicates
    a = kdis_oracle(X, Y, 0, range(1, KMAX + 1), "brute")
    b = kdis_oracle(X, Y, 0, range(1, KMAX + 1), "tree")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert all(np.array_equal(a[2][k], b[2][k]) for k in a[2])
    assert (a[2][39][np.isin(a[3], np.arange(100, 140))] == 0).all() and (a[2][1] >= 0).all()
    c = kdis_oracle(X, Y, 20000, (5, 64), "brute")
    d = kdis_oracle(X, Y, 20000, (5, 64), "tree")
    assert 0 < len(c[0]) < 3000 and all(np.array_equal(c[2][k], d[2][k]) for k in (5, 64))
    for v in (1, 2, 3, 127, 128, 129, 255, 256, 257, (1 << 30) - 1, 1 << 30, (1 << 31) - 4):
        e = v.bit_length() - 1
        assert int(logbin([v])[0]) == e * 128 + (((v >> (e - 7)) if e >= 7 else (v << (7 - e))) & 127)
    return True


if __name__ == "__main__":
    print(self_test())
