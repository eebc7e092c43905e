"""The numpy restatement of K28 (include/cloops_hip.h, cl_scc_moments) and of the host formulas of cloops_amd/similarity.py, written
independently of both, the case generators of the GPU tests and the kernel's tile constants."""
import math

import numpy as np

import matrix_cases as MC

TILE_I = 32                    # k_scc.hip K28_TI: bins of a tile of k28_moments
TILE_D = 32                    # k_scc.hip K28_TD: diagonals of a tile
HMAX = 20                      # CL_SCC_HMAX
BAND_MAX = 1 << 28             # CL_SCC_BAND_MAX
SIZES = (1, 2, TILE_I - 1, TILE_I, TILE_I + 1, 3 * TILE_I + 1)     # bins of a window, and its diagonals: both tile directions
HS = (0, 1, 2, HMAX)


# ---- the matrices and their box sums ------------------------------------------------------------------------------------------
def dense(bx, by, cnt, b0, nb):
    """the symmetric nb x nb matrix (int64) of the folded cells inside the window [b0, b0 + nb); a diagonal cell counts once"""
    A = np.zeros((nb, nb), np.int64)
    u, v, c = np.asarray(bx, np.int64) - b0, np.asarray(by, np.int64) - b0, np.asarray(cnt, np.int64)
    ok = (u >= 0) & (u < nb) & (v >= 0) & (v < nb)
    A[u[ok], v[ok]] = c[ok]
    A[v[ok], u[ok]] = c[ok]
    return A


def box_prefix(A, h):
    """S[i][j] = the sum of A over |u - i| <= h, |v - j| <= h inside the matrix, by 2D prefix sums"""
    nb = len(A)
    P = np.zeros((nb + 1, nb + 1), np.int64)
    P[1:, 1:] = np.cumsum(np.cumsum(A, 0), 1)
    lo, hi = np.maximum(np.arange(nb) - h, 0), np.minimum(np.arange(nb) + h + 1, nb)
    return P[hi][:, hi] - P[lo][:, hi] - P[hi][:, lo] + P[lo][:, lo]


def box_brute(A, h):
    """the same by loops over the box"""
    nb = len(A)
    S = np.zeros((nb, nb), np.int64)
    for i in range(nb):
        for j in range(nb):
            s = 0
            for u in range(max(0, i - h), min(nb, i + h + 1)):
                for v in range(max(0, j - h), min(nb, j + h + 1)):
                    s += int(A[u, v])
            S[i, j] = s
    return S


def moments_of(Sa, Sb, D):
    """per stratum d < D over the positions (i, i + d) with Sa != 0 or Sb != 0 -> six lists of Python ints: n, sx, sy, sxx, syy, sxy"""
    out = [[] for _ in range(6)]
    for d in range(D):
        x, y = [int(v) for v in np.diagonal(Sa, d)], [int(v) for v in np.diagonal(Sb, d)]
        keep = [(p, q) for p, q in zip(x, y) if p != 0 or q != 0]
        for k, v in enumerate((len(keep), sum(p for p, _ in keep), sum(q for _, q in keep), sum(p * p for p, _ in keep),
                               sum(q * q for _, q in keep), sum(p * q for p, q in keep))):
            out[k].append(v)
    return out


def moments_oracle(cells_a, cells_b, b0, nb, h, D, box=box_prefix):
    """cells_x = (bx, by, cnt) folded -> the six lists"""
    return moments_of(box(dense(*cells_a[:3], b0, nb), h), box(dense(*cells_b[:3], b0, nb), h), D)


def as_arrays(m):
    """the six lists as the dtypes the device returns (every value of a test fits)"""
    return (np.array(m[0], np.int64),) + tuple(np.array(c, np.uint64) for c in m[1:])


# ---- the host formulas ----------------------------------------------------------------------------------------------------------
def pearson(n, sx, sy, sxx, syy, sxy):
    if n < 2:
        return math.nan
    va, vb = n * sxx - sx * sx, n * syy - sy * sy
    if va <= 0 or vb <= 0:
        return math.nan
    return float(n * sxy - sx * sy) / (math.sqrt(float(va)) * math.sqrt(float(vb)))


def scc_oracle(m, ignore_diags=0):
    """the six lists -> dict(rho, weight, scc, pcc, pixels)"""
    D = len(m[0])
    rho = [pearson(*(int(c[d]) for c in m)) for d in range(D)]
    weight = [0.0 if (math.isnan(rho[d]) or d < ignore_diags) else int(m[0][d]) * (1.0 + 1.0 / int(m[0][d])) / 12.0 for d in range(D)]
    tw = sum(weight)
    scc = math.nan if not tw > 0 else sum(weight[d] * rho[d] for d in range(D) if weight[d] > 0) / tw
    tot = [sum(int(v) for v in c[ignore_diags:]) for c in m]
    return {"rho": rho, "weight": weight, "scc": scc, "pcc": pearson(*tot), "pixels": tot[0]}


def counted_pixels(Sa, Sb, D, ignore_diags=0):
    """the smoothed values of the counted positions of the strata ignore_diags <= d < D -> (x, y) float64"""
    x = np.concatenate([np.diagonal(Sa, d) for d in range(ignore_diags, D)] or [np.zeros(0)])
    y = np.concatenate([np.diagonal(Sb, d) for d in range(ignore_diags, D)] or [np.zeros(0)])
    keep = (x != 0) | (y != 0)
    return x[keep].astype(np.float64), y[keep].astype(np.float64)


def smax(h, max_count, n_kept):
    return min((2 * h + 1) ** 2 * max_count, 2 * n_kept)


def span_of(*cells):
    """the window the command takes: the bins all samples' cells span together -> (b0, nb); (0, 0) without cells"""
    lo = [int(c[0].min()) for c in cells if len(c[0])]
    hi = [int(c[1].max()) for c in cells if len(c[0])]
    return (min(lo), max(hi) - min(lo) + 1) if lo else (0, 0)


class OracleChrom(object):
    """the mat_* and scc_* methods of api.Chromosome that similarity.pair_chrom calls, from the restatement"""

    def __init__(self, X, Y):
        self.X, self.Y, self.cells = np.asarray(X, np.int64), np.asarray(Y, np.int64), None

    def mat_cells(self, res, cut=0, fold=False):
        assert fold
        self.cells = MC.cells_oracle(self.X, self.Y, cut, res, True)
        return len(self.cells[0]), self.cells[3], int(self.cells[2].max()) if len(self.cells[0]) else 0

    def mat_cells_get(self, first=0, count=None):
        n = len(self.cells[0])
        count = n - first if count is None else count
        return tuple(a[first:first + count] for a in self.cells[:3])

    def bal_marginals(self, ignore_diags=2):
        b0, nb = span_of(self.cells)
        return b0, nb, int(((self.cells[1] - self.cells[0]) >= ignore_diags).sum())

    def bal_free(self):
        pass

    def mat_free(self):
        self.cells = None

    def scc_moments(self, other, b0, nb, h=0, n_diags=None):
        return as_arrays(moments_oracle(self.cells, other.cells, b0, nb, h, nb if n_diags is None else n_diags))


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def sized(nb, seed):
    """rows at res 1 whose bins reach from below 0 to beyond nb - 1: a window [0, nb) cuts through them on both sides when nb > 2"""
    rng = np.random.default_rng(seed)
    m = 6 * nb + 40
    X = rng.integers(-5, nb + 5, m)
    Y = X + np.where(rng.random(m) < 0.5, rng.integers(0, 4, m), rng.integers(0, nb + 5, m))
    flip = rng.random(m) < 0.3
    return np.where(flip, Y, X).astype(np.int64), np.where(flip, X, Y).astype(np.int64)


def cut_window():
    """(X, Y of a, X, Y of b, res, b0, nb): rows over the bins -20 .. 150 of 100 bp, the window 10 .. 79 inside them"""
    Xa, Ya = MC.scattered(11, 2500, 17000, 6000, both=True)
    Xb, Yb = MC.scattered(12, 2500, 17000, 6000, both=True)
    return Xa - 2000, Ya - 2000, Xb - 2000, Yb - 2000, 100, 10, 70


def gapped():
    """(X, Y): two clusters of bins (res 1) with 2 * TILE_I empty bins between them, and a few rows that bridge the gap"""
    rng = np.random.default_rng(13)
    X1, X2 = rng.integers(0, 20, 300), rng.integers(20 + 2 * TILE_I, 40 + 2 * TILE_I, 300)
    X = np.concatenate([X1, X2, rng.integers(0, 20, 15)])
    Y = np.concatenate([X1 + rng.integers(0, 6, 300), X2 + rng.integers(0, 6, 300), rng.integers(20 + 2 * TILE_I, 40 + 2 * TILE_I, 15)])
    return X.astype(np.int64), Y.astype(np.int64)


HEAVY = 70000                  # duplicated rows of one cell: 70000^2 > 2^32


def heavy(seed):
    """(X, Y): HEAVY copies of one row in the cell (7, 9) of res 1 among 200 scattered rows over the bins 0 .. 39"""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 36, 200)
    Y = X + rng.integers(0, 4, 200)
    return np.concatenate([np.full(HEAVY, 7), X]).astype(np.int64), np.concatenate([np.full(HEAVY, 9), Y]).astype(np.int64)


def general():
    """two chromosomes of 3000 and 2600 rows over some 340 bins of 1000 bp"""
    return MC.scattered(21, 3000, 300000, 40000, both=True), MC.scattered(22, 2600, 300000, 40000, both=True)


def overflowing():
    """(X, Y): 2^20 copies of one row in one cell of res 1 and one row 2^24 bins away: the overflow rule refuses h = 0, nb = 2^24 + 1"""
    X = np.concatenate([np.full(1 << 20, 5), [5 + (1 << 24)]]).astype(np.int64)
    return X, X.copy()
