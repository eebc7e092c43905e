"""The numpy oracle of K25 (cl_bal_marginals / cl_bal_iterate / cl_bal_weights_get / cl_bal_cells_get), written from the definitions of
include/cloops_hip.h with np.bincount and not from cloops_amd.balance, a stand-in chromosome made of it for the host tier, and the
data makers of tests/test_balance_host.py and tests/test_gpu_balance.py."""
import numpy as np

import matrix_cases as mc

TILE = 2048                                                      # cells per workgroup of the marginals kernel (K25_TILE)
EPS = 2.0 ** -53


def span(bx, by):
    """-> (b0, nb) of folded ascending cells"""
    if len(bx) == 0:
        return 0, 0
    b0 = int(bx[0])
    return b0, int(np.max(by)) - b0 + 1


def used_cells(bx, by, ignore_diags):
    return (np.asarray(by, np.int64) - np.asarray(bx, np.int64)) >= int(ignore_diags)


def marginals_oracle(bx, by, cnt, ignore_diags):
    """-> (b0, nb, n_used, sum uint64[nb], nnz uint32[nb])"""
    bx, by, cnt = np.asarray(bx, np.int64), np.asarray(by, np.int64), np.asarray(cnt, np.int64)
    b0, nb = span(bx, by)
    u = used_cells(bx, by, ignore_diags)
    off = u & (bx != by)
    s = np.zeros(nb, np.int64)
    z = np.zeros(nb, np.int64)
    np.add.at(s, bx[u] - b0, cnt[u])
    np.add.at(s, by[off] - b0, cnt[off])
    np.add.at(z, bx[u] - b0, 1)
    np.add.at(z, by[off] - b0, 1)
    return b0, nb, int(u.sum()), s.astype(np.uint64), z.astype(np.uint32)


def valid_oracle(s, z, min_nnz=10, min_count=0, mad_max=5):
    """the mask of the definitions -> bool[nb]"""
    s, z = np.asarray(s).astype(np.float64), np.asarray(z).astype(np.int64)
    ok = (z >= min_nnz) & (s >= max(1, min_count))
    pos = s > 0
    if mad_max > 0 and pos.any():
        ls = np.log(s[pos])
        med = np.median(ls)
        mad = np.median(np.abs(ls - med))
        low = np.zeros(len(s), bool)
        low[pos] = ls >= med - mad_max * mad
        ok &= low
    return ok


def ice_oracle(bx, by, cnt, ignore_diags, valid, max_iters=200, tol=1e-5, perm=None):
    """-> dict(iters, converged, var, scale, weight float64[nb], w: the unscaled weights).  `perm`: one sort key per cell (cell_perm);
    the cells are put into that order before the sums are taken -- np.bincount adds in the order of its input, so two orders show how
    far the order of summation alone moves the result."""
    bx, by, cnt = np.asarray(bx, np.int64), np.asarray(by, np.int64), np.asarray(cnt, np.float64)
    b0, nb = span(bx, by)
    u = used_cells(bx, by, ignore_diags)
    bx, by, cnt = bx[u] - b0, by[u] - b0, cnt[u]
    if perm is not None:
        p = np.argsort(np.asarray(perm, np.float64)[u], kind="stable")         # (perm: one sort key per cell, cell_perm)
        bx, by, cnt = bx[p], by[p], cnt[p]
    off = bx != by
    w = np.where(np.asarray(valid, bool), 1.0, 0.0)
    iters, converged, var, scale = 0, False, float("nan"), float("nan")
    for _ in range(int(max_iters)):
        t = (w[bx] * cnt) * w[by]
        s = np.bincount(bx, t, nb) + np.bincount(by[off], t[off], nb)
        nz = s != 0
        if not nz.any():
            break
        mean = s[nz].sum() / nz.sum()
        q = s[nz] / mean
        var = float(np.mean((q - 1.0) ** 2))
        scale = float(mean)
        w[nz] = w[nz] / q
        iters += 1
        if var < tol:
            converged = True
            break
    weight = np.full(nb, np.nan)
    if iters > 0:
        pos = w > 0
        weight[pos] = w[pos] / np.sqrt(scale)
    return {"iters": iters, "converged": converged, "var": var, "scale": scale, "weight": weight, "w": w}


def cell_perm(n, seed):
    """a seeded ordering of n cells, as the keys ice_oracle sorts them by"""
    return np.random.default_rng(seed).random(n)


def balanced_oracle(bx, by, cnt, b0, weight):
    bx, by = np.asarray(bx, np.int64) - b0, np.asarray(by, np.int64) - b0
    return (np.asarray(cnt, np.float64) * weight[bx]) * weight[by]


def longest_row(bx, by, ignore_diags):
    """L: the most used cells in one row of the full symmetric matrix"""
    b0, nb, _, _, z = marginals_oracle(bx, by, np.ones(len(bx), np.int64), ignore_diags)
    return int(z.max()) if nb else 0


def one_step_bound(bx, by, ignore_diags):
    """relative bound on the difference of two orders of summation after one iteration: 4 (L + nb) 2^-53"""
    return 4.0 * (longest_row(bx, by, ignore_diags) + span(bx, by)[1]) * EPS


def rel_diff(a, b):
    """the largest relative difference of two weight vectors with NaN at the same places"""
    a, b = np.asarray(a), np.asarray(b)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(a)
    if not m.any():
        return 0.0
    return float(np.max(np.abs(a[m] - b[m]) / np.abs(b[m])))


class OracleChrom(mc.OracleChrom):
    """the mat_* and bal_* methods of api.Chromosome on the oracles"""

    def __init__(self, X, Y):
        mc.OracleChrom.__init__(self, X, Y)
        self.bal = None
        self.folded = False

    def mat_cells(self, res, cut=0, fold=False):
        self.bal, self.folded = None, bool(fold)
        return mc.OracleChrom.mat_cells(self, res, cut=cut, fold=fold)

    def mat_free(self):
        self.bal = None
        mc.OracleChrom.mat_free(self)

    def bal_marginals(self, ignore_diags=2):
        if self.cells is None or not self.folded:
            raise RuntimeError("bal_marginals needs folded cells")
        if ignore_diags < 0:
            raise RuntimeError("ignore_diags below 0")
        b0, nb, nu, s, z = marginals_oracle(self.cells[0], self.cells[1], self.cells[2], ignore_diags)
        self.bal = {"ign": int(ignore_diags), "b0": b0, "nb": nb, "sum": s, "nnz": z, "res": None}
        return b0, nb, nu

    def _state(self, iterated=False):
        if self.bal is None or (iterated and self.bal["res"] is None):
            raise RuntimeError("bal_* out of order")
        return self.bal

    def bal_marginals_get(self, first=0, count=None):
        st = self._state()
        count = st["nb"] - first if count is None else count
        if first < 0 or count < 0 or first + count > st["nb"]:
            raise RuntimeError("bal_marginals_get outside the bins")
        return st["sum"][first:first + count].copy(), st["nnz"][first:first + count].copy()

    def bal_iterate(self, valid, max_iters=200, tol=1e-5):
        st = self._state()
        if len(valid) != st["nb"]:
            raise ValueError("bal_iterate: the mask needs one entry per bin")
        r = ice_oracle(self.cells[0], self.cells[1], self.cells[2], st["ign"], valid, max_iters, tol)
        st["res"] = r
        return r["iters"], r["converged"], r["var"], r["scale"]

    def bal_weights(self, first=0, count=None):
        st = self._state(True)
        count = st["nb"] - first if count is None else count
        return st["res"]["weight"][first:first + count].copy()

    def bal_cells_get(self, first=0, count=None):
        st = self._state(True)
        n = len(self.cells[0])
        count = n - first if count is None else count
        if first < 0 or count < 0 or first + count > n:
            raise RuntimeError("bal_cells_get outside the cells")
        sl = slice(first, first + count)
        return balanced_oracle(self.cells[0][sl], self.cells[1][sl], self.cells[2][sl], st["b0"], st["res"]["weight"])

    def bal_free(self):
        self.bal = None


# ---- data ------------------------------------------------------------------------------------------------------
def planted(n=24, seed=5):
    """cells of A[i][j] = d_i d_j M[i][j], M an integer symmetric circulant with a full first row, d integers in [1, 6]: the balanced
    matrix is a multiple of M, whose rows have equal sums, so weight[i] d_i is the same for every i -> (bx, by, cnt, d)"""
    rng = np.random.default_rng(seed)
    half = rng.integers(1, 9, n // 2 + 1)
    row = np.array([half[min(k, n - k)] for k in range(n)], np.int64)              # row[k] = row[n - k]: symmetric
    M = np.array([[row[(j - i) % n] for j in range(n)] for i in range(n)], np.int64)
    d = rng.integers(1, 7, n).astype(np.int64)
    A = M * d[:, None] * d[None, :]
    i, j = np.triu_indices(n)
    return i.astype(np.int32), j.astype(np.int32), A[i, j].astype(np.uint32), d


def arrow(seed=11):
    """rows that make a row run and a column run of more than two tiles each: 7000 with X in bin 0 and Y uniform over 6000 bins of
    100 bp, 7000 with Y in the last bin and X uniform, 60000 near the diagonal -> (X, Y), res 100"""
    rng = np.random.default_rng(seed)
    nbins, res = 6000, 100
    X1 = rng.integers(0, res, 7000)
    Y1 = rng.integers(0, nbins * res, 7000)
    Y2 = (nbins - 1) * res + rng.integers(0, res, 7000)
    X2 = rng.integers(0, nbins * res, 7000)
    X3 = rng.integers(0, nbins * res - 800, 60000)
    Y3 = X3 + rng.integers(0, 800, 60000)
    return np.concatenate([X1, X2, X3]).astype(np.int64), np.concatenate([Y1, Y2, Y3]).astype(np.int64)


def with_cell_count(target, seed=3):
    """rows whose folded cells at res 1000 number exactly `target`: distinct cells drawn without replacement from a band, some of
    them twice -> (X, Y)"""
    rng = np.random.default_rng(seed)
    nb, width = 400, 40
    cells = [(i, j) for i in range(nb) for j in range(i, min(nb, i + width))]
    assert target <= len(cells)
    pick = rng.choice(len(cells), target, replace=False)
    X, Y = [], []
    for k in pick.tolist():
        i, j = cells[k]
        for _ in range(1 + (k % 3 == 0)):
            X.append(i * 1000 + int(rng.integers(0, 1000)))
            Y.append(j * 1000 + int(rng.integers(0, 1000)))
    X, Y = np.array(X, np.int64), np.array(Y, np.int64)
    lo, hi = np.minimum(X, Y), np.maximum(X, Y)
    return lo, hi


def gapped(seed=9):
    """scattered rows in two stretches with 60 empty bins of 1000 bp between them, and a few long rows across the gap -> (X, Y)"""
    Xa, Ya = mc.scattered(seed, 8000, 60000, 20000)
    Xb, Yb = mc.scattered(seed + 1, 8000, 60000, 20000)
    rng = np.random.default_rng(seed + 2)
    Xc = rng.integers(0, 60000, 300)
    Yc = 140000 + rng.integers(0, 60000, 300)
    return np.concatenate([Xa, Xb + 140000, Xc]), np.concatenate([np.minimum(Ya, 79999), Yb + 140000, Yc])
