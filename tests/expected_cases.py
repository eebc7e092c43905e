"""The numpy oracle of K26 (cl_exp_diagonals / cl_exp_diagonals_get / cl_exp_set / cl_exp_cells_get), written from the definitions of
include/cloops_hip.h and not from cloops_amd.expected or the kernels, the oracle of the host's smoothing in integer arithmetic, a
stand-in chromosome made of them for the host tier, and the data makers of tests/test_expected_host.py and tests/test_gpu_expected.py."""
import numpy as np

import balance_cases as BC
import matrix_cases as MC

TILE = BC.TILE                                                   # cells per workgroup of the sums per diagonal (K25_TILE, cl_segsum.h)
DIAG_BLOCK = 256                                                 # diagonals per workgroup of the pair kernel (K26_DB)
WINDOW = 512                                                     # mask words per LDS window of the pair kernel (K26_WIN): 64 bins a word
EPS = 2.0 ** -53


def pairs_oracle(valid, ign):
    """n_pairs[d] = #{i : valid[i] and valid[i + d]} for d >= ign, 0 below -> int64[nb]: the autocorrelation of the mask"""
    v = np.asarray(valid, bool).astype(np.int64)
    nb = len(v)
    if nb == 0:
        return np.zeros(0, np.int64)
    out = np.correlate(v, v, "full")[nb - 1:].astype(np.int64)              # [nb - 1 + d] = sum_i v[i + d] v[i], in int64
    out[:min(int(ign), nb)] = 0
    return out


def pairs_by_loop(valid, ign):
    """the same by the definition's own loop (small nb)"""
    v = np.asarray(valid, bool)
    nb = len(v)
    return np.array([0 if d < ign else sum(1 for i in range(nb - d) if v[i] and v[i + d]) for d in range(nb)], np.int64).reshape(nb)


def used_of(bx, by, b0, ign, valid):
    bx, by = np.asarray(bx, np.int64), np.asarray(by, np.int64)
    valid = np.asarray(valid, bool)
    return ((by - bx) >= int(ign)) & valid[bx - b0] & valid[by - b0]


def terms_of(bx, by, cnt, b0, w):
    """(w[bx] cnt) w[by] of every cell, in K25's order of operations"""
    w = np.asarray(w, np.float64)
    return (w[np.asarray(bx, np.int64) - b0] * np.asarray(cnt, np.float64)) * w[np.asarray(by, np.int64) - b0]


def diagonals_oracle(bx, by, cnt, b0, nb, ign, valid, w, perm=None):
    """-> (n_pairs int64[nb], cnt_sum uint64[nb], val_sum float64[nb], n_used).  valid: bool[nb]; w: nb weights (read on the valid bins
    only).  `perm`: one sort key per cell (BC.cell_perm): the cells are put into that order before the sums are taken -- np.bincount
    adds in the order of its input, so two orders show how far the order of summation alone moves val_sum."""
    bx, by, cnt = np.asarray(bx, np.int64), np.asarray(by, np.int64), np.asarray(cnt, np.int64)
    valid = np.asarray(valid, bool)
    if perm is not None:
        p = np.argsort(np.asarray(perm, np.float64), kind="stable")
        bx, by, cnt = bx[p], by[p], cnt[p]
    u = used_of(bx, by, b0, ign, valid)
    d = (by - bx)[u]
    cs = np.zeros(nb, np.int64)
    np.add.at(cs, d, cnt[u])
    t = terms_of(bx[u], by[u], cnt[u], b0, np.where(valid, np.asarray(w, np.float64), 0.0))
    vs = np.bincount(d, t, nb) if nb else np.zeros(0)
    return pairs_oracle(valid, ign), cs.astype(np.uint64), vs.astype(np.float64), int(u.sum())


def oe_oracle(bx, by, cnt, b0, nb, ign, valid, w, expected):
    """the O/E of every cell -> float64: NaN when the cell is not used or expected[by - bx] is NaN or 0"""
    bx, by = np.asarray(bx, np.int64), np.asarray(by, np.int64)
    valid, e = np.asarray(valid, bool), np.asarray(expected, np.float64)
    u = used_of(bx, by, b0, ign, valid)
    out = np.full(len(bx), np.nan)
    ed = np.full(len(bx), np.nan)
    ed[u] = e[(by - bx)[u]]
    ok = u & ~np.isnan(ed) & (ed != 0)
    out[ok] = terms_of(bx[ok], by[ok], np.asarray(cnt)[ok], b0, np.where(valid, np.asarray(w, np.float64), 0.0)) / ed[ok]
    return out


def edges_oracle(nd, P):
    """the group bounds over [0, nd) in integers: ceil(10 ** (k / P)) is the smallest e with e ** P >= 10 ** k -> list, 0 first, nd last"""
    if nd <= 0:
        return [0]
    out, k, e = [0], 0, 1
    while True:
        while e ** P < 10 ** k:
            e += 1
        if e >= nd:
            break
        if e > out[-1]:
            out.append(e)
        k += 1
    return out + [nd]


def smooth_oracle(n_pairs, val_sum, P):
    """-> (smoothed float64[nd], groups [(start, end, n_pairs, value_sum, value_avg)]) by plain loops"""
    nd = len(n_pairs)
    b = edges_oracle(nd, P)
    sm, groups = np.full(nd, np.nan), []
    for g in range(len(b) - 1):
        p = int(sum(int(n_pairs[d]) for d in range(b[g], b[g + 1])))
        v = 0.0
        for d in range(b[g], b[g + 1]):
            v += float(val_sum[d])
        a = v / p if p > 0 else float("nan")
        groups.append((b[g], b[g + 1], p, v, a))
        sm[b[g]:b[g + 1]] = a
    return sm, groups


def sum_bound(bx, by, b0, nb, ign, valid):
    """per diagonal the relative bound between two orders of summation of val_sum: every term carries two roundings, a diagonal of L
    positive terms adds at most L - 1 more: (L + 2) 2^-53 -> float64[nb] (and L)"""
    u = used_of(bx, by, b0, ign, valid)
    L = np.bincount((np.asarray(by, np.int64) - np.asarray(bx, np.int64))[u], minlength=nb) if nb else np.zeros(0, np.int64)
    return (L + 2) * EPS, L


class OracleChrom(BC.OracleChrom):
    """the mat_*, bal_* and exp_* methods of api.Chromosome on the oracles"""

    def __init__(self, X, Y):
        BC.OracleChrom.__init__(self, X, Y)
        self.exp = None

    def mat_cells(self, res, cut=0, fold=False):
        self.exp = None
        return BC.OracleChrom.mat_cells(self, res, cut=cut, fold=fold)

    def mat_free(self):
        self.exp = None
        BC.OracleChrom.mat_free(self)

    def bal_marginals(self, ignore_diags=2):
        self.exp = None
        return BC.OracleChrom.bal_marginals(self, ignore_diags)

    def bal_iterate(self, valid, max_iters=200, tol=1e-5):
        self.exp = None
        return BC.OracleChrom.bal_iterate(self, valid, max_iters, tol)

    def bal_free(self):
        self.exp = None
        BC.OracleChrom.bal_free(self)

    def exp_diagonals(self, valid=None, balanced=True):
        st = self._state(bool(balanced))
        nb = st["nb"]
        if balanced:
            if valid is not None:
                raise RuntimeError("exp_diagonals: the balanced mode takes no mask")
            w = st["res"]["weight"]
            v = ~np.isnan(w)
        else:
            v = np.ones(nb, bool) if valid is None else np.asarray(valid) != 0
            if len(v) != nb:
                raise ValueError("exp_diagonals: the mask needs one entry per bin")
            w = np.ones(nb)
        n_pairs, cs, vs, nu = diagonals_oracle(self.cells[0], self.cells[1], self.cells[2], st["b0"], nb, st["ign"], v, w)
        self.exp = {"valid": v, "w": w, "n_pairs": n_pairs, "cnt_sum": cs, "val_sum": vs, "expected": None}
        return nb, nu

    def _exp(self, need_expected=False):
        if self.exp is None or (need_expected and self.exp["expected"] is None):
            raise RuntimeError("exp_* out of order")
        return self.exp

    def exp_diagonals_get(self, first=0, count=None):
        ex = self._exp()
        nd = len(ex["n_pairs"])
        count = nd - first if count is None else count
        if first < 0 or count < 0 or first + count > nd:
            raise RuntimeError("exp_diagonals_get outside the diagonals")
        return tuple(ex[k][first:first + count].copy() for k in ("n_pairs", "cnt_sum", "val_sum"))

    def exp_set(self, expected):
        ex = self._exp()
        e = np.asarray(expected, np.float64)
        if e.ndim != 1 or len(e) != len(ex["n_pairs"]):
            raise RuntimeError("exp_set: one expected value per diagonal")
        ex["expected"] = e.copy()

    def exp_cells_get(self, first=0, count=None):
        ex = self._exp(True)
        n = len(self.cells[0])
        count = n - first if count is None else count
        if first < 0 or count < 0 or first + count > n:
            raise RuntimeError("exp_cells_get outside the cells")
        sl = slice(first, first + count)
        st = self.bal
        return oe_oracle(self.cells[0][sl], self.cells[1][sl], self.cells[2][sl], st["b0"], st["nb"], st["ign"], ex["valid"], ex["w"],
                         ex["expected"])

    def exp_free(self):
        self.exp = None


# ---- data ------------------------------------------------------------------------------------------------------
def spanning(nb, seed=0, filler=40):
    """rows at res 1 whose folded cells span exactly the bins 0 .. nb - 1: one row in cell (0, nb - 1) and some filler -> (X, Y)"""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, nb, filler)
    Y = rng.integers(0, nb, filler)
    X, Y = np.concatenate([[0], np.minimum(X, Y)]), np.concatenate([[nb - 1], np.maximum(X, Y)])
    return X.astype(np.int64), Y.astype(np.int64)


def one_diagonal(n_cells, d=3):
    """rows at res 1 with exactly n_cells cells, all on diagonal d (every third of them twice) -> (X, Y)"""
    i = np.arange(n_cells, dtype=np.int64)
    twice = i[::3]
    X = np.concatenate([i, twice])
    return X, X + d


def own_diagonals(n):
    """rows at res 1 with n cells, every one on a diagonal of its own: (k, 2 k) for k < n -> (X, Y)"""
    k = np.arange(n, dtype=np.int64)
    return k, 2 * k
