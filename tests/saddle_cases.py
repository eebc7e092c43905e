"""The numpy oracle of K30 (cl_sad_sums / cl_sad_get), written from the definitions of include/cloops_hip.h and not from
cloops_amd.saddle or the kernels: the pair set by the definition's own double loop and by per-class prefix counts, the three tables,
the bound between two orders of summation, a stand-in chromosome made of them for the host tier, and the data makers of
tests/test_saddle_host.py and tests/test_gpu_saddle.py."""
import numpy as np

import balance_cases as BC
import compartments_cases as CC
import expected_cases as EC
import matrix_cases as MC

TILE = 256                                                       # cells per step of a workgroup of the sums (K30_TILE): one per thread
CHUNKS = 1024                                                    # most chunks of consecutive tiles (K30_CHUNKS): up to there a chunk is one tile
WAVE = 64                                                        # cells a wave folds key by key
SCAN_TILE = 256                                                  # bins per workgroup of the pair counts (K30_PT)
CLASSES_MAX = 64
EPS = EC.EPS


def effective(valid, cls):
    """the class of a bin that takes part, -1 for every other bin"""
    cls = np.asarray(cls, np.int64)
    return np.where(np.asarray(valid, bool) & (cls >= 0), cls, -1)


def pairs_by_loop(valid, cls, n_cls, lo, hi):
    """pairs[a][b] by the definition's own double loop (small nb)"""
    kc = effective(valid, cls)
    nb = len(kc)
    out = np.zeros((n_cls, n_cls), np.int64)
    for i in range(nb):
        for j in range(i + 1, nb):
            if lo <= j - i < hi and kc[i] >= 0 and kc[j] >= 0:
                out[kc[i]][kc[j]] += 1
    return out


def pairs_by_prefix(valid, cls, n_cls, lo, hi):
    """the same as differences of per-class prefix counts: bin i of class a adds C_b(min(i + hi, nb)) - C_b(min(i + lo, nb)) to
    pairs[a][b], C_b(k) the bins below k of class b"""
    kc = effective(valid, cls)
    nb = len(kc)
    out = np.zeros((n_cls, n_cls), np.int64)
    if nb == 0 or hi <= lo:
        return out
    C = np.zeros((nb + 1, n_cls), np.int64)
    C[1:] = np.cumsum(kc[:, None] == np.arange(n_cls)[None, :], axis=0)
    i = np.arange(nb)
    D = C[np.minimum(i + hi, nb)] - C[np.minimum(i + lo, nb)]
    ok = kc >= 0
    np.add.at(out, kc[ok], D[ok])
    return out


def check_band(nb, ign, lo, hi):
    if nb == 0:
        return lo == 0 and hi == 0
    return max(int(ign), 1) <= lo <= hi <= nb


def tables_oracle(cells, b0, nb, ign, valid, w, expected, cls, n_cls, lo, hi, perm=None):
    """-> (sum float64, pairs int64, cells int64), each [n_cls, n_cls]; ValueError where cl_sad_sums refuses its arguments.  `perm`: one
    sort key per cell (BC.cell_perm): the cells are put into that order before the sums are taken -- np.bincount adds in the order of
    its input."""
    cls = np.asarray(cls, np.int64)
    if not 1 <= n_cls <= CLASSES_MAX or len(cls) != nb or (nb and (cls.min() < -1 or cls.max() >= n_cls)) or not check_band(nb, ign, lo, hi):
        raise ValueError("sad_sums: bad arguments")
    valid, e = np.asarray(valid, bool), np.asarray(expected, np.float64)
    vp = EC.pairs_oracle(valid, 0)
    for d in range(int(lo), int(hi)):
        if vp[d] > 0 and not (np.isfinite(e[d]) and e[d] > 0):
            raise ValueError("sad_sums: expected[%d] is no finite positive number" % d)
    bx, by, cnt = (np.asarray(a, np.int64) for a in cells)
    if perm is not None:
        p = np.argsort(np.asarray(perm, np.float64), kind="stable")
        bx, by, cnt = bx[p], by[p], cnt[p]
    kc = effective(valid, cls)
    ix, iy = bx - b0, by - b0
    d = by - bx
    inp = (d >= lo) & (d < hi)
    inp[inp] &= (kc[ix[inp]] >= 0) & (kc[iy[inp]] >= 0)
    K = n_cls * n_cls
    key = kc[ix[inp]] * n_cls + kc[iy[inp]]
    wv = np.where(valid, np.asarray(w, np.float64), 0.0)
    term = EC.terms_of(bx[inp], by[inp], cnt[inp], b0, wv) / e[d[inp]]
    s = np.bincount(key, term, K).reshape(n_cls, n_cls) if K else np.zeros((0, 0))
    c = np.bincount(key, minlength=K).reshape(n_cls, n_cls).astype(np.int64)
    return s.astype(np.float64), pairs_by_prefix(valid, cls, n_cls, lo, hi), c


def sum_bound(cells_table):
    """per entry the relative bound between the device's sum and the oracle's: the device's term may deviate 4 2^-53 relative from the
    oracle's (K26's O/E bound), and a sum of L non-negative terms in any order is within (L - 1) 2^-53 of the exact sum of its terms:
    (2 L + 4) 2^-53, L = cells[a][b]"""
    return (2.0 * np.asarray(cells_table, np.float64) + 4.0) * EPS


def within(got, want, cells_table):
    """whether every entry of two sum tables lies within sum_bound, and the largest deviation over its bound"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    allowed = sum_bound(cells_table) * np.abs(want)
    dev = np.abs(got - want)
    ok = bool(np.all(dev <= allowed))
    live = allowed > 0
    return ok, float(np.max(dev[live] / allowed[live])) if live.any() else 0.0


class OracleChrom(CC.OracleChrom):
    """the mat_*, bal_*, exp_*, eig_* and sad_* methods of api.Chromosome on the oracles"""

    def __init__(self, X, Y):
        CC.OracleChrom.__init__(self, X, Y)
        self.sad = None

    def mat_cells(self, res, cut=0, fold=False):
        self.sad = None
        return CC.OracleChrom.mat_cells(self, res, cut=cut, fold=fold)

    def mat_free(self):
        self.sad = None
        CC.OracleChrom.mat_free(self)

    def bal_marginals(self, ignore_diags=2):
        self.sad = None
        return CC.OracleChrom.bal_marginals(self, ignore_diags)

    def bal_iterate(self, valid, max_iters=200, tol=1e-5):
        self.sad = None
        return CC.OracleChrom.bal_iterate(self, valid, max_iters, tol)

    def bal_free(self):
        self.sad = None
        CC.OracleChrom.bal_free(self)

    def exp_diagonals(self, valid=None, balanced=True):
        self.sad = None
        return CC.OracleChrom.exp_diagonals(self, valid, balanced)

    def exp_set(self, expected):
        self.sad = None
        CC.OracleChrom.exp_set(self, expected)

    def exp_free(self):
        self.sad = None
        CC.OracleChrom.exp_free(self)

    def sad_sums(self, cls, n_cls, lo, hi):
        ex, st = self._exp(True), self.bal
        try:
            t = tables_oracle(self.cells, st["b0"], st["nb"], st["ign"], ex["valid"], ex["w"], ex["expected"], cls, int(n_cls), int(lo), int(hi))
        except ValueError as e:
            raise RuntimeError(str(e))
        self.sad = t
        return int(np.count_nonzero(effective(ex["valid"], cls) >= 0)), int(t[1].sum()), int(t[2].sum())

    def sad_get(self):
        if self.sad is None:
            raise RuntimeError("sad_get before sad_sums")
        return tuple(a.copy() for a in self.sad)

    def sad_free(self):
        self.sad = None


# ---- data ------------------------------------------------------------------------------------------------------
def row_of_cells(n_cells, first=3):
    """rows at res 1 with exactly n_cells cells in the one row of bin 0: (0, first) .. (0, first + n_cells - 1), every third of them
    twice, and nothing else -> (X, Y): b0 = 0, nb = first + n_cells"""
    j = first + np.arange(n_cells, dtype=np.int64)
    Y = np.concatenate([j, j[::3]])
    return np.zeros(len(Y), np.int64), Y


def rows_of(lengths, d0=1):
    """rows at res 1: bin i has the cells (i, i + d0) .. (i, i + d0 + lengths[i] - 1), 1 to 3 rows a cell -> (X, Y)"""
    X, Y = [], []
    for i, n in enumerate(lengths):
        for j in range(i + d0, i + d0 + n):
            X += [i] * (1 + (i + j) % 3)
            Y += [j] * (1 + (i + j) % 3)
    return np.array(X, np.int64), np.array(Y, np.int64)


def uniform_like(name, seed=11):
    """PETs of the size of CC.PLANTED[name] without compartments (delta = 0) -> (X, Y)"""
    p = dict(CC.PLANTED[name], delta=0.0, seed=seed)
    return CC.planted(**p)[:2]
