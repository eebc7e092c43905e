"""The numpy oracle of K24 (cl_mat_window / cl_mat_cells / cl_mat_v4c), written from the definitions of include/cloops_hip.h and not
from cloops_amd.matrix, a stand-in chromosome made of it for the host tier, and the data makers of tests/test_matrix_host.py and
tests/test_gpu_matrix.py."""
import numpy as np

EMPTY = np.zeros(0, np.int64)


def kept(X, Y, cut):
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    if cut > 0:
        m = (Y - X) >= cut
        X, Y = X[m], Y[m]
    return X, Y


def bins(p, res):
    return np.floor_divide(np.asarray(p, np.int64), np.int64(res))


def window_oracle(X, Y, cut, res, bx0, by0, nx, ny, mirror=False):
    """-> (uint32 [nx, ny], n_in, n_kept)"""
    X, Y = kept(X, Y, cut)
    bx, by = bins(X, res), bins(Y, res)
    out = np.zeros((nx, ny), np.int64)
    i, j = bx - bx0, by - by0
    ok = (i >= 0) & (i < nx) & (j >= 0) & (j < ny)
    np.add.at(out, (i[ok], j[ok]), 1)
    if mirror:
        i, j = by - bx0, bx - by0
        ok = (bx != by) & (i >= 0) & (i < nx) & (j >= 0) & (j < ny)
        np.add.at(out, (i[ok], j[ok]), 1)
    return out.astype(np.uint32), int(out.sum()), len(X)


def cells_oracle(X, Y, cut, res, fold=False):
    """-> (bx int32, by int32, cnt uint32) ascending by bx then by, n_kept"""
    X, Y = kept(X, Y, cut)
    if len(X) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint32), 0
    pairs = np.stack([bins(X, res), bins(Y, res)], 1)
    if fold:
        pairs = np.sort(pairs, axis=1)
    u, c = np.unique(pairs, axis=0, return_counts=True)
    return u[:, 0].astype(np.int32), u[:, 1].astype(np.int32), c.astype(np.uint32), len(X)


def v4c_oracle(X, Y, cut, res, v0, v1, b0, nb):
    """-> (uint32 [nb], n_x, n_y, n_kept)"""
    X, Y = kept(X, Y, cut)
    bx, by = bins(X, res), bins(Y, res)
    inx, iny = (X >= v0) & (X < v1), (Y >= v0) & (Y < v1)
    out = np.zeros(nb, np.int64)
    for sel, b in ((inx, by), (iny, bx)):
        k = b[sel] - b0
        k = k[(k >= 0) & (k < nb)]
        np.add.at(out, k, 1)
    return out.astype(np.uint32), int(inx.sum()), int(iny.sum()), len(X)


class OracleChrom(object):
    """the five mat_* methods of api.Chromosome on the oracle"""

    def __init__(self, X, Y):
        self.X, self.Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
        self.cells = None
        self.calls = []

    def mat_window(self, res, bx0, by0, nx, ny, cut=0, mirror=False):
        self.calls.append("window")
        return window_oracle(self.X, self.Y, cut, res, bx0, by0, nx, ny, mirror)

    def mat_cells(self, res, cut=0, fold=False):
        self.calls.append("cells")
        bx, by, cnt, nk = cells_oracle(self.X, self.Y, cut, res, fold)
        self.cells = (bx, by, cnt)
        return len(bx), nk, int(cnt.max()) if len(cnt) else 0

    def mat_cells_get(self, first=0, count=None):
        if self.cells is None:
            raise RuntimeError("mat_cells_get before mat_cells")
        n = len(self.cells[0])
        count = n - first if count is None else count
        if first < 0 or count < 0 or first + count > n:
            raise RuntimeError("mat_cells_get outside the cells")
        return tuple(a[first:first + count].copy() for a in self.cells)

    def mat_v4c(self, res, v0, v1, b0, nb, cut=0):
        self.calls.append("v4c")
        return v4c_oracle(self.X, self.Y, cut, res, v0, v1, b0, nb)

    def mat_free(self):
        self.cells = None


class Recording(object):
    """a stand-in chromosome that lists the calls made on it from outside as (name, args, keywords), an array written as its dtype's
    kind and length (`b[5]`); `fail`: the method that raises instead of running"""

    def __init__(self, inner, fail=None):
        self.inner, self.fail, self.log = inner, fail, []

    @staticmethod
    def _plain(v):
        if isinstance(v, np.ndarray):
            return "%s[%s]" % (v.dtype.kind, ",".join(str(n) for n in v.shape))
        return v.item() if isinstance(v, np.generic) else v

    def __getattr__(self, name):
        method = getattr(self.inner, name)
        if not callable(method):
            return method

        def call(*args, **kw):
            self.log.append((name, tuple(self._plain(a) for a in args), {k: self._plain(v) for k, v in kw.items()}))
            if name == self.fail:
                raise RuntimeError("%s fails" % name)
            return method(*args, **kw)
        return call


# ---- data ------------------------------------------------------------------------------------------------------
def twelve():
    """a hand-written example: twelve rows over the bins 0 .. 4 of 100 bp, one of them with Y < X, two duplicates"""
    X = np.array([10, 20, 120, 130, 130, 250, 260, 310, 90, 405, 399, 0], np.int64)
    Y = np.array([30, 150, 180, 330, 330, 270, 420, 350, 480, 120, 400, 499], np.int64)
    return X, Y


def scattered(seed, m, span=200000, width=30000, both=False):
    """m rows with X in [0, span) and Y = X + [0, width); `both`: a third of them with Y < X"""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, span, m)
    Y = X + rng.integers(0, width, m)
    if both:
        flip = rng.random(m) < 1.0 / 3
        X, Y = np.where(flip, Y, X), np.where(flip, X, Y)
    return X.astype(np.int64), Y.astype(np.int64)


def dense_scatter(bx, by, cnt, bx0, by0, nx, ny):
    """the cells scattered into a dense array over [bx0, bx0 + nx) x [by0, by0 + ny)"""
    out = np.zeros((nx, ny), np.int64)
    np.add.at(out, (np.asarray(bx, np.int64) - bx0, np.asarray(by, np.int64) - by0), np.asarray(cnt, np.int64))
    return out
