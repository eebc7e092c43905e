"""The numpy restatement of K29 (cl_dot_lambdas / cl_dot_hist / cl_dot_call and their gets), written from the definitions of
include/cloops_hip.h with dense matrices and brute-force sums and not from the kernels; the host rules of cloops_amd.dots (thresholds,
filter, components) by plain loops; a stand-in chromosome made of them for the host tier; and the data makers of
tests/test_dots_host.py and tests/test_gpu_dots.py."""
import numpy as np

import expected_cases as EC

TILE = 32                                                        # bins and diagonals of a tile of k29_lambdas (K29_TI, K29_TD)
WMAX, CHUNKS_MAX, CMAX = 16, 64, 4095                            # CL_DOT_WMAX, CL_DOT_CHUNKS_MAX, CL_DOT_CMAX
EPS = 2.0 ** -53
NO_THRESHOLD = 0xFFFFFFFF


def rtol(w):
    """the bound between the device's la and the restatement's: both form bit-equal non-negative terms; any order of adding at most
    T = (2w+1)^2 of them lies within (T - 1) u of the exact sum, two orders within 2 (T - 1) u of each other; NO and NE contribute that
    twice; the division, the multiplication and the division add a few u: (4 T + 8) 2^-53"""
    return (4 * (2 * w + 1) ** 2 + 8) * EPS


def masks(p, w):
    """the four neighbourhoods as bool [2w+1, 2w+1], entry [a + w, b + w], straight from the offset rules"""
    out = np.zeros((4, 2 * w + 1, 2 * w + 1), bool)
    for a in range(-w, w + 1):
        for b in range(-w, w + 1):
            inner = abs(a) <= p and abs(b) <= p
            out[0, a + w, b + w] = a != 0 and b != 0 and not inner
            out[1, a + w, b + w] = 1 <= a <= w and -w <= b <= -1 and not inner
            out[2, a + w, b + w] = abs(a) <= 1 and p < abs(b) <= w
            out[3, a + w, b + w] = abs(b) <= 1 and p < abs(a) <= w
    return out


def dense_VE(cells, b0, nb, ign, valid, w, expected):
    """the two symmetric nb x nb matrices of the definitions"""
    bx, by, cnt = (np.asarray(a, np.int64) for a in cells)
    valid, wt, e = np.asarray(valid, bool), np.where(np.asarray(valid, bool), np.asarray(w, np.float64), 0.0), np.asarray(expected, np.float64)
    u, v = bx - b0, by - b0
    used = ((v - u) >= ign) & valid[u] & valid[v]
    t = (wt[u] * cnt.astype(np.float64)) * wt[v]                            # K25's order of operations
    V = np.zeros((nb, nb))
    V[u[used], v[used]] = t[used]
    V[v[used], u[used]] = t[used]
    d = np.abs(np.arange(nb)[:, None] - np.arange(nb)[None, :])
    ok = valid[:, None] & valid[None, :] & (d >= ign)
    E = np.zeros((nb, nb))
    E[ok] = e[d[ok]]
    return V, E


def box_sums(M, mask):
    """S[i][j] = the sum of M[i + a][j + b] over the offsets of the mask, zero outside the matrix: one shifted slice per offset"""
    nb, w = len(M), (mask.shape[0] - 1) // 2
    P = np.zeros((nb + 2 * w, nb + 2 * w))
    P[w:w + nb, w:w + nb] = M
    S = np.zeros((nb, nb))
    for a in range(-w, w + 1):
        for b in range(-w, w + 1):
            if mask[a + w, b + w]:
                S += P[w + a:w + a + nb, w + b:w + b + nb]
    return S


def count_plane(cells, b0, nb, dmin, dmax):
    """the raw count of every pixel (i, d), dmin <= d < dmax: int64 [nb, dmax - dmin], 0 without a cell"""
    bx, by, cnt = (np.asarray(a, np.int64) for a in cells)
    out = np.zeros((nb, dmax - dmin), np.int64)
    d = by - bx
    m = (d >= dmin) & (d < dmax)
    out[bx[m] - b0, d[m] - dmin] = cnt[m]
    return out


def lambdas_oracle(cells, b0, nb, ign, valid, w, expected, p, wd, dmin, dmax):
    """-> (la float64 [4, nb, dmax - dmin], NaN as the definitions say; n_cand; n_full)"""
    valid, wt, e = np.asarray(valid, bool), np.asarray(w, np.float64), np.asarray(expected, np.float64)
    nd = dmax - dmin
    la = np.full((4, nb, nd), np.nan)
    if nb == 0:
        return la, 0, 0
    V, E = dense_VE(cells, b0, nb, ign, valid, wt, e)
    i = np.arange(nb)[:, None] + np.zeros((1, nd), np.int64)
    d = np.arange(dmin, dmax)[None, :] + np.zeros((nb, 1), np.int64)
    j = i + d
    cand = j < nb
    jj = np.where(cand, j, 0)
    cand &= valid[i] & valid[jj]
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, mask in enumerate(masks(p, wd)):
            NO, NE = box_sums(V, mask)[i, jj], box_sums(E, mask)[i, jj]
            x = ((NO / NE) * e[d]) / (wt[i] * wt[jj])
            la[k] = np.where(cand & (NE != 0), x, np.nan)
    full = ~np.isnan(la).any(axis=0)
    return la, int(cand.sum()), int(full.sum())


def chunk_of(x, edges):
    """the smallest l with x <= edges[l]: the number of edges below x (len(edges): beyond)"""
    return np.searchsorted(np.asarray(edges, np.float64), np.asarray(x, np.float64), side="left")


def hist_oracle(la, counts, edges):
    """la [4, nb, nd] and the pixels' raw counts [nb, nd] -> (hist uint64 [4, n_chunks, CMAX + 1], n_beyond)"""
    nch = len(edges)
    full = ~np.isnan(la).any(axis=0)
    ch = np.stack([chunk_of(np.where(full, la[k], 0.0), edges) for k in range(4)])
    beyond = full & (ch >= nch).any(axis=0)
    use = full & ~beyond
    c = np.minimum(np.asarray(counts, np.int64), CMAX)[use]
    hist = np.zeros((4, nch, CMAX + 1), np.uint64)
    for k in range(4):
        np.add.at(hist[k], (ch[k][use], c), np.uint64(1))
    return hist, int(beyond.sum())


def cells_la(cells, b0, nb, dmin, dmax, la):
    """the gather of the cells' pixels from the dense array -> [n, 4], NaN where the cell lies outside the diagonals"""
    bx, by = np.asarray(cells[0], np.int64), np.asarray(cells[1], np.int64)
    d = by - bx
    out = np.full((len(bx), 4), np.nan)
    m = (d >= dmin) & (d < dmax)
    out[m] = la[:, bx[m] - b0, d[m] - dmin].T
    return out


def call_oracle(cells, la4, edges, thr):
    """the ascending indices of the significant cells, from the cells' la [n, 4]"""
    cnt = np.asarray(cells[2], np.int64)
    nch = len(edges)
    full = ~np.isnan(la4).any(axis=1)
    ch = chunk_of(np.where(full[:, None], la4, 0.0), edges)
    ok = full & (ch < nch).all(axis=1)
    t = np.asarray(thr, np.int64)
    for k in range(4):
        ok &= cnt >= t[k][np.minimum(ch[:, k], nch - 1)]
    return np.flatnonzero(ok).astype(np.int64)


def thresholds_by_loop(hist, edges, fdr):
    """the rule of cloops_amd.dots.thresholds by its own loop over t"""
    from scipy.stats import poisson
    nk, nch, nc = hist.shape
    thr = np.full((nk, nch), NO_THRESHOLD, np.uint32)
    for k in range(nk):
        for l in range(nch):
            h = [int(x) for x in hist[k, l]]
            n = sum(h)
            for t in range(1, nc):
                ge = sum(h[t:])
                if ge == 0:
                    break
                if n * float(poisson.sf(t - 1, float(edges[l]))) <= fdr * ge:
                    thr[k, l] = t
                    break
    return thr


def components_by_flood(bx, by, r):
    """the connected components under Chebyshev distance <= r by a flood over all pairs -> a sorted list of sorted index lists"""
    n = len(bx)
    seen, out = [False] * n, []
    for s in range(n):
        if seen[s]:
            continue
        comp, todo = [], [s]
        seen[s] = True
        while todo:
            a = todo.pop()
            comp.append(a)
            for b in range(n):
                if not seen[b] and max(abs(int(bx[a]) - int(bx[b])), abs(int(by[a]) - int(by[b]))) <= r:
                    seen[b] = True
                    todo.append(b)
        out.append(sorted(comp))
    return sorted(out)


class OracleChrom(EC.OracleChrom):
    """the mat_*, bal_*, exp_* and dot_* methods of api.Chromosome on the restatements"""

    def __init__(self, X, Y):
        EC.OracleChrom.__init__(self, X, Y)
        self.dot = None

    def mat_cells(self, res, cut=0, fold=False):
        self.dot = None
        return EC.OracleChrom.mat_cells(self, res, cut=cut, fold=fold)

    def mat_free(self):
        self.dot = None
        EC.OracleChrom.mat_free(self)

    def bal_marginals(self, ignore_diags=2):
        self.dot = None
        return EC.OracleChrom.bal_marginals(self, ignore_diags)

    def bal_iterate(self, valid, max_iters=200, tol=1e-5):
        self.dot = None
        return EC.OracleChrom.bal_iterate(self, valid, max_iters, tol)

    def bal_free(self):
        self.dot = None
        EC.OracleChrom.bal_free(self)

    def exp_diagonals(self, valid=None, balanced=True):
        self.dot = None
        return EC.OracleChrom.exp_diagonals(self, valid, balanced)

    def exp_set(self, expected):
        self.dot = None
        EC.OracleChrom.exp_set(self, expected)

    def exp_free(self):
        self.dot = None
        EC.OracleChrom.exp_free(self)

    def dot_lambdas(self, p, w, dmin, dmax=None):
        ex, st = self._exp(True), self.bal
        nb, ign = st["nb"], st["ign"]
        dmax = nb if dmax is None else dmax
        if not 0 <= p < w <= WMAX:
            raise ValueError("dot_lambdas: needs 0 <= p < w <= %d" % WMAX)
        if (nb == 0 and (dmin, dmax) != (0, 0)) or (nb > 0 and not ign <= dmin < dmax <= nb):
            raise RuntimeError("dot_lambdas: dmin, dmax outside the rule")
        e = ex["expected"]
        for d in range(ign, min(nb, dmax + 2 * w)):
            if ex["n_pairs"][d] > 0 and not (np.isfinite(e[d]) and e[d] >= 0):
                raise RuntimeError("dot_lambdas: the rule on the expected values")
        la, nc, nf = lambdas_oracle(self.cells, st["b0"], nb, ign, ex["valid"], ex["w"], e, p, w, dmin, dmax)
        self.dot = {"la": la, "dmin": dmin, "dmax": dmax, "edges": None, "sig": None}
        return nc, nf

    def _dot(self, need=None):
        if self.dot is None or (need is not None and self.dot[need] is None):
            raise RuntimeError("dot_* out of order")
        return self.dot

    def dot_lambdas_get(self, kernel, first_bin=0, n_bins=None):
        dt = self._dot()
        nb = dt["la"].shape[1]
        n_bins = nb - first_bin if n_bins is None else n_bins
        if not 0 <= kernel < 4 or first_bin < 0 or n_bins < 0 or first_bin + n_bins > nb:
            raise RuntimeError("dot_lambdas_get outside")
        return dt["la"][kernel, first_bin:first_bin + n_bins].copy()

    def dot_cells(self, first=0, count=None):
        dt = self._dot()
        n = len(self.cells[0])
        count = n - first if count is None else count
        if first < 0 or count < 0 or first + count > n:
            raise RuntimeError("dot_cells outside the cells")
        sl = slice(first, first + count)
        return cells_la((self.cells[0][sl], self.cells[1][sl]), self.bal["b0"], self.bal["nb"], dt["dmin"], dt["dmax"], dt["la"])

    def dot_hist(self, edges):
        dt = self._dot()
        e = np.asarray(edges, np.float64)
        if e.ndim != 1 or not 1 <= len(e) <= CHUNKS_MAX or not (np.isfinite(e).all() and (e > 0).all() and (np.diff(e) > 0).all()):
            raise ValueError("dot_hist: the edges")
        dt["edges"], dt["sig"] = e, None
        return hist_oracle(dt["la"], count_plane(self.cells, self.bal["b0"], self.bal["nb"], dt["dmin"], dt["dmax"]), e)

    def dot_call(self, thr):
        dt = self._dot("edges")
        if np.asarray(thr).shape != (4, len(dt["edges"])):
            raise ValueError("dot_call: the thresholds")
        dt["sig"] = call_oracle(self.cells, self.dot_cells(), dt["edges"], thr)
        return len(dt["sig"])

    def dot_sig(self, first=0, count=None):
        sig = self._dot("sig")["sig"]
        count = len(sig) - first if count is None else count
        if first < 0 or count < 0 or first + count > len(sig):
            raise RuntimeError("dot_sig outside the list")
        return sig[first:first + count].copy()

    def dot_free(self):
        self.dot = None


# ---- data ------------------------------------------------------------------------------------------------------
def band_rows(nb, width, m, seed, shift=0):
    """rows at res 1 whose folded cells span exactly the bins shift .. shift + nb - 1: m rows with X uniform and Y - X uniform below
    `width` (kept inside the bins), and one row in cell (0, nb - 1) -> (X, Y)"""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, nb, m)
    Y = np.minimum(X + rng.integers(0, max(1, width), m), nb - 1)
    X, Y = np.concatenate([[0], X]), np.concatenate([[nb - 1], Y])
    return X.astype(np.int64) + shift, Y.astype(np.int64) + shift


def run_mask(n):
    """an invalid first and last bin and a run of invalid bins wider than a tile (where the bins reach that far)"""
    v = np.ones(n, bool)
    v[:1] = False
    v[n - 1:] = False
    v[20:20 + TILE + 4] = False
    return v


def sparse_mask(n):
    """every seventh bin invalid, and the last"""
    v = np.arange(n) % 7 != 3
    v[n - 1:] = False
    return v


def line_expected(n):
    return np.linspace(2.0, 0.5, n)


def zeros_expected(n):
    """a falling line with zeros on some diagonals, the main one among them"""
    e = np.linspace(3.0, 0.25, n)
    e[::5] = 0.0
    return e


# the shapes of the la tests: nb and nd = dmax - dmin each take every value of {1, 2, 31, 32, 33, 64, 65, 97}, (p, w) every pair of the
# six, ign 0, 2 and one above 2w, dmin = ign = 0 (footprints across the diagonal), w >= nb, a negative b0, masks, zeros, both modes.
# expected: None = cloops_amd.expected.expected_of of the device's own diagonals (NaN below ign), else a function of nb
LA_CASES = {
    "nb1":        dict(nb=1,  nd=1,  p=0,  w=1,  ign=0,  dmin=0,  raw=True,  mask=None,        expected=line_expected),
    "nb2":        dict(nb=2,  nd=2,  p=1,  w=3,  ign=0,  dmin=0,  raw=True,  mask=None,        expected=line_expected),
    "nb31":       dict(nb=31, nd=31, p=2,  w=5,  ign=0,  dmin=0,  raw=True,  mask=None,        expected=line_expected),
    "nb32":       dict(nb=32, nd=32, p=4,  w=7,  ign=0,  dmin=0,  raw=False, mask=None,        expected=None),
    "nb33":       dict(nb=33, nd=33, p=0,  w=16, ign=0,  dmin=0,  raw=True,  mask=None,        expected=zeros_expected),
    "nb64":       dict(nb=64, nd=64, p=15, w=16, ign=0,  dmin=0,  raw=True,  mask=sparse_mask, expected=line_expected),
    "nb65":       dict(nb=65, nd=65, p=2,  w=5,  ign=0,  dmin=0,  raw=False, mask=sparse_mask, expected=None),
    "nb97":       dict(nb=97, nd=97, p=1,  w=3,  ign=0,  dmin=0,  raw=True,  mask=run_mask,    expected=zeros_expected),
    "nd1":        dict(nb=97, nd=1,  p=2,  w=5,  ign=2,  dmin=5,  raw=True,  mask=None,        expected=None),
    "nd2":        dict(nb=97, nd=2,  p=0,  w=1,  ign=2,  dmin=3,  raw=False, mask=None,        expected=None),
    "nd31_neg":   dict(nb=97, nd=31, p=4,  w=7,  ign=2,  dmin=4,  raw=True,  mask=run_mask,    expected=None, shift=-40),
    "nd32_ign":   dict(nb=97, nd=32, p=2,  w=5,  ign=11, dmin=11, raw=True,  mask=None,        expected=None),
    "nd33_w16":   dict(nb=97, nd=33, p=0,  w=16, ign=2,  dmin=2,  raw=True,  mask=run_mask,    expected=None),
    "nd64_bal":   dict(nb=97, nd=64, p=15, w=16, ign=2,  dmin=17, raw=False, mask=sparse_mask, expected=None),
    "nd65_zeros": dict(nb=97, nd=65, p=1,  w=3,  ign=0,  dmin=3,  raw=True,  mask=None,        expected=zeros_expected),
}


def case_rows(name):
    """the rows of a case at res 1 -> (X, Y): some 25 rows per bin over a band as wide as the tested diagonals and their halo"""
    c = LA_CASES[name]
    seed = sorted(LA_CASES).index(name) + 1
    return band_rows(c["nb"], c["dmin"] + c["nd"] + 2 * c["w"], 25 * c["nb"], seed, c.get("shift", 0))


RECOVERY_SEED = 1                                                # (seeds 1, 2 and 3 all recover the eight and nothing else: test_dots_host.py)
PLANTED = ((50, 90), (120, 140), (200, 330), (260, 275), (300, 380), (10, 25), (350, 395), (3, 60))


def recovery_rows(seed, planted=True, nbins=400, res=1000, background=600000, extra=40, sd=300.0):
    """the recovery case: `background` PETs with X uniform over the window and Y - X log-uniform on [500, 400 000), those with Y beyond
    the window dropped, and `extra` PETs, normal with `sd` bp around the bins' centres, at each of the PLANTED bin pairs -> (X, Y)"""
    rng = np.random.default_rng(seed)
    span = nbins * res
    X = rng.integers(0, span, background)
    Y = X + np.exp(rng.uniform(np.log(500.0), np.log(400000.0), background)).astype(np.int64)
    keep = Y < span
    X, Y = X[keep], Y[keep]
    if planted:
        for a, b in PLANTED:
            px = np.rint((a + 0.5) * res + rng.normal(0.0, sd, extra)).astype(np.int64)
            py = np.rint((b + 0.5) * res + rng.normal(0.0, sd, extra)).astype(np.int64)
            X, Y = np.concatenate([X, px]), np.concatenate([Y, py])
    return X.astype(np.int64), Y.astype(np.int64)
