"""The numpy oracle of K27 (cl_eig_build / cl_eig_apply / cl_eig_iterate / cl_eig_vectors_get), written from the definitions of
include/cloops_hip.h and not from cloops_amd.compartments or the kernels: the dense matrix M, the same product in the sparse-plus-prefix
form with the bound between the two, the eigenpairs by np.linalg.eigh, a stand-in chromosome made of them for the host tier, and the
planted data of tests/test_compartments_host.py and tests/test_gpu_compartments.py."""
import numpy as np

import balance_cases as BC
import expected_cases as EC
import matrix_cases as MC

TILE = BC.TILE                                                   # cells per workgroup of K25's sums (the cell counts of the product's cases)
ROWS_PER_WG = 4                                                  # bins per workgroup of the block product (k27_mul: one wave each)
CELL_STEP = 8                                                    # cells a wave takes per step of a row (eight lanes per cell)
SCAN_TILE = 256                                                  # bins per workgroup of the band term's scan (K27_SB)
EIG_MAX, EIG_BLOCK = 6, 8
EPS = EC.EPS


def band_cells(bx, by, b0, nb, ign, valid, dmax):
    """the cells inside the band: used, ign <= by - bx < dmax"""
    d = np.asarray(by, np.int64) - np.asarray(bx, np.int64)
    return EC.used_of(bx, by, b0, ign, valid) & (d < int(dmax))


def cell_values(cells, b0, nb, ign, valid, w, expected, clip, dmax):
    """-> (in-band mask, min(oe, clip) of the cells inside the band); ValueError where cl_eig_build refuses the expected values"""
    bx, by, cnt = cells
    inb = band_cells(bx, by, b0, nb, ign, valid, dmax)
    e = np.asarray(expected, np.float64)
    pairs = EC.pairs_oracle(valid, ign)
    for d in range(int(ign), int(dmax)):
        if pairs[d] > 0 and not (np.isfinite(e[d]) and e[d] > 0):
            raise ValueError("expected[%d] is no finite positive number" % d)
    oe = EC.oe_oracle(np.asarray(bx)[inb], np.asarray(by)[inb], np.asarray(cnt)[inb], b0, nb, ign, valid, w, expected)
    return inb, np.minimum(oe, float(clip))


def dense_M(cells, b0, nb, ign, valid, w, expected, clip, dmax):
    """the definition: M[i][j] = min(oe, clip) - 1 on the valid pairs with ign <= |i - j| < dmax (oe = 0 without a cell), 0 elsewhere"""
    valid = np.asarray(valid, bool)
    i = np.arange(nb)
    d = np.abs(i[:, None] - i[None, :])
    band = valid[:, None] & valid[None, :] & (d >= int(ign)) & (d < int(dmax))
    M = np.where(band, -1.0, 0.0)
    inb, v = cell_values(cells, b0, nb, ign, valid, w, expected, clip, dmax)
    ix, iy = np.asarray(cells[0], np.int64)[inb] - b0, np.asarray(cells[1], np.int64)[inb] - b0
    M[ix, iy] = v - 1.0
    M[iy, ix] = v - 1.0
    return M


def band_term(valid, ign, dmax, x):
    """(B x)[i]: the sum of x over the valid j with ign <= |i - j| < dmax as differences of prefix sums -> like x ([n_vec, nb] or [nb])"""
    valid = np.asarray(valid, bool)
    nb = len(valid)
    x2 = np.atleast_2d(np.asarray(x, np.float64))
    P = np.concatenate([np.zeros((len(x2), 1)), np.cumsum(np.where(valid, x2, 0.0), axis=1)], axis=1)     # P[k] = the sum over j < k
    i = np.arange(nb)
    out = np.zeros_like(x2)
    if dmax > ign:
        at = lambda k: P[:, np.clip(k, 0, nb)]
        out = (at(i + dmax) - at(i + ign)) + (at(i - max(ign, 1) + 1) - at(i - dmax + 1))
    out = np.where(valid, out, 0.0)
    return out.reshape(np.shape(x))


def apply_sparse(cells, b0, nb, ign, valid, w, expected, clip, dmax, x):
    """M x in the sparse-plus-prefix form: S x over the cells (a diagonal cell once) minus the band term"""
    valid = np.asarray(valid, bool)
    x2 = np.atleast_2d(np.asarray(x, np.float64))
    xv = np.where(valid, x2, 0.0)
    inb, v = cell_values(cells, b0, nb, ign, valid, w, expected, clip, dmax)
    ix, iy = np.asarray(cells[0], np.int64)[inb] - b0, np.asarray(cells[1], np.int64)[inb] - b0
    off = ix != iy
    out = np.zeros_like(x2)
    for k in range(len(x2)):
        out[k] = np.bincount(ix, v * xv[k][iy], nb) + np.bincount(iy[off], v[off] * xv[k][ix[off]], nb)
    out = out - np.atleast_2d(band_term(valid, ign, dmax, x2))
    return np.where(valid, out, 0.0).reshape(np.shape(x))


def apply_bound(cells, b0, nb, ign, valid, w, expected, clip, dmax, x):
    """the absolute bound per entry between dense_M @ x and the sparse-plus-prefix form, whatever the order of their sums.  With s the
    cell values, A_i = sum_j |s_ij x_j|, X1 = the sum of |x| over the valid bins, L_i the cells of row i and N_i <= nb the entries of the
    band in row i:
      dense    every entry s - 1 carries one rounding, the product one, a dot product of N_i terms N_i - 1 more:  (N_i + 1)(A_i + X1);
      sparse   S x: L_i products and L_i - 1 additions: L_i A_i;  the band: four prefix sums of at most nb terms (nb - 1 additions
               each, of magnitude at most X1), one addition to the tile offset each, three more to combine them: (4 nb + 8) X1;
               the subtraction: A_i + X1.
    -> eps ((L_i + N_i + 2) A_i + (N_i + 4 nb + 10) X1) / (1 - (4 nb + 10) eps), like x"""
    valid = np.asarray(valid, bool)
    x2 = np.atleast_2d(np.asarray(x, np.float64))
    xa = np.where(valid, np.abs(x2), 0.0)
    inb, v = cell_values(cells, b0, nb, ign, valid, w, expected, clip, dmax)
    ix, iy = np.asarray(cells[0], np.int64)[inb] - b0, np.asarray(cells[1], np.int64)[inb] - b0
    off = ix != iy
    L = np.bincount(ix, minlength=nb) + np.bincount(iy[off], minlength=nb)
    i = np.arange(nb)
    N = np.abs(band_term(valid, ign, dmax, np.ones(nb)))
    out = np.zeros_like(x2)
    for k in range(len(x2)):
        A = np.bincount(ix, np.abs(v) * xa[k][iy], nb) + np.bincount(iy[off], np.abs(v[off]) * xa[k][ix[off]], nb)
        X1 = xa[k].sum()
        out[k] = EPS * ((L + N + 2) * A + (N + 4 * nb + 10) * X1) / (1.0 - (4 * nb + 10) * EPS)
    return out.reshape(np.shape(x))


def sign_rule(v):
    """the vector with its entry of largest magnitude positive (the lowest bin on a tie); NaN entries take no part"""
    v = np.asarray(v, np.float64)
    a = np.where(np.isnan(v), -1.0, np.abs(v))
    if len(v) == 0 or a.max() < 0:
        return v
    return -v if v[int(np.argmax(a))] < 0 else v


def eig_oracle(M, valid, n_eigs):
    """the n_eigs eigenpairs of M over the valid bins of largest |lambda|, by |lambda| descending -> (eigvals [n_eigs], vectors [n_eigs,
    nb], all eigenvalues by |lambda| descending); NaN on the invalid bins and for the pairs there are no valid bins for"""
    valid = np.asarray(valid, bool)
    nb, idx = len(valid), np.flatnonzero(valid)
    lam, vec = np.full(n_eigs, np.nan), np.full((n_eigs, nb), np.nan)
    if len(idx) == 0:
        return lam, vec, np.zeros(0)
    ev, U = np.linalg.eigh(np.asarray(M, np.float64)[np.ix_(idx, idx)])
    order = np.argsort(-np.abs(ev), kind="stable")
    for k in range(min(n_eigs, len(idx))):
        lam[k] = ev[order[k]]
        full = np.full(nb, np.nan)
        full[idx] = U[:, order[k]]
        vec[k] = sign_rule(full)
    return lam, vec, ev[order]


class OracleChrom(EC.OracleChrom):
    """the mat_*, bal_*, exp_* and eig_* methods of api.Chromosome on the oracles"""

    def __init__(self, X, Y):
        EC.OracleChrom.__init__(self, X, Y)
        self.eig = None

    def mat_cells(self, res, cut=0, fold=False):
        self.eig = None
        return EC.OracleChrom.mat_cells(self, res, cut=cut, fold=fold)

    def mat_free(self):
        self.eig = None
        EC.OracleChrom.mat_free(self)

    def bal_marginals(self, ignore_diags=2):
        self.eig = None
        return EC.OracleChrom.bal_marginals(self, ignore_diags)

    def bal_iterate(self, valid, max_iters=200, tol=1e-5):
        self.eig = None
        return EC.OracleChrom.bal_iterate(self, valid, max_iters, tol)

    def bal_free(self):
        self.eig = None
        EC.OracleChrom.bal_free(self)

    def exp_diagonals(self, valid=None, balanced=True):
        self.eig = None
        return EC.OracleChrom.exp_diagonals(self, valid, balanced)

    def exp_set(self, expected):
        self.eig = None
        EC.OracleChrom.exp_set(self, expected)

    def exp_free(self):
        self.eig = None
        EC.OracleChrom.exp_free(self)

    def eig_build(self, clip=float("inf"), dmax=None):
        ex, st = self._exp(True), self.bal
        nb, ign = st["nb"], st["ign"]
        dmax = nb if dmax is None else int(dmax)
        if not clip > 0:
            raise RuntimeError("eig_build: clip not above 0")
        if nb > 0 and not ign <= dmax <= nb:
            raise RuntimeError("eig_build: dmax outside [ign, nb]")
        try:
            M = dense_M(self.cells, st["b0"], nb, ign, ex["valid"], ex["w"], ex["expected"], clip, dmax)
        except ValueError as e:
            raise RuntimeError("eig_build: %s" % e)
        n_in = int(band_cells(self.cells[0], self.cells[1], st["b0"], nb, ign, ex["valid"], dmax).sum())
        self.eig = {"M": M, "valid": np.asarray(ex["valid"], bool), "vec": None}
        return int(np.count_nonzero(ex["valid"])), n_in

    def _eig(self, iterated=False):
        if self.eig is None or (iterated and self.eig["vec"] is None):
            raise RuntimeError("eig_* out of order")
        return self.eig

    def eig_apply(self, x):
        eg = self._eig()
        x = np.asarray(x, np.float64)
        return (eg["M"] @ np.where(eg["valid"], np.atleast_2d(x), 0.0).T).T.reshape(x.shape)

    def eig_iterate(self, n_eigs=3, max_iters=1000, tol=1e-8):
        eg = self._eig()
        if not 1 <= n_eigs <= EIG_MAX:
            raise ValueError("eig_iterate: n_eigs out of range")
        lam, vec, _ = eig_oracle(eg["M"], eg["valid"], n_eigs)
        have = min(n_eigs, int(eg["valid"].sum()))
        resid = np.full(n_eigs, np.nan)
        for k in range(have):
            v = np.where(eg["valid"], vec[k], 0.0)
            resid[k] = np.linalg.norm(eg["M"] @ v - lam[k] * v)
        eg["vec"] = vec
        if have == 0 or max_iters == 0:
            eg["vec"] = np.full_like(vec, np.nan)
            return 0, False, np.full(n_eigs, np.nan), np.full(n_eigs, np.nan)
        return 1, True, lam, resid

    def eig_vectors(self, which=0, first=0, count=None):
        eg = self._eig(True)
        nb = eg["vec"].shape[1]
        count = nb - first if count is None else count
        if not 0 <= which < len(eg["vec"]) or first < 0 or count < 0 or first + count > nb:
            raise RuntimeError("eig_vectors outside the vectors")
        return eg["vec"][which, first:first + count].copy()

    def eig_free(self):
        self.eig = None


# ---- data ------------------------------------------------------------------------------------------------------
def planted(nb, pets, block, delta, res=1000, seed=1):
    """`pets` PETs of a chromosome of nb bins of `res` bp with planted compartments: the compartment of bin i is (i // block) % 2; a
    candidate draws i uniform and d = floor(exp(u ln nb)), u uniform, and is kept when i + d lies inside the chromosome, with probability
    0.5 (1 + delta) when the two bins share a compartment and 0.5 (1 - delta) when they do not; the first `pets` kept candidates of
    4 `pets` drawn, with jitter inside the bins -> (X, Y, compartment [nb])"""
    rng = np.random.default_rng(seed)
    m = 4 * pets
    i = rng.integers(0, nb, m)
    d = np.floor(np.exp(rng.random(m) * np.log(nb))).astype(np.int64)
    comp = (np.arange(nb) // block) % 2
    j = i + d
    inside = j < nb
    same = comp[i] == comp[np.minimum(j, nb - 1)]
    keep = np.flatnonzero(inside & (rng.random(m) < 0.5 * (1.0 + np.where(same, delta, -delta))))[:pets]
    assert len(keep) == pets
    X = i[keep] * res + rng.integers(0, res, pets)
    Y = j[keep] * res + rng.integers(0, res, pets)
    return X.astype(np.int64), Y.astype(np.int64), comp


PLANTED = {"small": dict(nb=300, pets=200000, block=37, delta=0.5, seed=1), "large": dict(nb=1200, pets=1500000, block=110, delta=0.5, seed=1),
           "second": dict(nb=240, pets=150000, block=30, delta=0.5, seed=5)}            # (the second chromosome of the end-to-end test)


def stepped_rows(nb, lengths=(CELL_STEP - 1, CELL_STEP, CELL_STEP + 1, 2 * CELL_STEP - 1, 2 * CELL_STEP, 2 * CELL_STEP + 1, 1, 0), transpose=False):
    """rows at res 1 whose folded cells give bin i the cells (i, i + 1 .. i + lengths[i % len]) (cut at the last bin), 1 to 3 rows a
    cell, and one row in the last bin's diagonal cell: the runs of the cells as they lie have the steps of the block product's row
    walk minus one, exactly and plus one.  `transpose`: mirrored at the anti-diagonal, so that the runs of the transposed order have
    them -> (X, Y)"""
    X, Y = [nb - 1], [nb - 1]
    for i in range(nb):
        for j in range(i + 1, min(i + lengths[i % len(lengths)], nb - 1) + 1):
            X += [i] * (1 + (i + j) % 3)
            Y += [j] * (1 + (i + j) % 3)
    X, Y = np.array(X, np.int64), np.array(Y, np.int64)
    return (nb - 1 - Y, nb - 1 - X) if transpose else (X, Y)
_memo = {}


def planted_case(name, ign=2, clip_pct=99.9):
    """a planted case at res 1000 balanced by the oracle, with every diagonal's own average as its expected value (expected.py's
    `nosmooth`, the plain dense restatement), its dense M and spectrum, computed once and shared -> dict(X, Y, comp, cells,
    b0, nb, ign, valid, w, expected, clip, dmax, M, eigvals: all by |lambda| descending, vectors: the first EIG_MAX)"""
    key = (name, ign, clip_pct)
    if key in _memo:
        return _memo[key]
    from cloops_amd import expected
    X, Y, comp = planted(**PLANTED[name])
    ch = OracleChrom(X, Y)
    ch.mat_cells(1000, fold=True)
    b0, nb, _ = ch.bal_marginals(ign)
    s, z = ch.bal_marginals_get()
    ch.bal_iterate(BC.valid_oracle(s, z))
    w = ch.bal_weights()
    valid = ~np.isnan(w)
    ch.exp_diagonals()
    p, _, vs = ch.exp_diagonals_get()
    e, _ = expected.expected_of(p, vs, ign, nosmooth=True)
    ch.exp_set(e)
    oe = ch.exp_cells_get()
    clip = float(np.percentile(oe[~np.isnan(oe)], clip_pct))
    bad = [d for d in range(ign, nb) if p[d] > 0 and not (np.isfinite(e[d]) and e[d] > 0)]
    dmax = bad[0] if bad else nb
    M = dense_M(ch.cells, b0, nb, ign, valid, w, e, clip, dmax)
    lam, vec, ev = eig_oracle(M, valid, EIG_MAX)
    out = dict(X=X, Y=Y, comp=comp, cells=ch.cells, b0=b0, nb=nb, ign=ign, valid=valid, w=w, expected=e, clip=clip, dmax=dmax, M=M,
               eigvals=ev, vectors=vec, mask=BC.valid_oracle(s, z))
    _memo[key] = out
    return out


def gaps_of(ev):
    """per eigenvalue (by |lambda| descending) its distance to the nearest other one"""
    ev = np.asarray(ev, np.float64)
    d = np.abs(ev[:, None] - ev[None, :])
    np.fill_diagonal(d, np.inf)
    return d.min(axis=1)
