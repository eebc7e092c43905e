"""The numpy oracle of kernel K22, written from the definitions of include/cloops_hip.h (cl_dom_tracks) -- it does not call
cloops_amd.domains --: the three tracks in the brute-force form (the definition itself, one comparison per row and bin) and in the
range form (what the kernel does), the domain counts, a host stand-in for the domains_* methods of api.Chromosome that answers from
the oracle, and a seeded genome with planted domains.  Shared by tests/test_domains_host.py and tests/test_gpu_domains.py."""
import numpy as np

EMPTY = np.zeros(0, np.int64)


def kept_rows(X, Y, cut=0):
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    if cut > 0:
        keep = (Y - X) >= cut
        X, Y = X[keep], Y[keep]
    return X, Y


def bins_of(X, Y, res):
    """-> (bx, by, bmin, n_bins) of kept rows (numpy's // floors, also below zero)"""
    bx, by = X // res, Y // res
    bmin = int(min(bx.min(), by.min()))
    bmax = int(max(bx.max(), by.max()))
    return bx, by, bmin, bmax - bmin + 2


def tracks_oracle(X, Y, cut, res, w, form="range"):
    """-> (cross, up, down int64 over b = bmin .. bmax + 1, n_bins, bmin, n_kept); without kept rows: empty tracks and (0, 0, 0)"""
    X, Y = kept_rows(X, Y, cut)
    if len(X) == 0:
        return EMPTY, EMPTY, EMPTY, 0, 0, 0
    bx, by, bmin, nb = bins_of(X, Y, res)
    if form == "brute":
        cross, up, down = (np.zeros(nb, np.int64) for _ in range(3))
        for k in range(nb):
            b = bmin + k
            cross[k] = np.count_nonzero((b - w <= bx) & (bx < b) & (b <= by) & (by < b + w))
            up[k] = np.count_nonzero((b - w <= bx) & (bx <= by) & (by < b))
            down[k] = np.count_nonzero((b <= bx) & (bx <= by) & (by < b + w))
        return cross, up, down, nb, bmin, len(X)
    assert form == "range"
    fwd = bx <= by
    bx, by = bx[fwd], by[fwd]
    out = []
    for lo, hi in ((np.maximum(bx + 1, by - w + 1), np.minimum(bx + w, by)), (by + 1, bx + w), (by - w + 1, bx)):
        lo, hi = np.maximum(lo, bmin), np.minimum(hi, bmin + nb - 1)         # entries exist for bmin .. bmax + 1 only
        ok = lo <= hi
        d = np.zeros(nb + 1, np.int64)
        np.add.at(d, lo[ok] - bmin, 1)
        np.add.at(d, hi[ok] + 1 - bmin, -1)
        out.append(np.cumsum(d)[:nb])
    return out[0], out[1], out[2], nb, bmin, len(X)


def count_oracle(X, Y, cut, starts, ends):
    """-> (intra, nx, ny) int64 per interval [starts[k], ends[k]): one comparison per row and interval, or, beyond a few thousand
    intervals, searches in the sorted coordinates (ascending disjoint intervals only)"""
    X, Y = kept_rows(X, Y, cut)
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    if len(s) * max(1, len(X)) <= 5 * 10 ** 7:
        inx = (X[None, :] >= s[:, None]) & (X[None, :] < e[:, None])
        iny = (Y[None, :] >= s[:, None]) & (Y[None, :] < e[:, None])
        return (inx & iny).sum(1).astype(np.int64), inx.sum(1).astype(np.int64), iny.sum(1).astype(np.int64)
    SX, SY = np.sort(X), np.sort(Y)
    nx = np.maximum(0, np.searchsorted(SX, e, "left") - np.searchsorted(SX, s, "left"))
    ny = np.maximum(0, np.searchsorted(SY, e, "left") - np.searchsorted(SY, s, "left"))
    # both ends inside, for ascending disjoint intervals: only the last interval that starts at or below a row's X can hold the row
    # (of equal starts, the empty intervals come first), so one pass over the rows settles it
    assert np.all(e >= s) and np.all(s[1:] >= e[:-1])
    k = np.searchsorted(s, X, "right") - 1
    kk = np.maximum(k, 0)
    ok = (k >= 0) & (X < e[kk]) & (Y >= s[kk]) & (Y < e[kk])
    intra = np.zeros(len(s), np.int64)
    np.add.at(intra, kk[ok], 1)
    return intra, nx.astype(np.int64), ny.astype(np.int64)


class OracleChrom:
    """the domains_* methods of api.Chromosome answered by the oracle"""

    def __init__(self, X, Y):
        self.X, self.Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
        self.cut = None
        self.last = None
        self.calls = []

    def domains_tracks(self, cut=0, res=10000, w=10):
        self.cut = cut
        self.last = tracks_oracle(self.X, self.Y, cut, res, w)
        self.calls.append(("tracks", cut, res, w))
        return self.last[3], self.last[4], self.last[5]

    def domains_get(self, first=0, count=None):
        sl = slice(first, None if count is None else first + count)
        return tuple(a[sl].astype(np.uint32) for a in self.last[:3])

    def domains_count(self, starts, ends):
        self.calls.append(("count", len(starts)))
        return tuple(a.astype(np.uint32) for a in count_oracle(self.X, self.Y, self.cut, starts, ends))

    def domains_free(self):
        self.calls.append(("free",))
        self.last = None


PLANT_RES = 10000


def planted_genome(seed, blocks=12, per_bin=300, background=0.15, res=PLANT_RES):
    """`blocks` blocks of 15-59 bins of `res` bp laid end to end from position 0, `per_bin` PETs per bin with both ends uniform inside
    their block, plus `background` times as many rows with X uniform over the genome and Y - X uniform below 40 res (kept inside the
    genome), the rows shuffled -> (X, Y int64, the blocks' first bins, the bin behind the last block)"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(15, 60, blocks)
    first = np.concatenate([[0], np.cumsum(sizes)])
    xs, ys = [], []
    for a, n in zip(first[:-1], sizes):
        p = rng.integers(int(a) * res, int(a + n) * res, (int(n) * per_bin, 2))
        xs.append(p.min(1))
        ys.append(p.max(1))
    n_in = sum(len(x) for x in xs)
    G = int(first[-1]) * res
    d = rng.integers(0, 40 * res, int(n_in * background))
    bx = (rng.random(len(d)) * (G - d)).astype(np.int64)
    xs.append(bx)
    ys.append(bx + d)
    X, Y = np.concatenate(xs).astype(np.int64), np.concatenate(ys).astype(np.int64)
    o = rng.permutation(len(X))
    return X[o], Y[o], first[:-1].astype(np.int64), int(first[-1])
