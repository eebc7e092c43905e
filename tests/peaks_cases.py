"""The numpy oracle of kernel K21, written from the definitions of include/cloops_hip.h (cl_peak_sort) -- it does not call
cloops_amd.peaks --, a plain sequential DBSCAN in one dimension to hold it against, and a host stand-in for the peaks_* methods of
api.Chromosome that answers from the oracle.  Shared by tests/test_peaks_host.py and tests/test_gpu_peaks.py."""
from collections import deque

import numpy as np

EMPTY = np.zeros(0, np.int64)


def ends_of(X, Y, cut=0, ends=3):
    """S: the ascending multiset of the kept end points"""
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    if cut > 0:
        keep = (Y - X) >= cut
        X, Y = X[keep], Y[keep]
    return np.sort(np.concatenate(([X] if ends & 1 else []) + ([Y] if ends & 2 else []) + [EMPTY]))


def peaks_oracle(S, eps, minPts):
    """the closed form -> (start, end, n_points, n_cores) int64 per peak, and the number of cores"""
    lb = lambda x: np.searchsorted(S, x, "left")
    ub = lambda x: np.searchsorted(S, x, "right")
    n = ub(S + eps) - lb(S - eps)
    core = n >= minPts
    cp = S[core]
    if len(cp) == 0:
        return EMPTY, EMPTY, EMPTY, EMPTY, 0
    head = np.ones(len(cp), bool)
    head[1:] = (cp[1:] - cp[:-1]) > eps
    first = np.flatnonzero(head)
    last = np.append(first[1:] - 1, len(cp) - 1)
    a, b = cp[first], cp[last]
    left = a - eps
    left[1:] = np.maximum(left[1:], b[:-1] + eps + 1)
    i0, i1 = lb(left), ub(b + eps)
    return S[i0], S[i1 - 1] + 1, (i1 - i0).astype(np.int64), (last - first + 1).astype(np.int64), int(core.sum())


def sequential_dbscan(S, eps, minPts):
    """DBSCAN as it is written down, over the points of S in ascending order with a queue -> the clusters in the order they were
    opened as (start, end, n_points, n_cores) lists"""
    S = [int(v) for v in S]
    m = len(S)
    UNSEEN, NOISE = -2, -1
    label = [UNSEEN] * m

    def region(i):
        return [j for j in range(m) if abs(S[j] - S[i]) <= eps]

    cores = []
    k = 0
    for i in range(m):
        if label[i] != UNSEEN:
            continue
        nb = region(i)
        if len(nb) < minPts:
            label[i] = NOISE
            continue
        label[i] = k
        cores.append(1)
        queue = deque(nb)
        while queue:
            j = queue.popleft()
            if label[j] == NOISE:
                label[j] = k                                   # a border point: reached, not expanded
            if label[j] != UNSEEN:
                continue
            label[j] = k
            nj = region(j)
            if len(nj) >= minPts:
                cores[k] += 1
                queue.extend(nj)
        k += 1
    out = ([], [], [], [])
    for c in range(k):
        idx = [i for i in range(m) if label[i] == c]
        out[0].append(S[idx[0]])
        out[1].append(S[idx[-1]] + 1)
        out[2].append(len(idx))
        out[3].append(cores[c])
        assert idx == list(range(idx[0], idx[-1] + 1))          # a contiguous index range
    return out


def count_oracle(S, starts, ends):
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    return np.maximum(0, np.searchsorted(S, e, "left") - np.searchsorted(S, s, "left"))


def summit_oracle_loop(S, starts, ends, w):
    """-> (pos, cnt) int64: the member point with the largest n_w, the smallest position on ties; (-1, 0) without points"""
    nw = np.searchsorted(S, S + w, "right") - np.searchsorted(S, S - w, "left")
    pos, cnt = [], []
    for s, e in zip(np.asarray(starts, np.int64), np.asarray(ends, np.int64)):
        i0, i1 = np.searchsorted(S, s, "left"), np.searchsorted(S, e, "left")
        if i1 <= i0:
            pos.append(-1)
            cnt.append(0)
        else:
            j = i0 + int(np.argmax(nw[i0:i1]))                 # the first of the largest: S ascends
            pos.append(int(S[j]))
            cnt.append(int(nw[j]))
    return np.array(pos, np.int64), np.array(cnt, np.int64)


def summit_oracle(S, starts, ends, w):
    """the same for ascending, disjoint intervals without a loop (10^5 intervals): the largest of n_w (m + 1) + (m - index) over the
    index range of every interval gives the largest n_w and, among those, the smallest index"""
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    m = len(S)
    if len(s) == 0 or m == 0:
        return np.full(len(s), -1, np.int64), np.zeros(len(s), np.int64)
    assert np.all(e >= s) and np.all(s[1:] >= e[:-1])
    nw = np.searchsorted(S, S + w, "right") - np.searchsorted(S, S - w, "left")
    key = np.append(nw.astype(np.int64) * (m + 1) + (m - np.arange(m, dtype=np.int64)), 0)     # (one more: an index range may begin at m)
    i0, i1 = np.searchsorted(S, s, "left"), np.searchsorted(S, e, "left")
    top = np.maximum.reduceat(key, np.stack([i0, i1], 1).ravel())[0::2]
    idx = np.minimum(m - top % (m + 1), m - 1)
    has = i1 > i0
    return np.where(has, S[idx], -1).astype(np.int64), np.where(has, top // (m + 1), 0).astype(np.int64)


class OracleChrom:
    """the peaks_* methods of api.Chromosome answered by the oracle"""

    def __init__(self, X, Y):
        self.X, self.Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
        self.S = None
        self.last = None
        self.calls = []

    def peaks_sort(self, cut=0, ends=3):
        self.S = ends_of(self.X, self.Y, cut, ends)
        self.last = None
        self.calls.append("sort")
        return (len(self.S), int(self.S[0]), int(self.S[-1])) if len(self.S) else (0, 0, 0)

    def peaks_call(self, eps, minPts):
        r = peaks_oracle(self.S, eps, minPts)
        self.last = r
        self.calls.append("call")
        return len(r[0]), r[4], int(r[2].sum())

    def peaks_get(self, first=0, count=None):
        s, e, p, c = self.last[:4]
        sl = slice(first, None if count is None else first + count)
        return s[sl].astype(np.int32), e[sl].astype(np.int32), p[sl].astype(np.uint32), c[sl].astype(np.uint32)

    def peaks_count(self, starts, ends):
        self.calls.append("count")
        return count_oracle(self.S, starts, ends).astype(np.uint32)

    def peaks_summits(self, starts, ends, w):
        self.calls.append("summits")
        pos, cnt = summit_oracle(self.S, starts, ends, w)
        return pos.astype(np.int32), cnt.astype(np.uint32)

    def peaks_free(self):
        self.calls.append("free")
        self.S = None


def seeded_genome(seed=21, sizes=(("chr2", 6000), ("chr10", 4000), ("chrX", 800))):
    """a small genome with pile-ups: {name: (X, Y)}; half of the PETs fall into a few hundred sites"""
    rng = np.random.default_rng(seed)
    out = {}
    for name, n in sizes:
        sites = rng.integers(10000, 2000000, max(4, n // 40))
        X = np.where(rng.random(n) < 0.5, sites[rng.integers(0, len(sites), n)] + rng.integers(-60, 61, n), rng.integers(0, 2000000, n))
        Y = X + rng.integers(0, 30000, n)
        out[name] = (X.astype(np.int64), Y.astype(np.int64))
    return out
