"""Developer tool (numpy and scipy, no GPU): the share of the cores that k_union_c's domination test lets search, on one chromosome
of the bench genome, and a check that the survivors find the same (chain, chain) pairs as all cores.

Rotated coordinates p = X + Y, q = Y - X (neighbours: |dp| <= eps and |dq| <= eps); strips of eps in p from 0 (variant 2); the
cores of a strip in the order of (q, p): the core array of k_lists.hip.  A core is DOMINATED when a core in front of it AND a core
behind it in that array -- same strip, within eps in q -- have a smaller key (p, index).  The kernel looks at the K nearest cores on
either side only; a side without a dominator among them counts as not dominated.

    python tools/union_filter_model.py [--chrom 20] [--n-total 2e8] [--pairs]

--pairs also walks every core's window one strip below (slow: a Python loop per strip) and asserts the equality of the pair sets.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETTINGS = ((5000, 0, 50), (5000, 0, 20), (5000, 5000, 50), (5000, 5000, 20), (10000, 5500, 50), (10000, 5500, 20))
KS = (4, 8, 16)


def core_array(X, Y, eps, min_pts, cut):
    """-> (q, p, strip) of the cores of a run in the order of the core array: PETs with Y - X >= cut (cut 0: all), core = at least
    min_pts PETs of the run within eps in p and in q (itself included)"""
    from scipy.spatial import cKDTree
    X = np.asarray(X, np.int64)
    Y = np.asarray(Y, np.int64)
    keep = (Y - X) >= cut if cut > 0 else np.ones(len(X), bool)
    p, q = (X + Y)[keep], (Y - X)[keep]
    pts = np.stack([p, q], 1).astype(np.float64)
    cnt = cKDTree(pts).query_ball_point(pts, eps, p=np.inf, return_length=True, workers=-1)
    core = cnt >= min_pts
    p, q = p[core], q[core]
    strip = p // eps
    order = np.lexsort((p, q, strip))
    return q[order], p[order], strip[order]


def survivors(q, p, strip, eps, K):
    """the cores that are not dominated within K neighbours on both sides -> bool[n].  The arrays are in core-array order."""
    n = len(q)
    dl = np.zeros(n, bool)
    dr = np.zeros(n, bool)
    for d in range(1, K + 1):
        if d >= n:
            break
        a, b = slice(d, n), slice(0, n - d)              # a: the core, b: the one d in front of it
        near = (strip[a] == strip[b]) & (q[a] - q[b] <= eps)
        dl[a] |= near & (p[b] <= p[a])                   # in front: an equal p loses to the smaller index
        dr[b] |= near & (p[a] < p[b])                    # behind: it does not
    return ~(dl & dr)


def chains(q, strip, eps):
    """chain id per core: a core opens a chain when its predecessor is of another strip or more than eps in front of it in q"""
    n = len(q)
    if n == 0:
        return np.zeros(0, np.int64)
    opens = np.ones(n, bool)
    opens[1:] = (strip[1:] != strip[:-1]) | (q[1:] - q[:-1] > eps)
    return np.cumsum(opens) - 1


def pair_set(q, p, strip, eps, who):
    """the set of (chain, chain of the strip below) pairs the cores `who` (bool[n]) find: b is a neighbour of a one strip below iff
    |q_b - q_a| <= eps and p_b >= p_a - eps"""
    ch = chains(q, strip, eps)
    starts = {}
    us, first = np.unique(strip, return_index=True)
    ends = np.append(first[1:], len(q))
    for s, f, e in zip(us, first, ends):
        starts[int(s)] = (int(f), int(e))
    out = set()
    for a in np.flatnonzero(who):
        lo_hi = starts.get(int(strip[a]) - 1)
        if lo_hi is None:
            continue
        f, e = lo_hi
        j0 = f + np.searchsorted(q[f:e], q[a] - eps, "left")
        j1 = f + np.searchsorted(q[f:e], q[a] + eps, "right")
        hit = np.flatnonzero(p[j0:j1] >= p[a] - eps)
        for b in np.unique(ch[j0 + hit]):
            out.add((int(ch[a]), int(b)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chrom", type=int, default=20, help="index into the hg38 list (20 = chr21)")
    ap.add_argument("--n-total", type=float, default=2e8)
    ap.add_argument("--pairs", action="store_true")
    a = ap.parse_args()
    from cloops_amd.synth import synth_chrom, chrom_sizes
    name, length, n = chrom_sizes(int(a.n_total))[a.chrom]
    X, Y = synth_chrom(n, length, 3000 + a.chrom)
    print("%s: %d PETs" % (name, n))
    print("| eps | cut | minPts | cores | " + " | ".join("K = %d" % k for k in KS) + " |")
    for eps, cut, m in SETTINGS:
        q, p, strip = core_array(X, Y, eps, m, cut)
        shares = []
        for K in KS:
            sv = survivors(q, p, strip, eps, K)
            shares.append(sv.mean() if len(sv) else 0.0)
            if a.pairs:
                assert pair_set(q, p, strip, eps, sv) == pair_set(q, p, strip, eps, np.ones(len(q), bool)), (eps, cut, m, K)
        print("| %d | %d | %d | %.2f M | " % (eps, cut, m, len(q) / 1e6) + " | ".join("%.2f" % s for s in shares) + " |", flush=True)


if __name__ == "__main__":
    main()
