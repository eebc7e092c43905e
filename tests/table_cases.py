"""Seeded inputs for the cluster table and the candidate stage (K10) at their edges (no GPU needed).

The table {min_x, max_x, min_y, max_y, count} per id is filled by four label kernels through one helper (cl_table.h: a segmented
reduction over runs of equal labels in a wave, an LDS hash table of TAB_H = 512 slots per workgroup with 16 probes, direct global
atomics when the probes run out) and leaves the device through k_export_table; K10 classifies and appends from it.  The families:

  isolated              4096 + 37 PETs pairwise farther apart than eps, minPts 1: every PET is its own id, a workgroup sees more labels
                        than TAB_H holds (`_neg`: negative and reversed coordinates for variant 1 / block: the accumulators start at
                        INT_MAX / INT_MIN)
  isolated_pairs        the same with every PET doubled, minPts 2: the fallback on the route of minPts 2 .. 128 (every level and form)
  isolated_plus_giant   isolated PETs and one component of 3000 PETs interleaved with them in the kernels' order: LDS hits of one key
                        and fallbacks of its neighbours mix in every workgroup that holds a PET of it
  runs                  tight blobs of 2 .. 80 PETs and back, contiguous in X + Y order: runs of equal labels that start at every lane
                        and cross the row, half and wave boundaries
  many_ids              80000 isolated PETs, minPts 1: more ids than the pinned cache of the first export holds (n // 16 + 65536)
  classes_<K>           K clusters of 3 PETs of every class of pipe.py:83-97, interleaved (`classes_neg_<K>`: negative coordinates)

Every data set is a `Case`; tests/test_table_cases.py proves the stated conditions on the CPU oracle, tests/test_gpu_table.py and
tests/test_gpu_candidates.py run them on the GPU."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name X Y eps min_pts variants info")

EPS = 500
TAB_H = 512                     # cl_table.h
CAND_BLOCK = 2048               # cl_chrom.h
FINAL_CUT = 4000                # the mid-point distance of the marked boxes of `classes`
BIG_CUT = 10 ** 7               # removes every PET
ROT = ("v2", "v1", "block")
NEG = ("v1", "block")


def export_cache_rows(n):
    """rows of the pinned cache a result slot gets at its first export (finish_enqueue)"""
    return n // 16 + 65536


def _shuffled(rng, X, Y, *more):
    p = rng.permutation(len(X))
    return (np.asarray(X, np.int64)[p], np.asarray(Y, np.int64)[p]) + tuple(np.asarray(m)[p] for m in more)


def work_orders(X, Y, eps):
    """the orders of the rows in which the label kernels meet them: strip of X + Y (eps wide, counted from 0 for variant 2 and from
    the smallest X + Y for variant 1), then Y - X; X + Y alone; X alone (the cells of block follow X) -> {name: row order}"""
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    p, q = X + Y, Y - X
    return {"v2": np.lexsort((q, p // eps)), "v1": np.lexsort((q, (p - p.min()) // eps)), "p": np.argsort(p, kind="stable"),
            "x": np.argsort(X, kind="stable")}


def _isolated_xy(rng, n, x0=1000):
    """consecutive X differ by 3 .. 5 eps: any two PETs are farther apart than eps whatever their Y"""
    X = x0 + 4 * EPS * np.arange(n, dtype=np.int64) + rng.integers(0, EPS, n)
    return X, X + rng.integers(0, 50 * EPS, n)


def isolated(n=4096 + 37, name="isolated", seed=31001):
    rng = np.random.default_rng(seed)
    X, Y = _shuffled(rng, *_isolated_xy(rng, n))
    return Case(name, X, Y, EPS, 1, ROT, {})


def isolated_neg():
    """X on both sides of 0, half of the rows with Y < X"""
    rng = np.random.default_rng(31002)
    n = 4096 + 37
    X, Y = _isolated_xy(rng, n, x0=-2 * EPS * n)
    Y = np.where(rng.integers(0, 2, n) == 1, 2 * X - Y, Y)
    X, Y = _shuffled(rng, X, Y)
    return Case("isolated_neg", X, Y, EPS, 1, NEG, {})


def isolated_pairs():
    rng = np.random.default_rng(31003)
    n = 4096 + 37
    X, Y = _isolated_xy(rng, n)
    X, Y = _shuffled(rng, np.concatenate([X, X + 3]), np.concatenate([Y, Y + 5]))
    return Case("isolated_pairs", X, Y, EPS, 2, ROT, {"pairs": n})


GIANT = 3000
GIANT_PER_STRIP, ISOLATED_PER_STRIP, GIANT_PAD_STRIPS = 2, 4, 200


def isolated_plus_giant():
    """one component of 3000 PETs that lies BETWEEN isolated PETs in the order the kernels work in.  A tight blob would be 3000
    consecutive PETs there, in workgroups that hold a handful of labels; this one is a chain along the diagonal: in rotated
    coordinates p = X + Y, q = Y - X (the distance of two PETs is max(|dp|, |dq|)) two PETs of it per strip of eps in p, eps / 2
    apart, all at one q.  Every strip also holds four isolated PETs, each at a q of its own: a lattice of 4 eps, the four residues
    of the strip number mod 4 apart, so that two isolated PETs differ by 4 eps in q or by more than 3 eps in p (isolated under the
    weighted metric of the tests as well).  200 strips of isolated PETs alone lie in front of the chain and behind it."""
    rng = np.random.default_rng(31004)
    nstrips = GIANT // GIANT_PER_STRIP + 2 * GIANT_PAD_STRIPS
    p0, qg = 200 * EPS, 4 * EPS
    P, Q = [], []
    for s in range(nstrips):
        base = p0 + s * EPS
        for j in range(ISOLATED_PER_STRIP):
            P.append(base + 2 * int(rng.integers(0, EPS // 2)))
            Q.append(qg + 4 * EPS * (1 + 4 * j + s % 4))
    niso = len(P)
    for k in range(GIANT):                                               # p: eps / 4 and 3 eps / 4 into the strip; q: a few bp around qg
        s = GIANT_PAD_STRIPS + k // GIANT_PER_STRIP
        P.append(p0 + s * EPS + (EPS // 4 if k % 2 == 0 else 3 * EPS // 4) + 2 * int(rng.integers(-5, 6)))
        Q.append(qg + 2 * int(rng.integers(-5, 6)))
    P, Q = np.asarray(P, np.int64), np.asarray(Q, np.int64)              # both even: X and Y are integers
    member = np.arange(len(P)) >= niso
    X, Y, member = _shuffled(rng, (P - Q) // 2, (P + Q) // 2, member)
    return Case("isolated_plus_giant", X, Y, EPS, 1, ROT, {"giant": GIANT, "member": member})


RUN_SIZES = tuple(range(2, 81)) + tuple(range(80, 1, -1))


def runs():
    """blob k: RUN_SIZES[k] PETs around (c_k, c_k + 20 eps), c_k = 5000 + 10 eps k, jitter of at most eps / 8 per coordinate: any two
    PETs of a blob are within eps / 2 of each other, two blobs are 20 eps apart.  info["blob"]: the blob of every row"""
    rng = np.random.default_rng(31005)
    xs, ys, bl = [], [], []
    for k, m in enumerate(RUN_SIZES):
        c = 5000 + 10 * EPS * k
        xs.append(c + rng.integers(-EPS // 8, EPS // 8 + 1, m))
        ys.append(c + 20 * EPS + rng.integers(-EPS // 8, EPS // 8 + 1, m))
        bl.append(np.full(m, k))
    X, Y, blob = _shuffled(rng, np.concatenate(xs), np.concatenate(ys), np.concatenate(bl))
    return Case("runs", X, Y, EPS, 2, ROT, {"blob": blob, "sizes": RUN_SIZES})


def many_ids():
    c = isolated(80000, "many_ids", 31006)
    assert len(c.X) > export_cache_rows(len(c.X))
    return c


# ---- classes: the rules of pipe.py:83-97 and of the final cut (pipe.py:130-143) ----------------------------------------------
#: the cycle of blob kinds along the chromosome; "noise" is a blob of two PETs (no cluster at minPts 3)
KINDS = ("inter", "touch", "overlap", "degx", "mark_at", "degy", "noise", "mark_below")
#: what K10 makes of each kind: 0 = inter-ligation (appended), 1 = self-ligation, -1 = dropped
KIND_CLASS = {"inter": 0, "touch": 1, "overlap": 1, "degx": -1, "degy": -1, "mark_at": 0, "mark_below": 0}


def _blob_points(kind, c, a, b, D):
    """the PETs (x, y) of one blob at c; 1 <= a, b <= 20, D = the distance of the inter-ligation kinds"""
    F = FINAL_CUT
    if kind == "inter":
        return [(c, c + D + b), (c + a, c + D), (c + a + b, c + D + a + b)]
    if kind == "touch":                                    # max_x == min_y: self-ligation (pipe.py:97 is a strict <)
        w = 10 + a
        return [(c, c + w), (c + w // 2, c + w + 3), (c + w, c + w + 9)]
    if kind == "overlap":                                  # max_x > min_y
        return [(c, c + 4), (c + 6, c + 9 + a), (c + 3, c + 8)]
    if kind == "degx":                                     # min_x == max_x (pipe.py:83-85)
        return [(c, c + D), (c, c + D + 3), (c, c + D + 7 + a)]
    if kind == "degy":                                     # min_y == max_y
        return [(c, c + D), (c + 3, c + D), (c + 7 + a, c + D)]
    if kind == "mark_at":                                  # min_x + max_x odd, min_y + max_y even, mid-point distance F
        return [(c, c + F - 1), (c + 1, c + F + 1), (c, c + F)]
    if kind == "mark_below":                               # ... F - 1
        return [(c, c + F - 2), (c + 1, c + F), (c, c + F - 1)]
    if kind == "noise":
        return [(c, c + D), (c + 5, c + D + 5)]
    raise ValueError(kind)


def classes(total, negative=False):
    """`total` clusters of 3 PETs at minPts 3, one blob every 10 eps, kinds in the cycle KINDS.  info: "kind" (of every row),
    "counts" (clusters per kind)"""
    rng = np.random.default_rng(31100 + total + (7 if negative else 0))
    pts, kinds, counts = [], [], collections.Counter()
    i = made = 0
    while made < total:
        kind = KINDS[i % len(KINDS)]
        a, b = (int(v) for v in rng.integers(1, 21, 2))
        D = 3000 + int(rng.integers(0, 3000))
        p = _blob_points(kind, 10000 + 10 * EPS * i, a, b, D)
        pts += p
        kinds += [kind] * len(p)
        if kind != "noise":
            made += 1
            counts[kind] += 1
        i += 1
    P = np.asarray(pts, np.int64)
    if negative:
        P = P - (int(P.max()) + 10001)                     # (odd or even: both sums change sign, their parities stay)
    X, Y, kind = _shuffled(rng, P[:, 0], P[:, 1], np.asarray(kinds))
    name = "classes_%s%d" % ("neg_" if negative else "", total)
    return Case(name, X, Y, EPS, 3, NEG if negative else ROT, {"kind": kind, "counts": dict(counts), "total": total})


CLASS_TOTALS = (2047, 2048, 2049, 4097)
#: the sweep of tests/test_gpu_candidates.py: (eps, minPts, cut) per step.  The second step's cut removes every PET, the third makes
#: clusters of the two-PET blobs as well: every box of the first step comes back in it
SWEEP_STEPS = ((EPS, 3, 0), (EPS, 3, BIG_CUT), (EPS, 2, 0))

MAKERS = {"isolated": isolated, "isolated_neg": isolated_neg, "isolated_pairs": isolated_pairs, "isolated_plus_giant": isolated_plus_giant,
          "runs": runs, "many_ids": many_ids}
for _t in CLASS_TOTALS:
    MAKERS["classes_%d" % _t] = (lambda t=_t: classes(t))
MAKERS["classes_neg_2049"] = lambda: classes(2049, True)

#: the families of tests/test_gpu_table.py (many_ids has tests of its own there; one size of `classes` is enough for the producers)
TABLE_FAMILIES = ("isolated", "isolated_neg", "isolated_pairs", "isolated_plus_giant", "runs", "classes_2049", "classes_neg_2049")
CLASS_NAMES = tuple("classes_%d" % t for t in CLASS_TOTALS) + ("classes_neg_2049",)
_made = {}


def get(name):
    """the data set `name`, made once per process"""
    if name not in _made:
        _made[name] = MAKERS[name]()
    return _made[name]


def weighted_eps(wx, wy):
    """the eps of the weighted runs on these sets: under wx |dX| + wy |dY| <= max(wx, wy) eps every pair within eps stays a pair"""
    return EPS * max(wx, wy)
