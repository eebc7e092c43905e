"""Seeded inputs for blockDBSCAN's cell kernels (K6, cloops_amd/csrc/k_block.hip) at their grid, link and rank edges (no GPU needed).

Every data set is built in CELL coordinates of the grid it will get: a PET at the minimum of both coordinates (the "anchor", alone in
cell (0, 0), noise in every run) pins the origin, every other PET is placed at a chosen offset inside a chosen cell.  Sub-cases of one
set lie at least 4 cells apart unless the family says otherwise.  The families:

  cell_edge_<eps>     pairs of PETs one base pair on either side of a cell boundary, at cell multiples 1, 2, one in the middle and the
                      largest that fits, once along X and once along Y, minPts 2.  TOGETHER: the first and the last base pair of one
                      cell, 2 eps - 2 apart: a cluster only because they share the cell.  SPLIT: the same pair one base pair lower
                      along the tested axis: two cells, centroids farther apart than eps: noise.  eps 1 and 2 have no room for
                      that: duplicates and a step of (eps, 1) stand in, which check the division but not an off-by-one boundary.
                      For eps >= 1024 the set spans the whole domain, -(2^29 - 1) .. 2^29 - 1: the offsets divided reach 2^30 - 2;
                      for smaller eps the extent is 2^20 cells.  Around eps = 2^28 the domain is three or four cells wide: one tiny
                      set per sub-case (`cell_edge_<eps>_<axis><k><t|s>`)
  row_wrap_<nyb>      the Y extent is exactly 2^nyb cells; (r, 2^nyb - 1) and (r + 1, 0), consecutive sort keys, hold two PETs
                      each, in both row orders.  nyb 1: the two cells are diagonal neighbours as well, the four PETs sit around the
                      shared corner: noise at minPts 5 (4 PETs), one cluster at 4 -- counted twice they would be core at 5.
                      nyb 2, 3: the cells are far apart, no label can depend on the false neighbour (controls)
  centroid_tie        two adjacent cells of (1,1), (1,2), (2,3), (3,3), (3,7) PETs whose centroids are exactly eps apart, and
                      eps + 1 / lcm apart (1, 1/2, 1/6, 1/3, 1/21), minPts = the sum: a cluster iff linked.  No pair of PETs is within
                      eps (found by a seeded search over the spread across the axis); (1,1) admits no such arrangement: its centroids
                      ARE the pair.  One copy at each end of the domain, side by side at the low end, one above the other at the high
  pair_loop           two adjacent cells of (na, nb) PETs, {1..9}^2 and (1,64), (65,3), (130,129), in the four forward directions;
                      centroids farther apart than eps ((1,1) excepted), ONE pair of PETs exactly eps apart, every other pair far
                      apart; the two PETs of that pair cycle through the row order of their cells.  A twin of each with the pair
                      at eps + 1.  minPts = na + nb
  core_threshold      a cell of 4 PETs and its eight neighbours of 2 .. 9 PETs (direction q holds q + 2), the neighbours linked to
                      the centre and not to each other; in variant v the neighbour in direction v is out of reach:
                      psum = 48 - (v + 2), run at psum (centre core, one cluster without that neighbour) and psum + 1 (noise)
  border_rank         a non-core cell of one PET linked to one core cell of two, and of three, components that touch nowhere else
                      (`bridge`: they stay apart); each component is a core cell of 1 PET and a core cell of 5 behind it, minPts 6.
                      Row permutations make each component in turn the last one (the border PET takes the largest rank) and put the
                      border PET on row 0
  components          one PET per cell at offset (0, 0): orthogonal neighbours exactly eps apart, diagonal ones 2 eps, minPts 2.
                      Columns (consecutive in cell order) of 1 .. 8, 63, 64, 65, 200 cells; 256 columns of 4 back to back from a
                      cell index that is a multiple of 1024; rows of 2, 3, 5, 70 cells (far apart in cell order); a serpentine of
                      3130 cells.  Row permutations: cell order, reversed, shuffled
  cut_anchor          the PETs that hold the smallest X (row 0) and the smallest Y (last row) fall to every cut; the survivors'
                      minimum lies 37 / 6063 base pairs from them, at the next cut 41 / 14047 further; pairs that share a cell on
                      one grid and not on the other.  The largest cut leaves one PET

No family aims at the rule that deletes a cell whose 9-cell population is below minPts when all its neighbours are like that
(k_blk_alive): such a cell and all its neighbours have fewer than minPts PETs within reach, none of them can be core, so no label
depends on the deletion.

Every data set is a `Case`: name, X, Y, eps, runs ((minPts, cut) pairs), info.  info["sub"] numbers the sub-case of every row (-1:
anchors and padding), info["subs"][k]["expect"] maps a run's minPts to "one" (the rows of k are one cluster) or "noise";
info["perms"] lists named row permutations.  tests/test_block_cases.py proves the stated conditions on three CPU implementations,
tests/test_gpu_block.py runs the sets on the GPU."""
import collections
import math

import numpy as np

Case = collections.namedtuple("Case", "name X Y eps runs info")

LIM = 1 << 29                   # |X|, |Y| < LIM (include/cloops_hip.h)
LO = -(LIM - 1)
EPS = 1000
WG = 1024                       # cells per workgroup of k_blk_flatten (BIGTPB)
#: (dx, dy) of direction q in k_blk_neighbors; the reverse of q is 7 - q; a thread of k_blk_links has q = 4 .. 7
DIRS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


class _Set:
    """the PETs of one data set as offsets (ux, uy) >= 0 from the grid's origin (x0, y0)"""

    def __init__(self, eps, x0=0, y0=0, anchor=True):
        self.eps, self.x0, self.y0 = eps, x0, y0
        self.ux, self.uy, self.sub, self.subs = [], [], [], []
        if anchor:
            self.add(0, 0)

    def new_sub(self, **kw):
        self.subs.append(dict(kw))
        return len(self.subs) - 1

    def add(self, ux, uy, sub=-1, times=1):
        assert ux >= 0 and uy >= 0
        for _ in range(times):
            self.ux.append(int(ux))
            self.uy.append(int(uy))
            self.sub.append(sub)

    def cell(self, cx, cy, ox=0, oy=0, sub=-1, times=1):
        assert 0 <= ox < self.eps and 0 <= oy < self.eps and cx >= 0 and cy >= 0
        self.add(cx * self.eps + ox, cy * self.eps + oy, sub, times)

    def case(self, name, runs, order=None, **info):
        X = self.x0 + np.asarray(self.ux, np.int64)
        Y = self.y0 + np.asarray(self.uy, np.int64)
        sub = np.asarray(self.sub, np.int64)
        assert X.min() == self.x0 and Y.min() == self.y0 and max(abs(X).max(), abs(Y).max()) < LIM
        if order is not None:
            X, Y, sub = X[order], Y[order], sub[order]
        info.update(sub=sub, subs=self.subs)
        return Case(name, X, Y, self.eps, tuple(runs), info)


def _order_keeping_groups(rng, group):
    """a random row order that keeps the relative order of the rows of one group (a cell): the order inside a cell is the row order"""
    n = len(group)
    slot = rng.permutation(n)                                # the row every PET would get
    out = np.empty(n, np.int64)
    by_group = np.lexsort((np.arange(n), group))             # PETs by group, in construction order
    by_slot = np.lexsort((slot, group))                      # the rows of each group, ascending
    out[slot[by_slot]] = by_group
    return out                                               # out[row] = PET


# ---- cell_edge ------------------------------------------------------------------------------------------------------------------
CELL_EDGE_EPS = (1, 2, 3, 7) + tuple((1 << k) + d for k in (4, 10, 16, 20, 28) for d in (-1, 0, 1))
CELL_EDGE_ALONE = 200            # fewer cells than this across the domain: one set per sub-case


def cell_edge_span(eps):
    return min(2 * LIM - 2, eps << 20)


def cell_edge_kmax(eps):
    """the largest cell whose last base pair lies inside the span"""
    return (cell_edge_span(eps) + 1) // eps - 1


def _edge_pair(s, eps, axis, k, other, together, sub):
    """the pair of cell k along `axis` (0: X); `other`: the offset along the other axis, a cell's first base pair"""
    a = k * eps
    if eps >= 3:
        pts = [(a, other), (a + eps - 1, other + eps - 1)] if together else [(a - 1, other), (a + eps - 2, other + eps - 1)]
    else:
        pts = [(a + eps - 1, other + eps - 1)] * 2 if together else [(a - 1, other), (a + eps - 1, other + 1)]
    for t, o in pts:
        s.add(*((t, o) if axis == 0 else (o, t)), sub=sub)


def _cell_edge_ks(eps):
    kmax = cell_edge_kmax(eps)
    return sorted({1, 2, max(kmax // 2, 1), kmax})


def cell_edge(eps):
    assert cell_edge_kmax(eps) >= CELL_EDGE_ALONE
    s = _Set(eps, LO, LO)
    lane = 0
    for axis in (0, 1):
        for k in _cell_edge_ks(eps):
            for together in (True, False):
                lane += 1                                    # lanes 6 cells apart, far below the middle k
                sub = s.new_sub(kind="together" if together else "split", axis=axis, k=k, expect={2: "one" if together else "noise"})
                _edge_pair(s, eps, axis, k, 6 * lane * eps, together, sub)
    assert 6 * lane + 2 < cell_edge_kmax(eps) // 2 - 2
    return s.case("cell_edge_%d" % eps, [(2, 0)], whole_domain=cell_edge_span(eps) == 2 * LIM - 2)


def cell_edge_alone(eps, axis, k, together):
    """three PETs: the pair in cell k of the tested axis and cell 0 of the other, the anchor of the tested axis three cells up the other"""
    s = _Set(eps, LO, LO, anchor=False)
    s.add(*((0, 3 * eps) if axis == 0 else (3 * eps, 0)))
    sub = s.new_sub(kind="together" if together else "split", axis=axis, k=k, expect={2: "one" if together else "noise"})
    _edge_pair(s, eps, axis, k, 0, together, sub)
    return s.case("cell_edge_%d_%s%d%s" % (eps, "xy"[axis], k, "t" if together else "s"), [(2, 0)], whole_domain=True)


# ---- row_wrap -------------------------------------------------------------------------------------------------------------------
def row_wrap(nyb):
    s = _Set(EPS)
    top = (1 << nyb) - 1
    for r, first in ((10, "top"), (30, "bottom")):
        hi = [((r + 1) * EPS - 1, top * EPS), ((r + 1) * EPS - 2, top * EPS + 1)]          # cell (r, top), at its lower right corner
        lo = [((r + 1) * EPS, EPS - 1), ((r + 1) * EPS + 1, EPS - 2)]                      # cell (r + 1, 0), at its upper left corner
        if nyb == 1:
            subs = [s.new_sub(kind="corner", first=first, expect={5: "noise", 4: "one", 2: "one"})] * 2
        else:
            subs = [s.new_sub(kind=k, first=first, expect={2: "one", 3: "noise"}) for k in ("top", "bottom")]
        for pts, sub in ((hi, subs[0]), (lo, subs[1])) if first == "top" else ((lo, subs[1]), (hi, subs[0])):
            for p in pts:
                s.add(*p, sub=sub)
    return s.case("row_wrap_%d" % nyb, [(5, 0), (4, 0), (2, 0)] if nyb == 1 else [(2, 0), (3, 0)], nyb=nyb, rows=(10, 30))


# ---- centroid_tie ---------------------------------------------------------------------------------------------------------------
TIE_POPS = ((1, 1), (1, 2), (2, 3), (3, 3), (3, 7))


def _tie_spread(rng, a, b):
    """offsets across the axis: a and b distinct values, both of sum 0, any two of different cells 2 or more apart"""
    if (a, b) == (1, 1):
        return [0], [0]
    for _ in range(100000):
        ya = rng.choice(np.arange(-40, 41), a - 1, replace=False).tolist() if a > 1 else []
        yb = rng.choice(np.arange(-40, 41), b - 1, replace=False).tolist()
        ya.append(-sum(ya))
        yb.append(-sum(yb))
        if len(set(ya)) == a and len(set(yb)) == b and max(map(abs, ya + yb)) <= 40 and min(abs(p - q) for p in ya for q in yb) >= 2:
            return ya, yb
    raise AssertionError("no spread for %r" % ((a, b),))


def tie_step(a, b):
    """(p, q): p PETs of the first cell and q of the second moved one base pair along the axis put the centroids 1 / lcm(a, b) further
    apart: q / b - p / a = gcd / (a b)"""
    g = math.gcd(a, b)
    return next((p, q) for q in range(1, b + 1) for p in range(a) if q * a - p * b == g)


def centroid_tie():
    rng = np.random.default_rng(41001)
    s = _Set(EPS, LO, LO)
    ncell = (2 * LIM - 2) // EPS
    at = 0
    for end in (0, 1):
        for a, b in TIE_POPS:
            for step in (False, True):
                at += 1
                c0 = 6 * at if end == 0 else ncell - 6 * at                   # the cell along the diagonal of the domain
                ya, yb = _tie_spread(rng, a, b)
                p, q = tie_step(a, b) if step else (0, 0)
                sub = s.new_sub(kind="step" if step else "tie", pops=(a, b), end=end, expect={a + b: "noise" if step else "one"})
                for cell, ys, moved in ((0, ya, p), (1, yb, q)):
                    for i, y in enumerate(ys):
                        along = (c0 + cell) * EPS + 300 + (1 if i < moved else 0)
                        across = c0 * EPS + 500 + y
                        s.add(*((along, across) if end == 0 else (across, along)), sub=sub)
    order = rng.permutation(len(s.ux))
    return s.case("centroid_tie", [(m, 0) for m in sorted({a + b for a, b in TIE_POPS})], order=order)


# ---- pair_loop ------------------------------------------------------------------------------------------------------------------
PAIR_BIG = {(1, 64): ((0, 0), (0, 63), (0, 61)), (65, 3): ((64, 0), (63, 2), (0, 1)), (130, 129): ((129, 128), (128, 0))}
#: per forward direction: the deciding PETs of the two cells (offsets in their cells) and the corner boxes of the other PETs
_PAIR_GEOM = {(0, 1): ((500, 600), (500, 600), ((400, 600), (0, 50)), ((400, 600), (950, 999))),
              (1, 0): ((600, 500), (600, 500), ((0, 50), (400, 600)), ((950, 999), (400, 600))),
              (1, 1): ((800, 800), (300, 300), ((0, 50), (0, 50)), ((950, 999), (950, 999))),
              (1, -1): ((800, 199), (300, 699), ((0, 50), (949, 999)), ((950, 999), (0, 50)))}


def _pair_positions(n):
    return sorted({i for i in (0, 1, 2, 3, n - 4, n - 3, n - 2, n - 1) if 0 <= i < n})


def pair_loop():
    rng = np.random.default_rng(41002)
    s = _Set(EPS)
    group = [0]                                              # the cell of every PET, for the row order
    todo, t = [], 0
    for na in range(1, 10):
        for nb in range(1, 10):
            pa, pb = _pair_positions(na), _pair_positions(nb)
            todo.append((na, nb, pa[t % len(pa)], pb[(t // len(pa) + t) % len(pb)]))
            t += 1
    for (na, nb), pos in PAIR_BIG.items():
        todo += [(na, nb, ia, ib) for ia, ib in pos]
    at = 0
    for na, nb, ia, ib in todo:
        for apart in (0, 1):
            d = DIRS[4 + at % 4]
            cx, cy = 8 * (at % 50) + 5, 8 * (at // 50) + 5
            at += 1
            da, db, boxa, boxb = _PAIR_GEOM[d]
            db = (db[0] + apart, db[1]) if d[0] else (db[0], db[1] + apart)
            sub = s.new_sub(kind="apart" if apart else "at_eps", pops=(na, nb), pos=(ia, ib), dir=d,
                            expect={na + nb: "noise" if apart else "one"})
            for (ccx, ccy), n, i, dec, box in (((cx, cy), na, ia, da, boxa), ((cx + d[0], cy + d[1]), nb, ib, db, boxb)):
                for k in range(n):
                    o = dec if k == i else (int(rng.integers(box[0][0], box[0][1] + 1)), int(rng.integers(box[1][0], box[1][1] + 1)))
                    s.cell(ccx, ccy, o[0], o[1], sub=sub)
                    group.append(2 * sub + (1 if (ccx, ccy) != (cx, cy) else 0) + 1)
    order = _order_keeping_groups(rng, np.asarray(group))
    runs = [(m, 0) for m in sorted({na + nb for na, nb, _, _ in todo})]
    return s.case("pair_loop", runs, order=order)


# ---- core_threshold -------------------------------------------------------------------------------------------------------------
CORE_CENTRE = ((5, 5), (994, 5), (5, 994), (994, 994))
#: the neighbours' PETs relative to the centre cell's origin, in reach of the centre and of no other neighbour; and out of reach
CORE_NEAR = ((-1, -510), (-1, 500), (-1, 1510), (500, -1), (500, 1001), (1001, -510), (1001, 500), (1001, 1510))
CORE_FAR = ((-1000, -1000), (-1000, 500), (-1000, 1999), (500, -1000), (500, 1999), (1999, -1000), (1999, 500), (1999, 1999))
CORE_TOTAL = len(CORE_CENTRE) + sum(q + 2 for q in range(8))


def core_threshold():
    rng = np.random.default_rng(41003)
    s = _Set(EPS)
    run_m = sorted({CORE_TOTAL - (v + 2) + d for v in range(8) for d in (0, 1)})
    for v in range(8):
        bx, by = (8 * v + 6) * EPS, 6 * EPS
        psum = CORE_TOTAL - (v + 2)
        sub = s.new_sub(kind="linked", v=v, psum=psum, expect={m: "one" if m <= psum else "noise" for m in run_m})
        out = s.new_sub(kind="unlinked", v=v, expect={m: "noise" for m in run_m})
        for p in CORE_CENTRE:
            s.add(bx + p[0], by + p[1], sub=sub)
        for q in range(8):
            p = CORE_FAR[q] if q == v else CORE_NEAR[q]
            s.add(bx + p[0], by + p[1], sub=out if q == v else sub, times=q + 2)
    return s.case("core_threshold", [(m, 0) for m in run_m], order=rng.permutation(len(s.ux)))


# ---- border_rank ----------------------------------------------------------------------------------------------------------------
BORDER_MIN_PTS = 6
#: relative to the border cell's origin: the border PET, and per component its core cell's PET and the 5 PETs of the cell behind it
BORDER_B = (500, 500)
BORDER_K = (((-400, 500), (-1100, 500)), ((1400, 500), (2100, 500)), ((500, 1400), (500, 2100)))


def border_rank():
    s = _Set(EPS)
    blocks = {"anchor": [0]}
    for name, ncomp, cx in (("two", 2, 10), ("three", 3, 30)):
        bx, by = cx * EPS, 10 * EPS
        sub = s.new_sub(kind=name, ncomp=ncomp)
        blocks[name + "_b"] = [len(s.ux)]
        s.add(bx + BORDER_B[0], by + BORDER_B[1], sub=sub)
        for k in range(ncomp):
            blocks["%s_%d" % (name, k)] = list(range(len(s.ux), len(s.ux) + 6))
            s.add(bx + BORDER_K[k][0][0], by + BORDER_K[k][0][1], sub=sub)
            s.add(bx + BORDER_K[k][1][0], by + BORDER_K[k][1][1], sub=sub, times=5)
    role = np.zeros(len(s.ux), np.int64)                     # 0 anchor, 1 border PET, 2 + k: component k
    for name, rows in blocks.items():
        role[rows] = 0 if name == "anchor" else 1 if name.endswith("_b") else 2 + int(name[-1])

    def perm(names, flip=()):
        return np.concatenate([blocks[b][::-1] if b in flip else blocks[b] for b in names])
    perms = {
        "as_built": perm(["anchor", "two_b", "two_0", "two_1", "three_b", "three_0", "three_1", "three_2"]),
        "border_row_0": perm(["three_b", "two_b", "three_1", "two_1", "three_2", "two_0", "three_0", "anchor"], flip=("three_1", "two_0")),
        "border_last": perm(["three_2", "three_0", "anchor", "two_1", "three_1", "two_0", "two_b", "three_b"], flip=("three_2",)),
        "two_border_row_0": perm(["two_b", "three_0", "three_2", "two_0", "three_1", "three_b", "two_1", "anchor"], flip=("two_1", "three_0")),
    }
    return s.case("border_rank", [(BORDER_MIN_PTS, 0)], perms=perms, role=role)


# ---- components -----------------------------------------------------------------------------------------------------------------
COLUMN_LENGTHS = tuple(range(1, 9)) + (63, 64, 65, 200)
ROW_LENGTHS = (2, 3, 5, 70)
RUN_COUNT, RUN_LEN = 256, 4
SERP_COLS, SERP_LEN = 31, 100


def _components_cells(pad):
    """-> cells [(nx, ny)], component number per cell (-1: the anchor and the padding, single cells)"""
    cells, comp = [(0, 0)], [-1]
    k = 0

    def put(cs):
        nonlocal k
        cells.extend(cs)
        comp.extend([k] * len(cs))
        k += 1
    nx = 2
    for L in COLUMN_LENGTHS:
        put([(nx, 2 + j) for j in range(L)])
        nx += 2
    for j in range(pad):                                     # single cells two apart: noise
        cells.append((nx + 2 * (j // 600), 2 + 2 * (j % 600)))
        comp.append(-1)
    nx += 4
    run_nx = nx
    for i in range(RUN_COUNT):
        put([(nx, 2 + (RUN_LEN + 1) * i + j) for j in range(RUN_LEN)])
    nx += 4
    serp = []
    for c in range(SERP_COLS):
        col = [(nx + 2 * c, 2 + j) for j in range(SERP_LEN)]
        serp += col if c % 2 == 0 else col[::-1]
        if c + 1 < SERP_COLS:
            serp.append((nx + 2 * c + 1, 2 + SERP_LEN - 1 if c % 2 == 0 else 2))
    put(serp)
    top = 2 + (RUN_LEN + 1) * RUN_COUNT + 20
    for i, L in enumerate(ROW_LENGTHS):
        put([(2 + j, top + 2 * i) for j in range(L)])
    return cells, np.asarray(comp), run_nx


def components():
    rng = np.random.default_rng(41004)
    pad = 0
    for _ in range(2):                                       # pad until the run of 256 columns begins at a multiple of WG in cell order
        cells, comp, run_nx = _components_cells(pad)
        arr = np.asarray(cells, np.int64)
        order = np.lexsort((arr[:, 1], arr[:, 0]))
        first = int(np.flatnonzero(arr[order, 0] == run_nx)[0])
        pad += -first % WG
    assert first % WG == 0
    s = _Set(EPS, anchor=False)
    for cx, cy in cells:
        s.cell(cx, cy)
    n = len(cells)
    perms = {"cell_order": order, "reversed": order[::-1].copy(), "shuffled": rng.permutation(n)}
    return s.case("components", [(2, 0)], perms=perms, comp=comp, cells=arr, run_first=first)


# ---- cut_anchor -----------------------------------------------------------------------------------------------------------------
CUT_EPS = 100
CUTS = (5000, 10000, 500000)
CUT_LOW = ((1000, 1010), (5000, 990))                        # the holders of the smallest X (row 0) and the smallest Y (last row)
CUT_A1, CUT_A2 = (1037, 7053), (1078, 21100)                 # the minimum of the survivors of CUTS[0] and of CUTS[1]
CUT_LAST = (2013, 1002000)                                   # the one survivor of CUTS[2]


def cut_anchor():
    rng = np.random.default_rng(41005)
    s = _Set(CUT_EPS, 1000, 990, anchor=False)
    pts, sub = [], []

    def pair(origin, p, kind, expect):
        k = s.new_sub(kind=kind, expect=expect)
        for q in (p, (p[0] + 99, p[1] + 99)):
            pts.append((origin[0] + q[0], origin[1] + q[1]))
            sub.append(k)
    for a in (CUT_A1, CUT_A2, CUT_LAST):
        pts.append(a)
        sub.append(-1)
    # tier 1 (Y - X about 6000): one cell on the grid of A1, two on the grid of the unfiltered minimum; and the other way round
    pair(CUT_A1, (600, 600), "together_1", {(2, CUTS[0]): "one", (2, 0): "noise"})
    pair(CUT_A1, (1163, 1237), "split_1", {(2, CUTS[0]): "noise", (2, 0): "one"})
    # tier 2 (Y - X about 20000): one cell on the grid of A2, two on the grid of A1
    pair(CUT_A2, (600, 600), "together_2", {(2, CUTS[1]): "one", (2, CUTS[0]): "noise"})
    pair(CUT_A2, (1199, 1200), "split_2", {(2, CUTS[1]): "noise"})
    order = rng.permutation(len(pts))
    for x, y in [CUT_LOW[0]] + [pts[i] for i in order] + [CUT_LOW[1]]:
        s.add(x - s.x0, y - s.y0)
    s.sub = [-1] + [sub[i] for i in order] + [-1]
    runs = [(2, 0), (2, CUTS[0]), (2, CUTS[1]), (1, CUTS[2]), (2, CUTS[2])]
    return s.case("cut_anchor", runs)


# ---- the table of cases ---------------------------------------------------------------------------------------------------------
MAKERS = {}
for _e in CELL_EDGE_EPS:
    if cell_edge_kmax(_e) >= CELL_EDGE_ALONE:
        MAKERS["cell_edge_%d" % _e] = (lambda e=_e: cell_edge(e))
    else:
        for _a in (0, 1):
            for _k in range(1, cell_edge_kmax(_e) + 1):
                for _t in (True, False):
                    MAKERS["cell_edge_%d_%s%d%s" % (_e, "xy"[_a], _k, "t" if _t else "s")] = (lambda e=_e, a=_a, k=_k, t=_t: cell_edge_alone(e, a, k, t))
for _n in (1, 2, 3):
    MAKERS["row_wrap_%d" % _n] = (lambda n=_n: row_wrap(n))
MAKERS.update(centroid_tie=centroid_tie, pair_loop=pair_loop, core_threshold=core_threshold, border_rank=border_rank,
              components=components, cut_anchor=cut_anchor)
_made = {}


def names(prefix=""):
    return [n for n in MAKERS if n == prefix or n.startswith(prefix + "_") or not prefix]


def get(name):
    """the data set `name`, made once per process"""
    if name not in _made:
        _made[name] = MAKERS[name]()
    return _made[name]


def permuted(case):
    """-> [(permutation's name, X, Y, info's per-row arrays in that order)]: the case under each of its row permutations (as built
    if it lists none)"""
    perms = case.info.get("perms") or {"as_built": np.arange(len(case.X))}
    return [(pn, case.X[p], case.Y[p], p) for pn, p in perms.items()]
