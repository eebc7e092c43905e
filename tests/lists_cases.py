"""Constructed inputs for the list kernels of cloops_amd/csrc/k_lists.hip (no GPU needed): every family puts a hand-made structure
on one of the kernels' fixed sizes -- a tile edge, a halo, a step cap, the queue, a "not staged: global memory" branch.

Everything is made in rotated coordinates p = X + Y, q = Y - X (neighbours: |dp| <= eps and |dq| <= eps).  Variant 2 cuts p into
strips of eps from 0, variant 1 from the smallest p; inside a strip the layout is ordered by q.  All sets live on a handful of strips
that begin at P0 (a multiple of eps, the smallest p of every set, so that both variants see the same strips) with q far below p:
0 <= X <= Y holds throughout, p and q are even.  Strip 0 holds the anchor PET and the paddings, strip 1 stays empty, the structures
begin in strip 2 at q >= Q0.

    pad_noise(k)   k isolated PETs in strip 0: they shift every POSITION of the layout behind them by k, no core rank
    pad_cores(k)   tiny clusters in strip 0, k PETs in all, every one of them core: they shift positions AND core ranks by k

A `Case` carries X, Y (rows shuffled by a seeded generator unless a family needs an order), eps, the (minPts, cut) runs its GPU test
makes on one handle in that order, `kind` / `grp` (what every row was placed as: K_* below, and a family-specific group number) and
`info` (the family's parameters).  tests/test_lists_cases.py proves on a numpy model of the layout that every case has the
structure it claims and that the claimed path matters for the answer; tests/test_gpu_lists_edges.py runs them against the oracle.

Not reached at these sizes (30 000 PETs at the most), and said here so that the gap is not silent:
  * lh_pack's 16-bit fields (a hint of 65 535 positions and more).  The 12-bit fields of the K2 word (4095) are reached.
  * slots 3 and 4 of k_union_c's LU_MAXB = 4, and a window that touches three distinct chains: the chains of strip s-1 inside one
    core's q window of 2 eps are separated by gaps of more than eps, so a window touches at most TWO of them.  broken_ladder()
    reaches two; the third slot, the fourth and the "more chains than slots" union cannot be reached by any input.
  * the global-memory form of k_border_q's own-strip look (jl < clo or jr >= chi): the nearest cores of a walker's own strip are
    the cores next to its position, and a tile stages every core of its position range and BHQ > 0 more on either side.
  * a fifth component at a walker (see4's overflow flag) is excluded by the geometry.  Every four-corner walker holds four
    components while both of its walks are still open ("four components already: finish in place" of k_border_q), which must end
    without raising the flag; but no input can make the ANSWER depend on that branch: every component that can be adjacent has been
    seen by then.  What the answer does depend on is a fourth component behind a wall (corners_wall).
"""
import collections

import numpy as np

EPS = 1000
P0 = 40000000                    # p of strip 0
Q0 = 1000000                     # smallest q of a structure
NMAX = 30000

K_ANCHOR, K_NOISE, K_PADCORE, K_LINE, K_WALKER, K_WALL, K_HIT, K_SUPPORT, K_CELL, K_OTHER, K_SHORT, K_FAR, K_CORNER, K_BLOB = range(14)

Case = collections.namedtuple("Case", "name family X Y eps runs kind grp info")


class _Set:
    """rows as (p, q, kind, grp); finish() -> X, Y, kind, grp with the rows in `first` in front (in that order), the rest shuffled"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.p, self.q, self.kind, self.grp = [], [], [], []
        self.n = 0
        self.add(P0, 10 * EPS, K_ANCHOR)

    def add(self, p, q, kind, grp=0):
        p, q = np.broadcast_arrays(np.asarray(p, np.int64), np.asarray(q, np.int64))
        p, q = p.ravel(), q.ravel()
        rows = np.arange(self.n, self.n + len(p))
        self.p.append(p); self.q.append(q)
        self.kind.append(np.full(len(p), kind, np.int16)); self.grp.append(np.broadcast_to(np.asarray(grp, np.int32), p.shape).copy())
        self.n += len(p)
        return rows

    def pad_noise(self, k):
        """k isolated PETs in strip 0 (3 eps apart in q, more than eps from the anchor and from pad_cores)"""
        if k:
            self.add(P0 + 2, 20 * EPS + 3 * EPS * np.arange(k), K_NOISE)

    def pad_cores(self, k, size=3):
        """k PETs in strip 0 as clusters of `size` PETs 2 apart in q (the last cluster takes the remainder), 3 eps between clusters:
        every one of them has at least `size` neighbours, none more than size + size - 1"""
        assert k == 0 or k >= size
        if k:
            ncl = k // size
            which = np.minimum(np.arange(k) // size, ncl - 1)
            self.add(P0 + 500, 10000 * EPS + 3 * EPS * which + 2 * (np.arange(k) - which * size), K_PADCORE)

    def far(self):
        """one PET 400 strips up: S grows until n <= 80 S (lists_union_flatten then stages a halo of 128 cores, not 512)"""
        self.add(P0 + 400 * EPS, 10 * EPS, K_FAR)

    def arrays(self):
        return np.concatenate(self.p), np.concatenate(self.q), np.concatenate(self.kind), np.concatenate(self.grp)

    def position(self, p, q):
        """the position in the sorted layout of a PET at (p, q): PETs in earlier strips, or in its strip at smaller q"""
        P, Q, _, _ = self.arrays()
        s, S = (p - P0) // EPS, (P - P0) // EPS
        return int(((S < s) | ((S == s) & (Q < q))).sum())

    def finish(self, first=()):
        P, Q, kind, grp = self.arrays()
        assert self.n <= NMAX and ((P - Q) % 2 == 0).all() and (Q >= 0).all() and (Q <= P).all() and P.min() == P0
        first = np.asarray(first, np.int64)
        rest = np.setdiff1d(np.arange(self.n), first)
        order = np.concatenate([first, self.rng.permutation(rest)])
        self.row_of = np.empty(self.n, np.int64)
        self.row_of[order] = np.arange(self.n)
        X, Y = (P - Q) // 2, (P + Q) // 2
        return X[order], Y[order], kind[order], grp[order]


def _rows(idx):
    """rows of the builder, to be told as rows of the finished set (info values of this form are translated by _case)"""
    return ("rows", np.asarray(idx, np.int64).ravel())


def _case(name, family, st, runs, info, first=()):
    X, Y, kind, grp = st.finish(first)
    info = {k: (st.row_of[v[1]] if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], str) and v[0] == "rows" else v) for k, v in info.items()}
    return Case(name, family, X, Y, EPS, tuple(runs), kind, grp, info)


# ---- ladder -----------------------------------------------------------------------------------------------------------------------
LADDER_M = (127, 128, 129, 511, 512, 513, 1025, 2047, 2048, 2049)
LADDER_NS = 6
LADDER_STEP = 400                # q step of a line: every PET of a line has 5 neighbours on it (3 at its ends): core at minPts 3
LADDER_MIN_PTS = 3
UNT = 512                        # (lists_union_flatten; mirrored with its line in tests/test_lists_cases.py)


def _lines(st, m, spacing, ns=LADDER_NS, strip0=2, q0=Q0, skip=None):
    """ns anti-diagonal lines of m PETs: line s at p = P0 + strip0 eps + s spacing (constant), q = q0 + 400 i"""
    rows = []
    for s in range(ns):
        i = np.arange(m)
        if skip is not None and s in skip:
            i = np.setdiff1d(i, skip[s])
        rows.append(st.add(P0 + strip0 * EPS + s * spacing, q0 + LADDER_STEP * i, K_LINE, s))
    return rows


def ladder(m, spacing, halo, pad=0):
    """six adjacent strips with one line of m cores each, all lines at the same q.
    spacing = eps: every line is within reach of the next one, the ladder is one cluster; spacing = eps + 2: six clusters.
    halo = 512: the set as it is (n > 80 S); halo = 128: one more PET 400 strips up, so that n <= 80 S.
    pad: that many pad_cores in front of the ladder (they shift the core rank of every line by `pad`)."""
    st = _Set(1000 + m)
    st.pad_cores(pad)
    _lines(st, m, spacing)
    if halo == 128:
        st.far()
    return _case("ladder-m%d-s%d-h%d-p%d" % (m, spacing, halo, pad), "ladder", st, [(LADDER_MIN_PTS, 0)],
                 dict(m=m, spacing=spacing, halo=halo, pad=pad, ns=LADDER_NS))


#: the line length of the pad cases: longer than either halo, shorter than halo + tile -- a tile then holds cores of line s whose strip
#: below (line s-1) begins within one core of the first staged core
LADDER_PAD_M = {512: 513, 128: 129}


def ladder_pad(halo, d):
    """line 0's first core at rank 2 UNT - halo + d: for the tile that begins at 2 UNT the staged range begins at 2 UNT - halo, i.e.
    d cores in front of line 0 (d = -1: the line began one core earlier, 0: exactly there, +1: one core later)"""
    return ladder(LADDER_PAD_M[halo], EPS, halo, 2 * UNT - halo + d)


def ladder_tile(halo, d):
    """line 1's first core at core rank 2 UNT + d: one core in front of a tile's start, on it, one behind it"""
    m = LADDER_PAD_M[halo]
    return ladder(m, EPS, halo, 2 * UNT - m + d)


#: (m, halo) of ladder_link: line lengths of LADDER_M on both sides of the halo
LINKS = ((128, 128), (129, 128), (511, 128), (512, 128), (513, 128), (512, 512), (513, 512))


LINK_WALL = 20


def ladder_link(m, halo):
    """two adjacent strips with m cores each, the upper strip's first core on the tile start 2 UNT (pad_cores).  The upper strip is a
    line, 500 above its strip's lower edge.  Of the lower strip only ONE core, A, lies under it within reach -- exactly eps below the
    line's first core; in front of A in q, inside the windows of the line's first cores, 20 cores 2 further down (misses: a walk
    passes them, 4 or 8 per round, before it gets to A); the other cores of the lower strip follow far behind the line's end in q, a
    chain of their own.  The line's first three cores are the only link between the strips, and their strip below begins m cores in
    front of them: for m > halo in front of the first staged core (whose q is far beyond their window: no shortcut) -- they go to the
    overflow list; for m = halo exactly at the first staged core."""
    st = _Set(1500 + m)
    st.pad_cores(2 * UNT - m)
    st.add(P0 + 2 * EPS + 498, Q0 - 2 * (LINK_WALL - np.arange(LINK_WALL)), K_WALL, 0)
    st.add(P0 + 2 * EPS + 500, Q0, K_HIT, 0)
    st.add(P0 + 2 * EPS + 500, Q0 + LADDER_STEP * (m + 10 + np.arange(m - 1 - LINK_WALL)), K_LINE, 0)
    st.add(P0 + 3 * EPS + 500, Q0 + LADDER_STEP * np.arange(m), K_LINE, 1)
    if halo == 128:
        st.far()
    return _case("link-m%d-h%d" % (m, halo), "link", st, [(LADDER_MIN_PTS, 0)], dict(m=m, halo=halo))


# ---- broken ladder ----------------------------------------------------------------------------------------------------------------
BROKEN_M = (1025, 81)            # the strip below the link: longer than either halo (the link's cores overflow), shorter than both (staged)


def broken_ladder(halo, d, m=1025):
    """strip 2: a line of m with the three PETs around its middle g = m // 2 removed (a gap of 1600 in q): chains A and B, their tail
    and head doubled.  strip 3 (eps above): a line over A that ends 1200 in front of the gap's middle, one over B that begins 1200
    behind it -- each touches one chain -- and between them THREE PETs at one position over the middle of the gap, whose window holds
    A's tail and B's head: the only link between the two halves.  pad_cores puts the first of the three at core rank 4 UNT + d.
    m = 1025: strip 2 begins in front of the staged cores of the link's tile, the three go to the overflow list and k_union_overflow
    unites them with both chains; m = 81: their window is staged, k_union_c's walk notes two chains per lane."""
    g = m // 2
    st = _Set(2000 + halo + m)
    ncore_before = (m - 3 + 2) + (g - 2)                 # strip 2 with the doubled tail / head, and the line over A
    pad = 4 * UNT + d - ncore_before
    st.pad_cores(pad)
    _lines(st, m, EPS, ns=2, skip={0: np.arange(g - 1, g + 2), 1: np.arange(g - 2, g + 3)})
    st.add(P0 + 2 * EPS, Q0 + LADDER_STEP * np.array([g - 2, g + 2]), K_LINE, 10)     # the doubled tail of A and head of B
    link = st.add(np.full(3, P0 + 3 * EPS), Q0 + LADDER_STEP * g, K_LINE, 11)
    if halo == 128:
        st.far()
    return _case("broken-h%d-d%d-m%d" % (halo, d, m), "broken", st, [(LADDER_MIN_PTS, 0)], dict(halo=halo, d=d, m=m, pad=pad, link=_rows(link)))


# ---- cell across a tile (variant 2) ---------------------------------------------------------------------------------------------
LT = 2048
CELL_N = 300
CELL_K = (1, 64, 127, 128, 129, 299)
CELL_MIN_PTS = 5


def cell_tile(k, where):
    """one rotated cell (strip 2, q in [Q0, Q0 + eps)) of 300 PETs at distinct q, beginning at position LT - k of the layout; a second
    cluster of 6 PETs far away in strip 4.  Row 0 goes to the cell's first (where = "first") or last (where = "last") PET in sorted
    order, rows 1 .. 6 to the second cluster, every other PET of the cell has a later row: the cell's cluster comes first by its
    smallest row -- unless the minimum misses the part of the cell behind position LT."""
    st = _Set(3000 + k)
    q = Q0 + 2 * np.arange(CELL_N)
    p = P0 + 2 * EPS + 2 * st.rng.integers(0, EPS // 2, CELL_N)
    st.pad_noise(LT - k - 1)                             # the anchor + the padding in front of the cell
    cell = st.add(p, q, K_CELL)
    other = st.add(P0 + 4 * EPS + 10, Q0 + 2 * np.arange(6), K_OTHER)
    assert st.position(int(p[0]), int(q[0])) == LT - k
    first = [cell[0] if where == "first" else cell[-1]] + list(other)
    return _case("cell-k%d-%s" % (k, where), "cell", st, [(CELL_MIN_PTS, 0)], dict(k=k, where=where, cell=_rows(cell), other=_rows(other)), first)


# ---- miss walls ---------------------------------------------------------------------------------------------------------------------
#: cores in front of the walker's only neighbour: both sides of the 2 x 2 predicated candidates of pass 0, of one and two rounds of 16
#: lanes counted from the window's start (15, 16, 17, 33) and from where pass 0 leaves the walk (4 + 15, 4 + 16, 4 + 17), of the 254
#: cores of halo
WALL_K = (0, 1, 3, 4, 5, 15, 16, 17, 19, 20, 21, 33, 255, 300)
WALL_MIN_PTS = (5, 129)          # 5: the walkers arrive with K2's hints; 129: as LH_NONE (minPts 1 has no walkers: every PET is core)
BNQ, BNT = 1024, 2048            # (lists_border; mirrored with their line in tests/test_lists_cases.py)


def _wall_unit(st, s, qw, k, side, nsup, grp):
    """a walker in strip s at q = qw, at the strip's bottom edge in p (side +1: it looks into strip s + 1) or 2 below its top edge
    (side -1: strip s - 1).  In that strip: k wall cores 2 further than eps in p, at q = qw + eps - 2 k .. qw + eps - 2 (inside
    the walker's q window), the core h exactly eps away in p and in q, and nsup support PETs behind h in q (outside the window) that
    make h and the wall core.  -> (row of the walker, p and q of the walker)"""
    pw = P0 + s * EPS + (0 if side > 0 else EPS - 2)
    w = st.add(pw, qw, K_WALKER, grp)
    qh = qw + EPS
    st.add(pw + side * (EPS + 2), qh - 2 * (k - np.arange(k)), K_WALL, grp)
    st.add(pw + side * EPS, qh, K_HIT, grp)
    st.add(pw + side * (EPS + 2), qh + 2 + 2 * np.arange(nsup), K_SUPPORT, grp)
    return w, pw, qw


def miss_wall(k, min_pts, align="edge"):
    """two walkers alone in strip 4, 20 eps apart in q and next to each other in the layout: the first looks up into strip 5, the
    second down into strip 3.  align "edge": pad_noise puts the first on the LAST position of a 2048-position tile (the last of a
    1024-position tile too): its wall lies behind the tile's positions, among the halo cores; the second is the FIRST position of
    the next tile, its wall lies in front.  align "mid": 700 positions further on."""
    st = _Set(4000 + 10 * k + min_pts)
    ws = [_wall_unit(st, 4, Q0 + 20 * EPS * u, k, side, min_pts + 1, u) for u, side in enumerate((1, -1))]
    target = BNT - 1 if align == "edge" else BNT + 699
    st.pad_noise((target - st.position(ws[0][1], ws[0][2])) % BNT)
    return _case("wall-k%d-m%d-%s" % (k, min_pts, align), "wall", st, [(min_pts, 0)],
                 dict(k=k, min_pts=min_pts, align=align, walkers=_rows(np.concatenate([w[0] for w in ws]))))


WALLPOP_FILL = 4200


def wall_population(side):
    """the 12-bit hint fields of the K2 word: a walker of strip 4 with 4200 isolated PETs of its own strip between it and the strip
    it looks into (behind it in the layout for side +1, in front of it for side -1), a wall of 5: the hint leaves its field, the
    walker arrives as LH_NONE although minPts is 5"""
    st = _Set(4500 + side)
    if side > 0:
        w = _wall_unit(st, 4, Q0, 5, 1, 6, 0)
        st.add(P0 + 4 * EPS + 500, Q0 + 3 * EPS * (1 + np.arange(WALLPOP_FILL)), K_NOISE, 9)
    else:
        w = _wall_unit(st, 4, Q0 + 3 * EPS * (WALLPOP_FILL + 1), 5, -1, 6, 0)
        st.add(P0 + 4 * EPS + 500, Q0 + 3 * EPS * np.arange(WALLPOP_FILL), K_NOISE, 9)
    return _case("wallpop-%s" % ("up" if side > 0 else "down"), "wallpop", st, [(5, 0)], dict(side=side, k=5, walkers=_rows(w[0])))


# ---- four corners ---------------------------------------------------------------------------------------------------------------
CORNER_MIN_PTS = 6
CORNER_DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1))         # in (X, Y); rotated: (p + eps, q - eps), (p - eps, q + eps), (p + eps, q + eps), (p - eps, q - eps)


def _corners(st, pw, qw, grp, wall=0):
    """walker at (pw, qw).  In each of the four axis directions of (X, Y) one PET at distance eps and five at distance 2 eps -- at
    (2 eps - t) along the axis and t across, t = 0, +-1, +-2: exactly eps from the first.  At minPts 6 the walker has count 5, the
    first PET of a direction 7, the others 6: four components of six cores, the walker next to all of them.
    wall = k: k more cores in front (in q) of the corner at (p + eps, q + eps), 2 further than eps in p: inside the walker's window of
    strip s + 1 and no neighbours of the walker, but of that corner -- they belong to its component.
    -> rows (walker, [the six of every direction])"""
    x, y = (pw - qw) // 2, (pw + qw) // 2
    w = st.add(pw, qw, K_WALKER, grp)
    comps = []
    for c, (dx, dy) in enumerate(CORNER_DIRS):
        t = np.array([0, 1, -1, 2, -2])
        cx = np.concatenate([[x + dx * EPS], x + dx * (2 * EPS - np.abs(t)) + dy * t])
        cy = np.concatenate([[y + dy * EPS], y + dy * (2 * EPS - np.abs(t)) + dx * t])
        comps.append(st.add(cx + cy, cy - cx, K_CORNER, 4 * grp + c))
    if wall:
        st.add(pw + EPS + 2, qw + EPS - 2 * (wall - np.arange(wall)), K_WALL, 4 * grp + 2)
    return w, comps


def corners(order, tile=None):
    """two walkers with four corners each (the second 50 eps further in q and four strips up: no padding aligns it).  Rows: the two
    walkers, then the components -- order 0: in the order of CORNER_DIRS, order 1: reversed.  tile = (T, at): pad_noise puts the first
    walker on position T - 1 (at = -1) or T (at = 0).
    Every walker here holds four components after two steps of both walks, and both walks are still open (a step that hits does not
    look whether the window goes on): k_border_q's "four components already: finish in place"."""
    st = _Set(5000 + order)
    pw, qw = P0 + 4 * EPS + 300, Q0 + 300
    w, comps = _corners(st, pw, qw, 0)
    w2, comps2 = _corners(st, pw + 4 * EPS + 2, qw + 50 * EPS, 1)
    if tile:
        T, at = tile
        st.pad_noise((T + at - st.position(pw, qw)) % T)
    cs = list(comps) + list(comps2)
    if order:
        cs = cs[::-1]
    first = np.concatenate([w, w2] + cs)
    name = "corners-o%d" % order + ("-t%d%+d" % tile if tile else "")
    return _case(name, "corners", st, [(CORNER_MIN_PTS, 0)], dict(order=order, tile=tile, walkers=_rows(np.concatenate([w, w2]))), first)


def corners_wall(k, tile=None):
    """the corner behind a wall of k >= 5 cores (fewer would not be core at minPts 6) owns the walker: its rows come first, behind the
    walker's, then the other components'"""
    st = _Set(5500 + k)
    pw, qw = P0 + 4 * EPS + 300, Q0 + 300
    w, comps = _corners(st, pw, qw, 0, k)
    if tile:
        T, at = tile
        st.pad_noise((T + at - st.position(pw, qw)) % T)
    first = np.concatenate([w, comps[2], comps[0], comps[1], comps[3]])
    return _case("corners-wall%d" % k + ("-t%d%+d" % tile if tile else ""), "corners_wall", st, [(CORNER_MIN_PTS, 0)],
                 dict(k=k, tile=tile, walkers=_rows(w), owner=_rows(comps[2])), first)


# ---- crowded walker tile ----------------------------------------------------------------------------------------------------------
CROWD_W, CROWD_C = 500, 500
CROWD_MIN_PTS = 5


def crowded(at=0):
    """strip 4: 500 walkers 1002 apart in q at the strip's bottom edge, then a blob of 500 cores -- 1000 positions in a row, all in
    one 1024-position tile (pad_noise puts the first walker on a tile's first position + at).  strip 5: a wall 2 further than eps in
    p with a core every 200 in q along all the walkers, and for walker i the core h_i exactly eps away in p and in q: a walker's
    window begins with 5 wall cores, then h of its predecessor"""
    st = _Set(6000 + at)
    qw = Q0 + 1002 * np.arange(CROWD_W)
    pw = P0 + 4 * EPS
    w = st.add(pw, qw, K_WALKER)
    st.add(pw + 2 * st.rng.integers(0, 200, CROWD_C), qw[-1] + 3 * EPS + 2 * np.arange(CROWD_C), K_BLOB)
    st.add(pw + EPS + 2, np.arange(Q0 - EPS, qw[-1] + EPS + 1, 200), K_WALL)
    st.add(pw + EPS, qw + EPS, K_HIT)
    st.pad_noise((at - st.position(pw, int(qw[0]))) % BNT)
    return _case("crowded%+d" % at, "crowded", st, [(CROWD_MIN_PTS, 0)], dict(at=at, walkers=_rows(w)))


# ---- under a cut ------------------------------------------------------------------------------------------------------------------
CUT = 5000
CUT_SHORT = 40                   # short-distance PETs per strip: q < CUT, removed by the cut, in front of every strip's structure


def _short(st, strips):
    for s in strips:
        st.add(P0 + s * EPS + 2 * st.rng.integers(0, EPS // 2, CUT_SHORT), 2 * st.rng.permutation(CUT // 2)[:CUT_SHORT], K_SHORT, s)


def cut_ladder():
    """ladder(513, eps, halo 128) with 40 PETs of q < 5000 in each of its strips and the two in front"""
    st = _Set(7000)
    st.pad_cores(2 * UNT - 128)
    _lines(st, 513, EPS)
    _short(st, range(0, 8))
    st.far()
    return _case("cut-ladder", "cut", st, [(LADDER_MIN_PTS, 0), (LADDER_MIN_PTS, CUT)], dict(kindof="ladder", m=513, halo=128))


def cut_wall():
    """miss walls of 5 (up and down from strip 4) with 40 PETs of q < 5000 in strips 0 .. 6"""
    st = _Set(7001)
    ws = [_wall_unit(st, 4, Q0 + 20 * EPS * u, 5, side, 6, u) for u, side in enumerate((1, -1))]
    _short(st, range(0, 7))
    return _case("cut-wall", "cut", st, [(5, 0), (5, CUT)], dict(kindof="wall", k=5, walkers=_rows(np.concatenate([w[0] for w in ws]))))


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------
def _catalogue():
    """name -> (maker, arguments) of every case, in the order the families are described above"""
    cat = {}

    def put(f, *a):
        cat["%s(%s)" % (f.__name__, ",".join(str(x) for x in a))] = (f, a)
    for halo in (512, 128):
        for m in LADDER_M:
            for spacing in (EPS, EPS + 2):
                put(ladder, m, spacing, halo)
        for d in (-1, 0, 1):
            put(ladder_pad, halo, d)
            put(ladder_tile, halo, d)
            for m in BROKEN_M:
                put(broken_ladder, halo, d, m)
    for m, halo in LINKS:
        put(ladder_link, m, halo)
    for k in CELL_K:
        for where in ("first", "last"):
            put(cell_tile, k, where)
    for k in WALL_K:
        for m in WALL_MIN_PTS:
            put(miss_wall, k, m)
    for k in (5, 300):
        put(miss_wall, k, 5, "mid")
    put(wall_population, 1)
    put(wall_population, -1)
    for order in (0, 1):
        put(corners, order)
    for T in (BNQ, BNT):
        for at in (-1, 0):
            put(corners, 0, (T, at))
    for k in (5, 17):
        put(corners_wall, k)
    put(corners_wall, 17, (BNQ, -1))
    put(crowded, 0)
    put(crowded, 24)
    put(cut_ladder)
    put(cut_wall)
    return cat


_CATALOGUE = _catalogue()
_made = {}


def names(family=None):
    """the catalogue's keys, in order; `family`: those whose maker is that function name"""
    return [k for k, (f, a) in _CATALOGUE.items() if family is None or f.__name__ == family]


def get(name):
    """the case `name` of the catalogue, made once per process"""
    if name not in _made:
        f, a = _CATALOGUE[name]
        _made[name] = f(*a)
    return _made[name]
