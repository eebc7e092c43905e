"""CPU only: every case of tests/lists_cases.py has the structure it claims, and the path it aims at matters for the answer.

A numpy model of the layout the list kernels work on, written from the comments of cloops_amd/csrc/k_lists.hip and from
include/cloops_hip.h (it does not import cloops_amd): strips and the order by q, exact neighbour counts (oracle.neighbor_counts), core
and walker flags, positions, core ranks, chains, the cores-only strip table, the cross-strip core-core edges, which cores
k_union_c cannot serve from its staged range, and a walker's walks as k_border_q's pass 0 takes them.  The model is itself checked
against the oracle wherever it gives an answer (components of cores, owners of walkers, the order of variant 2's labels).

For every family: the structural claim in terms of the mirrored constants; the labels that would come out if the targeted branch
did nothing, which must differ from the oracle's; and that no setting is empty.  Where the issue of a size list includes values on
the near side of an edge (a wall of fewer than 4 cores, a line shorter than the halo, the smallest row on the cell's first PET), the
case is a control: the claim then is that the branch is NOT needed, and says so."""
import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import lists_cases as LC
import oracle

EPS = LC.EPS
LT = 2048            # k_lists.hip:74   positions per tile of k_classify / k_make_lists / k_base_keys
L_HALO = 128         # k_lists.hip:76   variant 2's halo of k_classify
LU_MAXB = 4          # k_lists.hip:767  slots of distinct chains per lane of k_union_c
LOOKBACK = 64        # k_lists.hip:861  cores per round of k_union_c's look-back for a chain head
STAGED_MAX = 2047    # k_lists.hip:956  a strip-below range is staged only if b - tb <= 2047
OVF_ROUND = 8        # k_lists.hip:1083 candidates per round of k_union_overflow
UNT = 512            # k_lists.hip:2109 cores per tile of k_union_c
HALO_BIG, HALO_SMALL, HALO_RULE = 512, 128, 80      # k_lists.hip:2117  halo 512 if n > 80 S, else 128
BNT, BHC = 2048, 256                                 # k_lists.hip:2145  k_border_w (variant 1): positions per tile, cores of halo
BNQ, BHQ = 1024, 254                                 # k_lists.hip:2145  k_border_q (variant 2)
KCAP, BQ_G = 2, 16                                   # k_lists.hip:2147  predicated steps (2 candidates each), lanes per queued walker
K2H_MASK = 0xfff                                     # cl_common.h:409   a hint of K2H_MASK positions and more is dropped
assert (UNT, BNQ, BNT, LT) == (LC.UNT, LC.BNQ, LC.BNT, LC.LT)

VARIANTS = ("v2", "v1")
_cnt, _lab, _lay = {}, {}, {}


def counts(name, cut):
    """exact neighbour counts among the rows the cut keeps, -1 at the others"""
    if (name, cut) not in _cnt:
        c = LC.get(name)
        keep = c.Y - c.X >= cut
        out = np.full(len(c.X), -1, np.int64)
        out[keep] = oracle.neighbor_counts(c.X[keep], c.Y[keep], c.eps)
        _cnt[(name, cut)] = out
    return _cnt[(name, cut)]


def labels(name, variant, m, cut):
    if (name, variant, m, cut) not in _lab:
        c = LC.get(name)
        _lab[(name, variant, m, cut)] = oracle.single_dbscan(variant, c.X, c.Y, c.eps, m, cut)["labels"]
    return _lab[(name, variant, m, cut)]


class Layout:
    """the sorted layout of one run and its two lists"""

    def __init__(self, name, variant, m, cut=0):
        c = LC.get(name)
        keep = np.flatnonzero(c.Y - c.X >= cut)
        p, q = c.X[keep] + c.Y[keep], c.Y[keep] - c.X[keep]
        a0 = 0 if variant == "v2" else int(p.min())
        strip = (p - a0) // EPS
        order = np.lexsort((q, strip))
        self.row, self.p, self.q, self.s = keep[order], p[order], q[order], strip[order] - strip.min()
        self.n, self.ntotal, self.S = len(order), len(c.X), int(strip.max() - strip.min()) + 1
        cnt = counts(name, cut)[self.row]
        self.cnt, self.core = cnt, cnt >= m
        self.walker = ~self.core & (cnt > 1)
        self.strip_start = np.searchsorted(self.s, np.arange(self.S + 2))
        self.rank = np.concatenate([[0], np.cumsum(self.core)])          # cores in front of a position
        self.pos_of_row = np.full(len(c.X), -1, np.int64)
        self.pos_of_row[self.row] = np.arange(self.n)
        ci = np.flatnonzero(self.core)
        self.C, self.cpos, self.cq, self.cp, self.cs, self.crow = len(ci), ci, self.q[ci], self.p[ci], self.s[ci], self.row[ci]
        self.cstrip = self.rank[self.strip_start]
        self.open = np.ones(self.C, bool)
        self.open[1:] = (self.cs[1:] != self.cs[:-1]) | (self.cq[1:] - self.cq[:-1] > EPS)
        self.head = np.maximum.accumulate(np.where(self.open, np.arange(self.C), 0))
        nh = np.where(self.open, np.arange(self.C), self.C)
        self.nexthead = np.concatenate([np.minimum.accumulate(nh[::-1])[::-1][1:], [self.C]])      # first chain head behind a core (cskip)
        self.halo = HALO_BIG if self.ntotal > HALO_RULE * self.S else HALO_SMALL

    # ---- cores: the cross-strip edges and the staged ranges of k_union_c ----
    def cross_edges(self, slack=0):
        """(i, j): core i, core j one strip below inside i's q window and within eps (+ slack) in p; and the windows [lo, hi)"""
        lo, hi = np.zeros(self.C, np.int64), np.zeros(self.C, np.int64)
        for s in range(1, self.S):
            a, b, e = self.cstrip[s - 1], self.cstrip[s], self.cstrip[s + 1]
            if a < b < e:
                lo[b:e] = a + np.searchsorted(self.cq[a:b], self.cq[b:e] - EPS, "left")
                hi[b:e] = a + np.searchsorted(self.cq[a:b], self.cq[b:e] + EPS, "right")
        w = hi - lo
        i = np.repeat(np.arange(self.C), w)
        j = lo[i] + np.arange(w.sum()) - np.repeat(np.cumsum(w) - w, w)
        hit = self.cp[j] >= self.cp[i] - EPS - slack
        return i[hit], j[hit], lo, hi

    def union_ranges(self):
        """per core what k_union_c<UNT, halo, true> does with its strip-below range [tb, b): overflow (listed for k_union_overflow),
        shortcut (tb = wbeg taken), tb, b and the first staged index `base` of its tile"""
        i = np.arange(self.C)
        base = (i // UNT) * UNT - self.halo
        wbeg = np.maximum(base, 0)
        tb = np.where(self.cs > 0, self.cstrip[np.maximum(self.cs - 1, 0)], 0)
        b = np.where(self.cs > 0, self.cstrip[self.cs], 0)
        has = tb < b
        short = has & (tb < wbeg) & (wbeg < b) & (self.cq[np.minimum(wbeg, self.C - 1)] < self.cq - EPS)
        tb2 = np.where(short, wbeg, tb)
        staged = (tb2 >= wbeg) & (b - tb2 <= STAGED_MAX)
        return has & ~staged, short, tb, b, base

    def components(self, ei, ej):
        """component number per core: chains + the given edges"""
        i = np.concatenate([np.arange(self.C), ei])
        j = np.concatenate([self.head, ej])
        return connected_components(coo_matrix((np.ones(len(i)), (i, j)), shape=(self.C, self.C)), directed=False)[1]

    def lookback_rounds(self):
        """rounds of 64 cores that the first wave of every tile of k_union_c looks back for the head of the first staged core's chain"""
        out = []
        for t0 in range(0, self.C, UNT):
            base = t0 - self.halo
            if base > 0 and not self.open[base]:
                out.append((base - 1 - self.head[base]) // LOOKBACK + 1)
        return out

    # ---- walkers: windows, hints, pass 0 of k_border_q ----
    def window(self, pos, side):
        """core indices [j0, j1) of strip s + side inside the q window of the PET at `pos`"""
        s = self.s[pos] + side
        if s < 0 or s >= self.S:
            return 0, 0
        a, b = self.cstrip[s], self.cstrip[s + 1]
        return a + np.searchsorted(self.cq[a:b], self.q[pos] - EPS, "left"), a + np.searchsorted(self.cq[a:b], self.q[pos] + EPS, "right")

    def hints(self, pos):
        """(da, db): positions back to the first PET of strip s - 1 with q >= q - eps, ahead to the first one of strip s + 1"""
        s, out = self.s[pos], []
        for t in (s - 1, s + 1):
            if t < 0 or t >= self.S:
                out.append(0)
                continue
            a, b = self.strip_start[t], self.strip_start[t + 1]
            out.append(abs(a + np.searchsorted(self.q[a:b], self.q[pos] - EPS, "left") - pos))
        return out

    def walk(self, pos, side, steps=None):
        """k_border_q's walk into strip s + side: two candidates per step, a hit settles its chain and the walk goes on behind it
        (cskip).  -> (cores hit, walk still open after `steps` steps, candidates looked at in front of the first hit)"""
        j, j1 = self.window(pos, side)
        seen, it, misses, on = [], 0, None, j < self.C and j < j1
        hit = lambda k: abs(self.cp[k] - self.p[pos]) <= EPS
        while on and (steps is None or it < steps):
            it += 1
            w0, w1 = j < j1, j + 1 < j1
            h0 = w0 and hit(j)
            h1 = w0 and not h0 and w1 and hit(j + 1)
            fin = not w0 or (not h0 and not w1)
            if h0 or h1:
                k = j if h0 else j + 1
                if misses is None:
                    misses = k - self.window(pos, side)[0]
                seen.append(k)
                j = self.nexthead[k]
            else:
                j += 2
            on = not fin and j < self.C
        if steps is None:
            on = False
        return seen, on, misses

    def own_strip(self, pos):
        """the nearest core on either side in the PET's own strip and q window"""
        c1, out = self.rank[pos], []
        if c1 > 0 and self.cs[c1 - 1] == self.s[pos] and self.cq[c1 - 1] >= self.q[pos] - EPS:
            out.append(c1 - 1)
        if c1 < self.C and self.cs[c1] == self.s[pos] and self.cq[c1] <= self.q[pos] + EPS:
            out.append(c1)
        return out

    def owner_v2(self, pos, lab, steps=None):
        """variant 2's label of a walker from the cores its walks reach: the adjacent component with the lowest key, i.e. (the
        labels go by key, test_cell_*) the lowest label; -1 = none reached"""
        seen = self.own_strip(pos) + self.walk(pos, -1, steps)[0] + self.walk(pos, 1, steps)[0]
        ls = [int(lab[self.crow[k]]) for k in seen]
        return min(ls) if ls else -1

    def staged_q(self, pos, NT=BNQ, HC=BHQ):
        """[clo, chi): the cores the border kernel stages for the tile of position `pos`"""
        t0 = (pos // NT) * NT
        return max(self.rank[t0] - HC, 0), min(self.rank[min(t0 + NT, self.n)] + HC, self.C)


def layout(name, variant, m, cut=0):
    if (name, variant, m, cut) not in _lay:
        _lay[(name, variant, m, cut)] = Layout(name, variant, m, cut)
    return _lay[(name, variant, m, cut)]


def same_partition(a, b):
    k = len(np.unique(np.stack([a, b], 1), axis=0))
    return k == len(np.unique(a)) == len(np.unique(b))


def check_core_model(L, lab):
    """the model's components of cores are the oracle's clusters of cores; -> (component per core with every edge, edges, ranges)"""
    ei, ej, lo, hi = L.cross_edges()
    full = L.components(ei, ej)
    cl = lab[L.crow]
    assert (cl >= 0).all() and same_partition(full, cl)
    return full, ei, ej


def max_chains_touched(L, ei, ej):
    if len(ei) == 0:
        return 0
    pairs = np.unique(np.stack([ei, L.head[ej]], 1), axis=0)
    return int(np.bincount(pairs[:, 0]).max())


# ---- every case -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.names())
def test_every_setting_forms_clusters_and_noise(name):
    """clusters and noise in every run of every variant; the rows a cut removes are noise; at most 30 000 PETs, 0 <= X <= Y"""
    c = LC.get(name)
    assert len(c.X) <= LC.NMAX and (c.X >= 0).all() and (c.X <= c.Y).all()
    for m, cut in c.runs:
        keep = c.Y - c.X >= cut
        for v in VARIANTS:
            lab = labels(name, v, m, cut)
            assert (lab[~keep] == -1).all()
            assert (lab >= 0).any() and (lab[keep] < 0).any() and m > 1, (v, m, cut)


@pytest.mark.parametrize("name", LC.names())
def test_a_window_touches_at_most_two_chains(name):
    """what the module's docstring says of LU_MAXB: no core's window one strip below holds cores of more than two chains"""
    c = LC.get(name)
    for m, cut in c.runs:
        for v in VARIANTS:
            L = layout(name, v, m, cut)
            ei, ej, _, _ = L.cross_edges()
            assert max_chains_touched(L, ei, ej) <= 2 < LU_MAXB


# ---- ladder -----------------------------------------------------------------------------------------------------------------------
def _ladder_checks(name, m_run, cut, m, spacing, halo):
    c = LC.get(name)
    for v in VARIANTS:
        L = layout(name, v, m_run, cut)
        lab = labels(name, v, m_run, cut)
        assert L.halo == halo and (L.n > HALO_RULE * L.S) == (halo == HALO_BIG)
        line = c.kind[L.crow] == LC.K_LINE
        assert L.core[L.pos_of_row[np.flatnonzero((c.kind == LC.K_LINE) | (c.kind == LC.K_PADCORE))]].all()      # every PET of a line is core
        upper = line & (c.grp[L.crow] > 0)
        full, ei, ej = check_core_model(L, lab)
        ovf, short, tb, b, base = L.union_ranges()
        assert not ovf[~upper].any()
        # Which cores overflow, worked out by hand.  Take a core of line s that is the o-th core of its tile (o = rank % UNT), and
        # let its strip below (line s - 1, m cores) begin in front of the tile's first staged core (tb < base).  The lines lie at
        # the same q, so the core's partner on line s - 1 is m ranks in front of it, and its window begins 2.5 steps of 400 in front
        # of that partner, i.e. m + 2.5 - o ranks in front of the tile start.  The staged range reaches `halo` ranks back.  If the
        # window begins inside it (m + 2.5 - o < halo) the shortcut tb = wbeg serves the core; otherwise it overflows:
        # overflow  <=>  o < m + 3 - halo.  A range longer than STAGED_MAX overflows whatever o is.
        lim = m + 3 - halo
        novf = int(ovf.sum())
        rk = np.arange(L.C)
        expect = upper & ((b - tb > STAGED_MAX) | ((tb < np.maximum(base, 0)) & (rk % UNT < lim)))
        assert np.array_equal(ovf, expect), v
        if m > STAGED_MAX or lim >= UNT:
            for s in range(1, 6):     # (nearly) every core of every upper line: its strip-below range begins before tile start - halo
                sel = line & (c.grp[L.crow] == s)
                assert ovf[sel].sum() >= m - 64 and ((tb < base) | (b - tb > STAGED_MAX))[sel].sum() >= m - 64, (v, s)
            if m > STAGED_MAX:
                assert (b - tb)[upper].min() > STAGED_MAX and ovf[upper].all()
        elif lim <= 0:
            assert novf == 0
        elif novf == 0:
            # (the lines fall on the tiles: every strip-below range begins exactly at the first staged core)
            assert m in (HALO_SMALL, HALO_BIG) and (tb >= base)[upper].all() and (tb == base)[upper].any()
        else:
            assert 0 < novf < upper.sum(), (v, novf)
        if m == STAGED_MAX:
            assert (b - tb)[upper].max() == STAGED_MAX
        rounds = L.lookback_rounds()
        if m >= 1025:                 # a chain head more than halo + 64 cores in front of a tile start: several rounds of look-back
            assert max(rounds) >= 2 and (np.arange(0, L.C, UNT) - L.head[np.arange(0, L.C, UNT)]).max() > halo + LOOKBACK
        # sensitivity
        if spacing == EPS:
            assert len(np.unique(lab[L.crow[line]])) == 1
            if novf:
                # overflow cores unite with nothing; and some of them have a hit, i.e. a cskip jump in the overflow walk
                drop = ovf[ei]
                whole = m > STAGED_MAX or lim >= UNT
                assert drop.any() and same_partition(L.components(ei[~drop], ej[~drop]), lab[L.crow]) == (not whole), v
                # (where only the first cores of a tile overflow -- the sizes at the halo's edge -- the rest of their line still
                #  unites the two chains: those sizes show that the boundary cores are listed and served, not that the answer
                #  hangs on them; ladder_link() is the form of the same sizes in which it does)
            else:
                # (control, the near side of the halo: no core overflows, every edge comes from a staged window)
                assert not same_partition(L.components(ei[:0], ej[:0]), lab[L.crow]), v
        else:
            # eps + 2: no edge, six clusters; a test in p that is off by 2 would make them one
            assert len(ei) == 0 and len(np.unique(lab[L.crow[line]])) == 6
            e2 = L.cross_edges(slack=2)
            assert len(e2[0]) and not same_partition(L.components(e2[0], e2[1]), lab[L.crow]), v
    return L


@pytest.mark.parametrize("name", LC.names("ladder"))
def test_ladder(name):
    c = LC.get(name)
    _ladder_checks(name, LC.LADDER_MIN_PTS, 0, c.info["m"], c.info["spacing"], c.info["halo"])


@pytest.mark.parametrize("name", LC.names("ladder_pad"))
def test_ladder_window_at_the_first_staged_core(name):
    """the tile that begins at core 2 UNT holds cores of line 1 whose strip below begins d cores from the first staged core;
    d = -1: one core in front of it -- the shortcut tb = wbeg serves those whose window begins later, the others overflow"""
    c = LC.get(name)
    d = c.info["pad"] - (2 * UNT - c.info["halo"])
    assert d in (-1, 0, 1)
    L = _ladder_checks(name, LC.LADDER_MIN_PTS, 0, c.info["m"], c.info["spacing"], c.info["halo"])
    ovf, short, tb, b, base = L.union_ranges()
    tile = np.arange(L.C) // UNT == 2
    sel = tile & (tb - base == d) & (tb < b)
    assert sel.sum() > 4
    if d < 0:
        assert short[sel].any() and ovf[sel].any() and not (short & ovf).any()
    else:
        assert not short[sel].any() and not ovf[sel].any()


@pytest.mark.parametrize("name", LC.names("ladder_tile"))
def test_ladder_line_begins_at_a_tile_edge(name):
    c = LC.get(name)
    d = c.info["pad"] + c.info["m"] - 2 * UNT
    assert d in (-1, 0, 1)
    L = _ladder_checks(name, LC.LADDER_MIN_PTS, 0, c.info["m"], c.info["spacing"], c.info["halo"])
    first = np.flatnonzero((c.kind[L.crow] == LC.K_LINE) & (c.grp[L.crow] == 1))[0]
    assert first == 2 * UNT + d and L.open[first]


@pytest.mark.parametrize("name", LC.names("ladder_link"))
def test_ladder_link(name):
    """the sizes at the halo's edge in the form in which the answer hangs on the overflow list: the three cores that link the two
    strips are the first of a tile and overflow (m > halo); without their edges the strips are two clusters.  m = halo: the strip
    below begins exactly at the first staged core, nothing overflows (control)"""
    c = LC.get(name)
    m, halo = c.info["m"], c.info["halo"]
    for v in VARIANTS:
        L = layout(name, v, LC.LADDER_MIN_PTS, 0)
        lab = labels(name, v, LC.LADDER_MIN_PTS, 0)
        assert L.halo == halo
        full, ei, ej = check_core_model(L, lab)
        ovf, short, tb, b, base = L.union_ranges()
        line = [np.flatnonzero((c.grp[L.crow] == s) & np.isin(c.kind[L.crow], (LC.K_LINE, LC.K_WALL, LC.K_HIT))) for s in (0, 1)]
        first = line[1][0]
        assert len(line[0]) == len(line[1]) == m and first == 2 * UNT and tb[first] == line[0][0] == first - m and base[first] == first - halo
        src = np.unique(ei[np.isin(ei, line[1])])
        A = line[0][LC.LINK_WALL]
        assert c.kind[L.crow[A]] == LC.K_HIT and L.cp[first] - L.cp[A] == EPS and L.cq[first] == L.cq[A]
        assert np.array_equal(src, line[1][:3]) and (ej[np.isin(ei, src)] == A).all() and not short[src].any()
        # the walk of the line's first core passes the 20 cores in front of A: rounds of 4 (staged) or 8 (overflow) candidates
        lo = L.cross_edges()[2]
        assert lo[first] == line[0][0] and A - lo[first] == LC.LINK_WALL > 2 * OVF_ROUND
        assert len(np.unique(lab[L.crow[np.concatenate(line)]])) == 2 and lab[L.crow[A]] == lab[L.crow[line[1][-1]]]
        drop = ovf[ei]
        if m > halo:
            assert ovf[src].all() and not same_partition(L.components(ei[~drop], ej[~drop]), lab[L.crow]), v
        else:
            assert not ovf.any()


# ---- broken ladder ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.names("broken_ladder"))
def test_broken_ladder(name):
    c = LC.get(name)
    for v in VARIANTS:
        L = layout(name, v, LC.LADDER_MIN_PTS, 0)
        lab = labels(name, v, LC.LADDER_MIN_PTS, 0)
        assert L.halo == c.info["halo"]
        full, ei, ej = check_core_model(L, lab)
        link = np.sort(np.searchsorted(L.cpos, L.pos_of_row[c.info["link"]]))
        assert (L.core[L.pos_of_row[c.info["link"]]]).all() and link[0] == 4 * UNT + c.info["d"] and (np.diff(link) == 1).all()
        assert L.open[link[0]] and L.nexthead[link[0]] == link[-1] + 1                     # a chain of their own
        # the long strip below begins in front of the staged cores of the link's tile: overflow list; the short one is staged
        assert L.union_ranges()[0][link].all() == (c.info["m"] > HALO_BIG) and L.union_ranges()[0][link].any() == (c.info["m"] > HALO_BIG)
        pairs = np.unique(np.stack([ei, L.head[ej]], 1), axis=0)
        touched = np.bincount(pairs[:, 0], minlength=L.C)
        assert (touched[link] == 2).all() and touched.max() == 2
        # strip 2 holds two chains; the tail of the first and the head of the second are doubled positions
        dup = L.pos_of_row[np.flatnonzero((c.kind == LC.K_LINE) & (c.grp == 10))]
        dq = np.sort(L.q[dup])
        for qd, is_tail in ((dq[0], True), (dq[1], False)):
            k = np.flatnonzero((L.cq == qd) & (L.cs == L.s[dup[0]]))
            assert len(k) == 2 and k[1] == k[0] + 1
            assert L.open[k[1] + 1] if is_tail else L.open[k[0]]
        # sensitivity: the second chain of a window is not united (every core keeps the first chain it touches)
        keep = np.ones(len(ei), bool)
        order = np.lexsort((ej, ei))
        first_chain = {}
        for t in order:
            i, h = int(ei[t]), int(L.head[ej[t]])
            first_chain.setdefault(i, h)
            keep[t] = first_chain[i] == h
        assert not keep.all() and not same_partition(L.components(ei[keep], ej[keep]), lab[L.crow]), v
        one = lab[L.crow[c.kind[L.crow] == LC.K_LINE]]
        assert len(np.unique(one)) == 1


# ---- cell across a tile -----------------------------------------------------------------------------------------------------------
def _cell_keys(L, lab, limit=None):
    """variant 2's key of every cluster: the smallest row of any PET of a rotated cell that holds one of its cores; limit(head
    position) -> the first position a truncated minimum no longer sees"""
    cellid = np.concatenate([[0], np.cumsum((L.s[1:] != L.s[:-1]) | (L.q[1:] // EPS != L.q[:-1] // EPS))])
    heads = np.searchsorted(cellid, np.arange(cellid[-1] + 1))
    rows = L.row.astype(np.int64).copy()
    if limit is not None:
        rows[np.arange(L.n) >= limit(heads[cellid])] = np.iinfo(np.int64).max
    cmin = np.minimum.reduceat(rows, heads)
    keys = {}
    for k in np.flatnonzero(L.core):
        l = int(lab[L.row[k]])
        keys[l] = min(keys.get(l, np.iinfo(np.int64).max), int(cmin[cellid[k]]))
    return keys


@pytest.mark.parametrize("name", LC.names("cell_tile"))
def test_cell_across_a_tile(name):
    c = LC.get(name)
    k, where = c.info["k"], c.info["where"]
    L = layout(name, "v2", LC.CELL_MIN_PTS, 0)
    lab = labels(name, "v2", LC.CELL_MIN_PTS, 0)
    pos = np.sort(L.pos_of_row[c.info["cell"]])
    # one rotated cell of 300 PETs, all core, from position LT - k on: k PETs in the first tile, 300 - k behind it
    assert len(pos) == LC.CELL_N > L_HALO and pos[0] == LT - k and (np.diff(pos) == 1).all()
    assert len(np.unique(L.s[pos])) == 1 and len(np.unique(L.q[pos] // EPS)) == 1 and L.core[pos].all()
    assert (L.p[pos] // EPS == L.p[pos[0]] // EPS).all()
    assert L.row[pos[0] if where == "first" else pos[-1]] == 0 and (pos >= LT).sum() == LC.CELL_N - k
    lc, lo = int(lab[c.info["cell"][0]]), int(lab[c.info["other"][0]])
    assert (lab[c.info["cell"]] == lc).all() and (lab[c.info["other"]] == lo).all() and {lc, lo} == {0, 1}
    # the model's keys order the labels
    keys = _cell_keys(L, lab)
    assert sorted(keys, key=keys.get) == sorted(keys) and lc == 0
    tile_only = _cell_keys(L, lab, lambda h: (h // LT + 1) * LT)
    with_halo = _cell_keys(L, lab, lambda h: (h // LT + 1) * LT + L_HALO)
    if where == "last":
        # the minimum over the first tile's part alone -- and over tile + halo, where the cell runs on behind the halo -- puts the
        # other cluster first
        assert tile_only[lc] > tile_only[lo]
        assert (with_halo[lc] > with_halo[lo]) == (LC.CELL_N - k > L_HALO)
    else:
        # (control: the smallest row sits in the first tile, a truncated minimum is the same)
        assert tile_only == keys and with_halo == keys


# ---- walkers ----------------------------------------------------------------------------------------------------------------------
def _walker_model_matches(L, lab, rows):
    for r in rows:
        pos = L.pos_of_row[r]
        assert L.walker[pos]
        assert L.owner_v2(pos, lab) == lab[r], r


def _queued(L, pos):
    """does k_border_q's pass 0 leave a walk of this walker open (it then asks for a queue entry)"""
    return L.walk(pos, -1, KCAP)[1] or L.walk(pos, 1, KCAP)[1]


@pytest.mark.parametrize("name", LC.names("miss_wall"))
def test_miss_wall(name):
    c = LC.get(name)
    k, m, align = c.info["k"], c.info["min_pts"], c.info["align"]
    up, down = c.info["walkers"]
    for v in VARIANTS:
        L = layout(name, v, m, 0)
        lab = labels(name, v, m, 0)
        wall = L.pos_of_row[np.flatnonzero(np.isin(c.kind, (LC.K_WALL, LC.K_HIT)))]
        assert L.core[wall].all()
        pu, pd = L.pos_of_row[up], L.pos_of_row[down]
        assert pd == pu + 1 and L.s[pu] == L.s[pd]
        if align == "edge":
            assert pu % BNT == BNT - 1 and pu % BNQ == BNQ - 1
        else:
            assert 256 < pu % BNQ < BNQ - 256
        for pos, side in ((pu, 1), (pd, -1)):
            # the walker's only neighbour is h: count 2; exactly k misses in front of it, nothing in the other strip or its own
            assert L.cnt[pos] == 2 and L.walker[pos] and lab[L.row[pos]] >= 0
            seen, _, misses = L.walk(pos, side)
            assert len(seen) == 1 and misses == k and c.kind[L.crow[seen[0]]] == LC.K_HIT
            assert L.cp[seen[0]] - L.p[pos] == side * EPS and L.cq[seen[0]] - L.q[pos] == EPS
            assert L.walk(pos, -side)[0] == [] and L.own_strip(pos) == []
            assert max(L.hints(pos)) < K2H_MASK               # (hinted at minPts 5; at minPts 129 no walker has hints)
            j0 = L.window(pos, side)[0]
            for NT, HC in ((BNQ, BHQ), (BNT, BHC)):
                clo, chi = L.staged_q(pos, NT, HC)
                if align == "edge" and k >= 255:
                    # h (up) / the walk's first core (down) lie outside the staged cores: global memory
                    assert seen[0] + 1 >= chi if side > 0 else j0 < clo
                elif k <= 33:
                    assert clo <= j0 and seen[0] + 1 < chi
            # sensitivity: a walk that ends after KCAP steps of 2 candidates finds nothing behind 4 misses and more
            cut_short = L.owner_v2(pos, lab, KCAP) if v == "v2" else (-1 if not L.walk(pos, side, KCAP)[0] else lab[L.row[pos]])
            assert (cut_short != lab[L.row[pos]]) == (k >= 2 * KCAP), (v, side)
            assert _queued(L, pos) or k < 2 * KCAP
        if v == "v2":
            _walker_model_matches(L, lab, (up, down))


def test_wall_sizes_straddle_the_steps():
    """the sizes of the miss walls lie on both sides of: the 2 x 2 candidates of pass 0; a round of BQ_G lanes of the queue's walk,
    which begins where pass 0 stopped; the cores of halo"""
    K = set(LC.WALL_K)
    assert {2 * KCAP - 1, 2 * KCAP, 2 * KCAP + 1} <= K
    assert {2 * KCAP + BQ_G - 1, 2 * KCAP + BQ_G, 2 * KCAP + BQ_G + 1} <= K and {BQ_G - 1, BQ_G, BQ_G + 1, 2 * BQ_G + 1} <= K
    assert max(k for k in K if k <= BHQ) < BHQ // 2 and BHQ + 1 in K and max(K) > BHC


@pytest.mark.parametrize("name", LC.names("wall_population"))
def test_wall_population_drops_the_hints(name):
    c = LC.get(name)
    side = c.info["side"]
    (w,) = c.info["walkers"]
    for v in VARIANTS:
        L = layout(name, v, 5, 0)
        lab = labels(name, v, 5, 0)
        pos = L.pos_of_row[w]
        da, db = L.hints(pos)
        assert (db if side > 0 else da) > K2H_MASK and (da if side > 0 else db) < K2H_MASK and max(da, db) < 0xffff
        assert L.cnt[pos] == 2 and L.walker[pos] and lab[w] >= 0 and L.walk(pos, side)[2] == 5
        assert L.walk(pos, side, KCAP)[0] == []
    _walker_model_matches(layout(name, "v2", 5, 0), labels(name, "v2", 5, 0), [w])


@pytest.mark.parametrize("name", LC.names("corners") + LC.names("corners_wall"))
def test_four_corners(name):
    c = LC.get(name)
    m = LC.CORNER_MIN_PTS
    lab2, lab1 = labels(name, "v2", m, 0), labels(name, "v1", m, 0)
    L = layout(name, "v2", m, 0)
    _walker_model_matches(L, lab2, c.info["walkers"])
    for u, w in enumerate(c.info["walkers"]):
        pos = L.pos_of_row[w]
        groups = [np.flatnonzero((c.kind == LC.K_CORNER) & (c.grp == 4 * u + d)) for d in range(4)]
        assert L.cnt[pos] == 5 and all(len(g) == 6 and L.core[L.pos_of_row[g]].all() for g in groups)
        ls = [int(lab2[g[0]]) for g in groups]
        assert len(set(ls)) == 4 and all((lab2[g] == l).all() for g, l in zip(groups, ls))
        assert lab2[w] == min(ls) and lab1[w] in [int(lab1[g[0]]) for g in groups]
        # after KCAP steps of both walks the walker holds four components and both walks are still open
        below, above = L.walk(pos, -1, KCAP), L.walk(pos, 1, KCAP)
        if not c.info.get("k"):
            assert len(below[0]) == 2 and len(above[0]) == 2 and below[1] and above[1] and L.own_strip(pos) == []
    w = c.info["walkers"][0]
    pos = L.pos_of_row[w]
    if c.info.get("tile"):
        T, at = c.info["tile"]
        assert pos % T == (T + at) % T
        assert layout(name, "v1", m, 0).pos_of_row[w] == pos
    if "k" in c.info:
        # the component behind the wall owns the walker; a walk that ends after KCAP steps does not get there
        assert lab2[w] == lab2[c.info["owner"][0]] and L.walk(pos, 1)[2] == 0
        assert L.owner_v2(pos, lab2, KCAP) not in (-1, int(lab2[w]))
        assert _queued(L, pos) and len(L.walk(pos, 1, KCAP)[0]) == 1
    else:
        # the answer depends on the variant and on the row order: taking the first component seen is not enough
        assert any(lab1[x] != lab2[x] for x in c.info["walkers"]) or c.info["order"] == 1
        other = LC.get("corners(%d)" % (1 - c.info["order"]))
        lo = labels("corners(%d)" % (1 - c.info["order"]), "v2", m, 0)
        mine = [d for d in range(4) if lab2[np.flatnonzero((c.kind == LC.K_CORNER) & (c.grp == d))[0]] == lab2[w]]
        theirs = [d for d in range(4) if lo[np.flatnonzero((other.kind == LC.K_CORNER) & (other.grp == d))[0]] == lo[other.info["walkers"][0]]]
        assert mine != theirs


# ---- crowded walker tile ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.names("crowded"))
def test_crowded_tile(name):
    c = LC.get(name)
    m = LC.CROWD_MIN_PTS
    ws = c.info["walkers"]
    for v in VARIANTS:
        L = layout(name, v, m, 0)
        lab = labels(name, v, m, 0)
        pos = np.sort(L.pos_of_row[ws])
        assert L.walker[pos].all() and (lab[ws] >= 0).all() and len(np.unique(pos // BNQ)) == 1 and pos[0] % BNQ == c.info["at"]
        t0 = (pos[0] // BNQ) * BNQ
        in_tile = np.arange(t0, t0 + BNQ)
        nwalk, ncore = int(L.walker[in_tile].sum()), int(L.core[in_tile].sum())
        assert nwalk > 256 and ncore >= 400 and nwalk + ncore >= 1000
        clo, chi = L.staged_q(pos[0])
        qbase = (chi - clo + 1) & ~1
        qcap = (BNQ + 2 * BHQ - qbase) >> 1
        queued = sum(_queued(L, p) for p in pos)
        assert chi - clo >= ncore + BHQ and 0 < qcap < queued, (qcap, queued)
        # every walker has 4 misses or more in front of its first hit
        assert min(L.walk(p, 1)[2] for p in pos) >= 2 * KCAP
        if v == "v2":
            _walker_model_matches(L, lab, ws[::7])
            assert all(L.owner_v2(p, lab, KCAP) == -1 for p in pos[::7])


# ---- under a cut ------------------------------------------------------------------------------------------------------------------
def test_cut_ladder():
    name = "cut_ladder()"
    c = LC.get(name)
    assert c.runs == ((LC.LADDER_MIN_PTS, 0), (LC.LADDER_MIN_PTS, LC.CUT))
    _ladder_checks(name, LC.LADDER_MIN_PTS, LC.CUT, c.info["m"], EPS, c.info["halo"])
    L0, L1 = layout(name, "v2", LC.LADDER_MIN_PTS, 0), layout(name, "v2", LC.LADDER_MIN_PTS, LC.CUT)
    # the cut removes PETs from the front of every strip of the ladder and of the strips in front of it
    removed = np.bincount(L0.s, minlength=L0.S) - np.bincount(L1.s, minlength=L0.S)
    assert (removed[:8] == LC.CUT_SHORT).all() and L1.n == L0.n - 8 * LC.CUT_SHORT
    check_core_model(L0, labels(name, "v2", LC.LADDER_MIN_PTS, 0))


def test_cut_wall():
    name = "cut_wall()"
    c = LC.get(name)
    up, down = c.info["walkers"]
    k = c.info["k"]
    for v in VARIANTS:
        L0, L1 = layout(name, v, 5, 0), layout(name, v, 5, LC.CUT)
        lab = labels(name, v, 5, LC.CUT)
        removed = np.bincount(L0.s, minlength=L0.S) - np.bincount(L1.s, minlength=L0.S)
        for w, side in ((up, 1), (down, -1)):
            p0, p1 = L0.pos_of_row[w], L1.pos_of_row[w]
            s = L1.s[p1]
            assert L1.walker[p1] and L1.cnt[p1] == 2 and lab[w] >= 0 and L1.walk(p1, side)[2] == k
            # the hints were made on the layout of cut 0: they shift by what the cut removes from the walker's own strip (dA)
            # and from the strip above (dB), both non-zero
            dA, dB = removed[s], removed[s + 1]
            assert dA == dB == LC.CUT_SHORT
            (a0, b0), (a1, b1) = L0.hints(p0), L1.hints(p1)
            assert a0 - a1 == dA and b0 - b1 == dB and max(a0, b0) < K2H_MASK
        # sensitivity: with the hint ahead unshifted the walk of the walker that looks up begins dB positions behind its window's
        # start -- behind h and its supports: nothing found
        p1 = L1.pos_of_row[up]
        start = min(p1 + L0.hints(L0.pos_of_row[up])[1], L1.n)
        j0, j1 = L1.window(p1, 1)
        assert L1.rank[start] >= j1 > j0 + k
    _walker_model_matches(layout(name, "v2", 5, LC.CUT), labels(name, "v2", 5, LC.CUT), (up, down))
    _walker_model_matches(layout(name, "v2", 5, 0), labels(name, "v2", 5, 0), (up, down))
