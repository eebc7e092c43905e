"""CPU only: every case of tests/block_cases.py gets the same labels from the three CPU implementations of blockDBSCAN (the C oracle,
the numpy closed form, the reference's own class where it is present), has the outcome it claims, and the rule it aims at matters
for the answer: the closed form with that one rule changed (the keyword arguments of closed_form_model.labels_block) gives other
labels on the family.  Where a size list includes values at which the rule cannot matter (eps 1 and 2, nyb 2 and 3) the case is a
control and the test says so."""
import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import block_cases as BC
import closed_form_model as CFM
import oracle
import refload

_lab = {}


def kept(X, Y, cut):
    return np.flatnonzero(Y - X >= cut) if cut > 0 else np.arange(len(X))


def labels(name, perm_name, m, cut):
    """the oracle's labels of one run under one row permutation, -1 at the rows the cut removes (oracle.single_dbscan)"""
    key = (name, perm_name, m, cut)
    if key not in _lab:
        c = BC.get(name)
        X, Y = next((X, Y) for pn, X, Y, _ in BC.permuted(c) if pn == perm_name)
        _lab[key] = oracle.single_dbscan("block", X, Y, c.eps, m, cut)["labels"]
    return _lab[key]


def model(name, perm_name, m, cut, **rule):
    c = BC.get(name)
    X, Y = next((X, Y) for pn, X, Y, _ in BC.permuted(c) if pn == perm_name)
    keep = kept(X, Y, cut)
    out = np.full(len(X), -1, np.int32)
    if len(keep):
        out[keep] = CFM.labels_block(X[keep], Y[keep], c.eps, m, **rule)
    return out


def settings(name):
    c = BC.get(name)
    return [(pn, m, cut) for pn, _, _, _ in BC.permuted(c) for m, cut in c.runs]


def differs_somewhere(name, **rule):
    return any(not np.array_equal(model(name, pn, m, cut, **rule), labels(name, pn, m, cut)) for pn, m, cut in settings(name))


# ---- three implementations ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BC.names())
def test_oracle_and_closed_form_agree(name):
    c = BC.get(name)
    assert max(abs(c.X).max(), abs(c.Y).max()) < BC.LIM and len(c.X) <= 6000
    for pn, m, cut in settings(name):
        assert np.array_equal(model(name, pn, m, cut), labels(name, pn, m, cut)), (pn, m, cut)


@pytest.mark.skipif(not refload.available(), reason="the reference checkout is not present")
@pytest.mark.parametrize("name", BC.names())
def test_reference_class_agrees(name):
    c = BC.get(name)
    for pn, X, Y, _ in BC.permuted(c):
        for m, cut in c.runs:
            keep = kept(X, Y, cut)
            got = np.full(len(X), -1, np.int32)
            mat = np.stack([keep, X[keep], Y[keep]], 1).astype(np.int64)
            got[keep] = refload.labels_dict_to_array(refload.ref_labels("block", mat, c.eps, m), keep)
            assert np.array_equal(got, labels(name, pn, m, cut)), (pn, m, cut)


# ---- the claimed outcomes -------------------------------------------------------------------------------------------------------
def _expected(sub, m, cut):
    e = sub.get("expect", {})
    return e[(m, cut)] if (m, cut) in e else e.get(m) if cut == 0 else None


@pytest.mark.parametrize("name", BC.names())
def test_every_sub_case_has_the_outcome_it_claims(name):
    c = BC.get(name)
    claims = 0
    for pn, X, Y, p in BC.permuted(c):
        sub = c.info["sub"][p]
        for m, cut in c.runs:
            lab = labels(name, pn, m, cut)
            assert (lab[sub < 0] == -1).all() or name in ("cut_anchor", "components"), (pn, m, cut)     # anchors are noise
            for k, s in enumerate(c.info["subs"]):
                want = _expected(s, m, cut)
                rows = lab[sub == k]
                if want == "one":
                    assert rows[0] >= 0 and (rows == rows[0]).all() and (lab == rows[0]).sum() == len(rows), (pn, m, cut, s)
                elif want == "noise":
                    assert (rows == -1).all(), (pn, m, cut, s)
                claims += want is not None
    assert claims or name in ("border_rank", "components")


def test_sub_cases_lie_four_cells_apart():
    """PETs of different sub-cases (and the anchor) are more than 4 eps apart along one axis at least -- the dense `components`
    excepted, whose cells are its sub-cases, and `cut_anchor`, which has one grid per cut and places its pairs by hand"""
    for name in BC.names():
        if name in ("components", "cut_anchor"):
            continue
        c = BC.get(name)
        sub = c.info["sub"].copy()
        if name == "core_threshold":                             # the neighbour out of reach belongs to its variant
            sub = np.asarray([c.info["subs"][k]["v"] if k >= 0 else -1 for k in sub])
        if name.startswith("row_wrap"):                          # the two cells of an arrangement belong together
            sub = np.asarray([("top", "bottom").index(c.info["subs"][k]["first"]) if k >= 0 else -1 for k in sub])
        far = 4 * c.eps
        if len(c.X) == 3:                                        # a set of its own around eps = 2^28: the domain is 3 or 4 cells wide,
            far = c.eps                                          # the anchor lies in a cell that is no neighbour of the pair's
            nx, ny = (c.X - c.X.min()) // c.eps, (c.Y - c.Y.min()) // c.eps
            a = int(np.flatnonzero(sub < 0)[0])
            assert all(max(abs(nx[i] - nx[a]), abs(ny[i] - ny[a])) >= 2 for i in np.flatnonzero(sub >= 0)), name
        order = np.argsort(c.X, kind="stable")
        X, Y, sub = c.X[order], c.Y[order], sub[order]
        lo = np.searchsorted(X, X - far, "left")
        for i in range(len(X)):
            near = np.arange(lo[i], i)
            near = near[(abs(Y[near] - Y[i]) <= far) & ((sub[near] != sub[i]) | (sub[i] < 0))]
            assert len(near) == 0, (name, i)


# ---- cell_edge ------------------------------------------------------------------------------------------------------------------
def _edge_groups():
    return sorted({n.split("_")[2] for n in BC.names("cell_edge")}, key=int)


def test_cell_edge_sizes():
    assert [int(e) for e in _edge_groups()] == sorted(BC.CELL_EDGE_EPS)
    whole = [n for n in BC.names("cell_edge") if BC.get(n).info["whole_domain"]]
    assert whole and all(BC.get(n).X.min() == -(BC.LIM - 1) for n in whole)
    top = max(int(max(BC.get(n).X.max(), BC.get(n).Y.max())) for n in whole)
    assert top > BC.LIM - 1 - 2048                               # the offsets that are divided reach (nearly) 2^30
    for n in BC.names("cell_edge"):
        c = BC.get(n)
        assert (c.X.max() - c.X.min()) // c.eps <= 1 << 20       # the cell-row table stays small


@pytest.mark.parametrize("eps", BC.CELL_EDGE_EPS)
def test_cell_edge_depends_on_the_boundary(eps):
    for name in [n for n in BC.names("cell_edge") if int(n.split("_")[2]) == eps]:
        c = BC.get(name)
        kinds = {s["kind"] for s in c.info["subs"]}
        assert kinds <= {"together", "split"}
        if eps < 3:
            continue                                             # (control: a cell of 1 or 2 base pairs has no room for the pair)
        X, Y = c.X - c.X.min(), c.Y - c.Y.min()
        for k, s in enumerate(c.info["subs"]):
            rows = np.flatnonzero(c.info["sub"] == k)
            u = (X if s["axis"] == 0 else Y)[rows]
            v = (Y if s["axis"] == 0 else X)[rows]
            assert abs(u[1] - u[0]) + abs(v[1] - v[0]) == 2 * eps - 2 and len(np.unique(v // eps)) == 1
            if s["kind"] == "together":
                assert sorted(u % eps) == [0, eps - 1] and len(np.unique(u // eps)) == 1 and u[0] // eps == s["k"]
            else:
                assert sorted(u % eps) == [eps - 2, eps - 1] and sorted(u // eps) == [s["k"] - 1, s["k"]]
        for axis in sorted({s["axis"] for s in c.info["subs"]}):
            for shift in (1, -1):
                if shift == -1 and kinds == {"split"}:
                    continue                                     # (a lone split pair stays split when the boundary moves up)
                got = CFM.labels_block(c.X, c.Y, eps, 2, cell_shift=(shift, 0) if axis == 0 else (0, shift))
                assert not np.array_equal(got, labels(name, "as_built", 2, 0)), (name, axis, shift)


# ---- row_wrap -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nyb", (1, 2, 3))
def test_row_wrap(nyb):
    name = "row_wrap_%d" % nyb
    c = BC.get(name)
    top = (1 << nyb) - 1
    assert (c.Y.max() - c.Y.min()) // c.eps == top               # k_blk's nyb = bits_for(that) = nyb
    nx, ny = (c.X - c.X.min()) // c.eps, (c.Y - c.Y.min()) // c.eps
    key = np.unique((nx << nyb) | ny)
    for r in c.info["rows"]:
        a, b = (r << nyb) | top, ((r + 1) << nyb) | 0
        assert b == a + 1 and a in key and b in key              # consecutive sort keys, both occupied, two PETs each
        assert ((nx == r) & (ny == top)).sum() == 2 and ((nx == r + 1) & (ny == 0)).sum() == 2
    wrapped = differs_somewhere(name, wrap_nyb=nyb)
    if nyb == 1:
        # the answer hangs on counting (r + 1, 0) once: as a same-row neighbour too it makes both cells core at minPts 5
        got = model(name, "as_built", 5, 0, wrap_nyb=1)
        assert wrapped and (got[c.info["sub"] >= 0] >= 0).all() and (labels(name, "as_built", 5, 0) == -1).all()
    else:
        assert not wrapped                                       # (control: the two cells are too far apart to be linked)


# ---- centroid_tie ---------------------------------------------------------------------------------------------------------------
def test_centroid_tie():
    from fractions import Fraction as F
    c = BC.get("centroid_tie")
    seen = set()
    for k, s in enumerate(c.info["subs"]):
        rows = np.flatnonzero(c.info["sub"] == k)
        X, Y = c.X[rows], c.Y[rows]
        cell = ((X - c.X.min()) // c.eps) * (1 << 32) + (Y - c.Y.min()) // c.eps
        ids = np.unique(cell)
        A, B = rows[cell == ids[0]], rows[cell == ids[1]]
        a, b = s["pops"]
        assert len(ids) == 2 and (len(A), len(B)) == (a, b)
        cen = [(F(int(c.X[g].sum()), len(g)), F(int(c.Y[g].sum()), len(g))) for g in (A, B)]
        d = abs(cen[0][0] - cen[1][0]) + abs(cen[0][1] - cen[1][1])
        lcm = a * b // np.gcd(a, b)
        assert d == (c.eps + F(1, lcm) if s["kind"] == "step" else c.eps), s
        pd = np.abs(c.X[A][:, None] - c.X[B][None, :]) + np.abs(c.Y[A][:, None] - c.Y[B][None, :])
        if (a, b) == (1, 1):
            assert pd.min() == d                                 # (the centroids are the PETs: no arrangement without a pair at eps)
        else:
            assert pd.min() > c.eps
        assert abs(int(c.X[A].sum())) > 2 ** 29 or a == 1        # the sums leave int32
        seen.add((s["pops"], s["kind"], s["end"]))
    assert len(seen) == 2 * 2 * len(BC.TIE_POPS)
    assert c.X.min() == c.Y.min() == -(BC.LIM - 1) and min(c.X.max(), c.Y.max()) > BC.LIM - 100 * c.eps
    # the rule: without the centroid test, or with a strict one, the ties are not linked
    for rule in ("lt", "off"):
        for m, cut in c.runs:
            got = model("centroid_tie", "as_built", m, cut, centroid=rule)
            for k, s in enumerate(c.info["subs"]):
                if sum(s["pops"]) == m and s["kind"] == "tie" and s["pops"] != (1, 1):
                    assert (got[c.info["sub"] == k] == -1).all(), (rule, s)


# ---- pair_loop ------------------------------------------------------------------------------------------------------------------
def test_pair_loop():
    c = BC.get("pair_loop")
    nx, ny = c.X // c.eps, c.Y // c.eps
    tail_hits, residues, dirs = 0, set(), set()
    for k, s in enumerate(c.info["subs"]):
        rows = np.flatnonzero(c.info["sub"] == k)                # ascending rows: the order inside a cell
        cell = nx[rows] * (1 << 32) + ny[rows]
        ids = np.unique(cell)                                    # ascending (nx, ny): the first is the cell whose thread tests the pair
        A, B = rows[cell == ids[0]], rows[cell == ids[1]]
        na, nb = s["pops"]
        assert (len(A), len(B)) == (na, nb)
        assert (int(nx[B[0]] - nx[A[0]]), int(ny[B[0]] - ny[A[0]])) == s["dir"]
        pd = np.abs(c.X[A][:, None] - c.X[B][None, :]) + np.abs(c.Y[A][:, None] - c.Y[B][None, :])
        want = c.eps + (1 if s["kind"] == "apart" else 0)
        ia, ib = np.argwhere(pd <= c.eps + 1)[0]
        assert (pd <= c.eps + 1).sum() == 1 and pd[ia, ib] == want and (ia, ib) == s["pos"] and np.sort(pd.ravel())[1:].min(initial=9999) > c.eps + 200
        dc = abs(c.X[A].mean() - c.X[B].mean()) + abs(c.Y[A].mean() - c.Y[B].mean())
        assert dc > c.eps or (na, nb) == (1, 1)
        inner, pos = (na, ia) if na > nb else (nb, ib)           # the larger cell is walked inside, the later one on a tie
        residues.add((int(pos) % 4, pos >= inner - inner % 4))
        dirs.add(s["dir"])
        if s["kind"] == "at_eps" and pos >= inner - inner % 4 and (na, nb) != (1, 1):
            tail_hits += 1
    assert {r for r, _ in residues} == {0, 1, 2, 3} and {(r, True) for r in (0, 1, 2)} <= residues and {(r, False) for r in range(4)} <= residues
    assert dirs == set(BC.DIRS[4:]) and tail_hits >= 20
    assert {(1, 64), (65, 3), (130, 129)} <= {s["pops"] for s in c.info["subs"]}
    # the rule: a walk in fours without its tail misses the pairs whose PET of the larger cell lies in the tail
    missed = 0
    for m, cut in c.runs:
        got, want = model("pair_loop", "as_built", m, cut, pair_tail=False), labels("pair_loop", "as_built", m, cut)
        missed += int((got != want).any())
    assert missed >= 10


# ---- core_threshold -------------------------------------------------------------------------------------------------------------
def test_core_threshold():
    c = BC.get("core_threshold")
    nx, ny = c.X // c.eps, c.Y // c.eps
    for v in range(8):
        linked = next(k for k, s in enumerate(c.info["subs"]) if s["kind"] == "linked" and s["v"] == v)
        out = next(k for k, s in enumerate(c.info["subs"]) if s["kind"] == "unlinked" and s["v"] == v)
        rows = np.flatnonzero(np.isin(c.info["sub"], (linked, out)))
        cx, cy = 8 * v + 6, 6
        pops = {}
        for q, (dx, dy) in enumerate(BC.DIRS):
            sel = rows[(nx[rows] == cx + dx) & (ny[rows] == cy + dy)]
            pops[q] = len(sel)
            centre = rows[(nx[rows] == cx) & (ny[rows] == cy)]
            pd = np.abs(c.X[sel][:, None] - c.X[centre][None, :]) + np.abs(c.Y[sel][:, None] - c.Y[centre][None, :])
            dc = abs(c.X[sel].mean() - c.X[centre].mean()) + abs(c.Y[sel].mean() - c.Y[centre].mean())
            assert (pd.min() > c.eps and dc > c.eps) if q == v else pd.min() <= c.eps
            assert (c.info["sub"][sel] == (out if q == v else linked)).all()
        assert pops == {q: q + 2 for q in range(8)} and len(centre) == 4
        assert c.info["subs"][linked]["psum"] == 4 + sum(pops.values()) - pops[v]
    # (the neighbours' populations differ, so the sum tells which directions were counted: a link bit set for direction q of the
    # neighbour instead of 7 - q leaves the centre with the populations of directions 4 .. 7 at most)


# ---- border_rank ----------------------------------------------------------------------------------------------------------------
def test_border_rank():
    c = BC.get("border_rank")
    m = BC.BORDER_MIN_PTS
    highest = {"two": set(), "three": set()}
    for pn, X, Y, p in BC.permuted(c):
        lab = labels("border_rank", pn, m, 0)
        role, sub = c.info["role"][p], c.info["sub"][p]
        for k, s in enumerate(c.info["subs"]):
            comps = [np.flatnonzero((sub == k) & (role == 2 + j)) for j in range(s["ncomp"])]
            ls = [int(lab[r[0]]) for r in comps]
            assert all((lab[r] == l).all() and l >= 0 for r, l in zip(comps, ls)) and len(set(ls)) == s["ncomp"]      # `bridge`: they stay apart
            first = [int(r.min()) for r in comps]
            assert np.array_equal(np.argsort(first), np.argsort(ls))                   # ranks by the smallest row of the core cells
            b = np.flatnonzero((sub == k) & (role == 1))
            assert len(b) == 1 and lab[b[0]] == max(ls)
            highest[s["kind"]].add(int(np.argmax(ls)))
            if b[0] == 0:
                assert pn in ("border_row_0", "two_border_row_0")
    assert highest == {"two": {0, 1}, "three": {0, 1, 2}}
    assert differs_somewhere("border_rank", border="min")
    # with the border PET on row 0 its component's earliest row belongs to a non-core cell
    for pn in ("border_row_0", "two_border_row_0"):
        assert not np.array_equal(model("border_rank", pn, m, 0, rank_over="all"), labels("border_rank", pn, m, 0)), pn
    assert np.array_equal(model("border_rank", "border_last", m, 0, rank_over="all"), labels("border_rank", "border_last", m, 0))


# ---- components -----------------------------------------------------------------------------------------------------------------
def test_components():
    c = BC.get("components")
    cells, comp = c.info["cells"], c.info["comp"]
    n = len(cells)
    assert (c.X == cells[:, 0] * c.eps).all() and (c.Y == cells[:, 1] * c.eps).all()
    # the components as built are the connected components of orthogonal adjacency
    lut = {(int(a), int(b)): i for i, (a, b) in enumerate(cells)}
    ei, ej = [], []
    for (a, b), i in lut.items():
        for d in ((1, 0), (0, 1)):
            j = lut.get((a + d[0], b + d[1]))
            if j is not None:
                ei.append(i)
                ej.append(j)
    cc = connected_components(coo_matrix((np.ones(len(ei)), (ei, ej)), shape=(n, n)), directed=False)[1]
    sizes = np.bincount(cc)
    for k in range(comp.max() + 1):
        sel = comp == k
        assert len(np.unique(cc[sel])) == 1 and sizes[cc[sel][0]] == sel.sum()
    assert (sizes[cc[comp < 0]] == 1).all()
    order = c.info["perms"]["cell_order"]
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)                                    # the index of every cell in cell order
    by_size = {int((comp == k).sum()) for k in range(comp.max() + 1)}
    assert set(BC.COLUMN_LENGTHS + BC.ROW_LENGTHS) - {1} <= by_size and max(by_size) >= 3000
    serp = np.flatnonzero(comp == np.argmax(np.bincount(comp[comp >= 0])))
    assert len(np.unique(pos[serp] // BC.WG)) >= 3               # the serpentine crosses workgroups
    run = np.sort(pos[np.isin(comp, np.flatnonzero(np.bincount(comp[comp >= 0]) == BC.RUN_LEN)[-BC.RUN_COUNT:])])
    assert run[0] == c.info["run_first"] and run[0] % BC.WG == 0 and len(run) == BC.WG and run[-1] - run[0] == BC.WG - 1
    where, monotone = set(), {}
    for pn, X, Y, p in BC.permuted(c):
        lab = labels("components", pn, 2, 0)
        row = np.empty(n, np.int64)
        row[p] = np.arange(n)                                    # the row of every cell under this permutation
        l_cell = lab[row]
        single = comp < 0
        assert (l_cell[single | (comp == 0)] == -1).all()        # single cells (the column of 1 among them) are noise
        ks = [k for k in range(comp.max() + 1) if (comp == k).sum() > 1]
        firsts, labs, firstpos = [], [], []
        for k in ks:
            sel = np.flatnonzero(comp == k)
            assert (l_cell[sel] == l_cell[sel[0]]).all() and l_cell[sel[0]] >= 0
            firsts.append(row[sel].min())
            labs.append(l_cell[sel[0]])
            firstpos.append(pos[sel].min())
            at = np.sort(pos[sel]).tolist().index(pos[sel[np.argmin(row[sel])]])
            where.add("first" if at == 0 else "last" if at == len(sel) - 1 else "middle")
        assert np.array_equal(np.argsort(firsts), np.argsort(labs)) and sorted(labs) == list(range(len(ks)))
        monotone[pn] = bool((np.diff(np.asarray(labs)[np.argsort(firstpos)]) > 0).all())
    assert where == {"first", "middle", "last"} and monotone["cell_order"] and not monotone["shuffled"] and not monotone["reversed"]


# ---- cut_anchor -----------------------------------------------------------------------------------------------------------------
def test_cut_anchor():
    c = BC.get("cut_anchor")
    assert (c.X[0], c.Y[0]) == BC.CUT_LOW[0] and (c.X[-1], c.Y[-1]) == BC.CUT_LOW[1]
    assert c.X.argmin() == 0 and c.Y.argmin() == len(c.X) - 1
    for cut, want in zip(BC.CUTS, (BC.CUT_A1, BC.CUT_A2, BC.CUT_LAST)):
        keep = kept(c.X, c.Y, cut)
        assert 0 not in keep and len(c.X) - 1 not in keep        # row 0 and the last row are filtered
        assert (c.X[keep].min(), c.Y[keep].min()) == want
        assert (want[0] - c.X.min()) % c.eps and (want[1] - c.Y.min()) % c.eps
    assert len(kept(c.X, c.Y, BC.CUTS[2])) == 1
    assert (BC.CUT_A2[0] - BC.CUT_A1[0]) % c.eps and (BC.CUT_A2[1] - BC.CUT_A1[1]) % c.eps
    one = labels("cut_anchor", "as_built", 1, BC.CUTS[2])
    assert (one >= 0).sum() == 1 and (labels("cut_anchor", "as_built", 2, BC.CUTS[2]) == -1).all()
    # the rule: a grid anchored at the minimum of ALL rows gives other labels under every cut that leaves a pair
    for cut in BC.CUTS[:2]:
        got = model("cut_anchor", "as_built", 2, cut, origin=(c.X.min(), c.Y.min()))
        assert not np.array_equal(got, labels("cut_anchor", "as_built", 2, cut)), cut
