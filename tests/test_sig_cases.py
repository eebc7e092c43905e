"""CPU: the reference and the cases of tests/sig_cases.py.  `mask_counts` against the set model of fake_backend (the stand-in of K8
in the host tests), against the reference's own getCorLink / getCounts / getPETsforRegions where the reference checkout is
present, against `brute_counts` (the yardstick of K11) on the shared columns; and the facts every case is built for, so that
none of them degenerates unnoticed."""
import numpy as np
import pytest

import fake_backend
import refload
import sig_cases as S
from test_quant import brute_counts

CASE_CUTS = [(name, k) for name in S.NAMES for k in range(3)]
ids = lambda p: "%s-%s" % (p[0], ("cut0", "part", "none")[p[1]])


def _cut(name, k):
    return S.cuts_of(S.case(name))[k]


@pytest.mark.parametrize("name_k", CASE_CUTS, ids=ids)
def test_mask_counts_equal_set_model(name_k):
    name, cut = name_k[0], _cut(*name_k)
    c = S.case(name)
    want, n = S.reference(name, cut)
    got, n2 = fake_backend.FakeChromosome(c.X, c.Y).sig_counts(c.windows, cut)
    assert n == n2
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", S.NAMES)
def test_cuts_keep_all_part_none(name):
    c = S.case(name)
    d = c.Y - c.X
    part, none = c.cuts
    assert int((d >= none).sum()) == 0 and S.reference(name, none)[1] == 0
    assert not S.reference(name, none)[0].any()
    kept = int((d >= part).sum())
    assert S.reference(name, part)[1] == kept and S.reference(name, 0)[1] == len(d)
    assert (0 < kept < len(d)) if len(d) > 1 else kept == 1


@pytest.mark.parametrize("name_k", CASE_CUTS, ids=ids)
def test_identities(name_k):
    table, n = S.reference(name_k[0], _cut(*name_k))
    c_a, c_b, rab, c_ab = S.split(table)
    assert (c_ab <= np.minimum(c_a[:, :, None], c_b[:, None, :])).all()
    assert (rab <= c_ab[:, 0, 0]).all()
    assert table.min() >= 0 and table.max() <= n


@pytest.mark.parametrize("name_k", [(n, k) for n in S.NAMES for k in (0, 1)], ids=ids)
def test_mask_counts_equal_reference_functions(name_k):
    """the reference's model as getGenomeCoverage builds it from parseJd's rows, its getCounts per window and end, its
    getPETsforRegions for rab; set sizes of all 22 windows for up to 200 records, the 121 intersections for up to 25"""
    if not refload.available():
        pytest.skip("reference checkout not present")
    ns = refload.ref_cmodel_namespace()
    name, cut = name_k[0], _cut(*name_k)
    c = S.case(name)
    mat = np.stack([np.arange(len(c.X)), c.X, c.Y], 1)
    if cut > 0:                                                            # parseJd(f, cut), io.py:213-216
        mat = mat[np.where(mat[:, 2] - mat[:, 1] >= cut)[0], :]
    if mat.shape[0] < 2:                                                   # getGenomeCoverage builds no model of fewer than 2 PETs
        assert name.startswith("tiny")
        return
    model = [list(ns["getCorLink"](mat[:, 1])), list(ns["getCorLink"](mat[:, 2]))]
    want, n = S.reference(name, cut)
    assert n == mat.shape[0]
    w = c.windows.astype(np.int64)
    recs = np.arange(len(w)) if len(w) <= 200 else np.random.default_rng(5).choice(len(w), 200, replace=False)
    for q, r in enumerate(recs):
        iv = [[int(w[r, k]), int(w[r, 22 + k])] for k in range(22)]
        sets = [ns["getCounts"](v, model[0]) | ns["getCounts"](v, model[1]) for v in iv]
        assert [len(s) for s in sets] == want[r, :22].tolist(), (name, r)
        ra, rb, rab = ns["getPETsforRegions"](iv[0], iv[11], model)
        assert (ra, rb, rab) == (want[r, 0], want[r, 11], want[r, 22]), (name, r)
        if q < 25:
            assert [len(sets[k] & sets[11 + l]) for k in range(11) for l in range(11)] == want[r, 23:].tolist(), (name, r)


@pytest.mark.parametrize("name_k", [(n, k) for n in S.NAMES for k in (0, 1)], ids=ids)
def test_shared_columns_equal_brute_counts(name_k):
    """K11's yardstick and K8's agree where the kernels' outputs mean the same: |S(A_0)|, |S(B_0)|, rab"""
    name, cut = name_k[0], _cut(*name_k)
    c = S.case(name)
    w = c.windows[:300]
    q, nq = brute_counts(c.X, c.Y, w, cut)
    s, ns = S.reference(name, cut)
    assert nq == ns
    assert np.array_equal(q[:, 0], s[:300, 0]) and np.array_equal(q[:, 1], s[:300, 11]) and np.array_equal(q[:, 2], s[:300, 22])


# ---- the facts the cases are built for -------------------------------------------------------------------------------------------
def _ends_in(v, lo, hi):
    return (v >= lo) & (v <= hi)


def test_stride_slices_sizes():
    c = S.case("stride_slices")
    lo, hi = S.hulls(c.windows)
    assert len(c.windows) == len(S.STRIDE_SIZES) == 6 and S.STRIDE_SIZES == (0, 1, 255, 256, 257, 513) and S.TPB == 256
    for q, s in enumerate(S.STRIDE_SIZES):
        for side in (0, 1):
            bx, by = _ends_in(c.X, lo[q, side], hi[q, side]), _ends_in(c.Y, lo[q, side], hi[q, side])
            assert (int(bx.sum()), int(by.sum()), int((bx & by).sum())) == (s, s, 0)
    w = c.windows.astype(np.int64)
    for v in (c.X, c.Y):                                    # an end is in the hull of ONE side of one record, the partner in no window
        n_hulls = (_ends_in(v[:, None, None], lo[None], hi[None])).sum((1, 2))
        assert n_hulls.max() == 1
    in_any = lambda v: (_ends_in(v[:, None], w[:, :22].reshape(-1), w[:, 22:].reshape(-1))).any(1)
    assert not (in_any(c.X) & in_any(c.Y)).any()
    table = S.reference("stride_slices", 0)[0]
    c_a, c_b, rab, c_ab = S.split(table)
    assert not rab.any() and not c_ab.any()
    assert c_a[0].sum() == 0 and c_b[0].sum() == 0 and (c_a[2:].sum(1) > 0).all() and (c_b[2:].sum(1) > 0).all()
    assert c_a[5].sum() > 2 * S.TPB                                        # most ends of a hull fall into a window of it


def test_on_the_bounds_counts():
    c = S.case("on_the_bounds")
    w = c.windows[0].astype(np.int64)
    lo, hi = np.sort(w[:22]), np.sort(w[22:])
    assert (lo[1:] > hi[:-1] + 2).all()                                    # disjoint, lo - 1 and hi + 1 in no other window
    c_a, c_b, rab, c_ab = S.split(S.reference("on_the_bounds", 0)[0])
    assert c_a[0].tolist() == [6] * 11 and c_b[0].tolist() == [7] * 11 and rab[0] == 1
    assert np.array_equal(c_ab[0], 2 * np.eye(11, dtype=c_ab.dtype))
    for v in (w[:22], w[22:], w[:22] - 1, w[22:] + 1):
        assert np.isin(v, c.X).all() and np.isin(v, c.Y).all()
    assert (c_a[1] > 0).all() and (c_b[1] > 0).all()                       # the one-point windows hold their PETs
    assert (c_a[2] > c_a[0]).all() and (c_b[2] > c_b[0]).all()             # one wider: the PETs on lo - 1 and hi + 1


def test_hull_with_holes_groups():
    c = S.case("hull_with_holes")
    w = c.windows[0].astype(np.int64)
    g = {name: c.info["group"] == k for k, name in enumerate(c.info["groups"])}
    in_wins = lambda v, side: _ends_in(v[:, None], w[11 * side:11 * side + 11], w[22 + 11 * side:33 + 11 * side])
    lo, hi = S.hulls(c.windows[:1])
    in_hull = lambda v, side: _ends_in(v, lo[0, side], hi[0, side])
    assert (np.diff(w[:11]) < 0).any() and (np.diff(w[11:22]) < 0).any() and w[0] != w[:11].min()      # not in ascending order
    for name, side in (("hole_a_win_a", 0), ("hole_b_win_b", 1)):
        m = g[name]
        assert m.sum() == c.info["m"]
        assert in_hull(c.X[m], side).all() and not in_wins(c.X[m], side).any() and in_wins(c.Y[m], side).any(1).all()
        assert not _ends_in(c.X[m], w[11 * side], w[22 + 11 * side]).any()          # window 0 does not tell them from the others
    for name, side in (("win_a_win_a", 0), ("win_b_win_b", 1)):
        m = g[name]
        kx, ky = in_wins(c.X[m], side).argmax(1), in_wins(c.Y[m], side).argmax(1)
        assert in_wins(c.X[m], side).any(1).all() and in_wins(c.Y[m], side).any(1).all() and (kx != ky).all()
    for name, side in (("same_point_a", 0), ("same_point_b", 1)):
        assert (c.X[g[name]] == c.Y[g[name]]).all() and in_wins(c.X[g[name]], side).any(1).all()
    m = g["hole_a_hole_a"]
    assert in_hull(c.X[m], 0).all() and in_hull(c.Y[m], 0).all() and not in_wins(c.X[m], 0).any() and not in_wins(c.Y[m], 0).any()
    assert (c.Y < c.X).any()
    # every PET counted once: a PET of S(A_k) is in exactly one window per end here, so the sizes add up to the ends in windows
    c_a, c_b, rab, c_ab = S.split(S.reference("hull_with_holes", 0)[0])
    for side, cnt in ((0, c_a[0]), (1, c_b[0])):
        assert np.array_equal(cnt, (in_wins(c.X, side) | in_wins(c.Y, side)).sum(0))
    assert np.array_equal(c_a[1], c_b[0]) and np.array_equal(c_b[1], c_a[0]) and np.array_equal(c_ab[1], c_ab[0].T)


def test_directed_counts():
    c = S.case("directed")
    c_a, c_b, rab, c_ab = S.split(S.reference("directed", 0)[0])
    m = c.info["m"]
    assert rab.tolist() == [m, m] and c_ab[:, 0, 0].tolist() == [2 * m, 2 * m]
    w = c.windows.astype(np.int64)
    for r, reversed_kind in ((0, "other"), (1, "first")):
        first = _ends_in(c.X, w[r, 0], w[r, 22]) & _ends_in(c.Y, w[r, 11], w[r, 33])
        other = _ends_in(c.X, w[r, 11], w[r, 33]) & _ends_in(c.Y, w[r, 0], w[r, 22])
        assert first.sum() == other.sum() == m
        rev = first if reversed_kind == "first" else other
        fwd = other if reversed_kind == "first" else first
        assert (c.Y[rev] < c.X[rev]).all() and (c.Y[fwd] > c.X[fwd]).all()
    cut1 = S.split(S.reference("directed", 1)[0])                          # without the reversed rows
    assert cut1[2].tolist() == [m, 0] and cut1[3][:, 0, 0].tolist() == [m, m]


def test_overlapping_sides_records():
    c = S.case("overlapping_sides")
    (a, b, e, f), (a1, b1, e1, f1), (a2, b2, e2, f2), (a3, b3, e3, f3) = c.info["records"]
    assert (a, b) == (e, f) and a1 < e1 < f1 < b1 and a2 < e2 < b2 < f2 and e3 < a3 < f3 < b3
    assert c.X.min() >= 0 and c.Y.min() >= 0 and (c.Y < c.X).any()
    c_a, c_b, rab, c_ab = S.split(S.reference("overlapping_sides", 0)[0])
    assert np.array_equal(c_a[0], c_b[0]) and np.array_equal(np.diag(c_ab[0]), c_a[0]) and np.array_equal(c_ab[0], c_ab[0].T)
    assert c_ab[1, 0, 0] == c_b[1, 0] > 0                                  # B_0 inside A_0
    assert 0 < c_ab[2, 0, 0] < min(c_a[2, 0], c_b[2, 0]) and (rab > 0).all()


def test_extremes_windows():
    c = S.case("extremes")
    w = c.windows.astype(np.int64)
    for v in (S.CMAX, -S.CMAX, 0, -1):
        assert (c.X == v).any() and (c.Y == v).any()
    assert (c.Y < c.X).any() and (c.Y == c.X).any()
    have = {(int(a), int(b)) for a, b in zip(w[:, :22].reshape(-1), w[:, 22:].reshape(-1))}
    for iv in ((S.I32_MIN, S.I32_MAX), (-S.BIAS, -S.BIAS + 1), (-S.BIAS - 1, -S.BIAS - 1), (S.CMAX, S.I32_MAX), (S.CMAX, S.CMAX),
               (-S.CMAX, -S.CMAX), (0, 0)):
        assert iv in have, iv
    lo, hi = S.hulls(c.windows)
    assert (lo[1, 0], hi[1, 0]) == (S.CMAX, S.I32_MAX) and lo[1, 1] == S.I32_MIN           # a hull that ends at the top of int32
    assert (lo[2, 0], hi[2, 0]) == (1000, 1090) and _ends_in(c.X, 1000, 1090).any()          # inverted windows, a hull with PETs
    for cut in S.cuts_of(c)[:2]:
        table, n = S.reference("extremes", cut)
        for r, ks in c.info["inverted"].items():
            assert (w[r, ks] > w[r, [22 + k for k in ks]]).all()
            assert not table[r, ks].any()                                                    # an inverted window counts nothing
            others = [k for k in range(22) if k not in ks]
            assert (w[r, others] <= w[r, [22 + k for k in others]]).all() and table[r, others].any()
        assert table[0, 0] == table[0, 21] == n                                              # the whole of int32 holds every PET
        assert table[0, 1] == 0 and table[0, 11] == 0 and table[0, 17] == 0 and table[0, 18] == 0      # below / above the domain
        assert table[1, 0] > 0 and table[1, 11] > 0 and table[0, 2] > 0 and table[0, 3] > 0
        r = c.info["clamped_record"]
        zero = [k for k in range(22) if (w[r, k], w[r, 22 + k]) == (0, 0)]
        assert len(zero) >= 2 and (table[r, zero] > 0).all()                                 # [0, 0] windows with PETs at 0
    assert S.reference("extremes", 1)[1] < S.reference("extremes", 0)[1]


def test_pile_up_counts():
    c = S.case("pile_up")
    r, k, l = c.info["pile"]
    c_a, c_b, rab, c_ab = S.split(S.reference("pile_up", 0)[0])
    assert len(c.X) == 70000 and len(c.windows) == 3
    assert min(c_a[r, k], c_b[r, l], c_ab[r, k, l]) >= 66000 > 65536
    w = c.windows.astype(np.int64)
    assert (w[r, k], w[r, 22 + k]) == (w[r, 11 + l], w[r, 33 + l]) == S.PILE
    assert (c_a[1:, 0] > 0).all() and (c_b[1:, 0] > 0).all()


def test_duplicates_rows():
    c = S.case("duplicates")
    rows, counts = np.unique(np.stack([c.X, c.Y], 1), axis=0, return_counts=True)
    assert len(rows) == c.info["distinct"] == 300 and counts.min() >= 1 and counts.max() == 40 and len(np.unique(counts)) >= 30
    w = c.windows.astype(np.int64)
    assert np.isin(w, np.concatenate([c.X, c.Y])).all() and (w[:, :22] <= w[:, 22:]).all()
    assert (S.reference("duplicates", 0)[0][:, :22] > 0).all()


def test_many_records_kinds():
    c = S.case("many_records")
    w = c.windows.astype(np.int64)
    assert len(w) == S.MANY == 5000 and len(c.X) == 2000 and (c.Y >= c.X).all() and c.X.min() >= 0
    table = S.reference("many_records", 0)[0]
    assert c.info["prefixes"] == (3, 2)
    head = slice(0, 300)                                                   # every kind among the first records as well
    clamped = ((w[:, 1:11] == 0) & (w[:, 23:33] == 0)).any(1)
    empty = ~table[:, :22].any(1)
    same = (c.info["records"][:, 0] == c.info["records"][:, 2]) & (c.info["records"][:, 1] == c.info["records"][:, 3])
    for kind in (clamped, empty, same):
        assert kind.sum() >= 400 and kind[head].sum() >= 10
    assert (table[:, 22] > 0).sum() >= 500 and (table[:, 23:].reshape(-1, 11, 11)[:, 1:, 1:] > 0).any()


def test_tiny_cases():
    for n in (1, 2):
        c = S.case("tiny_%d" % n)
        assert len(c.X) == n and len(c.windows) == 2
        assert S.reference(c.name, 0)[0][0, [0, 11, 22]].tolist() == [n, n, 1]
