"""CPU only: the inputs of tests/test_gpu_table.py and tests/test_gpu_candidates.py reach what they name.  Every condition a family of
tests/table_cases.py states is checked here on the oracle alone, so that a GPU test on it cannot pass on an input that misses its
path (one id per workgroup, no run across a lane boundary, a class of pipe.py:83-97 that does not occur)."""
import numpy as np
import pytest

import oracle
import table_cases as T
from table_check import label_stats, table_from_labels

_lab = {}


def _labels(name, variant):
    key = (name, variant)
    if key not in _lab:
        c = T.get(name)
        _lab[key] = oracle.single_dbscan(variant, c.X, c.Y, c.eps, c.min_pts, 0)["labels"]
    return _lab[key]


def _cases_variants(names):
    return [(n, v) for n in names for v in (T.NEG if "neg" in n else T.ROT)]


def test_reference_table_on_a_hand_made_example():
    """table_from_labels itself: ids 0 and 2 in use, id 1 a gap (zeros), noise ignored, negative coordinates"""
    X = np.array([5, -7, 9, 100, -3, 4])
    Y = np.array([50, 70, -90, 1000, 30, 40])
    lab = np.array([2, 0, 2, -1, 0, 2])
    t = table_from_labels(X, Y, lab, 3)
    assert t.tolist() == [(-7, -3, 30, 70, 2), (0, 0, 0, 0, 0), (4, 9, -90, 50, 3)]
    assert label_stats(lab) == (2, 2) and label_stats(np.array([-1, -1])) == (0, -1)
    assert len(table_from_labels(X, Y, np.full(6, -1), 0)) == 0


@pytest.mark.parametrize("name", ["isolated", "isolated_neg", "many_ids"])
def test_isolated_every_pet_is_its_own_id(name):
    c = T.get(name)
    n = len(c.X)
    xs = np.sort(c.X)
    assert (np.diff(xs) > c.eps).all()                                   # pairwise farther apart than eps, whatever Y is
    assert n > 8 * T.TAB_H if name != "many_ids" else n > T.export_cache_rows(n)
    if name == "isolated_neg":
        assert (c.X < 0).any() and (c.X > 0).any() and (c.Y < c.X).sum() > n // 4 and (c.Y > c.X).sum() > n // 4
    else:
        assert (c.X >= 0).all() and (c.X <= c.Y).all()
    assert np.abs(c.X).max() < 1 << 29 and np.abs(c.Y).max() < 1 << 29
    for v in c.variants:
        lab = _labels(name, v)
        nc, ml = label_stats(lab)
        assert (lab >= 0).all() and nc == n and ml == n - 1, v
        assert (np.bincount(lab) == 1).all(), v
        if name == "many_ids":
            assert ml + 1 > T.export_cache_rows(n)


def test_isolated_pairs_two_pets_per_id():
    c = T.get("isolated_pairs")
    for v in c.variants:
        lab = _labels(c.name, v)
        assert (lab >= 0).all() and label_stats(lab) == (c.info["pairs"], c.info["pairs"] - 1), v
        assert (np.bincount(lab) == 2).all() and c.info["pairs"] > 8 * T.TAB_H, v


def test_isolated_plus_giant_is_one_component_between_isolated_pets():
    c = T.get("isolated_plus_giant")
    n = len(c.X)
    for v in c.variants:
        lab = _labels(c.name, v)
        cnt = np.sort(np.bincount(lab[lab >= 0]))
        assert (lab >= 0).all() and len(cnt) == n - T.GIANT + 1 and cnt[-1] == T.GIANT and (cnt[:-1] == 1).all(), v
        assert len(np.unique(lab[c.info["member"]])) == 1 and int(c.info["member"].sum()) == T.GIANT, v


@pytest.mark.parametrize("order", ["v2", "v1", "p", "x"])
def test_isolated_plus_giant_every_workgroup_with_the_giant_overflows_the_lds_table(order):
    """in every order the kernels work in, every aligned window of 1024 and of 4096 rows (a workgroup's share: 1024 threads, one
    or four PETs each) that holds a PET of the large component holds more than TAB_H labels -- so does every window of 1024
    consecutive rows wherever it starts: the component's key hits its LDS slot while its neighbours run out of probes"""
    c = T.get("isolated_plus_giant")
    m = c.info["member"][T.work_orders(c.X, c.Y, c.eps)[order]]
    n = len(m)
    seen = 0
    for w in (1024, 4096):
        for s in range(0, n, w):
            g = int(m[s:s + w].sum())
            if g:
                seen += 1
                assert len(m[s:s + w]) - g + 1 > T.TAB_H, (w, s, g)
    assert seen >= 6
    iso = np.concatenate([[0], np.cumsum(~m)])
    gi = np.concatenate([[0], np.cumsum(m)])
    s = np.arange(0, n - 1024 + 1)
    has = gi[s + 1024] - gi[s] > 0
    assert has.sum() > 4000 and ((iso[s + 1024] - iso[s])[has] + 1 > T.TAB_H).all()
    # the tail: whatever window ends the rows holds no PET of the component, or more than TAB_H isolated ones behind it
    last = int(np.flatnonzero(m)[-1])
    assert n - 1 - last > T.TAB_H


def _run_bounds(order="p"):
    c = T.get("runs")
    order = T.work_orders(c.X, c.Y, c.eps)[order]
    b = c.info["blob"][order]
    starts = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1]]))
    return c, order, starts, np.concatenate([starts[1:], [len(b)]])


def test_runs_every_blob_is_one_cluster_of_its_size():
    c, order, starts, ends = _run_bounds()
    sizes = np.asarray(c.info["sizes"])
    assert 6000 < len(c.X) < 7000 and len(starts) == len(sizes)          # contiguous in X + Y order: one run per blob
    assert np.array_equal(ends - starts, sizes)
    for v in c.variants:
        lab = _labels("runs", v)
        assert (lab >= 0).all() and label_stats(lab)[0] == len(sizes), v
        t = table_from_labels(c.X, c.Y, lab, lab.max() + 1)
        first = lab[order][starts]                                       # the id of every blob
        assert len(np.unique(first)) == len(sizes), v
        assert np.array_equal(t["count"][first], sizes), v
        assert all((lab[order][s:e] == lab[order][s]).all() for s, e in zip(starts, ends)), v


@pytest.mark.parametrize("order", ["p", "v2", "v1", "x"])
def test_runs_start_at_every_lane_and_cross_every_boundary(order):
    """in X + Y order, in the strip-then-distance order of variant 2 and of variant 1, and in X order: the same 158 runs at the
    same places (no strip holds PETs of two blobs)"""
    _, _, starts, ends = _run_bounds(order)
    _, _, s0, e0 = _run_bounds("p")
    assert np.array_equal(starts, s0) and np.array_equal(ends, e0)
    assert set((starts % 64).tolist()) == set(range(64))
    for first_lane_behind in (16, 32, 0):                                # 15|16, 31|32, 63|64
        m = np.arange(1, int(ends[-1]))
        m = m[m % 64 == first_lane_behind]
        k = np.searchsorted(starts, m, side="right") - 1                 # the run of position m
        assert (starts[k] <= m - 1).any(), first_lane_behind           # ... holds the position in front of it too
    # and runs that end exactly at / begin exactly behind a boundary
    assert (ends % 16 == 0).any() and (ends % 64 == 0).any() and (starts % 16 == 15).any()


@pytest.mark.parametrize("name", T.TABLE_FAMILIES)
def test_weighted_metric_leaves_every_family_as_it_is(name):
    """the runs of tests/test_gpu_table.py under 7 |dX| + 3 |dY| <= 7 eps: the sequential oracle on the scaled matrix makes the same
    clusters of the same rows as variant 1 does unweighted, so every condition above holds for the weighted producer too"""
    c = T.get(name)
    a = _labels(name, "v1")
    b = oracle.labels("v1", c.X * 7, c.Y * 3, T.weighted_eps(7, 3), c.min_pts)
    assert np.array_equal(a < 0, b < 0)
    sel = a >= 0
    pairs = np.unique(np.stack([a[sel], b[sel]], 1), axis=0)
    assert len(pairs) == label_stats(a)[0] == label_stats(b)[0]           # a bijection between the ids: the same partition
    assert np.array_equal(oracle.labels("v1", c.X, c.Y, T.weighted_eps(1, 1), c.min_pts), a)


def test_runs_extremes_sit_at_four_different_pets():
    c, order, starts, ends = _run_bounds()
    x, y = c.X[order], c.Y[order]
    four = 0
    for s, e in zip(starts, ends):
        four += len({int(np.argmin(x[s:e])), int(np.argmax(x[s:e])), int(np.argmin(y[s:e])), int(np.argmax(y[s:e]))}) == 4
    assert 2 * four > len(starts), four


@pytest.mark.parametrize("name,variant", _cases_variants(T.CLASS_NAMES))
def test_classes_counts_per_kind_and_mix_per_block(name, variant):
    c = T.get(name)
    cnt = c.info["counts"]
    total = c.info["total"]
    assert sum(cnt.values()) == total and set(cnt) == set(T.KIND_CLASS)
    if "neg" in name:
        assert (c.X < 0).all() and (c.Y < 0).all()
    lab = _labels(name, variant)
    nc, ml = label_stats(lab)
    assert nc == total and ml == total - 1
    assert ((lab < 0) == (c.info["kind"] == "noise")).all()
    t = table_from_labels(c.X, c.Y, lab, ml + 1)
    b = {f: t[f].astype(np.int64) for f in t.dtype.names}
    assert (b["count"] == 3).all()
    degx, degy = b["min_x"] == b["max_x"], b["min_y"] == b["max_y"]
    ok = ~degx & ~degy
    inter = ok & (b["max_x"] < b["min_y"])
    assert int(degx.sum()) == cnt["degx"] and int(degy.sum()) == cnt["degy"] and not (degx & degy).any()
    assert int(inter.sum()) == cnt["inter"] + cnt["mark_at"] + cnt["mark_below"]
    assert int((ok & (b["max_x"] == b["min_y"])).sum()) == cnt["touch"]
    assert int((ok & (b["max_x"] > b["min_y"])).sum()) == cnt["overlap"]
    # the marked boxes: an odd sum in X, an even one in Y, floor mid-points final_cut or final_cut - 1 apart
    sx, sy = b["min_x"] + b["max_x"], b["min_y"] + b["max_y"]
    marked = inter & (sx % 2 == 1) & (sy % 2 == 0)
    d = sy // 2 - sx // 2
    assert int((marked & (d == T.FINAL_CUT)).sum()) == cnt["mark_at"] > 0
    assert int((marked & (d == T.FINAL_CUT - 1)).sum()) == cnt["mark_below"] > 0
    assert int(marked.sum()) == cnt["mark_at"] + cnt["mark_below"]
    if "neg" in name:                                                    # truncation toward zero would move these mid-points
        assert (sx[marked] < 0).all() and (-((-sx[marked]) // 2) != sx[marked] // 2).all()
    assert (inter & (d < T.FINAL_CUT)).sum() > 100 and (inter & (d > T.FINAL_CUT)).sum() > 100
    # every kind among the first and the last 256 ids of the first block of CAND_BLOCK ids
    kind_of = np.empty(ml + 1, dtype=c.info["kind"].dtype)
    kind_of[lab[lab >= 0]] = c.info["kind"][lab >= 0]
    for lo, hi in ((0, 256), (T.CAND_BLOCK - 256, min(total, T.CAND_BLOCK))):
        assert set(kind_of[lo:hi].tolist()) == set(T.KIND_CLASS), (lo, hi)


def test_sweep_steps_make_boxes_come_back():
    """the three steps of the candidate tests: nothing passes the second step's cut; every box of the first step is a box of the
    third, which has new ones too (the two-PET blobs)"""
    c = T.get("classes_2049")
    (e0, m0, c0), (e1, m1, c1), (e2, m2, c2) = T.SWEEP_STEPS
    assert not (c.Y - c.X >= c1).any()
    a = oracle.single_dbscan("v2", c.X, c.Y, e0, m0, c0)["dataI"]
    b = oracle.single_dbscan("v2", c.X, c.Y, e2, m2, c2)["dataI"]
    sa, sb = set(map(tuple, a)), set(map(tuple, b))
    assert len(sa) == len(a) and len(sb) == len(b)                       # (no identical boxes inside a step)
    assert sa < sb and len(sb - sa) > 100
