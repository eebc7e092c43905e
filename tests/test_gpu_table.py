"""GPU: the whole cluster table, every row, through every kernel that fills it and every form a run comes back in -- against numpy on
the ORACLE's labels (tests/table_check.py; exact integer equality, no tolerance anywhere).

The inputs are the families of tests/table_cases.py; tests/test_table_cases.py proves on the CPU that each of them is what it says:
more ids per workgroup than the LDS table of cl_table.h holds (the fallback to global atomics), runs of equal labels that start at
every lane and cross the row / half / wave boundaries of the segmented reduction, more ids than the pinned cache of the first export
(the second export of cl_wait), every class of pipe.py:83-97.

  producer            variants / levels                          forms
  k_final_labels      v2, v1 at traversal 0, 1, 2                rows, no labels
  k_final_lists       v2, v1 at traversal 3, 4                   rows, no labels, pairs, row mask
  k_blk_point_labels  block                                      rows, no labels
  k64_final           cluster_weighted (1, 1) and (7, 3)         rows

The level is the one SET: a run takes min(set, 3) at minPts 1 (and outside 2 .. 128, or with the count cache off), and the library
has no entry that tells which level a run took.  With the defaults of these handles run_sort_and_count takes level 4 for minPts
2 .. 128; levels 3 and 4 share k_final_lists, so the table's producer is the same either way.
"""
import ctypes

import numpy as np
import pytest

import oracle
import table_cases as T
from table_check import check_table, label_stats, table_from_labels
from cloops_amd import _lib, api

pytestmark = pytest.mark.gpu

LEVELS = (0, 1, 2, 3, 4)
_ref = {}


def _want(name, variant, cut=0, eps=None, m=None):
    """the oracle's labels of one setting, computed once per module"""
    c = T.get(name)
    key = (name, variant, cut, eps or c.eps, m or c.min_pts)
    if key not in _ref:
        _ref[key] = oracle.single_dbscan(variant, c.X, c.Y, key[3], key[4], cut)["labels"]
    return _ref[key]


def _rot_cases():
    return [(n, v) for n in T.TABLE_FAMILIES for v in T.get(n).variants if v != "block"]


def _labels_of_pairs(n, pairs):
    lab = np.full(n, -1, np.int32)
    assert len(np.unique(pairs[:, 0])) == len(pairs)
    lab[pairs[:, 0]] = pairs[:, 1]
    return lab


# ---- producers x forms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", _rot_cases())
def test_rotated_variants_every_level_and_form(name, variant):
    c = T.get(name)
    want = _want(name, variant)
    n = len(c.X)
    ch = api.Chromosome(c.X, c.Y)
    try:
        for level in LEVELS:
            ch.set_traversal(level)
            got = ch.cluster(variant, c.eps, c.min_pts)
            assert np.array_equal(got.labels, want), (level, int((got.labels != want).sum()))
            check_table(c.X, c.Y, want, got, (level, "rows"))
            got = ch.cluster(variant, c.eps, c.min_pts, want_labels=False)
            assert got.labels is None
            check_table(c.X, c.Y, want, got, (level, "no labels"))
            if level >= 3 and 2 <= c.min_pts <= 128:                     # the list forms (include/cloops_hip.h)
                ch.cluster_pairs_async(variant, c.eps, c.min_pts)
                res, pairs = ch.wait_pairs(copy=True)
                assert np.array_equal(_labels_of_pairs(n, pairs), want), level
                check_table(c.X, c.Y, want, res, (level, "pairs"))
                ch.cluster_rowmask_async(variant, c.eps, c.min_pts)
                res, mask, labs = ch.wait_rowmask(copy=True)
                lab = np.full(n, -1, np.int32)
                lab[ch.rows_of_mask(mask)] = labs
                assert np.array_equal(lab, want), level
                check_table(c.X, c.Y, want, res, (level, "row mask"))
    finally:
        ch.close()


@pytest.mark.parametrize("name", T.TABLE_FAMILIES)
def test_block_variant(name):
    c = T.get(name)
    want = _want(name, "block")
    ch = api.Chromosome(c.X, c.Y)
    try:
        got = ch.cluster("block", c.eps, c.min_pts)
        assert np.array_equal(got.labels, want)
        check_table(c.X, c.Y, want, got, "rows")
        got = ch.cluster("block", c.eps, c.min_pts, want_labels=False)
        check_table(c.X, c.Y, want, got, "no labels")
    finally:
        ch.close()


@pytest.mark.parametrize("wx,wy", [(1, 1), (7, 3)])
@pytest.mark.parametrize("name", T.TABLE_FAMILIES)
def test_weighted_metric(name, wx, wy):
    """boxes in UNSCALED coordinates against the sequential oracle on the explicitly scaled 64-bit matrix (the scaled runs make
    the clusters of the unweighted ones: tests/test_table_cases.py::test_weighted_metric_leaves_every_family_as_it_is)"""
    c = T.get(name)
    eps = T.weighted_eps(wx, wy)
    want = oracle.labels("v1", c.X * wx, c.Y * wy, eps, c.min_pts)
    if (wx, wy) == (1, 1):
        assert np.array_equal(want, _want(name, "v1"))
    assert label_stats(want)[0] > 100
    ch = api.Chromosome(c.X, c.Y)
    try:
        got = ch.cluster_weighted(eps, c.min_pts, wx, wy)
        assert np.array_equal(got.labels, want)
        check_table(c.X, c.Y, want, got)
    finally:
        ch.close()


# ---- where the table sits: two result slots, a cut change, a second run ----------------------------------------------------------
@pytest.mark.parametrize("variant", T.ROT)
@pytest.mark.parametrize("name,cut", [("runs", 20 * T.EPS), ("classes_2049", T.FINAL_CUT)])
def test_both_result_slots_across_cut_changes(name, cut, variant):
    """runs alternate between two result slots (finish_enqueue flips the slot at every run): the cuts below put a run right after
    a cut change and a repeated run on EACH slot"""
    cuts = (0, cut, cut, cut, 0, 0, 0, cut)
    kinds = {(k & 1, cuts[k] != cuts[k - 1]) for k in range(1, len(cuts))}
    assert kinds == {(0, True), (0, False), (1, True), (1, False)}       # (slot, the cut has changed)
    c = T.get(name)
    keep = c.Y - c.X >= cut
    assert 0.2 < keep.mean() < 0.8
    ch = api.Chromosome(c.X, c.Y)
    try:
        for k, ct in enumerate(cuts):
            want = _want(name, variant, ct)
            got = ch.cluster(variant, c.eps, c.min_pts, ct)
            assert np.array_equal(got.labels, want), (k, ct)
            check_table(c.X, c.Y, want, got, (k, ct))
    finally:
        ch.close()


# ---- more ids than the pinned cache of the first export --------------------------------------------------------------------------
FEW_CUT = 48 * T.EPS               # keeps about 4 % of the isolated PETs


@pytest.mark.parametrize("variant", T.ROT)
def test_many_ids_first_run_then_few_then_many(variant):
    """first run of a fresh handle (slot 0: the cache is too small, cl_wait exports again), few ids (slot 1: its first cache),
    many (slot 0: large enough now), many (slot 1: too small after all)"""
    c = T.get("many_ids")
    ch = api.Chromosome(c.X, c.Y)
    try:
        for k, cut in enumerate((0, FEW_CUT, 0, 0)):
            want = _want("many_ids", variant, cut)
            nc = label_stats(want)[0]
            assert nc > T.export_cache_rows(len(c.X)) if cut == 0 else 1000 < nc < 10000
            got = ch.cluster(variant, c.eps, c.min_pts, cut)
            assert np.array_equal(got.labels, want), k
            check_table(c.X, c.Y, want, got, k)
    finally:
        ch.close()


@pytest.mark.parametrize("variant", ["v2", "block"])
def test_many_ids_two_runs_in_flight(variant):
    c = T.get("many_ids")
    ch = api.Chromosome(c.X, c.Y)
    try:
        cuts = (0, 0, FEW_CUT, 0)
        ch.cluster_async(variant, c.eps, c.min_pts, cuts[0])
        for k in range(len(cuts)):
            if k + 1 < len(cuts):
                ch.cluster_async(variant, c.eps, c.min_pts, cuts[k + 1])
            got = ch.wait(copy=True)
            want = _want("many_ids", variant, cuts[k])
            assert np.array_equal(got.labels, want), k
            check_table(c.X, c.Y, want, got, k)
    finally:
        ch.close()


def test_many_ids_weighted():
    c = T.get("many_ids")
    want = _want("many_ids", "v1")
    ch = api.Chromosome(c.X, c.Y)
    try:
        for k in range(2):
            got = ch.cluster_weighted(c.eps, c.min_pts, 1, 1)
            assert np.array_equal(got.labels, want)
            check_table(c.X, c.Y, want, got, k)
    finally:
        ch.close()


# ---- the export switched off ---------------------------------------------------------------------------------------------------
def _get_boxes(ch, K):
    buf = np.zeros(max(K, 1), api.BOX_DTYPE)
    rc = _lib.load().cl_get_boxes(ch._h, buf.ctypes.data_as(ctypes.c_void_p))
    return rc, buf[:K]


@pytest.mark.parametrize("name", ["classes_2049", "isolated_plus_giant", "many_ids"])
@pytest.mark.parametrize("variant", ["v2", "block"])
def test_export_off_counts_ids_and_refuses_the_rows(name, variant):
    """want_boxes=False: no rows, the header's two numbers as from the labels, cl_get_boxes refuses, K10 reads the device table all
    the same; then the same run with the export on (the slot's first cache) on the same handle"""
    c = T.get(name)
    want = _want(name, variant)
    nc, ml = label_stats(want)
    t = table_from_labels(c.X, c.Y, want, ml + 1).copy()
    ok = (t["count"] > 0) & (t["min_x"] != t["max_x"]) & (t["min_y"] != t["max_y"])
    inter = ok & (t["max_x"] < t["min_y"])
    counts = (int(inter.sum()), int((ok & ~inter).sum()))
    ch = api.Chromosome(c.X, c.Y)
    try:
        for k in range(2):                                               # both slots
            ch.cluster_async(variant, c.eps, c.min_pts, want_boxes=False)
            got = ch.wait()
            assert got.boxes is None and np.array_equal(got.labels, want)
            assert (got.n_clusters, got.max_label) == (nc, ml), k
            rc, _ = _get_boxes(ch, ml + 1)
            assert rc == _lib.CL_ERR_ARG, k
            ch.cand_reset()
            assert ch.cand_append(0) == counts, k
        for k in range(2):
            ch.cluster_async(variant, c.eps, c.min_pts, want_boxes=True)
            got = ch.wait()
            check_table(c.X, c.Y, want, got, k)
            rc, rows = _get_boxes(ch, ml + 1)
            assert rc == _lib.CL_OK and np.array_equal(rows, t), k
            ch.cand_reset()
            assert ch.cand_append(0) == counts, k
    finally:
        ch.close()


def test_weighted_run_after_an_export_off_run_has_its_table():
    """cluster_weighted always returns boxes: it must switch the export back on"""
    c = T.get("runs")
    want = _want("runs", "v1")
    ch = api.Chromosome(c.X, c.Y)
    try:
        ch.cluster_async("v1", c.eps, c.min_pts, want_boxes=False)
        assert ch.wait().boxes is None
        got = ch.cluster_weighted(c.eps, c.min_pts, 1, 1)
        assert np.array_equal(got.labels, want)
        check_table(c.X, c.Y, want, got)
    finally:
        ch.close()
