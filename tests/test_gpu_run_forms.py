"""GPU: the forms of a run (plain, pairs, row mask, sweep step, block, weighted, exact counts) one after the other and two at a
time on ONE handle.  What one call asked for must not reach the next, each wait returns the result of its own form, and the working
set of one run kind must not reach the next kind.  Labels, tables and counts are exact against the sequential oracle.

One synthetic chromosome (n = 20 000, as tests/test_gpu_edges.py::test_failed_arena_reservation_is_harmless makes it) at eps 500,
and at eps 1000 where the base layout is replaced in mid-sequence."""
import ctypes

import numpy as np
import pytest

import oracle
from cloops_amd import _lib, api
from table_check import check_table, label_stats

pytestmark = pytest.mark.gpu

N = 20000
EPS, EPS2, M = 500, 1000, 4
WX, WY = 2, 1
_data = {}
_ref = {}


def _xy():
    if not _data:
        rng = np.random.default_rng(3)
        X = rng.integers(0, 400000, N)
        _data["xy"] = (X, X + rng.integers(0, 30000, N))
    return _data["xy"]


def _oracle(variant, eps, m, cut):
    """oracle.single_dbscan of one setting, computed once per module"""
    key = (variant, eps, m, cut)
    if key not in _ref:
        X, Y = _xy()
        _ref[key] = oracle.single_dbscan(variant, X, Y, eps, m, cut)
    return _ref[key]


def _weighted():
    if "w" not in _ref:
        X, Y = _xy()
        _ref["w"] = oracle.labels("v1", X.astype(np.int64) * WX, Y.astype(np.int64) * WY, EPS, M)
    return _ref["w"]


def _counts(eps, cut):
    key = ("counts", eps, cut)
    if key not in _ref:
        X, Y = _xy()
        keep = Y - X >= cut
        out = np.full(N, -1, np.int32)
        out[keep] = oracle.neighbor_counts(X[keep], Y[keep], eps)
        _ref[key] = out
    return _ref[key]


def _check_plain(res, variant, eps, m, cut, tag):
    """row labels, the two header numbers and every row of the exported table"""
    X, Y = _xy()
    want = _oracle(variant, eps, m, cut)["labels"]
    assert res.labels is not None and np.array_equal(res.labels, want), (tag, variant, eps, m, cut)
    check_table(X, Y, want, res, (tag, variant, eps, m, cut))


def _check_header(res, want, tag):
    nc, ml = label_stats(want)
    assert res.labels is None and (res.n_clusters, res.max_label) == (nc, ml), tag


def _check_pairs(res, pairs, variant, eps, m, cut, tag):
    want = _oracle(variant, eps, m, cut)["labels"]
    got = np.full(N, -1, np.int32)
    got[pairs[:, 0]] = pairs[:, 1]
    assert len(pairs) == int((want >= 0).sum()) and len(np.unique(pairs[:, 0])) == len(pairs), tag
    assert np.array_equal(got, want), tag
    _check_header(res, want, tag)


def _check_rowmask(ch, res, mask, labels, variant, eps, m, cut, tag):
    want = _oracle(variant, eps, m, cut)["labels"]
    rows = ch.rows_of_mask(mask)
    assert np.array_equal(rows, np.flatnonzero(want >= 0)), tag
    assert np.array_equal(labels, want[rows]), tag
    _check_header(res, want, tag)


def _step(ch, variant, eps, m, cut, step, tag):
    """one sweep step: enqueue, wait, step_result against the oracle's classified tables"""
    ref = _oracle(variant, eps, m, cut)
    ch.step_async(variant, eps, m, cut, step)
    res = ch.wait()
    ni, ns, st = ch.step_result()
    assert res.labels is None and res.boxes is None, tag
    assert (ni, ns) == (len(ref["dataI"]), len(ref["dataS"])), tag
    assert st["n_all"] == [len(ref["dis"]), len(ref["dss"])], tag


def _get_boxes(ch, max_label):
    out = np.zeros(max(max_label + 1, 1), api.BOX_DTYPE)
    _lib.check(ch._lib.cl_get_boxes(ch._h, out.ctypes.data_as(ctypes.c_void_p)))
    return out[: max_label + 1]


# ---- what a call asked for does not reach the next run ---------------------------------------------
def _leak(ch):
    cut = 300
    ch.cluster_pairs_async("v2", EPS, M, cut)
    _check_pairs(*ch.wait_pairs(copy=True), "v2", EPS, M, cut, "pairs")
    _check_plain(ch.cluster("v2", EPS, M, cut), "v2", EPS, M, cut, "plain after pairs")

    ch.cluster_rowmask_async("v1", EPS, M, cut)
    _check_rowmask(ch, *ch.wait_rowmask(copy=True), "v1", EPS, M, cut, "rowmask")
    _check_plain(ch.cluster("v1", EPS, M, cut), "v1", EPS, M, cut, "plain after rowmask")

    ch.cand_reset()
    _step(ch, "v2", EPS, M, cut, 0, "step")
    res = ch.cluster("v2", EPS, M, 0)
    _check_plain(res, "v2", EPS, M, 0, "plain after step")
    assert np.array_equal(_get_boxes(ch, res.max_label), res.boxes)                # cl_get_boxes works again
    with pytest.raises(_lib.CloopsHipError) as ei:                                  # ... and the last run was no step
        ch.step_result()
    assert ei.value.code == _lib.CL_ERR_ARG
    _step(ch, "v2", EPS, M, 0, 1, "step after plain")
    _step(ch, "v1", EPS, M, cut, 2, "step after step")
    _check_plain(ch.cluster("v1", EPS, M, cut), "v1", EPS, M, cut, "plain after two steps")


# ---- two runs in flight, of different forms ---------------------------------------------------------
def _check_last(ch, res, form, variant, eps, m, cut, tag):
    """what the handle answers from the record of the last completed run, against the form that was waited for last"""
    want = _oracle(variant, eps, m, cut)["labels"]
    # the labelled PETs: counted by the pairs and the row-mask form only
    assert int(ch._lib.cl_last_n_labelled(ch._h)) == (0 if form == "plain" else int((want >= 0).sum())), tag
    # row labels on the device: every form but the pairs, which replace them
    assert bool(ch._lib.cl_labels_device(ch._h)) == (form != "pairs"), tag
    assert np.array_equal(_get_boxes(ch, res.max_label), res.boxes), tag
    with pytest.raises(_lib.CloopsHipError) as ei:                                  # none of them was a sweep step
        ch.step_result()
    assert ei.value.code == _lib.CL_ERR_ARG, tag


def _in_flight(ch):
    ch.cluster_async("v2", EPS, M, 0)
    ch.cluster_pairs_async("v2", EPS, M, 300)
    _check_plain(ch.wait(copy=True), "v2", EPS, M, 0, "plain in front of pairs")
    res, pairs = ch.wait_pairs(copy=True)
    _check_pairs(res, pairs, "v2", EPS, M, 300, "pairs behind plain")
    _check_last(ch, res, "pairs", "v2", EPS, M, 300, "record behind plain, pairs")

    ch.cluster_pairs_async("v1", EPS, M, 300)
    ch.cluster_rowmask_async("v2", EPS, M, 150)
    _check_pairs(*ch.wait_pairs(copy=True), "v1", EPS, M, 300, "pairs in front of rowmask")
    res, mask, labels = ch.wait_rowmask(copy=True)
    _check_rowmask(ch, res, mask, labels, "v2", EPS, M, 150, "rowmask behind pairs")
    _check_last(ch, res, "rowmask", "v2", EPS, M, 150, "record behind pairs, rowmask")

    ch.cluster_rowmask_async("v2", EPS, M, 0)
    ch.cluster_async("v1", EPS, M, 300)
    _check_rowmask(ch, *ch.wait_rowmask(copy=True), "v2", EPS, M, 0, "rowmask in front of plain")
    res = ch.wait(copy=True)
    _check_plain(res, "v1", EPS, M, 300, "plain behind rowmask")
    _check_last(ch, res, "plain", "v1", EPS, M, 300, "record behind rowmask, plain")


# ---- the working set across the kinds of run --------------------------------------------------------
ROTATED = (("v2", EPS, 0), ("v1", EPS, 300), ("v2", EPS, 300), ("v2", EPS, 300), ("v2", EPS, 150), ("v2", EPS2, 300), ("v2", EPS, 150))
# cl_last_region_mode after each run of ROTATED (default switches; with the count cache or the kept layout off): not derived by hand,
# observed on the commit before the working set became one struct -- the refactored handle reproduces it
MODES = [0, 0, 0, 2, 2, 0, 0]
MODES_OFF = [0] * len(ROTATED)


def _working_set(ch):
    """-> cl_last_region_mode after every rotated run"""
    X, Y = _xy()
    modes = []

    def rotated(k):
        variant, eps, cut = ROTATED[k]
        _check_plain(ch.cluster(variant, eps, M, cut), variant, eps, M, cut, ("rotated", k))
        modes.append(ch.last_region_mode())

    rotated(0)
    _check_plain(ch.cluster("block", EPS, M, 0), "block", EPS, M, 0, "block")
    got = ch.cluster_weighted(EPS, M, WX, WY)
    assert np.array_equal(got.labels, _weighted()), "weighted"
    check_table(X, Y, _weighted(), got, "weighted")
    assert np.array_equal(ch.neighbor_counts(EPS, 300), _counts(EPS, 300)), "exact counts"
    _check_plain(ch.cluster("v2", EPS, 129, 300), "v2", EPS, 129, 300, "minPts 129")
    for k in range(1, len(ROTATED)):
        rotated(k)
    _check_plain(ch.cluster("block", EPS, M, 300), "block", EPS, M, 300, "block behind rotated runs under a cut")
    return modes


def _handle(switch):
    ch = api.Chromosome(*_xy())
    if switch == "nocounts":
        ch.set_count_reuse(False)
    if switch == "nolayout":
        ch.set_layout_reuse(False)
    return ch


def test_request_does_not_leak():
    ch = _handle(None)
    try:
        _leak(ch)
    finally:
        ch.close()


def test_two_runs_in_flight():
    ch = _handle(None)
    try:
        _in_flight(ch)
    finally:
        ch.close()


def test_working_set_across_run_kinds():
    ch = _handle(None)
    try:
        modes = _working_set(ch)
    finally:
        ch.close()
    print("last_region_mode:", modes)
    assert modes == MODES


def _block_and_weighted_timing(ch):
    """one block and one weighted run, labels against the oracle -> [(ms_band, n_queried)] of the two"""
    out = []
    _check_plain(ch.cluster("block", EPS, M, 0), "block", EPS, M, 0, "block, timed")
    out.append((ch.timing()["ms_band"], ch.timing()["n_queried"]))
    got = ch.cluster_weighted(EPS, M, WX, WY)
    assert np.array_equal(got.labels, _weighted()), "weighted, timed"
    out.append((ch.timing()["ms_band"], ch.timing()["n_queried"]))
    return out


def test_timing_record_does_not_outlive_its_run():
    """the band time and the queried PETs that cl_get_timing reports belong to the run that was waited for: a block or a weighted run
    has neither, whatever the slot held before.

    The first FOUR runs of ROTATED, not five: a run that re-uses the counts of its eps (cl_last_region_mode 2: runs 3 and 4) queries
    its cut band only and reports n_queried == 0 by definition (include/cloops_hip.h: "0 = none ran"), so after five runs neither slot
    would hold a count to inherit.  Run 2 makes the words of its eps under a cut: the whole layout (n_queried > 0) and its band
    (ms_band > 0).  After four runs slot 0 holds run 2 and slot 1 holds run 3 (ms_band > 0); the block run then takes slot 0 and the
    weighted run slot 1, so each of the two figures has a slot it could be inherited from."""
    fresh = _handle(None)
    try:
        fresh.set_profiling(True)
        first = _block_and_weighted_timing(fresh)
    finally:
        fresh.close()
    assert first == [(0.0, 0), (0.0, 0)]
    ch = _handle(None)
    try:
        ch.set_profiling(True)
        for k, (variant, eps, cut) in enumerate(ROTATED[:4]):
            _check_plain(ch.cluster(variant, eps, M, cut), variant, eps, M, cut, ("rotated, timed", k))
            tm = ch.timing()
            if k == 2:                                                              # not vacuous: slot 0 holds both figures
                assert ch.last_region_mode() == 0 and tm["ms_band"] > 0 and 0 < tm["n_queried"] <= N
            if k == 3:                                                              # ... and slot 1 a band query's time
                assert ch.last_region_mode() == 2 and tm["ms_band"] > 0 and tm["n_queried"] == 0
        behind = _block_and_weighted_timing(ch)
    finally:
        ch.close()
    assert behind == [(0.0, 0), (0.0, 0)]


def test_exact_counts_write_no_slot():
    """cl_neighbor_counts enqueues no run and writes no result slot.  The handle has no result behind it, as ever (the workspace the
    distance statistics would read holds the counts' layout: cl_dist_summary refuses), so the slot is read through the next runs:
    the block run that takes the slot the counts worked in, and the weighted run behind it, report nothing of a region query, and the
    next plain run has the statistics of the one in front of the counts."""
    ch = _handle(None)
    try:
        ch.set_profiling(True)
        ch.cluster_async("v2", EPS, M, 0)
        _check_plain(ch.wait(copy=True), "v2", EPS, M, 0, "plain in front of exact counts")
        before = ch.dist_summary(0)
        assert np.array_equal(ch.neighbor_counts(EPS, 300), _counts(EPS, 300)), "exact counts"
        with pytest.raises(_lib.CloopsHipError) as ei:
            ch.dist_summary(0)
        assert ei.value.code == _lib.CL_ERR_ARG
        assert _block_and_weighted_timing(ch) == [(0.0, 0), (0.0, 0)]
        ch.cluster_async("v2", EPS, M, 0)
        _check_plain(ch.wait(copy=True), "v2", EPS, M, 0, "plain behind exact counts")
        after = ch.dist_summary(0)
        assert all(np.array_equal(before[k], after[k]) for k in ("n_all", "n_pos", "loghist")), "the same run, the same statistics"
    finally:
        ch.close()


@pytest.mark.parametrize("switch", [None, "nocounts", "nolayout"], ids=["default", "nocounts", "nolayout"])
def test_every_form_on_one_handle(switch):
    """the three sequences one after the other on one handle, also with the count cache and with the kept layout switched off"""
    ch = _handle(switch)
    try:
        _leak(ch)
        _in_flight(ch)
        modes = _working_set(ch)
        _leak(ch)
    finally:
        ch.close()
    print("last_region_mode (%s):" % switch, modes)
    assert modes == (MODES if switch is None else MODES_OFF)
