"""GPU: every route of the region query against the sequential oracle (bit-exact, no tolerance anywhere).

minPts 2 .. 128 runs on the clustering kernels (k_region_core / k_region_keys) with the count cache; minPts 1, minPts >= 129 and the
exact counts of cl_neighbor_counts share k_region_count: no cache, traversal level <= 3 on a copy of the layout, plain counts as words.
The data sets of tests/route_cases.py form clusters at minPts in the hundreds (tests/test_route_cases.py pins that on the CPU), so
that this second class is asked for more than "nothing is core"."""
import ctypes

import numpy as np
import pytest

import oracle
import route_cases as R
from cloops_amd import _lib, api
from table_check import check_table

pytestmark = pytest.mark.gpu

ROT = ["v2", "v1"]
_ref = {}
_cnt = {}


def _oracle(name, variant, m, cut):
    """oracle.single_dbscan of one setting, computed once per module"""
    key = (name, variant, m, cut)
    if key not in _ref:
        c = R.get(name)
        _ref[key] = oracle.single_dbscan(variant, c.X, c.Y, c.eps, m, cut)
    return _ref[key]


def _counts(name, cut=0):
    """oracle.neighbor_counts of the rows the cut keeps, at those rows; -1 elsewhere (include/cloops_hip.h, cl_neighbor_counts)"""
    key = (name, cut)
    if key not in _cnt:
        c = R.get(name)
        keep = c.Y - c.X >= cut
        out = np.full(len(c.X), -1, np.int32)
        out[keep] = oracle.neighbor_counts(c.X[keep], c.Y[keep], c.eps)
        _cnt[key] = out
    return _cnt[key]


def _check(got, name, variant, m, cut, boxes=True, tag=None):
    c = R.get(name)
    want = _oracle(name, variant, m, cut)["labels"]
    assert np.array_equal(got.labels, want), (name, variant, m, cut, tag, int((got.labels != want).sum()))
    assert got.n_clusters == len(np.unique(want[want >= 0])), (name, variant, m, cut, tag)
    if boxes:
        check_table(c.X, c.Y, want, got, (name, variant, m, cut, tag))     # every row of the cluster table


def _cached_class(m):
    return 2 <= m <= 128


# ---- the minPts classes ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["v2", "v1", "block"])
@pytest.mark.parametrize("name", ["sparse", "mid", "long"])
def test_min_pts_classes(name, variant):
    """labels, number of clusters and every row of the cluster table on both sides of 128 and of 1, without and with a cut;
    a run outside 2 .. 128 makes a full region query every time"""
    c = R.get(name)
    ch = api.Chromosome(c.X, c.Y)
    try:
        for cut in (0, c.cut):
            for m in c.min_pts:
                got = ch.cluster(variant, c.eps, m, cut)
                if variant != "block" and not _cached_class(m):
                    assert ch.last_region_mode() == 0, (m, cut)
                _check(got, name, variant, m, cut)
    finally:
        ch.close()


# ---- levels and switches at minPts > 128 ------------------------------------------------------------
@pytest.mark.parametrize("counts", [True, False], ids=["counts", "nocounts"])
@pytest.mark.parametrize("layout", [True, False], ids=["layout", "nolayout"])
@pytest.mark.parametrize("level", [0, 2, 3, 4])
@pytest.mark.parametrize("name", R.DENSE)
def test_levels_and_switches_above_128(name, level, layout, counts):
    """the run falls to level min(traversal, 3) with uncached words whatever the switches say: same labels every time"""
    c = R.get(name)
    ch = api.Chromosome(c.X, c.Y)
    try:
        ch.set_traversal(level)
        ch.set_layout_reuse(layout)
        ch.set_count_reuse(counts)
        for variant in ROT:
            for m in R.LEVEL_MIN_PTS:
                for cut in (0, c.cut):
                    got = ch.cluster(variant, c.eps, m, cut)
                    assert ch.last_region_mode() == 0
                    _check(got, name, variant, m, cut, boxes=False, tag=(level, layout, counts))
    finally:
        ch.close()


# ---- one handle across the classes ----------------------------------------------------------------
@pytest.mark.parametrize("variant", ROT)
def test_one_handle_across_the_classes(variant):
    """an uncacheable run between cached runs neither uses nor damages the base layout, the count cache and variant 2's cell minima:
    every run of the announced sweep equals the oracle and a fresh handle"""
    c = R.get("mid")
    ch = api.Chromosome(c.X, c.Y)
    try:
        ch.sweep_plan([c.eps], list(R.ONE_HANDLE_MIN_PTS))
        for m, cut in R.one_handle_runs():
            got = ch.cluster(variant, c.eps, m, cut)
            if not _cached_class(m):
                assert ch.last_region_mode() == 0, (m, cut)
            _check(got, "mid", variant, m, cut)
            fresh = api.Chromosome(c.X, c.Y)
            try:
                alone = fresh.cluster(variant, c.eps, m, cut)
            finally:
                fresh.close()
            assert np.array_equal(got.labels, alone.labels) and got.n_clusters == alone.n_clusters and got.max_label == alone.max_label, (m, cut)
            assert np.array_equal(got.boxes, alone.boxes), (m, cut)
    finally:
        ch.close()


# ---- refusals --------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ROT)
def test_list_forms_are_refused_above_128(variant):
    """the pairs and row-mask forms need the list form of a run with cached words: minPts 129 is an argument error, nothing is in
    flight afterwards (cl_cluster refuses a handle with runs in flight) and the handle's next run equals the oracle"""
    c = R.get("mid")
    ch = api.Chromosome(c.X, c.Y)
    try:
        _check(ch.cluster(variant, c.eps, 128, c.cut), "mid", variant, 128, c.cut)
        for enqueue in (ch.cluster_pairs_async, ch.cluster_rowmask_async):
            with pytest.raises(_lib.CloopsHipError) as ei:
                enqueue(variant, c.eps, 129, c.cut)
            assert ei.value.code == _lib.CL_ERR_ARG
            assert ch._inflight == []
            _check(ch.cluster(variant, c.eps, 129, c.cut), "mid", variant, 129, c.cut)
            _check(ch.cluster(variant, c.eps, 128, c.cut), "mid", variant, 128, c.cut)
    finally:
        ch.close()


# ---- sweep step ------------------------------------------------------------------------------------
def _combined(step_boxes, final_cut):
    """combineTwice + filterClusterByDis (cLoops/pipe.py:130-174) on lists of [minX, maxX, minY, maxY], in append order"""
    out, known = [], set()
    for boxes in step_boxes:
        new = [b for b in boxes if tuple(b) not in known]
        out += new
        known |= set(tuple(b) for b in new)
    return [b for b in out if (b[2] + b[3]) // 2 - (b[0] + b[1]) // 2 >= final_cut]


@pytest.mark.parametrize("m", R.LEVEL_MIN_PTS)
@pytest.mark.parametrize("variant", ROT)
def test_sweep_step_above_128(variant, m):
    """cl_cluster_step_async on uncached words: the classification of the table, the distance summary and the candidates of two
    chained steps (cut 0, then the data set's cut) against the oracle's lists"""
    from test_gpu_dist_stats import _check_sums
    c = R.get("mid")
    ch = api.Chromosome(c.X, c.Y)
    try:
        ch.set_device_labels(False)
        ch.cand_reset()
        ch.sweep_plan([c.eps], [m])
        inter = []
        for step, cut in enumerate((0, c.cut)):
            ref = _oracle("mid", variant, m, cut)
            ch.step_async(variant, c.eps, m, cut, step)
            assert ch.last_region_mode() == 0
            ch.wait()
            ni, ns, st = ch.step_result()
            assert (ni, ns) == (len(ref["dataI"]), len(ref["dataS"])), (step, cut)
            assert ni + ns >= 2
            assert st["n_all"] == [len(ref["dis"]), len(ref["dss"])]
            _check_sums(st, 0, ref["dis"])
            _check_sums(st, 1, ref["dss"])
            inter.append(ref["dataI"])
        want = _combined(inter, c.cut)
        got = ch.cand_finish(c.cut, sum(len(b) for b in inter))
        assert len(want) > 0 and got.tolist() == want
    finally:
        ch.close()


def test_sweep_fast_equals_sweep_across_128():
    """the sweep driver over minPts 160, 129, 100 on one chromosome: the fused steps against the reference-shaped sweep"""
    from cloops_amd import pipe
    c = R.get("mid")
    pipe.CACHE.clear()
    fs = [pipe.CACHE.put_arrays("chrR-chrR", c.X, c.Y)]
    try:
        fast = pipe.runSweepFast(fs, [c.eps], list(R.SWEEP_MIN_PTS), cut=0)
        slow = pipe.runSweep(fs, [c.eps], list(R.SWEEP_MIN_PTS), cut=0)
        assert fast[1] == slow[1] and fast[2] == slow[2]
        assert [s.get("cut_out") for s in fast[3]] == [s.get("cut_out") for s in slow[3]]
        assert [s["n_in"] for s in fast[3]] == [s["n_in"] for s in slow[3]]
        assert fast[0].keys() == slow[0].keys() and len(fast[0]) == 1
        for k in fast[0]:
            want = np.asarray([[r[1], r[2], r[4], r[5]] for r in slow[0][k]["records"]], dtype=np.int64).reshape(-1, 4)
            assert len(want) > 0 and np.array_equal(fast[0][k]["boxes"], want), k
    finally:
        pipe.CACHE.clear()


# ---- exact counts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "mid", "long"])
def test_exact_counts(name):
    """cl_neighbor_counts where its searches leave the common path: windows past the 31st and the 120th position, strips longer than
    255, strips outside the staged window.  Under a cut: the counts among the kept rows, -1 at the rows the cut removes."""
    c = R.get(name)
    ch = api.Chromosome(c.X, c.Y)
    try:
        for cut in (0, c.cut, 0):
            got = ch.neighbor_counts(c.eps, cut)
            want = _counts(name, cut)
            assert np.array_equal(got, want), (name, cut, int((got != want).sum()))
            assert (got[c.Y - c.X < cut] == -1).all() and (got[c.Y - c.X >= cut] >= 1).all()
    finally:
        ch.close()


def test_exact_counts_without_layout_reuse_and_between_runs():
    """every call sorts for itself (the cut rides in the keys); and on a handle with cached words of the same eps the counts neither
    use nor damage them"""
    c = R.get("long")
    ch = api.Chromosome(c.X, c.Y)
    try:
        ch.set_layout_reuse(False)
        for cut in (c.cut, 0):
            assert np.array_equal(ch.neighbor_counts(c.eps, cut), _counts("long", cut)), cut
    finally:
        ch.close()
    ch = api.Chromosome(c.X, c.Y)
    try:
        _check(ch.cluster("v1", c.eps, 128, 0), "long", "v1", 128, 0)
        assert np.array_equal(ch.neighbor_counts(c.eps, c.cut), _counts("long", c.cut))
        _check(ch.cluster("v1", c.eps, 128, c.cut), "long", "v1", 128, c.cut)
        _check(ch.cluster("v1", c.eps, 129, c.cut), "long", "v1", 129, c.cut)
    finally:
        ch.close()


# ---- sparse grid and large cut ----------------------------------------------------------------------
@pytest.mark.parametrize("m", [3, 5])
@pytest.mark.parametrize("variant", ROT)
def test_sparse_grid_under_a_changing_cut(variant, m):
    """more than 8 strips per PET: the band re-map is declined, every new cut makes its words again; only the repeated cut finds them"""
    c = R.get("sparse_grid")
    ch = api.Chromosome(c.X, c.Y)
    try:
        modes = []
        for cut in R.SPARSE_GRID_CUTS:
            got = ch.cluster(variant, c.eps, m, cut)
            modes.append(ch.last_region_mode())
            _check(got, "sparse_grid", variant, m, cut)
        assert modes == [0, 0, 0, 0, 1], modes
    finally:
        ch.close()


@pytest.mark.parametrize("level", [4, 3])
@pytest.mark.parametrize("variant", ROT)
def test_cuts_past_the_distance_histogram(variant, level):
    """a cut of 65536 and more: the upload's histogram does not tell how many PETs pass, the run learns it on the device"""
    c = R.get("large_cut")
    ch = api.Chromosome(c.X, c.Y)
    try:
        ch.set_traversal(level)
        for m in c.min_pts:
            for cut in R.LARGE_CUTS:
                got = ch.cluster(variant, c.eps, m, cut)
                _check(got, "large_cut", variant, m, cut, tag=level)
                assert ch.last_n_in() == int((c.Y - c.X >= cut).sum())
    finally:
        ch.close()
