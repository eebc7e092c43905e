"""GPU: the list kernels of k_lists.hip at their tile edges, halos, step caps, queue and "not staged" branches, against the sequential
oracle (bit-exact: labels, number of clusters, every row of the cluster table; no tolerance anywhere).

The inputs are the constructed cases of tests/lists_cases.py; tests/test_lists_cases.py proves on the CPU that each of them reaches the
path it names and that the answer depends on it.  Every case runs variant 2 and variant 1 at the traversal levels 4, 3 and 2 (the list
kernels) and at 1 and 0 (the tile kernels for the border rule, then for everything: the other implementation on the same inputs), every
run twice on its handle (the same labels both times: nothing may depend on the order of atomics).  A run whose kernels raise the device
overflow flag comes back as an error of cl_cluster, i.e. as an exception here: none of these cases may raise one."""
import numpy as np
import pytest

import lists_cases as LC
import oracle
from cloops_amd import api
from table_check import check_table

pytestmark = pytest.mark.gpu

ROT = ("v2", "v1")
LEVELS = (4, 3, 2, 1, 0)          # 4, 3, 2: the list kernels (2 and 3 differ in the label kernel only); 1: k_union_c with the tile kernels' border rule;
                                  # 0: the tile kernels over every PET, an implementation of their own
_ref = {}


def _oracle(name, variant, m, cut):
    key = (name, variant, m, cut)
    if key not in _ref:
        c = LC.get(name)
        _ref[key] = oracle.single_dbscan(variant, c.X, c.Y, c.eps, m, cut)["labels"]
    return _ref[key]


def _check(got, name, variant, m, cut, tag):
    c = LC.get(name)
    want = _oracle(name, variant, m, cut)
    assert np.array_equal(got.labels, want), (name, variant, m, cut, tag, int((got.labels != want).sum()))
    assert got.n_clusters == len(np.unique(want[want >= 0])), (name, variant, m, cut, tag)
    check_table(c.X, c.Y, want, got, (name, variant, m, cut, tag))         # every row of the cluster table


def _pairs_equal_rows(ch, name, variant, m, cut, tag):
    """the (row, label) pairs of cl_cluster_pairs_async, put back at their rows, are the row-aligned labels"""
    ch.cluster_pairs_async(variant, LC.get(name).eps, m, cut)
    res, pairs = ch.wait_pairs(copy=True)
    want = _oracle(name, variant, m, cut)
    lab = np.full(len(want), -1, np.int32)
    assert len(np.unique(pairs[:, 0])) == len(pairs)
    lab[pairs[:, 0]] = pairs[:, 1]
    assert np.array_equal(lab, want) and res.n_clusters == len(np.unique(want[want >= 0])), (name, variant, m, cut, tag)


def _run(name, pairs=False):
    """one handle: every level, both variants, the case's runs in their order, each run twice"""
    c = LC.get(name)
    ch = api.Chromosome(c.X, c.Y)
    try:
        for level in LEVELS:
            ch.set_traversal(level)
            for variant in ROT:
                for m, cut in c.runs:
                    got = ch.cluster(variant, c.eps, m, cut)
                    _check(got, name, variant, m, cut, level)
                    again = ch.cluster(variant, c.eps, m, cut)
                    assert np.array_equal(again.labels, got.labels) and again.n_clusters == got.n_clusters, (name, variant, m, cut, level)
                    if pairs and level >= 3:
                        _pairs_equal_rows(ch, name, variant, m, cut, level)
    finally:
        ch.close()


def _ladders(halo, spacing):
    return [n for n in LC.names("ladder") if LC.get(n).info["halo"] == halo and LC.get(n).info["spacing"] == spacing]


@pytest.mark.parametrize("spacing", [LC.EPS, LC.EPS + 2])
@pytest.mark.parametrize("halo", [512, 128])
def test_ladder(halo, spacing):
    """k_union_c's look-back for a chain head, the staged window and its shortcut, the overflow list and k_union_overflow: lines of
    127 .. 2049 cores in adjacent strips, exactly eps apart (one cluster) and eps + 2 (six)"""
    for name in _ladders(halo, spacing):
        _run(name)


@pytest.mark.parametrize("family", ["ladder_pad", "ladder_tile", "ladder_link", "broken_ladder"])
def test_ladder_at_the_tile_edges(family):
    """a strip below that begins one core in front of, at and behind the first staged core; a line that begins one core in front of,
    at and behind a tile; two strips whose only link are three cores of the overflow list; a window that touches two chains (staged and
    on the overflow list), doubled cores at a chain's tail and head"""
    for name in LC.names(family):
        _run(name)


def test_cell_across_a_tile():
    """variant 2's cell minimum where the cell runs on behind the tile of k_classify / k_base_keys by 1 .. 299 PETs"""
    for name in LC.names("cell_tile"):
        _run(name)


@pytest.mark.parametrize("min_pts", LC.WALL_MIN_PTS)
def test_miss_walls(min_pts):
    """k_border_q / k_border_w: 0 .. 300 cores to step over in front of a walker's only neighbour, one strip up and one strip down, at
    a tile's last and first position; with K2's hints (minPts 5) and without (129)"""
    for name in LC.names("miss_wall"):
        if LC.get(name).info["min_pts"] == min_pts:
            _run(name)


def test_hints_that_leave_their_field():
    for name in LC.names("wall_population"):
        _run(name)


def test_four_corners():
    """a walker with four adjacent components, in two row orders, on both sides of a tile edge, the owner behind a wall; also as pairs"""
    for name in LC.names("corners") + LC.names("corners_wall"):
        _run(name, pairs=True)


def test_crowded_tile():
    """more than 256 walkers in a tile of k_border_q, more open walks than the queue holds; also as pairs"""
    for name in LC.names("crowded"):
        _run(name, pairs=True)


@pytest.mark.parametrize("name", ["cut_ladder()", "cut_wall()"])
@pytest.mark.parametrize("level", LEVELS)
def test_under_a_cut(name, level):
    """a run at cut 0, then the run under the cut on the same handle (the counts of the first run, at level 4 the band query; the
    hints shifted by what the cut removes), twice; and the run under the cut on a fresh handle"""
    c = LC.get(name)
    for variant in ROT:
        ch = api.Chromosome(c.X, c.Y)
        try:
            ch.set_traversal(level)
            first = None
            for m, cut in c.runs + c.runs[-1:]:
                got = ch.cluster(variant, c.eps, m, cut)
                _check(got, name, variant, m, cut, level)
                first = got if cut else first
        finally:
            ch.close()
        m, cut = c.runs[-1]
        assert cut > 0
        ch = api.Chromosome(c.X, c.Y)
        try:
            ch.set_traversal(level)
            alone = ch.cluster(variant, c.eps, m, cut)
            _check(alone, name, variant, m, cut, (level, "fresh"))
            assert np.array_equal(alone.labels, first.labels)
        finally:
            ch.close()
