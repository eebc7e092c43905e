"""GPU: blockDBSCAN's kernels (K6, cloops_amd/csrc/k_block.hip) on the constructed inputs of tests/block_cases.py -- labels, the number
of clusters and every row of the cluster table against the sequential oracle (oracle.single_dbscan("block", ...)), exact integer
equality, no tolerance anywhere.  tests/test_block_cases.py proves on the CPU that each family is what it says and that the rule it
aims at decides its labels.

One handle per data set and row permutation.  Every (minPts, cut) runs twice with the same answer (nothing hangs on the order of
the atomics), with a run of variant 1 on the same handle in between where the coordinates allow one (K6 keeps its cell arrays in
buffers the rotated variants use under other meanings), and once more without labels.

The grid refusals (CL_ERR_GRID) of run_block, run_weighted and make_grid return before anything is allocated or launched; the handle
then serves a valid request.  Nothing here runs just below a limit: that would allocate a table of 2^28 rows."""
import numpy as np
import pytest

import block_cases as BC
import oracle
from table_check import check_table, label_stats
from cloops_amd import _lib, api

pytestmark = pytest.mark.gpu

_ref = {}


def _want(variant, name, pn, X, Y, eps, m, cut):
    key = (variant, name, pn, eps, m, cut)
    if key not in _ref:
        _ref[key] = oracle.single_dbscan(variant, X, Y, eps, m, cut)["labels"]
    return _ref[key]


def _v1_fits(X, Y, eps):
    """make_grid takes this extent (and the strip table stays small)"""
    p = X + Y
    S = int(p.max() - p.min()) // eps + 1
    return S <= 1 << 22 and (S + 2) << int(eps - 1).bit_length() <= 2 ** 31 - 1


def _check(X, Y, want, got, tag):
    assert np.array_equal(got.labels, want), (tag, int((got.labels != want).sum()), np.flatnonzero(got.labels != want)[:8].tolist())
    assert got.n_clusters == label_stats(want)[0], tag
    check_table(X, Y, want, got, tag)


def _run_case(name):
    c = BC.get(name)
    for pn, X, Y, _ in BC.permuted(c):
        between = _v1_fits(X, Y, c.eps)
        ch = api.Chromosome(X, Y)
        try:
            for m, cut in c.runs:
                want = _want("block", name, pn, X, Y, c.eps, m, cut)
                first = ch.cluster("block", c.eps, m, cut)
                _check(X, Y, want, first, (name, pn, m, cut, "first"))
                if between:
                    got = ch.cluster("v1", c.eps, m, cut)
                    _check(X, Y, _want("v1", name, pn, X, Y, c.eps, m, cut), got, (name, pn, m, cut, "v1"))
                again = ch.cluster("block", c.eps, m, cut)
                _check(X, Y, want, again, (name, pn, m, cut, "again"))
                assert np.array_equal(first.labels, again.labels) and first.n_clusters == again.n_clusters
                got = ch.cluster("block", c.eps, m, cut, want_labels=False)
                assert got.labels is None
                check_table(X, Y, want, got, (name, pn, m, cut, "no labels"))
        finally:
            ch.close()


@pytest.mark.parametrize("eps", BC.CELL_EDGE_EPS)
def test_cell_edge(eps):
    for name in [n for n in BC.names("cell_edge") if int(n.split("_")[2]) == eps]:
        _run_case(name)


@pytest.mark.parametrize("name", BC.names("row_wrap") + ["centroid_tie", "pair_loop", "core_threshold", "border_rank", "components", "cut_anchor"])
def test_family(name):
    _run_case(name)


def test_variant_1_runs_in_between_somewhere():
    """the run of variant 1 between two block runs is not left out everywhere"""
    fits = {n: _v1_fits(BC.get(n).X, BC.get(n).Y, BC.get(n).eps) for n in BC.names()}
    assert all(fits[n] for n in ("pair_loop", "core_threshold", "border_rank", "components", "cut_anchor", "row_wrap_1", "cell_edge_17"))
    assert not fits["centroid_tie"]                              # (it spans the domain: X + Y leaves make_grid's range)


# ---- grid refusals --------------------------------------------------------------------------------------------------------------
WIDE_X = np.asarray([0, 3, (1 << 28) + 1], np.int64)             # an X extent of 2^28 + 1, 0 <= X <= Y
WIDE_Y = np.asarray([1, 4, (1 << 28) + 5], np.int64)
FULL = np.asarray([-(BC.LIM - 1), -(BC.LIM - 1) + 3, BC.LIM - 1], np.int64)       # X + Y spans 2^31 - 4


def _refused(call):
    with pytest.raises(_lib.CloopsHipError) as e:
        call()
    assert e.value.code == _lib.CL_ERR_GRID, e.value


def _valid(ch, X, Y):
    """eps 1000, minPts 2 on the same handle: the first two PETs are a cluster"""
    want = oracle.single_dbscan("block", X, Y, 1000, 2)["labels"]
    assert want.tolist() == [0, 0, -1]
    _check(X, Y, want, ch.cluster("block", 1000, 2), "valid")


def test_block_refuses_more_than_2_28_cell_rows():
    assert (WIDE_X.max() - WIDE_X.min()) // 1 + 1 > 1 << 28      # run_block's R
    ch = api.Chromosome(WIDE_X, WIDE_Y)
    try:
        _refused(lambda: ch.cluster("block", 1, 2))
        _valid(ch, WIDE_X, WIDE_Y)
        _refused(lambda: ch.cluster("block", 1, 2, 3))           # under a cut the table still spans the upload's extent
        _valid(ch, WIDE_X, WIDE_Y)
    finally:
        ch.close()


def test_weighted_refuses_more_than_2_28_strips():
    assert ((WIDE_X + WIDE_Y).max() - (WIDE_X + WIDE_Y).min()) // 1 + 1 > 1 << 28      # run_weighted's S at weights (1, 1)
    ch = api.Chromosome(WIDE_X, WIDE_Y)
    try:
        _refused(lambda: ch.cluster_weighted(1, 2, 1, 1))
        _valid(ch, WIDE_X, WIDE_Y)
        got = ch.cluster_weighted(1000, 2, 1, 1)
        _check(WIDE_X, WIDE_Y, oracle.labels("v1", WIDE_X, WIDE_Y, 1000, 2), got, "weighted")
    finally:
        ch.close()


@pytest.mark.parametrize("variant", ["v1", "v2"])
def test_rotated_refuses_more_than_2_28_strips(variant):
    p = WIDE_X + WIDE_Y
    assert int(p.max()) // 1 - int(p.min()) // 1 + 1 > 1 << 28   # make_grid's S
    ch = api.Chromosome(WIDE_X, WIDE_Y)
    try:
        _refused(lambda: ch.cluster(variant, 1, 2))
        _valid(ch, WIDE_X, WIDE_Y)
        got = ch.cluster(variant, 1000, 2)
        _check(WIDE_X, WIDE_Y, oracle.labels(variant, WIDE_X, WIDE_Y, 1000, 2), got, variant)
    finally:
        ch.close()


def test_rotated_refuses_an_extent_the_strip_coordinate_cannot_hold():
    eps = 1025
    p = FULL + FULL
    S = int(p.max() - p.min()) // eps + 1
    assert S <= 1 << 28 and (S + 2) << int(eps - 1).bit_length() > 2 ** 31 - 1      # make_grid's second refusal, not its first
    ch = api.Chromosome(FULL, FULL)
    try:
        _refused(lambda: ch.cluster("v1", eps, 2))
        _valid(ch, FULL, FULL)
    finally:
        ch.close()
