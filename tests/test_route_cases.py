"""CPU only: the inputs of tests/test_gpu_routes.py are not empty.  Conditions on the data sets of tests/route_cases.py, checked
on the oracle alone, so that a GPU test on them cannot pass on "nothing is core"."""
import numpy as np
import pytest

import oracle
import route_cases as R

_counts = {}


def _exact(name):
    if name not in _counts:
        c = R.get(name)
        _counts[name] = oracle.neighbor_counts(c.X, c.Y, c.eps)
    return _counts[name]


@pytest.mark.parametrize("name,lo,hi", [("sparse", 0, 4), ("mid", 80, 250), ("long", 450, 10 ** 9)])
def test_mean_strip_population_band(name, lo, hi):
    """far from the shape thresholds of cl_launch_region (40 and 400), for both origins of the grid"""
    c = R.get(name)
    assert len(c.X) <= 30000
    for variant in ("v2", "v1"):
        assert lo <= len(c.X) // R.grid_strips(c.X, c.Y, c.eps, variant) <= hi, variant


def test_sparse_grid_declines_the_band_remap():
    c = R.get("sparse_grid")
    for variant in ("v2", "v1"):
        assert R.grid_strips(c.X, c.Y, c.eps, variant) > 8 * len(c.X)


@pytest.mark.parametrize("name", sorted(R.MAKERS))
def test_every_setting_forms_clusters_and_noise(name):
    """at least 2 clusters, 100 clustered PETs and 100 noise PETs among those the cut keeps, for every variant the GPU tests run.
    (minPts 1 has no noise by definition -- every PET is its own neighbour: there the rule is that NO kept PET is noise)"""
    c = R.get(name)
    assert len(c.X) <= 30000 and (c.X >= 0).all() and (c.X <= c.Y).all()
    for m, cut in R.settings(name):
        keep = c.Y - c.X >= cut
        for variant in ("v2", "v1", "block"):
            lab = oracle.single_dbscan(variant, c.X, c.Y, c.eps, m, cut)["labels"]
            assert (lab[~keep] == -1).all()
            assert len(np.unique(lab[lab >= 0])) >= 2, (variant, m, cut)
            assert int((lab >= 0).sum()) >= 100, (variant, m, cut)
            noise = int((lab[keep] < 0).sum())
            assert noise == 0 if m == 1 else noise >= 100, (variant, m, cut, noise)


def test_cuts_differ_in_what_they_keep():
    """every cut of a data set removes PETs and leaves others; 65535 and 65536 differ in a few rows"""
    for name in sorted(R.MAKERS):
        c = R.get(name)
        kept = [int((c.Y - c.X >= cut).sum()) for cut in sorted(set(cut for _, cut in R.settings(name)))]
        assert all(a > b for a, b in zip(kept, kept[1:])) and kept[-1] > 1000, (name, kept)


@pytest.mark.parametrize("name", R.DENSE)
def test_dense_sets_tell_the_variants_apart(name):
    c = R.get(name)
    assert any(not np.array_equal(oracle.single_dbscan("v1", c.X, c.Y, c.eps, m, cut)["labels"],
                                  oracle.single_dbscan("v2", c.X, c.Y, c.eps, m, cut)["labels"]) for m, cut in R.settings(name))


@pytest.mark.parametrize("name", R.DENSE)
def test_dense_sets_have_windows_past_the_staged_span(name):
    """exact counts above 255 (longer than any staged search) for at least a third of the PETs"""
    assert 3 * int((_exact(name) > 255).sum()) >= len(_exact(name))


def test_sparse_set_sits_on_the_class_boundary():
    cnt = _exact("sparse")
    assert (cnt == 128).any() and (cnt == 129).any() and (cnt >= 400).any()
    assert np.median(cnt) == 1
