"""Pins the C oracle against the labels the REAL reference classes produced (tests/golden/families.npz and
tests/golden/reference_checks.npz, made by tests/golden/make_golden.py and make_golden_reference_checks.py).

Plain equality of label arrays (ids included) on the adversarial families of SURVEY.md
Appendix A plus a clumpy family, for all three variants."""
import numpy as np
import pytest

import golden_util as G
import oracle


def _check(variant, family, k, ids, X, Y, eps, minPts):
    ref = G.oracle_reference_labels(family, k, variant)
    got = oracle.labels(variant, X, Y, eps, minPts)
    assert np.array_equal(ref, got), (variant, eps, minPts, len(X), int((ref != got).sum()))
    return ref


@pytest.mark.parametrize("variant", ["v1", "v2", "block"])
@pytest.mark.parametrize("family,seed,ncase", [("adversarial", 0, 120), ("plain", 1, 120), ("clumpy", 2, 120)])
def test_oracle_matches_reference(variant, family, seed, ncase):
    nclustered = 0
    for k, ids, X, Y, eps, minPts in G.oracle_family(family, seed, ncase):
        ref = _check(variant, family, k, ids, X, Y, eps, minPts)
        nclustered += int((ref >= 0).sum())
    assert nclustered > 0
