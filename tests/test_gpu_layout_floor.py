"""GPU: an eps' base layout without the rows far below the sweep's cut (cl_chrom::Base::floor_q, cl_base_rows).

Inside an announced sweep the layout that a run under a cut builds leaves out the rows with Y - X < cut / 2; a later run of the eps
whose cut lies below that floor rebuilds the layout with every row.  Every run of every chain here is compared with the sequential C
oracle at the cut the chain handed in (oracle.single_dbscan), the way test_gpu_sweeps.test_chain_equals_oracle_on_one_chromosome does:
PETs that entered, inter- / self-ligation boxes, the estimator's cut and fragment size from the oracle's distance lists, and the
surviving candidate boxes of the whole chain.  cl_base_rows tells "floored" from "rebuilt".

Chromosomes: synth_chrom at 100 k - 200 k PETs on chr1 scaled to 1/83 of its length (the strips as full as on the 200 M genome)."""
import numpy as np
import pytest

import oracle
from cloops_amd import api, pipe, ests
from cloops_amd.synth import synth_chrom

pytestmark = pytest.mark.gpu

CHR1_LEN = 248956422
DCUM_BINS = 65537                                         # the upload's distance histogram: a floor needs cut / 2 below it


def _chrom(n=200000, seed=9100):
    return synth_chrom(n, CHR1_LEN // 83, seed)


def _rows_at(X, Y, floor):
    return int(((Y.astype(np.int64) - X) >= floor).sum())


def _chain(X, Y, eps, mps, forced, variant="v2", traversal=None):
    """the chained sweep over one chromosome with the cuts of `forced` (None: the step's own estimate) against the oracle, run by run
    -> [(eps, minPts, cut_in, cl_base_rows behind the run)]"""
    pipe.CACHE.clear()
    f = pipe.CACHE.put_arrays("chrF-chrF", X, Y)
    seen_rows = []
    try:
        if traversal is not None:
            pipe.CACHE.get(f).chrom.set_traversal(traversal)
        probe = lambda ff, ep, m, cut_in, res: seen_rows.append((ep, m, cut_in, pipe.CACHE.get(ff).chrom.base_rows()))
        forced = list(forced) + [None] * (len(eps) * len(mps) - len(forced))
        dataI, final_cut, cuts, steps = pipe.runSweepFast([f], eps, mps, cut=0, variant=variant, forced_cuts=forced, probe=probe)
        settings = [(ep, m) for ep in eps for m in mps]
        assert len(steps) == len(settings) == len(seen_rows)
        d = Y.astype(np.int64) - X
        dmin = int(d.min())
        v0 = dmin if variant == "v1" else 0                 # the layout's q is Y - X - v0
        cut, seen, want_rows, want_cuts = 0, set(), [], []
        layout_eps, floor = None, 0                         # the rule of the layout's floor, step by step
        for k, ((ep, m), st) in enumerate(zip(settings, steps)):
            eff = cut if cut > dmin else 0                  # (a cut that removes nothing is no cut)
            if layout_eps != ep:
                layout_eps, floor = ep, (eff // 2 if (eff // 2 < DCUM_BINS and eff // 2 > v0) else 0)
            elif eff < floor:
                floor = 0
            assert seen_rows[k][3] == int((d >= floor).sum()), (ep, m, cut, floor)
            ref = oracle.single_dbscan(variant, X, Y, ep, m, cut)
            rI = ref["dataI"]
            assert st["cut_in"] == cut and seen_rows[k][:3] == (ep, m, cut)
            assert (st["n_inter"], st["n_self"]) == (len(rI), len(ref["dataS"])), (ep, m, cut)
            assert st["n_in"] == int((d >= cut).sum()), (ep, m, cut)
            for b in rI:                                    # combineTwice: first appearance of an exact box wins
                if tuple(b) not in seen:
                    want_rows.append(b)
            seen.update(tuple(b) for b in rI)
            nxt = None
            if len(rI) and len(ref["dis"]) and len(ref["dss"]):
                cut2, frags = ests.estIntSelCutFrag(ref["dis"], ref["dss"])
                assert st["frags"] == frags, (ep, m, cut)
                if forced[k] is None:
                    assert st["cut_out"] == cut2, (ep, m, cut)
                nxt = cut2
            if forced[k] is not None:
                nxt = int(forced[k])
                assert st["cut_out"] == nxt
            if nxt is not None:
                want_cuts.append(nxt)
                cut = nxt
        assert final_cut == min(c for c in want_cuts if c > 0)
        want = np.asarray(want_rows, dtype=np.int64).reshape(-1, 4)
        want = want[((want[:, 2] + want[:, 3]) // 2 - (want[:, 0] + want[:, 1]) // 2) >= final_cut]      # filterClusterByDis
        got = dataI[("chrF", "chrF")]["boxes"] if ("chrF", "chrF") in dataI else np.zeros((0, 4), np.int64)
        order = lambda a: a[np.lexsort(a.T[::-1])]
        assert np.array_equal(order(np.asarray(got, dtype=np.int64).reshape(-1, 4)), order(want))
        return seen_rows
    finally:
        pipe.CACHE.clear()


@pytest.mark.parametrize("variant", ["v2", "v1"])
def test_floor_is_kept_above_it_and_dropped_below_it(variant):
    """inside eps 7500 the cuts are 4000 (the layout is built: floor 2000), 2500 (>= the floor: the same layout) and 1500 (below it:
    rebuilt with every row); eps 10000 then builds under 1500 (floor 750)"""
    X, Y = _chrom()
    n = len(X)
    rows = _chain(X, Y, [5000, 7500, 10000], [50, 30, 20], [None, None, 4000, 2500, 1500, 1500], variant)
    assert [r[3] for r in rows[:3]] == [n, n, n]                                      # eps 5000: built at cut 0
    assert rows[3][2:] == (4000, _rows_at(X, Y, 2000)) and rows[4][2:] == (2500, _rows_at(X, Y, 2000))
    assert rows[3][3] < n
    assert rows[5][2:] == (1500, n)
    assert rows[6][2:] == (1500, _rows_at(X, Y, 750)) and rows[6][3] < n


def test_floor_and_cut_in_one_rotated_cell():
    """eps 10000 under cut 3000: the floor (1500) and the cut go through the same rotated cell of every strip -- variant 2's cell
    minima of the floored layout are wrong exactly there, where the cut's own pass recomputes them"""
    X, Y = _chrom(seed=9101)
    rows = _chain(X, Y, [5000, 10000], [30, 20], [None, 3000], "v2")
    assert rows[2][2:] == (3000, _rows_at(X, Y, 1500)) and rows[2][3] < len(X)


def test_strips_emptied_by_the_floor_and_a_chromosome_of_short_pets():
    X, Y = _chrom(seed=9102)
    X, Y = X.astype(np.int64), Y.astype(np.int64)
    p, d = X + Y, Y - X
    rng = np.random.default_rng(5)
    short = np.minimum(d, rng.integers(50, 1500, len(X)))
    lo, hi, mid = p < p.min() + 20000, p > p.max() - 20000, np.abs(p - (p.min() + p.max()) // 2) < 15000
    Y = np.where(lo | mid, X + short, Y)                    # (X + Y only falls: the first strips hold nothing but these rows)
    X = np.where(hi, Y - short, X)                          # (X + Y only rises: the same for the last strips)
    X, Y = X.astype(np.int32), Y.astype(np.int32)
    rows = _chain(X, Y, [5000, 7500], [30, 20], [None, 4000], "v2")
    assert rows[2][2:] == (4000, _rows_at(X, Y, 2000)) and rows[2][3] < len(X)
    # short PETs only: the floor removes every row
    Xs, Ys = _chrom(100000, 9103)
    Ys = (Xs.astype(np.int64) + np.minimum(Ys.astype(np.int64) - Xs, rng.integers(50, 1500, len(Xs)))).astype(np.int32)
    rows = _chain(Xs, Ys, [5000, 7500], [30, 20], [None, 4000, 4000], "v2")
    assert rows[2][2:] == (4000, 0) and rows[3][2:] == (4000, 0)


@pytest.mark.parametrize("target", [2048 * 50 - 1, 2048 * 50, 2048 * 50 + 1, 1024 * 101 - 1, 1024 * 101 + 1])
def test_rows_at_tile_edges(target):
    """the floored layout ends one short of, on and one behind an edge of the list tiles (2048 positions) and of the region query's
    (1024)"""
    X, Y = _chrom(seed=9104)
    alive = np.flatnonzero((Y.astype(np.int64) - X) >= 2000)
    assert len(alive) > target
    drop = alive[target:]                                   # rows above the floor, left out of the chromosome
    keep = np.ones(len(X), bool)
    keep[drop] = False
    X, Y = X[keep], Y[keep]
    assert _rows_at(X, Y, 2000) == target
    rows = _chain(X, Y, [5000, 7500], [30, 20], [None, 4000, 2600], "v2")
    assert rows[2][2:] == (4000, target) and rows[3][2:] == (2600, target)


@pytest.mark.parametrize("level", [3, 4])
def test_traversal_levels_on_a_floored_chain(level):
    X, Y = _chrom(seed=9105)
    rows = _chain(X, Y, [5000, 7500], [30, 20], [None, 4000, 3000], "v2", traversal=level)
    assert rows[2][3] == rows[3][3] == _rows_at(X, Y, 2000) < len(X)


def test_row_aligned_labels_on_a_floored_layout():
    X, Y = _chrom(seed=9106)
    ch = api.Chromosome(X, Y, device=0)
    try:
        ch.sweep_plan([5000, 7500], [30, 20])
        for eps, m, cut in ((5000, 30, 0), (7500, 30, 4000), (7500, 20, 2500)):
            got = ch.cluster("v2", eps, m, cut).labels
            want = oracle.single_dbscan("v2", X, Y, eps, m, cut)["labels"]
            assert np.array_equal(got, want), (eps, m, cut)
            if cut:
                assert ch.base_rows() == _rows_at(X, Y, 2000) < len(X)
                assert (got[(Y.astype(np.int64) - X) < 2000] == -1).all()
        ch.sweep_plan([], [])
        # a one-off run outside a plan keeps every row
        got = ch.cluster("v2", 10000, 30, 4000).labels
        assert np.array_equal(got, oracle.single_dbscan("v2", X, Y, 10000, 30, 4000)["labels"]) and ch.base_rows() == len(X)
    finally:
        ch.close()


def test_no_floor_beyond_the_distance_histogram():
    """cut / 2 at or beyond the upload's distance histogram: the host cannot know the rows of a floored layout -- no floor"""
    X, Y = _chrom(seed=9107)
    rows = _chain(X, Y, [5000, 7500], [30, 20], [None, 2 * DCUM_BINS, 2 * DCUM_BINS + 2], "v2")
    assert rows[2][2:] == (2 * DCUM_BINS, len(X)) and rows[3][3] == len(X)
