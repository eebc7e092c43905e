"""CPU: the host arithmetic that turns the sweep's reduced distance statistics into a cut (ests.py,
pipe.runSweepFast) on inputs where it is fragile -- groups of (nearly) equal distances, 2**cut on
or near an integer -- against the reference's estIntSelCutFrag on the distance lists; and the
log bins of the exact median (ests.logbin / logbin_range) over all 3840 bins."""
import math

import numpy as np
import pytest

import dist_stats_cases as C
import fake_backend
from cloops_amd import api, ests, pipe


@pytest.fixture()
def fake_gpu(monkeypatch):
    monkeypatch.setattr(api, "Chromosome", fake_backend.FakeChromosome)
    monkeypatch.setattr(api, "device_count", lambda: 1)
    pipe.CACHE.clear()
    yield
    pipe.CACHE.clear()


# ---- the sweep chain on degenerate groups ----------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_sweep_fast_chain_on_degenerate_groups(fake_gpu, tmp_path, name):
    """runSweepFast (statistics) == runSweep (the oracle's dis / dss lists through estIntSelCutFrag).  With a
    degenerate group the one-pass squared deviation cancels to noise -- negative on self_equal, where it used to
    end in int(2 ** nan)"""
    X, Y = C.case(name)
    f = C.write_jd(tmp_path, "chrA", X, Y)
    want = pipe.runSweep([f], [500, 1000], [5], cut=C.CUT)
    got = pipe.runSweepFast([f], [500, 1000], [5], cut=C.CUT)
    assert got[2] == want[2] and got[1] == want[1]
    assert [s.get("frags") for s in got[3]] == [s.get("frags") for s in want[3]]
    assert all(math.isfinite(c) for c in got[2])


def test_sweep_fast_self_equal_is_the_reference_value(fake_gpu, tmp_path):
    """the repro of the NaN cut: 1001 PETs at 33333 below cut 40000 -> (33333, 33332) from the lists, settled by the
    recheck (the statistics cannot tell 2**cut from the integer 33333)"""
    X, Y = C.case("self_equal")
    f = C.write_jd(tmp_path, "chrA", X, Y)
    _, cut, cuts, steps = pipe.runSweepFast([f], [500], [5], cut=C.CUT)
    assert cuts == [C.CUT, 33333] and steps[0]["frags"] == 33332
    assert steps[0].get("cut_rechecked")


def test_sweep_fast_two_chromosomes_degenerate(fake_gpu, tmp_path):
    """the statistics of two chromosomes are summed on the host before the cut"""
    fs = [C.write_jd(tmp_path, "chr%d" % k, *C.case(nm, seed=k)) for k, nm in ((1, "self_equal"), (2, "both_equal"))]
    want = pipe.runSweep(fs, [500, 1000], [5], cut=C.CUT)
    got = pipe.runSweepFast(fs, [500, 1000], [5], cut=C.CUT)
    assert got[2] == want[2]


def test_sweep_fast_several_ranks_stays_finite(fake_gpu, tmp_path):
    """with `allsum` (several ranks) there is no recheck: the cut comes from the statistics, finite, inside the stated
    range, and that range contains the reference's cut"""
    X, Y = C.case("self_equal")
    f = C.write_jd(tmp_path, "chrA", X, Y)
    _, _, want, _ = pipe.runSweep([f], [500], [5], cut=C.CUT)
    _, _, cuts, steps = pipe.runSweepFast([f], [500], [5], cut=C.CUT, allsum=lambda a: a.copy())
    lo, hi = steps[0]["cut_range"]
    assert lo <= cuts[1] <= hi and lo <= want[1] <= hi
    assert not steps[0].get("cut_rechecked")


# ---- estIntSelCutFrag_bounded against estIntSelCutFrag ---------------------------------------------
def _sums(di, ds, order):
    """(n_all, n_pos, sumx, sumxx) as the reductions make them, in one of several summation orders"""
    out = ([], [], [], [])
    for a in (di, ds):
        a = np.abs(np.asarray(a, np.int64))
        out[0].append(len(a))
        a = a[a > 0]
        out[1].append(len(a))
        x = np.log2(a.astype(np.float64)) - 11.0
        if order == "pairwise":                         # numpy (the CPU stand-in of the backend)
            s, ss = float(np.sum(x)), float(np.sum(x * x))
        elif order == "step":                           # the sweep step's k7_summary: 256 x 1024 threads
            s, ss = C.grid_sum(x, 256, 1024), C.grid_sum(x * x, 256, 1024)
        else:                                           # cl_dist_summary: 2048 x 256
            s, ss = C.grid_sum(x, 2048, 256), C.grid_sum(x * x, 2048, 256)
        out[2].append(s)
        out[3].append(ss)
    return out


def _median_pair(ds):
    a = np.sort(np.abs(np.asarray(ds, np.int64)))
    a = a[a > 0]
    n = len(a)
    return int(a[(n - 1) // 2]), int(a[n // 2])


def _lists(rng, kind):
    n_i, n_s = rng.randint(2, 3000), rng.randint(2, 3000)
    di = rng.randint(10 ** 4, 10 ** 7, n_i)
    if kind == "spread":
        ds = np.exp(rng.uniform(np.log(50), np.log(40000), n_s)).astype(np.int64)
    elif kind == "equal":
        ds = np.full(n_s, rng.randint(1, 2 ** 30))
    elif kind == "equal_inter":
        ds = np.exp(rng.uniform(np.log(50), np.log(40000), n_s)).astype(np.int64)
        di = np.full(n_i, rng.randint(10 ** 4, 2 ** 30))
    elif kind == "near_equal":                       # one outlier in a sea of equal distances
        ds = np.full(n_s, rng.randint(100, 10 ** 6))
        ds[0] += 1
    else:                                            # two distances
        ds = rng.choice(rng.randint(100, 10 ** 6, 2), n_s)
    ds = ds * rng.choice([-1, 1], n_s)               # (signs: ests.py:42-43 takes |d|)
    if rng.rand() < 0.3:
        ds[: rng.randint(1, 4)] = 0                  # d = 0 counts in n_all only
    return di, ds


@pytest.mark.parametrize("kind", ["spread", "equal", "equal_inter", "near_equal", "two"])
def test_bounded_cut_contains_the_reference(kind):
    """on 200 seeded list pairs per kind and three summation orders: the reference's int(2 ** cut) lies inside the
    bound; where the bound is a single integer, the statistics' cut IS the reference's; where the two differ, the
    bound is wider than one integer (the recheck fires)"""
    rng = np.random.RandomState({"spread": 1, "equal": 2, "equal_inter": 3, "near_equal": 4, "two": 5}[kind])
    settled = 0
    for _ in range(200):
        di, ds = _lists(rng, kind)
        want = ests.estIntSelCutFrag(di, ds)
        for order in ("pairwise", "step", "summary"):
            n_all, n_pos, sx, sxx = _sums(di, ds, order)
            rcut, rfrags, (lo, hi), margin = ests.estIntSelCutFrag_bounded(n_all, n_pos, sx, sxx, 11.0, _median_pair(ds))
            assert lo <= want[0] <= hi, (kind, order, want, lo, hi)
            assert lo <= rcut <= hi
            assert rfrags == want[1]
            if lo == hi:
                settled += 1
                assert rcut == want[0]
    if kind == "spread":
        assert settled >= 0.95 * 600                 # the bound is not vacuous on ordinary data


def test_bounded_cut_on_an_integer():
    """2**cut exactly an integer (cut1 = log2 of a power of two with a zero spread): the bound straddles it"""
    ds = np.full(501, 4096)
    di = np.arange(10 ** 5, 10 ** 5 + 300)
    n_all, n_pos, sx, sxx = _sums(di, ds, "step")
    rcut, _, (lo, hi), margin = ests.estIntSelCutFrag_bounded(n_all, n_pos, sx, sxx, 11.0, (4096, 4096))
    assert ests.estIntSelCutFrag(di, ds)[0] in (lo, hi) and rcut in (lo, hi)
    assert margin < 1e-6


def test_from_stats_never_nan_on_negative_sqdev():
    """the one-pass squared deviation of a degenerate group can come out below zero: the cut stays finite and equals
    what the reference makes of a zero spread"""
    rcut, rfrags = ests.estIntSelCutFrag_from_stats([400, 1001], [400 * 21.0, 1001 * 15.0], [5.0, -1.7e-5], (32768, 32768))
    assert (rcut, rfrags) == (32768, 32768)
    rcut, _ = ests.estIntSelCutFrag_from_stats([400, 1001], [400 * 21.0, 1001 * 15.0], [-3e-9, -1.7e-5], (32768, 32768))
    assert rcut == 32768                             # both spreads 0: cut2 = 0/0 and min() keeps cut1, as the reference


def test_sweep_fast_recheck_is_rare_on_ordinary_data(fake_gpu, tmp_path):
    """the bound must not turn every step into a recheck: the chr21 chain settles from the statistics alone"""
    import pipe_checks
    f = pipe_checks.write_chr21_jd(tmp_path)
    _, _, cuts, steps = pipe.runSweepFast([f], [500, 1000, 2000], [5], cut=0)
    assert cuts == [0, 4601, 13532, 11103]
    assert not any(s.get("cut_rechecked") for s in steps)


# ---- the log bins of the exact median -------------------------------------------------------------
def test_logbin_ranges_cover_every_bin():
    """all 3840 bins: [lo, hi) non-empty, every distance in it maps back to the bin, the ranges of the reachable
    bins tile 1 .. 2^30 in order, and octaves below 7 reach exactly 2^e of their 128 bins"""
    reach = {}
    nxt = 1
    for b in range(3840):
        lo, hi = ests.logbin_range(b)
        e, m = divmod(b, 128)
        assert 1 <= lo < hi <= 2 ** 30
        assert 2 ** e <= lo and hi <= 2 ** (e + 1)
        if ests.logbin(lo) != b:                      # a bin no distance reaches (octaves 0..6 only)
            assert e < 7
            continue
        reach[e] = reach.get(e, 0) + 1
        assert lo == nxt, b                           # contiguous, ascending
        assert ests.logbin(hi - 1) == b and (hi == 2 ** 30 or ests.logbin(hi) > b)
        if e >= 7:
            assert hi - lo == 1 << (e - 7)
        nxt = hi
    assert nxt == 2 ** 30
    assert [reach[e] for e in range(30)] == [min(2 ** e, 128) for e in range(30)]
    assert ests.logbin_range(3839) == (2 ** 30 - 2 ** 22, 2 ** 30)


def test_logbin_round_trip_and_monotone():
    d = np.concatenate([np.arange(1, 1 << 17), np.random.RandomState(7).randint(1, 2 ** 30, 20000),
                        [2 ** e + k for e in range(1, 30) for k in (-1, 0, 1)], [2 ** 30 - 1]])
    d = np.unique(d)
    bins = np.array([ests.logbin(v) for v in d])
    assert np.all(np.diff(bins) >= 0)                 # monotone in d
    assert bins.min() == 0 and bins.max() == 3839
    for v, b in zip(d.tolist(), bins.tolist()):
        lo, hi = ests.logbin_range(b)
        assert lo <= v < hi
        e = v.bit_length() - 1
        assert b == e * 128 + (((v << 7) >> e) & 127)        # the 7 bits below the leading one
