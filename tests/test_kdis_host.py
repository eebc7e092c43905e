"""CPU: the host side of the eps estimate (cloops_amd.esteps) -- quantiles and Otsu's threshold on hand-made histograms whose answer is
plain, zeros and rows without a neighbour, the estimate on the oracle's k-distances of seeded mixtures of background and loops, pure
background, the two file formats, argument checks and the -k parser -- and the oracle's own self-test (tests/kdis_cases.py)."""
import json

import numpy as np
import pytest

import kdis_cases as KC
from cloops_amd import esteps
from cloops_amd.ests import logbin, logbin_range

BINS = KC.BINS


def spikes(*pairs):
    h = np.zeros(BINS, np.int64)
    for d, n in pairs:
        h[logbin(d)] += n
    return h


def test_oracle_self_test():
    assert KC.self_test()


def test_constants_agree():
    from cloops_amd import _lib
    assert (esteps.BINS, esteps.KMAX) == (_lib.CL_KDIS_BINS, _lib.CL_KDIS_KMAX) == (KC.BINS, KC.KMAX)
    assert logbin((1 << 31) - 4) == BINS - 1 and logbin_range(BINS - 1)[1] == 1 << 31
    assert esteps.HEAD[:5] == ("k", "minPts", "n", "n_zero", "n_none") and len(esteps.HEAD) == 5 + 9 + 3


# ---- quantiles ------------------------------------------------------------------------------------------
def test_quantiles_on_spikes():
    h = spikes((100, 50), (5000, 50))                              # 100 rows: half at 100, half at 5000
    lo5000 = logbin_range(logbin(5000))[0]
    assert esteps.quantiles_of(h, 0) == [100, 100, 100, 100, 100, lo5000, lo5000, lo5000, lo5000]
    assert esteps.quantiles_of(h, 0, (50, 51)) == [100, lo5000]    # rank 50 is the last row of the lower spike
    # zeros come first: 100 zeros in front of the 100 rows above
    assert esteps.quantiles_of(h, 100) == [0, 0, 0, 0, 0, 100, lo5000, lo5000, lo5000]
    assert esteps.quantiles_of(h, 100, (50, 51, 75, 76)) == [0, 100, 100, lo5000]
    # one row; no row
    assert esteps.quantiles_of(spikes((7, 1)), 0) == [7] * 9
    assert esteps.quantiles_of(np.zeros(BINS, np.int64), 3) == [0] * 9
    assert esteps.quantiles_of(np.zeros(BINS, np.int64), 0) == [None] * 9
    # a bin wider than one value gives its lower bound
    assert logbin_range(logbin(1000)) == (1000, 1004) and esteps.quantiles_of(spikes((1003, 4)), 0, (50,)) == [1000]
    with pytest.raises(ValueError):
        esteps.quantiles_of(np.zeros(10, np.int64), 0)
    with pytest.raises(ValueError):
        esteps.quantiles_of(np.zeros(BINS), 0)


# ---- Otsu -------------------------------------------------------------------------------------------------
def test_otsu_two_spikes():
    h = spikes((300, 30), (40000, 70))
    o = esteps.otsu_of(h)
    # every t between the spikes has the same classes and the same criterion: the first maximum is the lower spike's own bin
    assert o["bin"] == logbin(300) and o["eps"] == logbin_range(logbin(300) + 1)[0]
    assert 300 < o["eps"] <= 40000 and o["share_below"] == 0.3
    assert abs(o["eta"] - 1.0) < 1e-12                             # two spikes: the classes explain all of the variance
    # zeros count in the share, not in the threshold
    z = esteps.otsu_of(h, 100)
    assert (z["bin"], z["eps"], z["eta"]) == (o["bin"], o["eps"], o["eta"]) and z["share_below"] == 130 / 200.0


def test_otsu_two_clouds():
    rng = np.random.default_rng(5)
    d = np.concatenate([np.exp2(rng.normal(9, 0.4, 4000)), np.exp2(rng.normal(15, 0.5, 6000))]).astype(np.int64)
    h, nz, nn = KC.hist_oracle(d)
    o = esteps.otsu_of(h, nz)
    assert d[:4000].max() < d[4000:].min()                         # the clouds do not touch: the threshold lies in the gap
    assert d[:4000].max() < o["eps"] <= d[4000:].min() and o["share_below"] == 0.4 and 0.9 < o["eta"] <= 1.0
    # against the definition, bin by bin
    idx = np.arange(BINS)
    best, best_t = -1.0, None
    for t in np.flatnonzero(h)[0] + np.arange(np.flatnonzero(h)[-1] - np.flatnonzero(h)[0]):
        a, b = h[:t + 1], h[t + 1:]
        wa, wb = a.sum(), b.sum()
        ma, mb = (a * idx[:t + 1]).sum() / wa, (b * idx[t + 1:]).sum() / wb
        v = wa * wb * (ma - mb) ** 2
        if v > best * (1 + 1e-12):
            best, best_t = v, int(t)
    assert o["bin"] == best_t
    var = (h * idx ** 2).sum() / h.sum() - ((h * idx).sum() / h.sum()) ** 2
    assert abs(o["eta"] - best / h.sum() ** 2 / var) < 1e-9


def test_otsu_needs_two_bins():
    none = {"eps": None, "share_below": None, "eta": None, "bin": None}
    assert esteps.otsu_of(spikes((500, 1000))) == none
    assert esteps.otsu_of(spikes((500, 1000)), 50) == none         # zeros are no second bin
    assert esteps.otsu_of(np.zeros(BINS, np.int64)) == none
    e = esteps.estimate_of(spikes((500, 1000)), 50, 7)
    assert (e["n"], e["n_zero"], e["n_none"], e["eps"], e["share_below"], e["eta"]) == (1057, 50, 7, None, None, None)
    assert e["quantiles"]["q1"] == 0 and e["quantiles"]["q5"] == 500          # 1050 rows with a distance: rank 11 / 53
    last = esteps.otsu_of(spikes((1 << 30, 5), ((1 << 31) - 4, 5)))           # the last bin occupied: t + 1 stays a bin
    assert last["eps"] == logbin_range(logbin(1 << 30) + 1)[0]


def test_rows_without_a_neighbour_are_left_out():
    h = spikes((300, 30), (40000, 70))
    a, b = esteps.estimate_of(h, 0, 0), esteps.estimate_of(h, 0, 1000)
    assert b["n"] == a["n"] + 1000 and b["n_none"] == 1000
    assert {k: v for k, v in a.items() if k not in ("n", "n_none")} == {k: v for k, v in b.items() if k not in ("n", "n_none")}
    only = esteps.estimate_of(np.zeros(BINS, np.int64), 0, 12)
    assert only["n"] == 12 and only["eps"] is None and set(only["quantiles"].values()) == {None}


# ---- the estimate on mixtures -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixtures():
    """per mixture (seeds: KC.MIXTURE_SEEDS): the loop mask in table order and the oracle's d_k for k = 5, 10, 20 -- made once"""
    out = []
    for par, seed in zip(KC.MIXTURES, KC.MIXTURE_SEEDS):
        X, Y, loop = KC.mixture(seed, *par)
        _, _, d, rows = KC.kdis_oracle(X, Y, 0, (5, 10, 20))
        out.append((loop[rows], d))
    return out


@pytest.mark.parametrize("k", [5, 10, 20])
@pytest.mark.parametrize("mix", [0, 1, 2])
def test_estimate_separates_loops_from_background(mixtures, mix, k):
    loop, d = mixtures[mix]
    h, nz, nn = KC.hist_oracle(d[k])
    e = esteps.estimate_of(h, nz, nn)
    below = d[k] < e["eps"]
    print("mixture %d k %d: eps %d, loops below %.4f, background below %.4f, eta %.3f"
          % (mix, k, e["eps"], below[loop].mean(), below[~loop].mean(), e["eta"]))
    assert below[loop].all()                                       # 100 % of the loop PETs
    assert below[~loop].mean() <= 0.05                             # at most 5 % of the background PETs
    assert e["share_below"] == below.mean() and 0.0 < e["eta"] <= 1.0


def test_pure_background():
    rng = np.random.default_rng(8)
    X = rng.integers(0, 2000000, 8000)
    Y = X + rng.integers(1000, 400001, 8000)
    d = KC.kdis_oracle(X, Y, 0, (9,))[2][9]
    e = esteps.estimate_of(*KC.hist_oracle(d))
    assert e["n"] == 8000 and e["eps"] is not None and isinstance(e["eta"], float) and 0.0 <= e["eta"] <= 1.0      # reported, whatever it is


# ---- formats and arguments ---------------------------------------------------------------------------------
def test_outputs():
    data = {"chr2": KC.mixture(1, 600, 6, 30, 300)[:2], "chr10": KC.mixture(2, 500, 5, 40, 300)[:2], "chrM": (np.arange(7), np.arange(7) + 9)}
    ks = [4, 9, 19]
    per = {name: esteps.chrom_kdis(KC.OracleChrom(X, Y), ks, 0) for name, (X, Y) in data.items()}
    texts, js, sums = esteps.outputs_of(per, ks, 0)
    assert sorted(texts) == sorted(esteps.SUFFIXES)
    assert json.loads(texts["_kdis.json"]) == js
    assert js["k"] == ks and js["cut"] == 0 and js["chroms"] == {"chr2": {"n": 780}, "chr10": {"n": 700}, "chrM": {"n": 7}}
    assert js["total"] == {"n": 1487} and js["quantiles"] == list(esteps.QUANTILES)
    lines = texts["_kdis.txt"].splitlines()
    assert lines[0].split("\t") == list(esteps.HEAD) and len(lines) == 4
    for line, k in zip(lines[1:], ks):
        f = line.split("\t")
        e = js["estimates"][str(k)]
        assert f[:3] == [str(k), str(k + 1), "1487"] and len(f) == len(esteps.HEAD)
        assert e["n"] == 1487 and e["n_none"] == (7 if k >= 7 else 0) == int(f[4])          # chrM has 6 other rows
        assert [int(v) for v in f[5:14]] == [e["quantiles"]["q%d" % q] for q in esteps.QUANTILES]
        assert int(f[14]) == e["eps"] and float(f[15]) == e["share_below"] and float(f[16]) == e["eta"]
        # the histograms of the chromosomes add: the same estimate from all rows' d_k
        allh = sum(KC.hist_oracle(KC.kdis_oracle(X, Y, 0, [k])[2][k])[0] for X, Y in data.values())
        assert np.array_equal(sums[k][0], allh) and e["eps"] == esteps.otsu_of(allh, sums[k][1])["eps"]
    # no estimate: NA in the text, null in the json
    per = {"chrM": esteps.chrom_kdis(KC.OracleChrom(*data["chrM"]), [7], 0)}
    texts, js, _ = esteps.outputs_of(per, [7], 0)
    assert texts["_kdis.txt"].splitlines()[1].split("\t") == ["7", "8", "7", "0", "7"] + ["NA"] * 12
    assert js["estimates"]["7"]["eps"] is None


def test_k_parser_and_argument_checks():
    assert esteps.k_list("4,9,19") == [4, 9, 19] and esteps.k_list("19,4,9,4") == [4, 9, 19] and esteps.k_list(5) == [5]
    assert esteps.k_list((1, 64)) == [1, 64] and esteps.k_list("1,2,3,4,5,6,7,8") == list(range(1, 9))
    for bad in ("", "0", "65", "4,x", "1,2,3,4,5,6,7,8,9", "-3", None, 2.5):
        with pytest.raises(ValueError):
            esteps.k_list(bad)
    assert esteps.check_args("9,4", "0") == ([4, 9], 0)
    with pytest.raises(ValueError):
        esteps.check_args("4", "x")
    op = esteps.help(["-d", "jd", "-o", "out"])
    assert (op.k, op.cut, op.chroms, op.plot) == ("4,9,19", 0, "", False)
    op = esteps.help(["-d", "jd", "-o", "out", "-k", "5", "-cut", "1000", "-c", "chr1,chr2", "-plot"])
    assert (op.k, op.cut, op.chroms, op.plot) == ("5", 1000, "chr1,chr2", True)
    with pytest.raises(ValueError):
        esteps.jd2esteps("/nonexistent/jd", "out")


def test_pipe_takes_the_flag():
    import inspect
    from cloops_amd import pipe
    sig = inspect.signature(pipe.pipe).parameters
    assert sig["kdis"].default == 0 and sig["kdis_k"].default == (4, 9, 19)
