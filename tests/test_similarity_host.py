"""CPU: the restatement of K28 (tests/similarity_cases.py) against itself, the host formulas of cloops_amd/similarity.py on hand cases,
the conditions the GPU cases rely on, the argument checks, the files' text, the overflow rule's arithmetic and the orderings an SCC has
to show on synthetic data."""
import json
import math

import numpy as np
import pytest

import matrix_cases as MC
import similarity_cases as SC
from cloops_amd import similarity as S


def cells(X, Y, res=1, cut=0):
    return MC.cells_oracle(X, Y, cut, res, True)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,h", [(1, 0), (1, 3), (2, 1), (7, 0), (7, 1), (7, 2), (7, 9), (19, 3), (33, 20)])
def test_the_two_box_forms_agree(nb, h):
    c = cells(*SC.sized(nb, 3))
    A = SC.dense(*c[:3], 0, nb)
    assert np.array_equal(A, A.T) and (nb < 3 or A.any())
    P, B = SC.box_prefix(A, h), SC.box_brute(A, h)
    assert np.array_equal(P, B) and np.array_equal(P, P.T)
    if h == 0:
        assert np.array_equal(P, A)
    if h >= nb:
        assert (P == A.sum()).all()                                          # every box is the whole window


def test_dense_counts_a_diagonal_cell_once_and_leaves_the_outside_out():
    bx, by, cnt = np.array([0, 2, 2, 9]), np.array([0, 3, 9, 9]), np.array([5, 7, 11, 13])
    A = SC.dense(bx, by, cnt, 0, 4)
    assert A.tolist() == [[5, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 7], [0, 0, 7, 0]]
    assert SC.dense(bx, by, cnt, 2, 8)[0].tolist() == [0, 7, 0, 0, 0, 0, 0, 11]
    m = SC.moments_of(SC.box_prefix(A, 0), SC.box_prefix(2 * A, 0), 4)
    assert m == [[1, 1, 0, 0], [5, 7, 0, 0], [10, 14, 0, 0], [25, 49, 0, 0], [100, 196, 0, 0], [50, 98, 0, 0]]


# ---- the host formulas on hand cases -------------------------------------------------------------------------------------------------
def test_a_sample_against_itself():
    c = cells(*SC.general()[0], res=1000)
    b0, nb = SC.span_of(c)
    m = SC.moments_oracle(c, c, b0, nb, 1, 40)
    got = S.combine(SC.as_arrays(m))
    with_var = [d for d in range(40) if m[0][d] >= 2 and m[0][d] * m[3][d] > m[1][d] ** 2]
    assert len(with_var) == 40
    # num = va = vb exactly; v / (sqrt(v) sqrt(v)) carries the roundings of v itself, one square root, the product and the division,
    # each at most 2^-53 relative: rho is 1 within 5 2^-53, and scc, a weighted mean of such values, within one rounding more per term
    near = lambda r, k: abs(r - 1.0) <= k * 2.0 ** -53
    assert all(near(got["rho"][d], 5) for d in with_var) and near(got["scc"], 5 + 2 * 40 + 1) and near(got["pcc"], 5)
    assert got["n"] == m[0] and got["pixels"] == sum(m[0])


def test_nan_strata_have_no_weight():
    # stratum 0: one point; 1: no spread in x; 2: no spread in y; 3: three points on a line; 4: empty
    pts = [[(3, 4)], [(2, 1), (2, 5)], [(1, 7), (3, 7)], [(1, 2), (2, 4), (3, 6)], []]
    m = [[len(p) for p in pts], [sum(x for x, _ in p) for p in pts], [sum(y for _, y in p) for p in pts], [sum(x * x for x, _ in p) for p in pts],
         [sum(y * y for _, y in p) for p in pts], [sum(x * y for x, y in p) for p in pts]]
    got = S.combine(SC.as_arrays(m))
    assert [math.isnan(r) for r in got["rho"]] == [True, True, True, False, True]
    assert abs(got["rho"][3] - 1.0) <= 5 * 2.0 ** -53 and got["scc"] == got["rho"][3]                # (the roundings of the formula; one stratum: w rho / w)
    assert got["weight"] == [0.0, 0.0, 0.0, 3 * (1.0 + 1.0 / 3) / 12.0, 0.0] and got["pixels"] == 8
    none = S.combine(SC.as_arrays([c[:3] for c in m]))
    assert math.isnan(none["scc"]) and none["weight"] == [0.0] * 3
    empty = S.combine(SC.as_arrays([[] for _ in range(6)]))
    assert math.isnan(empty["scc"]) and math.isnan(empty["pcc"]) and empty["pixels"] == 0 and empty["rho"] == []


def test_ignore_diags_is_honoured():
    (Xa, Ya), (Xb, Yb) = SC.general()
    ca, cb = cells(Xa, Ya, 1000), cells(Xb, Yb, 1000)
    b0, nb = SC.span_of(ca, cb)
    m = SC.moments_oracle(ca, cb, b0, nb, 1, 30)
    full, cutoff = S.combine(SC.as_arrays(m)), S.combine(SC.as_arrays(m), ignore_diags=3)
    assert cutoff["weight"][:3] == [0.0] * 3 and cutoff["weight"][3:] == full["weight"][3:] and min(full["weight"][:3]) > 0
    assert cutoff["rho"] == full["rho"] and cutoff["pixels"] == sum(m[0][3:]) and cutoff["scc"] != full["scc"]
    want = SC.scc_oracle(m, 3)
    assert abs(cutoff["scc"] - want["scc"]) <= 1e-12 and abs(cutoff["pcc"] - want["pcc"]) <= 1e-12
    assert cutoff["pcc"] == S.combine(SC.as_arrays([c[3:] for c in m]))["pcc"]
    beyond = S.combine(SC.as_arrays(m), ignore_diags=30)
    assert math.isnan(beyond["scc"]) and math.isnan(beyond["pcc"]) and beyond["pixels"] == 0


@pytest.mark.parametrize("h,ign", [(0, 0), (1, 0), (3, 2)])
def test_pcc_is_numpys(h, ign):
    """both sides are a handful of correctly rounded operations on exact integers: 1e-12 is three orders above their rounding"""
    (Xa, Ya), (Xb, Yb) = SC.general()
    ca, cb = cells(Xa, Ya, 1000), cells(Xb, Yb, 1000)
    b0, nb = SC.span_of(ca, cb)
    Sa, Sb = SC.box_prefix(SC.dense(*ca[:3], b0, nb), h), SC.box_prefix(SC.dense(*cb[:3], b0, nb), h)
    x, y = SC.counted_pixels(Sa, Sb, 60, ign)
    got = S.combine(SC.as_arrays(SC.moments_of(Sa, Sb, 60)), ign)
    assert len(x) == got["pixels"] > 1000
    assert abs(got["pcc"] - np.corrcoef(x, y)[0, 1]) <= 1e-12
    for d in (ign, 17, 35):
        xd, yd = SC.counted_pixels(Sa, Sb, d + 1, d)
        assert abs(got["rho"][d] - np.corrcoef(xd, yd)[0, 1]) <= 1e-12
    want = SC.scc_oracle(SC.moments_of(Sa, Sb, 60), ign)
    assert abs(got["scc"] - want["scc"]) <= 1e-12 and -1.0 <= got["scc"] <= 1.0


# ---- what the GPU cases rely on ------------------------------------------------------------------------------------------------------
def test_the_gpu_cases_reach_their_edges():
    # sizes: both tile directions, h beyond the window and beyond half the diagonals
    assert SC.SIZES == (1, 2, 31, 32, 33, 97) and SC.HS == (0, 1, 2, 20) and SC.HMAX == S.HMAX and SC.BAND_MAX == S.BAND_MAX
    for nb in SC.SIZES:
        c = cells(*SC.sized(nb, nb))
        assert c[0].min() < 0 and c[1].max() >= nb                           # cells outside the window on both sides
        A = SC.dense(*c[:3], 0, nb)
        assert A.any() and (nb < 3 or np.triu(A, 1).any())
    # a box that crosses the diagonal: the lower triangle's copy of a cell changes sums of the band
    c = cells(*SC.sized(33, 33))
    A = SC.dense(*c[:3], 0, 33)
    for h in (1, 2, 20):
        full, upper = SC.box_prefix(A, h), SC.box_prefix(np.triu(A), h)
        assert any((np.diagonal(full, d) != np.diagonal(upper, d)).any() for d in range(3))
    # the window that cuts through the data
    Xa, Ya, Xb, Yb, res, b0, nb = SC.cut_window()
    for c in (cells(Xa, Ya, res), cells(Xb, Yb, res)):
        inside = (c[0] >= b0) & (c[1] < b0 + nb)
        assert c[0].min() < 0 and c[0].min() < b0 and c[1].max() >= b0 + nb and inside.any()
        assert ((c[0] < b0) & (c[1] >= b0) & (c[1] < b0 + nb)).any() and ((c[0] >= b0) & (c[0] < b0 + nb) & (c[1] >= b0 + nb)).any()
    # a gap wider than a tile
    c = cells(*SC.gapped())
    used = np.union1d(c[0], c[1])
    assert np.diff(used).max() > SC.TILE_I and (c[1] - c[0]).max() > 2 * SC.TILE_I
    # squares beyond 2^32, sums that need 64 bits
    ca, cb = cells(*SC.heavy(1)), cells(*SC.heavy(2))
    assert ca[2].max() >= SC.HEAVY and cb[2].max() >= SC.HEAVY
    m = SC.moments_oracle(ca, cb, 0, 40, 1, 10)
    assert max(m[3]) > 1 << 34 and max(m[5]) > 1 << 34 and max(m[1]) > 1 << 17
    assert S.scc_fits(S.smax_of(1, int(ca[2].max()), ca[3]), S.smax_of(1, int(cb[2].max()), cb[3]), 40)
    # the general case
    (Xa, Ya), (Xb, Yb) = SC.general()
    ca, cb = cells(Xa, Ya, 1000), cells(Xb, Yb, 1000)
    assert 300 < SC.span_of(ca, cb)[1] < 400 and len(Xa) > 2000 and len(Xb) > 2000 and len(cells(Xa, Ya, 1000, 9000)[0]) < len(ca[0])
    # the refused one
    X, Y = SC.overflowing()
    c = cells(X, Y)
    nb = SC.span_of(c)[1]
    assert nb == (1 << 24) + 1 and nb <= S.BAND_MAX and not S.scc_fits(S.smax_of(0, int(c[2].max()), c[3]), 0, nb)


def test_the_overflow_rule_at_its_boundary():
    """max(Smax)^2 nb < 2^64, one step on either side"""
    assert S.smax_of(0, 9, 100) == 9 and S.smax_of(1, 9, 100) == 81 and S.smax_of(2, 9, 100) == 200 and S.smax_of(20, 1, 10 ** 6) == 1681
    assert SC.smax(3, 5, 1000) == S.smax_of(3, 5, 1000) == 245
    assert S.scc_fits(1 << 31, 0, 3) and S.scc_fits(0, 1 << 31, 3) and not S.scc_fits(1 << 31, 0, 4) and not S.scc_fits(1, 1 << 31, 4)
    assert S.scc_fits((1 << 32) - 1, 5, 1) and not S.scc_fits(1 << 32, 5, 1) and not S.scc_fits(5, 1 << 32, 1)
    s = 3037000499                                                           # floor(sqrt(2^63)): s^2 2 < 2^64 <= (s + 1)^2 2
    assert S.scc_fits(s, s, 2) and not S.scc_fits(s + 1, 1, 2) and s * s * 2 < 1 << 64 <= (s + 1) ** 2 * 2
    assert S.scc_fits(1 << 20, 1 << 20, (1 << 24) - 1) and not S.scc_fits(1 << 20, 1 << 20, 1 << 24)
    assert S.scc_fits(0, 0, 1 << 28)


# ---- the command's arguments and texts -------------------------------------------------------------------------------------------------
def test_argument_checks(tmp_path):
    ok = dict(res=1000, h=1, dmax=50000, ignore_diags=0)
    assert S.check_args(2, **ok) == (1000, 1, 50000, 0)
    for bad in (dict(n_samples=1), dict(n_samples=0), dict(res=0), dict(res=-5), dict(h=-1), dict(h=21), dict(h=1.5), dict(dmax=-1),
                dict(ignore_diags=-1), dict(names=["a"]), dict(names=["a", "a"]), dict(names=["a", "b", "c"]), dict(names=["a", "b c"]),
                dict(names=["a", ""])):
        kw = dict(ok, n_samples=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            S.check_args(**kw)
    assert S.check_args(3, names=["a", "b", "c"], **ok) == (1000, 1, 50000, 0)
    out = str(tmp_path / "o")
    for f in (lambda: S.jds2similarity([str(tmp_path)], out), lambda: S.jds2similarity([str(tmp_path)] * 2, out, h=21),
              lambda: S.jds2similarity([str(tmp_path)] * 2, out, res=0), lambda: S.jds2similarity([str(tmp_path)] * 2, out, dmax=-1),
              lambda: S.jds2similarity([str(tmp_path)] * 2, out, names=["one"]), lambda: S.main(["-d", str(tmp_path), "-o", out])):
        with pytest.raises(ValueError):
            f()
    assert list(tmp_path.iterdir()) == []
    with pytest.raises(ValueError):
        S.band_check(1 << 20, 257, 0)
    S.band_check(1 << 20, 256, 0)
    S.band_check(1 << 20, 176, 20)
    with pytest.raises(ValueError):
        S.band_check(1 << 20, 177, 20)
    op = S.help(["-d", "a,b", "-o", "x", "-h", "3", "-res", "5000", "-names", "A,B"])
    assert (op.d, op.h, op.res, op.dmax, op.cut, op.ignorediags, op.names) == ("a,b", 3, 5000, 5000000, 0, 0, "A,B")
    assert S.default_names(["/x/rep1/", "y/rep2"]) == ["rep1", "rep2"] and S.default_names(["/x/r", "/y/r"]) == ["s1", "s2"]


def records():
    """three samples over two chromosomes from the restatement's stand-in; `c` has no chrB, and a fifth of the others' depth"""
    (Xa, Ya), (Xb, Yb) = SC.general()
    data = {"a": {"chrA": (Xa, Ya), "chrB": (Xb[:900], Yb[:900])}, "b": {"chrA": (Xb, Yb), "chrB": (Xa[:800], Ya[:800])},
            "c": {"chrA": (Xa[:500], Ya[:500])}}
    names = sorted(data)
    pairs = []
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            per = {c: S.pair_chrom(SC.OracleChrom(*data[a][c]), SC.OracleChrom(*data[b][c]), 1000, h=1, dmax=20000, ignore_diags=1)
                   for c in sorted(set(data[a]) & set(data[b]))}
            pairs.append({"a": a, "b": b, "chroms": per, "skipped": sorted(set(data[a]) ^ set(data[b]))})
    return names, pairs


def test_the_text_of_the_four_files():
    names, pairs = records()
    args = {"res": 1000, "h": 1, "dmax": 20000, "cut": 0, "ignore_diags": 1, "samples": ["da", "db", "dc"]}
    texts, js = S.similarity_outputs(names, pairs, args)
    assert sorted(texts) == sorted(S.SUFFIXES)
    rows = texts["_scc.txt"].splitlines()
    assert rows[0].startswith("# genome rows: the plain mean") and rows[1].split("\t") == ["sampleA", "sampleB", "chrom", "bins", "diags", "h", "pixels", "scc", "pcc", "keptA", "keptB"]
    body = [r.split("\t") for r in rows[2:]]
    assert [r[:3] for r in body] == [["a", "b", "chrA"], ["a", "b", "chrB"], ["a", "b", "genome"], ["a", "c", "chrA"], ["a", "c", "genome"],
                                     ["b", "c", "chrA"], ["b", "c", "genome"]]
    r0 = pairs[0]["chroms"]["chrA"]
    assert r0["diags"] == 21 and body[0][3:7] == [str(r0["bins"]), "21", "1", str(r0["pixels"])] and body[0][9:] == ["3000", "2600"]
    assert float(body[0][7]) == r0["scc"] and float(body[0][8]) == r0["pcc"] and -1 < r0["scc"] < 1
    g = S.genome_of(pairs[0]["chroms"])
    assert g["scc"] == (r0["scc"] + pairs[0]["chroms"]["chrB"]["scc"]) / 2 and float(body[2][7]) == g["scc"] and body[2][4] == "."
    assert body[2][9:] == ["3900", "3400"] and int(body[2][3]) == r0["bins"] + pairs[0]["chroms"]["chrB"]["bins"]
    strata = [r.split("\t") for r in texts["_scc_strata.txt"].splitlines()]
    assert strata[0] == ["sampleA", "sampleB", "chrom", "d", "n", "rho", "weight"] and len(strata) == 1 + 21 * 4
    assert strata[1][:5] == ["a", "b", "chrA", "0", str(r0["n"][0])] and strata[1][6] == "0.0" and float(strata[2][6]) == r0["weight"][1] > 0
    assert float(strata[2][5]) == r0["rho"][1]
    mat = [r.split("\t") for r in texts["_scc_matrix.txt"].splitlines()]
    assert mat[0] == ["", "a", "b", "c"] and [r[0] for r in mat[1:]] == names and all(mat[k + 1][k + 1] == "1" for k in range(3))
    assert mat[1][2] == mat[2][1] == body[2][7] and mat[1][3] == mat[3][1] == body[4][7] and mat[2][3] == mat[3][2] == body[6][7]
    assert json.loads(texts["_scc.json"]) == js and js["args"] == args and js["samples"] == names
    assert [p["skipped"] for p in js["pairs"]] == [[], ["chrB"], ["chrB"]]
    assert js["pairs"][0]["chroms"]["chrA"]["scc"] == r0["scc"] and "rho" not in js["pairs"][0]["chroms"]["chrA"]
    assert len(js["warnings"]) == 2 and all("depth" in w and " c " in w for w in js["warnings"])
    assert S.fnum(float("nan")) == "nan" and float(S.fnum(0.1 + 0.2)) == 0.1 + 0.2
    assert math.isnan(S.finite_mean([float("nan")])) and S.finite_mean([float("nan"), 0.5, 0.25]) == 0.375
    # a pair without a shared chromosome: NaN everywhere, no failure
    texts, js = S.similarity_outputs(["x", "y"], [{"a": "x", "b": "y", "chroms": {}, "skipped": ["chr1"]}], args)
    assert texts["_scc.txt"].splitlines()[2].split("\t") == ["x", "y", "genome", "0", ".", "1", "0", "nan", "nan", "0", "0"]
    assert texts["_scc_matrix.txt"].splitlines()[1] == "x\t1\tnan" and js["pairs"][0]["genome"]["scc"] is None


def test_a_handle_against_itself_is_prepared_and_freed_once():
    calls = []

    class Counting(SC.OracleChrom):
        def mat_cells(self, *a, **k):
            calls.append("cells")
            return SC.OracleChrom.mat_cells(self, *a, **k)

        def mat_free(self):
            calls.append("free")
            SC.OracleChrom.mat_free(self)
    ch = Counting(*SC.general()[0])
    rec = S.pair_chrom(ch, ch, 1000, h=1, dmax=30000)
    assert calls == ["cells", "free"] and rec["keptA"] == rec["keptB"] == 3000 and abs(rec["scc"] - 1.0) <= 100 * 2.0 ** -53
    # a failing free of the first handle does not skip the second's
    class Failing(Counting):
        def mat_free(self):
            raise RuntimeError("free failed")
    del calls[:]
    other = Counting(*SC.general()[1])
    with pytest.raises(RuntimeError):
        S.pair_chrom(Failing(*SC.general()[0]), other, 1000)
    assert calls.count("free") == 1 and other.cells is None


def test_an_empty_pair_of_samples():
    rec = S.pair_chrom(SC.OracleChrom(MC.EMPTY, MC.EMPTY), SC.OracleChrom(MC.EMPTY, MC.EMPTY), 1000)
    assert (rec["bins"], rec["diags"], rec["pixels"], rec["n"]) == (0, 0, 0, []) and math.isnan(rec["scc"]) and math.isnan(rec["pcc"])
    rec = S.pair_chrom(SC.OracleChrom([1500], [7800]), SC.OracleChrom(MC.EMPTY, MC.EMPTY), 1000, h=0, dmax=100000)
    assert (rec["b0"], rec["bins"], rec["diags"], rec["keptA"], rec["keptB"]) == (1, 7, 7, 1, 0) and rec["n"] == [0] * 6 + [1]


# ---- the orderings an SCC has to show -------------------------------------------------------------------------------------------------
def test_orderings_on_synthetic_data():
    """two halves of one sample are more alike than either is to another sample, at every h, and smoothing raises both.  A copy of a
    half with its bins permuted shares nothing with the other half but the depth: it scores below both at every h, and below 0 without
    smoothing, where the two supports hardly meet and a position counted for one sample is mostly a zero of the other.  (Under a
    box of h = 3 the supports overlap and the score is 0 within a few hundredths, of either sign depending on the permutation.)"""
    from cloops_amd.synth import synth_chrom
    X, Y = synth_chrom(60000, 46709983, 7)
    X8, Y8 = synth_chrom(60000, 46709983, 8)
    half = np.random.default_rng(0).random(len(X)) < 0.5
    res, D = 100000, 50
    c1, c2, c8 = cells(X[half], Y[half], res), cells(X[~half], Y[~half], res), cells(X8, Y8, res)
    b0, nb = SC.span_of(c1, c2, c8)
    perm = np.random.default_rng(1).permutation(nb)
    px, py = perm[c1[0] - b0] + b0, perm[c1[1] - b0] + b0
    cp = (np.minimum(px, py), np.maximum(px, py), c1[2])
    halves, other, shuffled = [], [], []
    for h in (0, 1, 3):
        halves.append(SC.scc_oracle(SC.moments_oracle(c1, c2, b0, nb, h, D))["scc"])
        other.append(SC.scc_oracle(SC.moments_oracle(c1, c8, b0, nb, h, D))["scc"])
        shuffled.append(SC.scc_oracle(SC.moments_oracle(cp, c2, b0, nb, h, D))["scc"])
    print("scc of the halves %s, against the other sample %s, against the permuted half %s" % (halves, other, shuffled))
    assert all(a > b for a, b in zip(halves, other))
    assert halves[0] < halves[1] < halves[2] and other[0] < other[1] < other[2]
    assert all(s < b for s, b in zip(shuffled, other)) and shuffled[0] < 0 and shuffled[1] < 0
