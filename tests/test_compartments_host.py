"""CPU: the numpy oracle of K27 against itself (the dense matrix against the sparse-plus-prefix form within the derived bound, the
spectral gaps of the planted data the GPU tests lean on) and the host side of cloops_amd.compartments on the stand-in chromosome: dmax,
the clip, the orientation, the compartment runs, the texts, the json and the refusals."""
import json
import os
import threading

import numpy as np
import pytest

import balance_cases as BC
import compartments_cases as CC
import expected_cases as EC
import matrix_cases as MC
from cloops_amd import balance, compartments, expected, matrix


class Record(object):
    def __init__(self, X, Y):
        self.chrom, self.lock = CC.OracleChrom(X, Y), threading.Lock()


@pytest.fixture
def standin(monkeypatch):
    """matrix._records (which compartments reads) served by stand-in chromosomes: the small planted case and 4000 scattered rows"""
    c = CC.planted_case("small")
    recs = {"chr1": Record(c["X"], c["Y"]), "chr2": Record(*MC.scattered(1, 4000, 60000, 20000, both=True))}
    monkeypatch.setattr(matrix, "_records", lambda jd, chroms=(): [(n, recs[n]) for n in sorted(recs) if len(chroms) == 0 or n in chroms])
    return recs


def _read(prefix, suffixes):
    out = {}
    for s in suffixes:
        with open(prefix + s) as fh:
            out[s] = fh.read()
    return out


def state_of(X, Y, res, ign, raw=False, mask=None):
    """the oracle's state up to exp_set -> (cells, b0, nb, valid, w, expected)"""
    ch = CC.OracleChrom(X, Y)
    ch.mat_cells(res, fold=True)
    b0, nb, _ = ch.bal_marginals(ign)
    s, z = ch.bal_marginals_get()
    m = BC.valid_oracle(s, z, 1, 0, 0) if mask is None else mask(nb)
    if raw:
        ch.exp_diagonals(valid=m, balanced=False)
        valid, w = np.asarray(m, bool), np.ones(nb)
    else:
        ch.bal_iterate(m)
        w = ch.bal_weights()
        valid = ~np.isnan(w)
        ch.exp_diagonals()
    p, _, vs = ch.exp_diagonals_get()
    e, _ = expected.expected_of(p, vs, ign)
    return ch.cells, b0, nb, valid, w, e, p


# ---- the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ign,raw", [(0, False), (2, False), (2, True), (1, True)])
def test_the_two_forms_of_the_product_agree(ign, raw):
    X, Y = MC.scattered(3, 20000, 150000, 40000, both=True)
    cells, b0, nb, valid, w, e, p = state_of(X, Y, 1000, ign, raw, mask=lambda nb: np.arange(nb) % 7 != 3)
    oe = EC.oe_oracle(*cells, b0, nb, ign, valid, w, e)
    rng = np.random.default_rng(ign)
    x = rng.standard_normal((3, nb))
    full = compartments.pick_dmax(p, e, ign)
    worst = 0.0
    for clip in (float(np.nanpercentile(oe, 90)), float("inf")):
        for dmax in sorted({ign, (ign + full) // 2, full}):
            M = CC.dense_M(cells, b0, nb, ign, valid, w, e, clip, dmax)
            assert np.array_equal(M, M.T) and not M[~valid].any() and not M[:, ~valid].any()
            d = np.abs(np.arange(nb)[:, None] - np.arange(nb)[None, :])
            assert not M[(d < ign) | (d >= dmax)].any() and (dmax == ign or M.min() == -1.0)
            assert M.max() <= clip - 1.0 or dmax == ign
            want = (M @ np.where(valid, x, 0.0).T).T
            got = CC.apply_sparse(cells, b0, nb, ign, valid, w, e, clip, dmax, x)
            bound = CC.apply_bound(cells, b0, nb, ign, valid, w, e, clip, dmax, x)
            assert np.all(np.abs(got - want) <= bound), (clip, dmax, np.max(np.abs(got - want) / bound))
            worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(bound, 1e-300))))
            assert dmax == ign or np.abs(want).max() > 1.0
            one = CC.apply_sparse(cells, b0, nb, ign, valid, w, e, clip, dmax, x[1])
            assert one.shape == (nb,) and np.array_equal(one, got[1])
    print("K27 oracle: the sparse form against the dense one, largest deviation over its bound %.3g" % worst)
    assert 0.0 < worst <= 1.0


def test_the_dense_matrix_by_its_own_loop():
    """dense_M against the definition's loop on the twelve rows, raw: expected = 1 everywhere, so oe is the count"""
    X, Y = MC.twelve()
    cells = MC.cells_oracle(X, Y, 0, 100, True)[:3]
    valid = np.array([True, True, False, True, True])
    M = CC.dense_M(cells, 0, 5, 1, valid, np.ones(5), np.ones(5), 1.5, 4)
    cnt = MC.dense_scatter(*cells, 0, 0, 5, 5)
    for i in range(5):
        for j in range(5):
            c = cnt[min(i, j)][max(i, j)]
            want = min(float(c), 1.5) - 1.0 if valid[i] and valid[j] and 1 <= abs(i - j) < 4 else 0.0
            assert M[i][j] == want, (i, j)
    with pytest.raises(ValueError):
        CC.dense_M(cells, 0, 5, 1, valid, np.ones(5), np.array([1, 1, 0, 1, 1.0]), 1.5, 4)
    assert CC.dense_M(cells, 0, 5, 1, valid, np.ones(5), np.array([1, 1, 0, 1, 1.0]), 1.5, 2).shape == (5, 5)   # dmax keeps the zero out


@pytest.mark.parametrize("name", ["small", "large"])
def test_the_planted_data_has_the_gaps_the_gpu_tests_lean_on(name):
    """Each of the first three reference eigenvalues lies at least 5 % of |lambda_0| from every other eigenvalue (|lambda_k -
    lambda_j|: the gap Davis-Kahan divides by).  At seed 1, res 1000, ignore_diags 2, a 99.9 clip, `pets` counted as kept PETs and
    every diagonal's own average as its expected value this restatement gives 108.9, -68.0, 42.5, -38.2 (gaps 0.61, 0.27, 0.063 of
    |lambda_0|; Pearson of E1 with the plant 0.956) at 300 bins and 445.1, -266.1, 149.3, -132.2 (0.66, 0.30, 0.063; 0.959) at 1200:
    near the figures the feature was specified with (125.2, -74.5, 49.9, -45.4 and 465.4, -271.4, 150.2, -137.2), not equal to them."""
    c = CC.planted_case(name)
    ev = c["eigvals"]
    gaps = CC.gaps_of(ev)
    r = compartments.pearson(c["vectors"][0], c["comp"].astype(np.float64))
    print("planted %s: nb %d, PETs %d, leading eigenvalues %s, gaps over |lambda_0| %s, Pearson of E1 with the plant %.3f" %
          (name, c["nb"], len(c["X"]), np.round(ev[:4], 1).tolist(), np.round(gaps[:3] / abs(ev[0]), 3).tolist(), r))
    assert np.all(gaps[:3] >= 0.05 * abs(ev[0]))
    assert abs(r) > 0.8
    assert c["ign"] < c["dmax"] <= c["nb"] and np.isfinite(c["clip"]) and c["valid"].sum() > 0.9 * c["nb"]


def test_eig_oracle_orders_and_signs():
    M = np.diag([1.0, -3.0, 2.0, 0.0])
    M[0, 2] = M[2, 0] = 0.5
    valid = np.array([True, True, True, False])
    lam, vec, ev = CC.eig_oracle(M, valid, 6)
    assert lam[0] == -3.0 and abs(lam[1]) > abs(lam[2]) and np.isnan(lam[3:]).all() and len(ev) == 3
    assert np.isnan(vec[:3, 3]).all() and np.isnan(vec[3:]).all()
    for k in range(3):
        v = np.where(valid, vec[k], 0.0)
        assert abs(np.linalg.norm(v) - 1.0) < 1e-15 and v[np.argmax(np.abs(v))] > 0 and np.allclose(M @ v, lam[k] * v, atol=1e-15)
    assert np.array_equal(CC.sign_rule(np.array([0.5, -0.5, np.nan])), [0.5, -0.5, np.nan], equal_nan=True)
    assert np.array_equal(CC.sign_rule(np.array([-0.5, 0.5])), [0.5, -0.5])


# ---- the host functions --------------------------------------------------------------------------------------------------
def test_dmax_and_the_clip():
    p = np.array([5, 4, 3, 2, 0, 1])
    e = np.array([np.nan, np.nan, 1.0, 2.0, np.nan, 0.5])
    assert compartments.pick_dmax(p, e, 2) == 6                               # (a diagonal without pairs may have any value)
    assert compartments.pick_dmax(p, np.array([np.nan, np.nan, 1.0, 0.0, 1.0, 1.0]), 2) == 3
    assert compartments.pick_dmax(p, np.array([np.nan, np.nan, 1.0, 1.0, 1.0, np.inf]), 2) == 5
    assert compartments.pick_dmax(p, np.array([np.nan, 1.0, 1.0, -1.0, 1.0, 1.0]), 0) == 0
    assert compartments.pick_dmax(p, e, 7) == 6 and compartments.pick_dmax(np.zeros(0), np.zeros(0), 2) == 0
    oe = np.array([np.nan, 1.0, 2.0, 3.0, 4.0, np.nan, 5.0])
    assert compartments.clip_of(oe, 50) == 3.0 and compartments.clip_of(oe, 100) == float("inf")
    assert compartments.clip_of(oe, 99.9) == float(np.percentile([1.0, 2.0, 3.0, 4.0, 5.0], 99.9))
    assert compartments.clip_of(np.array([np.nan]), 50) == float("inf") and compartments.clip_of(np.zeros(0), 50) == float("inf")


def test_orientation():
    v = np.array([0.5, -0.5, np.nan, 0.5, -0.5])
    cov = np.array([10.0, 1.0, 7.0, 9.0, 2.0])
    out, flip, r = compartments.orient(v, cov)
    assert not flip and r > 0.9 and np.array_equal(out, v, equal_nan=True)
    out, flip, r = compartments.orient(v, -cov)
    assert flip and r < -0.9 and np.array_equal(out, -v, equal_nan=True)
    out, flip, r = compartments.orient(v, np.array([1.0, 1.0, 5.0, 1.0, 1.0]))  # no spread over the valid bins: NaN
    assert not flip and np.isnan(r) and np.array_equal(out, v, equal_nan=True)
    out, flip, r = compartments.orient(np.array([1.0, -1.0, 1.0, -1.0]), np.array([1.0, 1.0, 2.0, 2.0]))
    assert not flip and r == 0.0                                              # a zero correlation leaves the sign
    out, flip, r = compartments.orient(v, np.array([np.nan, np.nan, 1.0, 1.0, 2.0]))   # the bins without a track value take no part
    assert flip and r == -1.0
    # a phase track: the overlap-length-weighted mean per bin
    t = compartments.bin_track([0, 150, 390, 1000], [100, 250, 410, 1100], [2.0, 4.0, 6.0, 9.0], 0, 5, 100)
    assert np.array_equal(t, [2.0, 4.0, 4.0, 6.0, 6.0], equal_nan=True)
    t = compartments.bin_track([50, 80], [100, 120], [1.0, 3.0], 0, 3, 100)
    assert t[0] == (50 * 1.0 + 20 * 3.0) / 70 and t[1] == 3.0 and np.isnan(t[2])
    t = compartments.bin_track([-250], [-150], [5.0], -3, 3, 100)
    assert np.array_equal(t, [5.0, 5.0, np.nan], equal_nan=True)


def test_the_runs():
    valid = np.array([1, 1, 1, 0, 1, 1, 1, 1, 1, 1], bool)
    e1 = np.array([1.0, 2.0, -1.0, -5.0, -2.0, 0.0, 3.0, np.nan, 4.0, 4.0])
    runs = compartments.compartment_runs(valid, e1)
    assert runs == [(0, 2, "A", 1.5), (2, 3, "B", -1.0), (4, 5, "B", -2.0), (6, 7, "A", 3.0), (8, 10, "A", 4.0)]
    assert compartments.format_runs("chr3", 100, -2, valid, e1) == ("chr3\t-200\t0\tA\t1.5\nchr3\t0\t100\tB\t-1\nchr3\t200\t300\tB\t-2\n"
                                                                   "chr3\t400\t500\tA\t3\nchr3\t600\t800\tA\t4\n")
    assert compartments.compartment_runs(np.zeros(0, bool), np.zeros(0)) == [] and compartments.compartment_runs(np.zeros(3, bool), np.ones(3)) == []
    assert compartments.format_eigs("c", 10, 1, np.array([True, False]), np.array([[0.25, np.nan], [-1.0, np.nan]])) == \
        "c\t10\t20\t1\t0.25\t-1\nc\t20\t30\t0\tnan\tnan\n"
    assert compartments.format_bedgraph("c", 10, 1, np.array([True, False, True]), np.array([0.25, np.nan, -3.0])) == "c\t10\t20\t0.25\nc\t30\t40\t-3\n"


def test_the_texts_and_the_json(standin, tmp_path):
    out = os.path.join(str(tmp_path), "c")
    js = compartments.jd2compartments("jd", out, res=1000, chroms={"chr1"}, n_eigs=3, nosmooth=True)
    got = _read(out, compartments.SUFFIXES)
    assert sorted(os.listdir(str(tmp_path))) == sorted("c" + s for s in compartments.SUFFIXES)
    c = CC.planted_case("small")
    st = js["chroms"]["chr1"]
    assert (st["b0"], st["nb"], st["n_valid"], st["dmax"], st["clip"]) == (c["b0"], c["nb"], int(c["valid"].sum()), c["dmax"], balance._num(c["clip"]))
    assert st["eigvals"] == [balance._num(x) for x in c["eigvals"][:3].tolist()] and st["eig_converged"] and st["converged"] and st["eig_iters"] == 1
    assert st["n_in"] == int(CC.band_cells(c["cells"][0], c["cells"][1], c["b0"], c["nb"], 2, c["valid"], c["dmax"]).sum())
    assert len(st["resid"]) == 3 and max(st["resid"]) < 1e-10 and len(st["flipped"]) == 3 and len(st["phase_corr"]) == 3
    assert js["args"] == {"res": 1000, "cut": 0, "raw": False, "per_decade": 10, "nosmooth": True, "ignore_diags": 2, "min_nnz": 10, "min_count": 0,
                          "mad_max": 5.0, "tol": 1e-5, "max_iters": 200, "n_eigs": 3, "clip": 99.9, "eig_tol": 1e-8, "eig_iters": 1000, "phase": None}
    assert got["_eigs.json"] == json.dumps(js, indent=1, sort_keys=True) + "\n" and json.loads(got["_eigs.json"]) == js
    # the table: the oracle's vectors, oriented by the coverage and scaled by sqrt(|lambda|)
    rows = [line.split("\t") for line in got["_eigs.txt"].splitlines()]
    assert len(rows) == c["nb"] and all(len(r) == 7 and r[0] == "chr1" for r in rows)
    assert [int(r[1]) for r in rows] == [(c["b0"] + i) * 1000 for i in range(c["nb"])] and [int(r[3]) for r in rows] == c["valid"].astype(int).tolist()
    E1 = np.array([float(r[4]) for r in rows])
    cov = np.where(c["valid"], BC.marginals_oracle(*c["cells"], 2)[3].astype(np.float64), np.nan)
    want = c["vectors"][0] * np.sqrt(abs(c["eigvals"][0]))
    if compartments.pearson(c["vectors"][0], cov) < 0:
        want = -want
    assert st["flipped"][0] == bool(compartments.pearson(c["vectors"][0], cov) < 0)
    assert np.array_equal(np.isnan(E1), ~c["valid"]) and np.allclose(E1[c["valid"]], want[c["valid"]], rtol=1e-9, atol=0)
    assert abs(compartments.pearson(E1, c["comp"].astype(np.float64))) > 0.8
    # the bedGraph holds the valid bins, the runs tile them by sign
    bg = [line.split("\t") for line in got["_E1.bedGraph"].splitlines()]
    assert len(bg) == int(c["valid"].sum()) and [b[3] for b in bg] == [r[4] for r in rows if r[3] == "1"]
    runs = [line.split("\t") for line in got["_compartments.bed"].splitlines()]
    mine = compartments.compartment_runs(c["valid"], E1)                      # (of the table's ten digits: the means agree to nine)
    assert [(int(r[1]), int(r[2]), r[3]) for r in runs] == [((c["b0"] + s) * 1000, (c["b0"] + e) * 1000, n) for s, e, n, _ in mine]
    assert np.allclose([float(r[4]) for r in runs], [m for _, _, _, m in mine], rtol=1e-9, atol=0)
    assert {r[3] for r in runs} == {"A", "B"} and all((float(r[4]) > 0) == (r[3] == "A") for r in runs)
    assert sum((int(r[2]) - int(r[1])) // 1000 for r in runs) == int((c["valid"] & (E1 != 0)).sum())
    ch = standin["chr1"].chrom
    assert ch.cells is None and ch.bal is None and ch.exp is None and ch.eig is None       # freed


def test_a_phase_track_orients_the_vectors(standin, tmp_path):
    c = CC.planted_case("small")
    track = os.path.join(str(tmp_path), "t.bedGraph")
    out = os.path.join(str(tmp_path), "p")
    for sign in (1.0, -1.0):
        with open(track, "w") as fh:
            fh.write("track type=bedGraph\n")
            for i in range(0, c["nb"], 2):                                   # every second bin: the others take no part
                fh.write("chr1\t%d\t%d\t%g\n" % (i * 1000, i * 1000 + 1000, sign * (1.0 if c["comp"][i] else -1.0)))
        js = compartments.jd2compartments("jd", out, res=1000, chroms={"chr1"}, n_eigs=1, phase=track)
        E1 = np.array([float(line.split("\t")[4]) for line in _read(out, compartments.SUFFIXES)["_eigs.txt"].splitlines()])
        r = compartments.pearson(E1, c["comp"].astype(np.float64))
        assert abs(r) > 0.8 and (r > 0) == (sign > 0) and js["chroms"]["chr1"]["phase_corr"][0] is not None
        assert js["args"]["phase"] == track
    # a track without the chromosome: no bin takes part, the device's sign stays
    with open(track, "w") as fh:
        fh.write("chr7\t0\t1000\t1\n")
    js = compartments.jd2compartments("jd", out, res=1000, chroms={"chr1"}, n_eigs=1, phase=track)
    assert js["chroms"]["chr1"]["flipped"] == [False] and js["chroms"]["chr1"]["phase_corr"] == [None]


def test_a_chromosome_with_fewer_bins_than_ignored_diagonals(standin, tmp_path, caplog):
    """one bin at ignore_diags = 2: no band and no matrix; NaN rows, a warning, and the other chromosomes are written as ever"""
    standin["chrM"] = Record(np.array([100, 200, 300]), np.array([150, 900, 420]))
    out = os.path.join(str(tmp_path), "s")
    with caplog.at_level("WARNING"):
        js = compartments.jd2compartments("jd", out, res=1000, chroms={"chr1", "chrM"}, n_eigs=2, nosmooth=True)
    st = js["chroms"]["chrM"]
    assert (st["nb"], st["dmax"], st["n_in"], st["eig_iters"], st["eig_converged"]) == (1, 1, 0, 0, False)
    assert st["eigvals"] == [None, None] and st["resid"] == [None, None] and st["flipped"] == [False, False]
    assert "chrM" in caplog.text and "fewer" in caplog.text
    got = _read(out, compartments.SUFFIXES)
    lines = [l for l in got["_eigs.txt"].splitlines() if l.startswith("chrM\t")]
    assert len(lines) == 1 and lines[0].split("\t")[4:] == ["nan", "nan"] and "chrM" not in got["_compartments.bed"]
    assert js["chroms"]["chr1"]["eig_converged"] and len(got["_eigs.txt"].splitlines()) == 1 + js["chroms"]["chr1"]["nb"]
    assert standin["chrM"].chrom.cells is None                                # freed


def test_raw_mode_and_both_chromosomes(standin, tmp_path):
    out = os.path.join(str(tmp_path), "b")
    js = compartments.jd2compartments("jd", out, res=2000, raw=True, n_eigs=2, clip=100, min_nnz=3)
    assert list(js["chroms"]) == ["chr1", "chr2"] and all(not js["chroms"][n]["converged"] and js["chroms"][n]["eig_converged"] for n in js["chroms"])
    assert all(js["chroms"][n]["clip"] is None or js["chroms"][n]["clip"] == float("inf") for n in js["chroms"])
    got = _read(out, compartments.SUFFIXES)
    assert got["_eigs.txt"].startswith("chr1\t") and "\nchr2\t" in got["_eigs.txt"] and len(got["_eigs.txt"].splitlines()[0].split("\t")) == 6


# ---- refusals and the command line -------------------------------------------------------------------------------------
def test_nothing_is_written_when_an_argument_is_refused(standin, tmp_path):
    out = os.path.join(str(tmp_path), "r")
    J = compartments.jd2compartments
    bad = [lambda: J("jd", out, res=0), lambda: J("jd", out, ignore_diags=-1), lambda: J("jd", out, tol=-1e-9), lambda: J("jd", out, per_decade=0),
           lambda: J("jd", out, n_eigs=0), lambda: J("jd", out, n_eigs=7), lambda: J("jd", out, n_eigs=2.5), lambda: J("jd", out, n_eigs=None),
           lambda: J("jd", out, clip=0), lambda: J("jd", out, clip=100.5), lambda: J("jd", out, clip=float("nan")), lambda: J("jd", out, eig_tol=-1.0),
           lambda: J("jd", out, eig_tol=float("nan")), lambda: J("jd", out, eig_iters=-1), lambda: J("jd", out, eig_iters=1.5),
           lambda: J("jd", out, phase=os.path.join(str(tmp_path), "missing.bedGraph"))]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    assert os.listdir(str(tmp_path)) == []
    assert all(r.chrom.calls == [] for r in standin.values())                # ... and before any work on a chromosome
    broken = os.path.join(str(tmp_path), "broken.bedGraph")
    with open(broken, "w") as fh:
        fh.write("chr1\t0\tx\t1\n")
    with pytest.raises(ValueError):
        J("jd", out, phase=broken)
    assert os.listdir(str(tmp_path)) == ["broken.bedGraph"]


def test_help_defaults_and_overrides():
    op = compartments.help(["-d", "jd", "-o", "out"])
    assert (op.d, op.output, op.res, op.cut, op.chroms, op.neigs, op.clip, op.eigtol, op.eigiters, op.phase, op.raw, op.perdecade, op.nosmooth,
            op.ignorediags, op.minnnz, op.mincount, op.mad, op.tol, op.maxiters) == \
        ("jd", "out", 100000, 0, "", 3, 99.9, 1e-8, 1000, None, False, 10, False, 2, 10, 0, 5.0, 1e-5, 200)
    op = compartments.help(["-d", "jd", "-o", "out", "-res", "2500", "-neigs", "5", "-clip", "100", "-eigtol", "1e-6", "-eigiters", "50", "-phase",
                            "gc.bedGraph", "-c", "chr1", "-cut", "3", "-raw"])
    assert (op.res, op.neigs, op.clip, op.eigtol, op.eigiters, op.phase, op.chroms, op.cut, op.raw) == (2500, 5, 100.0, 1e-6, 50, "gc.bedGraph", "chr1", 3, True)
    for bad in ([], ["-d", "jd"], ["-d", "jd", "-o", "out", "-neigs", "x"], ["-d", "jd", "-o", "out", "-raw", "1"]):
        with pytest.raises(SystemExit):
            compartments.help(bad)


def test_main_writes_the_files(standin, tmp_path):
    out = os.path.join(str(tmp_path), "m")
    assert compartments.main(["-d", "jd", "-o", out, "-res", "1000", "-c", "chr1", "-neigs", "2"]) == 0
    first = _read(out, compartments.SUFFIXES)
    compartments.jd2compartments("jd", out, res=1000, chroms={"chr1"}, n_eigs=2)
    assert _read(out, compartments.SUFFIXES) == first
    with pytest.raises(ValueError):
        compartments.main(["-d", "jd", "-o", os.path.join(str(tmp_path), "z"), "-neigs", "0"])
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("z")]


def test_suffixes_are_its_own():
    assert compartments.SUFFIXES == ("_eigs.txt", "_E1.bedGraph", "_compartments.bed", "_eigs.json")
    assert set(compartments.SUFFIXES).isdisjoint(matrix.SUFFIXES) and set(compartments.SUFFIXES).isdisjoint(balance.SUFFIXES)
    assert set(compartments.SUFFIXES).isdisjoint(expected.SUFFIXES)


def test_the_stand_in_keeps_the_order_of_calls():
    X, Y = MC.scattered(1, 4000, 60000, 20000, both=True)
    ch = CC.OracleChrom(X, Y)
    ch.mat_cells(2000, fold=True)
    b0, nb, _ = ch.bal_marginals(2)
    ch.exp_diagonals(balanced=False)
    with pytest.raises(RuntimeError):
        ch.eig_build()                                                       # before exp_set
    p, _, vs = ch.exp_diagonals_get()
    e, _ = expected.expected_of(p, vs, 2)
    ch.exp_set(e)
    for f in (lambda: ch.eig_apply(np.zeros(nb)), lambda: ch.eig_iterate(), lambda: ch.eig_vectors(0)):
        with pytest.raises(RuntimeError):
            f()
    nv, n_in = ch.eig_build(float("inf"), compartments.pick_dmax(p, e, 2))
    assert nv == nb and n_in > 100
    with pytest.raises(RuntimeError):
        ch.eig_vectors(0)
    it, cv, lam, resid = ch.eig_iterate(2)
    assert (it, cv) == (1, True) and abs(lam[0]) >= abs(lam[1]) and len(ch.eig_vectors(1)) == nb
    with pytest.raises(RuntimeError):
        ch.eig_vectors(2)
    bad = e.copy()
    bad[5] = 0.0
    ch.exp_set(bad)
    with pytest.raises(RuntimeError):
        ch.eig_apply(np.zeros(nb))                                            # exp_set dropped the matrix
    with pytest.raises(RuntimeError):
        ch.eig_build(float("inf"), nb)                                        # the rule on the expected values
    assert ch.eig_build(float("inf"), 5)[0] == nb
    ch.bal_marginals(2)
    with pytest.raises(RuntimeError):
        ch.eig_build()


# ---- the walk down the device state, the options and the clean-up that the commands share -------------------------------------
def test_the_calls_on_the_device_and_no_more():
    head = [("mat_cells", (100,), {"cut": 0, "fold": True}), ("bal_marginals", (2,), {}), ("bal_marginals_get", (0, 5), {})]
    tail = [("exp_diagonals_get", (0, 5), {}), ("exp_set", ("f[5]",), {}), ("exp_cells_get", (0, 7), {}), ("exp_cells_get", (7, 3), {}),
            ("eig_build", (float("inf"), 5), {}), ("eig_iterate", (2,), {"max_iters": 1000, "tol": 1e-8}), ("eig_vectors", (0, 0, 5), {}),
            ("eig_vectors", (1, 0, 5), {}), ("mat_free", (), {})]
    ch = MC.Recording(CC.OracleChrom(*MC.twelve()))
    compartments.compartments_chrom(ch, "chr1", 100, n_eigs=2, clip=100, ignore_diags=2, min_nnz=1, chunk=7)
    assert ch.log == head + [("bal_iterate", ("b[5]",), {"max_iters": 200, "tol": 1e-5}), ("bal_weights", (0, 5), {}), ("exp_diagonals", (), {})] + tail
    ch = MC.Recording(CC.OracleChrom(*MC.twelve()))
    compartments.compartments_chrom(ch, "chr1", 100, n_eigs=2, clip=100, ignore_diags=2, min_nnz=1, chunk=7, raw=True)
    assert ch.log == head + [("exp_diagonals", (), {"valid": "b[5]", "balanced": False})] + tail


def test_main_hands_every_option_on(standin, tmp_path):
    out = os.path.join(str(tmp_path), "o")
    kw = dict(res=2000, cut=20, n_eigs=2, clip=95.0, eig_tol=1e-6, eig_iters=77, phase=None, raw=True, per_decade=4, nosmooth=True, ignore_diags=1,
              min_nnz=3, min_count=1, mad_max=2.5, tol=1e-8, max_iters=30)
    js = compartments.jd2compartments("jd", out + "k", chroms={"chr1", "chr2"}, **kw)
    assert js["args"] == kw
    assert compartments.main(["-d", "jd", "-o", out + "m", "-res", "2000", "-cut", "20", "-c", "chr1,chr2", "-neigs", "2", "-clip", "95", "-eigtol",
                              "1e-6", "-eigiters", "77", "-raw", "-perdecade", "4", "-nosmooth", "-ignorediags", "1", "-minnnz", "3", "-mincount",
                              "1", "-mad", "2.5", "-tol", "1e-8", "-maxiters", "30"]) == 0
    assert _read(out + "m", compartments.SUFFIXES) == _read(out + "k", compartments.SUFFIXES)


@pytest.mark.parametrize("step", ["bal_iterate", "bal_weights", "exp_set", "eig_build", "eig_vectors"])
def test_a_failing_step_frees_the_cells_once_and_writes_nothing(step, standin, tmp_path):
    standin["chr1"].chrom = ch = MC.Recording(standin["chr1"].chrom, fail=step)
    with pytest.raises(RuntimeError):
        compartments.jd2compartments("jd", os.path.join(str(tmp_path), "f"), res=2000, n_eigs=2)
    assert [c[0] for c in ch.log].count("mat_free") == 1 and ch.log[-1][0] == "mat_free" and ch.log[-2][0] == step
    assert os.listdir(str(tmp_path)) == [] and standin["chr2"].chrom.calls == []
