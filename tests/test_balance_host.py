"""CPU: the oracle of K25 on a planted case and on the hand-written rows, the mask's rules, the host side of cloops_amd.balance -- the
four texts byte for byte through the oracle's stand-in chromosome, the command line, and that a refused argument writes nothing."""
import json
import os
import threading

import numpy as np
import pytest

import balance_cases as BC
import matrix_cases as MC
from cloops_amd import balance, matrix


class Record(object):
    def __init__(self, X, Y):
        self.chrom, self.lock = BC.OracleChrom(X, Y), threading.Lock()


@pytest.fixture
def standin(monkeypatch):
    """matrix._records (which balance reads) served by stand-in chromosomes: chr1 = the twelve rows, chr2 = 300 scattered ones"""
    recs = {"chr1": Record(*MC.twelve()), "chr2": Record(*MC.scattered(1, 300, 5000, 900, both=True))}
    monkeypatch.setattr(matrix, "_records", lambda jd, chroms=(): [(n, recs[n]) for n in sorted(recs) if len(chroms) == 0 or n in chroms])
    return recs


def _read(prefix, suffixes):
    out = {}
    for s in suffixes:
        with open(prefix + s) as fh:
            out[s] = fh.read()
    return out


# ---- the oracle ------------------------------------------------------------------------------------------------------
def test_oracle_recovers_a_planted_bias():
    bx, by, cnt, d = BC.planted()
    b0, nb, nu, s, z = BC.marginals_oracle(bx, by, cnt, 0)
    assert (b0, nb, nu) == (0, 24, 24 * 25 // 2) and (z == 24).all()
    o = BC.ice_oracle(bx, by, cnt, 0, np.ones(nb, bool), 200, 1e-12)
    assert o["converged"] and 0 < o["iters"] < 50 and o["var"] < 1e-12
    wd = o["weight"] * d
    # var < tol bounds the spread of the balanced rows' sums (|s / mean - 1| < sqrt(nb tol)), and weight d is the root of that ratio
    assert np.ptp(wd) / wd.mean() < np.sqrt(24 * 1e-12)
    bal = BC.balanced_oracle(bx, by, cnt, b0, o["weight"])
    full = MC.dense_scatter(bx, by, np.zeros(len(bx)), 0, 0, 24, 24).astype(np.float64)
    np.add.at(full, (bx, by), bal)
    full = full + np.triu(full, 1).T
    assert np.allclose(full.sum(1), 1.0, rtol=0, atol=1e-5)                  # rows of the balanced matrix sum to 1
    # another order of the cells moves the result by rounding only
    p = BC.ice_oracle(bx, by, cnt, 0, np.ones(nb, bool), 200, 1e-12, perm=BC.cell_perm(len(bx), 1))
    assert p["iters"] == o["iters"] and BC.rel_diff(p["weight"], o["weight"]) < 1e-13


def test_oracle_on_the_twelve_rows():
    bx, by, cnt, _ = MC.cells_oracle(*MC.twelve(), 0, 100, True)
    b0, nb, nu, s, z = BC.marginals_oracle(bx, by, cnt, 0)
    assert (b0, nb, nu) == (0, 5, 10) and s.tolist() == [4, 5, 2, 4, 5] and z.tolist() == [3, 4, 2, 3, 4]
    assert s.dtype == np.uint64 and z.dtype == np.uint32
    b0, nb, nu, s, z = BC.marginals_oracle(bx, by, cnt, 2)                   # (0,4,2) (1,3,2) (1,4,1) (2,4,1) are used
    assert (b0, nb, nu) == (0, 5, 4) and s.tolist() == [2, 3, 1, 2, 4] and z.tolist() == [1, 2, 1, 1, 3]
    assert BC.marginals_oracle(bx, by, cnt, 5)[2] == 0 and not BC.marginals_oracle(bx, by, cnt, 5)[3].any()
    o = BC.ice_oracle(bx, by, cnt, 2, np.ones(5, bool), 50, 1e-5)            # bipartite ({0, 1, 2} against {3, 4}): it oscillates
    assert (o["iters"], o["converged"]) == (50, False) and abs(o["var"] - 0.0726643) < 1e-6
    o = BC.ice_oracle(bx, by, cnt, 0, np.ones(5, bool), 200, 1e-5)
    assert (o["iters"], o["converged"]) == (16, True) and 0.5e-5 < o["var"] < 1e-5
    # a masked bin: NaN, and its cells do not enter the others' sums -- the same as balancing without those cells
    v = np.array([1, 1, 0, 1, 1], bool)
    m = BC.ice_oracle(bx, by, cnt, 0, v, 200, 1e-8)
    keep = (bx != 2) & (by != 2)
    q = BC.ice_oracle(bx[keep], by[keep], cnt[keep], 0, v, 200, 1e-8)
    assert np.isnan(m["weight"][2]) and np.array_equal(m["weight"], q["weight"], equal_nan=True)
    # nothing used, no iterations, an empty input
    o = BC.ice_oracle(bx, by, cnt, 5, np.ones(5, bool))
    assert (o["iters"], o["converged"]) == (0, False) and np.isnan([o["var"], o["scale"]]).all() and np.isnan(o["weight"]).all()
    o = BC.ice_oracle(bx, by, cnt, 0, np.ones(5, bool), 0)
    assert o["iters"] == 0 and np.isnan(o["weight"]).all()
    e = np.zeros(0, np.int32)
    assert BC.marginals_oracle(e, e, e, 2)[:3] == (0, 0, 0) and BC.ice_oracle(e, e, e, 2, np.zeros(0, bool))["iters"] == 0


def test_mask_rules():
    for f in (balance.valid_bins, BC.valid_oracle):
        s = np.array([100, 120, 90, 110, 1, 0, 105, 95], np.uint64)
        z = np.array([12, 12, 9, 30, 12, 0, 10, 11], np.uint32)
        assert f(s, z, 10, 0, 0).tolist() == [True, True, False, True, True, False, True, True]          # nnz alone (and sum >= 1)
        assert f(s, z, 0, 100, 0).tolist() == [True, True, False, True, False, False, True, False]       # sum >= min_count
        assert f(s, z, 0, 0, 0).tolist() == [True, True, True, True, True, False, True, True]            # sum >= 1 always
        # log(sum): med = log(100), mad = log(100 / 90) or so; the bin with sum 1 lies 40 mads below
        assert f(s, z, 0, 0, 5).tolist() == [True, True, True, True, False, False, True, True]
        assert f(s, z, 0, 0, 60).tolist() == [True, True, True, True, True, False, True, True]
        assert f(s, z, 10, 0, 5).tolist() == [True, True, False, True, False, False, True, True]
        zero = np.zeros(4, np.uint64)
        assert f(zero, np.zeros(4, np.uint32), 0, 0, 5).tolist() == [False] * 4                          # no sum > 0: no median, nothing valid
        assert f(zero[:0], zero[:0], 10, 0, 5).tolist() == []
        same = np.full(6, 50, np.uint64)
        assert f(same, np.full(6, 20, np.uint32), 10, 0, 5).all()                                         # mad = 0: log(sum) >= med holds
    rng = np.random.default_rng(2)
    s, z = rng.integers(0, 5000, 500), rng.integers(0, 40, 500)
    for args in ((10, 0, 5), (0, 300, 0), (5, 0, 1.5)):
        assert np.array_equal(balance.valid_bins(s, z, *args), BC.valid_oracle(s, z, *args))


# ---- the texts -------------------------------------------------------------------------------------------------------
BINS_TXT = ("chr1\t0\t100\t4\t3\t0.6023442088\nchr1\t100\t200\t5\t4\t0.4005422796\nchr1\t200\t300\t2\t2\t0.8470209617\n"
            "chr1\t300\t400\t4\t3\t0.584239627\nchr1\t400\t500\t5\t4\t0.3292309946\n")
CELLS_TXT = ("chr1\t0\t100\tchr1\t0\t100\t1\t0.3628185459\nchr1\t0\t100\tchr1\t100\t200\t1\t0.2412643225\n"
             "chr1\t0\t100\tchr1\t400\t500\t2\t0.3966207659\nchr1\t100\t200\tchr1\t100\t200\t1\t0.1604341177\n"
             "chr1\t100\t200\tchr1\t300\t400\t2\t0.468025344\nchr1\t100\t200\tchr1\t400\t500\t1\t0.1318709331\n"
             "chr1\t200\t300\tchr1\t200\t300\t1\t0.7174445096\nchr1\t200\t300\tchr1\t400\t500\t1\t0.2788655537\n"
             "chr1\t300\t400\tchr1\t300\t400\t1\t0.3413359417\nchr1\t300\t400\tchr1\t400\t500\t1\t0.1923497935\n")
MATRIX_TXT = ("\tchr1:100-200\tchr1:200-300\tchr1:300-400\nchr1:100-200\t0.1604341177\t0\t0.468025344\n"
              "chr1:200-300\t0\t0.7174445096\t0\nchr1:300-400\t0.468025344\t0\t0.3413359417\n")
ARGS = dict(res=100, ignore_diags=0, min_nnz=1)


def test_the_four_texts(standin, tmp_path):
    out = os.path.join(str(tmp_path), "b")
    js = balance.jd2balance("jd", out, chroms={"chr1"}, region="chr1:100-400", **ARGS)
    got = _read(out, balance.SUFFIXES)
    assert (got["_balance.txt"], got["_balanced_cells.txt"], got["_balanced_matrix.txt"]) == (BINS_TXT, CELLS_TXT, MATRIX_TXT)
    st = js["chroms"]["chr1"]
    assert {k: st[k] for k in ("b0", "nb", "n_used", "n_valid", "iters", "converged")} == \
        {"b0": 0, "nb": 5, "n_used": 10, "n_valid": 5, "iters": 16, "converged": True}
    assert abs(st["var"] - 7.1631827641550376e-06) < 1e-15 and abs(st["scale"] - 4.352666867779687) < 1e-9
    assert js["args"] == {"res": 100, "cut": 0, "ignore_diags": 0, "min_nnz": 1, "min_count": 0, "mad_max": 5.0, "tol": 1e-5, "max_iters": 200,
                          "region": "chr1:100-400"}
    assert got["_balance.json"] == json.dumps(js, indent=1, sort_keys=True) + "\n" and json.loads(got["_balance.json"]) == js
    assert sorted(os.listdir(str(tmp_path))) == sorted("b" + s for s in balance.SUFFIXES)
    assert standin["chr1"].chrom.cells is None and standin["chr1"].chrom.bal is None              # freed


def test_chromosomes_in_name_order_chunks_and_nan(standin, tmp_path):
    out = os.path.join(str(tmp_path), "c")
    js = balance.jd2balance("jd", out, **ARGS)
    got = _read(out, balance.SUFFIXES[:3])
    assert not os.path.exists(out + balance.SUFFIXES[3])                      # no region: three files
    names = [line.split("\t")[0] for line in got["_balance.txt"].splitlines()]
    assert names == sorted(names) and set(names) == {"chr1", "chr2"} and sorted(js["chroms"]) == ["chr1", "chr2"]
    assert got["_balance.txt"].startswith(BINS_TXT) and got["_balanced_cells.txt"].startswith(CELLS_TXT)
    assert all(len(line.split("\t")) == 8 for line in got["_balanced_cells.txt"].splitlines())
    # the seven bg2 columns are those of matrix.jd2cells
    matrix.jd2cells("jd", out, res=100)
    with open(out + "_cells.txt") as fh:
        assert fh.read().splitlines() == ["\t".join(line.split("\t")[:7]) for line in got["_balanced_cells.txt"].splitlines()]
    ch = standin["chr2"].chrom
    whole = balance.balance_chrom(ch, "chr2", 250, ignore_diags=1, min_nnz=2)
    assert balance.balance_chrom(ch, "chr2", 250, ignore_diags=1, min_nnz=2, chunk=7) == whole and whole["cells"].count("\n") > 7
    assert "\tnan\n" in whole["bins"] and "\tnan\n" in whole["cells"] and whole["stats"]["n_valid"] < whole["stats"]["nb"]
    # a chromosome that does not converge is reported, not dropped; NaN goes into the json as null
    js = balance.jd2balance("jd", out, chroms={"chr1"}, res=100, ignore_diags=2, min_nnz=1, max_iters=50)
    st = js["chroms"]["chr1"]
    assert (st["iters"], st["converged"], st["n_used"]) == (50, False, 4) and abs(st["var"] - 0.0726643) < 1e-6
    js = balance.jd2balance("jd", out, chroms={"chr1"}, res=100, ignore_diags=5, min_nnz=0)
    st = js["chroms"]["chr1"]
    assert (st["iters"], st["converged"], st["var"], st["scale"], st["n_valid"]) == (0, False, None, None, 0)
    assert "null" in _read(out, ["_balance.json"])["_balance.json"]
    assert all(line.endswith("\t0\t0\tnan") for line in _read(out, ["_balance.txt"])["_balance.txt"].splitlines())


def test_formats_and_region_weights():
    assert balance.fmt(float("nan")) == "nan" and balance.fmt(0.0) == "0" and balance.fmt(1.0 / 3) == "0.3333333333"
    assert balance.fmt(12345678901.5) == "1.23456789e+10" and balance.fmt(2.5e-7) == "2.5e-07"
    w = balance.weights_over(3, np.array([1.0, 2.0, 3.0]), 1, 7)              # bins 1 .. 7 against weights of the bins 3 .. 5
    assert np.array_equal(w, [np.nan, np.nan, 1.0, 2.0, 3.0, np.nan, np.nan], equal_nan=True)
    assert np.isnan(balance.weights_over(3, np.array([1.0]), 10, 2)).all() and np.isnan(balance.weights_over(0, np.zeros(0), 0, 2)).all()
    assert np.array_equal(balance.weights_over(-2, np.array([5.0, 6.0, 7.0]), -1, 2), [6.0, 7.0])
    t = balance.format_balanced_matrix("c", 10, -1, 4, np.array([[np.nan, 0.25]]))
    assert t == "\tc:40-50\tc:50-60\nc:-10-0\tnan\t0.25\n"
    assert balance.format_bins("c", 10, -1, [3], [2], [np.nan]) == "c\t-10\t0\t3\t2\tnan\n"


def test_a_region_beyond_the_bins_is_nan(standin, tmp_path):
    out = os.path.join(str(tmp_path), "n")
    balance.jd2balance("jd", out, chroms={"chr1"}, region="chr1:400-700", **ARGS)
    rows = _read(out, balance.SUFFIXES[3:])["_balanced_matrix.txt"].splitlines()
    assert rows[0] == "\tchr1:400-500\tchr1:500-600\tchr1:600-700"
    assert rows[1].split("\t")[2:] == ["nan", "nan"] and rows[2].split("\t")[1:] == ["nan"] * 3 and rows[1].split("\t")[1] == "0"


# ---- refusals and the command line -------------------------------------------------------------------------------------
def test_nothing_is_written_when_an_argument_is_refused(standin, tmp_path):
    out = os.path.join(str(tmp_path), "r")
    J = balance.jd2balance
    bad = [lambda: J("jd", out, res=0), lambda: J("jd", out, res="x"), lambda: J("jd", out, res=1 << 29), lambda: J("jd", out, ignore_diags=-1),
           lambda: J("jd", out, min_nnz=-1), lambda: J("jd", out, min_count=-3), lambda: J("jd", out, mad_max=-0.5),
           lambda: J("jd", out, mad_max=float("nan")), lambda: J("jd", out, tol=-1e-9), lambda: J("jd", out, tol=float("nan")),
           lambda: J("jd", out, max_iters=-1), lambda: J("jd", out, max_iters="many"), lambda: J("jd", out, region="chr1:500-0"),
           lambda: J("jd", out, region="chr1"), lambda: J("jd", out, region="chr9:0-500"),
           lambda: J("jd", out, chroms={"chr2"}, region="chr1:0-500"),                   # the region's chromosome is not balanced
           lambda: J("jd", out, region="chr1:0-100000", res=10)]                          # 10 000 bins a side
    for f in bad:
        with pytest.raises(ValueError):
            f()
    assert os.listdir(str(tmp_path)) == []
    assert all(r.chrom.calls == [] for r in standin.values())                # ... and before any work on a chromosome


def test_a_missing_directory_is_refused(tmp_path):
    with pytest.raises(ValueError):
        balance.jd2balance("/nonexistent/jd", os.path.join(str(tmp_path), "x"))
    assert os.listdir(str(tmp_path)) == []


def test_help_defaults_and_overrides():
    op = balance.help(["-d", "jd", "-o", "out"])
    assert (op.d, op.output, op.res, op.cut, op.chroms, op.ignorediags, op.minnnz, op.mincount, op.mad, op.tol, op.maxiters, op.region) == \
        ("jd", "out", 10000, 0, "", 2, 10, 0, 5.0, 1e-5, 200, None)
    op = balance.help(["-d", "jd", "-o", "out", "-res", "2500", "-cut", "3", "-c", "chr1,chr2", "-ignorediags", "1", "-minnnz", "4", "-mincount",
                       "7", "-mad", "2.5", "-tol", "1e-8", "-maxiters", "500", "-r", "chr1:0-100000"])
    assert (op.res, op.cut, op.chroms, op.ignorediags, op.minnnz, op.mincount, op.mad, op.tol, op.maxiters, op.region) == \
        (2500, 3, "chr1,chr2", 1, 4, 7, 2.5, 1e-8, 500, "chr1:0-100000")
    for bad in ([], ["-d", "jd"], ["-o", "out"], ["-d", "jd", "-o", "out", "-res", "x"], ["-d", "jd", "-o", "out", "-tol", "small"],
                ["cells", "-d", "jd", "-o", "out"]):
        with pytest.raises(SystemExit):
            balance.help(bad)


def test_main_writes_the_files(standin, tmp_path):
    out = os.path.join(str(tmp_path), "m")
    assert balance.main(["-d", "jd", "-o", out, "-res", "100", "-c", "chr1", "-ignorediags", "0", "-minnnz", "1", "-r", "chr1:100-400"]) == 0
    got = _read(out, balance.SUFFIXES)
    assert (got["_balance.txt"], got["_balanced_cells.txt"], got["_balanced_matrix.txt"]) == (BINS_TXT, CELLS_TXT, MATRIX_TXT)


def test_suffixes_are_its_own():
    assert balance.SUFFIXES == ("_balance.txt", "_balanced_cells.txt", "_balance.json", "_balanced_matrix.txt")
    assert set(balance.SUFFIXES).isdisjoint(matrix.SUFFIXES)
    assert matrix.SUFFIXES == ("_matrix.txt", "_matrix.json", "_cells.txt", "_cells.json", "_v4c.bedGraph", "_v4c.json")


def test_the_stand_in_keeps_the_order_of_calls():
    ch = BC.OracleChrom(*MC.twelve())
    with pytest.raises(RuntimeError):
        ch.bal_marginals(2)                                                  # no cells
    ch.mat_cells(100, fold=False)
    with pytest.raises(RuntimeError):
        ch.bal_marginals(2)                                                  # not folded
    ch.mat_cells(100, fold=True)
    with pytest.raises(RuntimeError):
        ch.bal_iterate(np.ones(5, bool))
    assert ch.bal_marginals(2) == (0, 5, 4)
    with pytest.raises(RuntimeError):
        ch.bal_weights()
    with pytest.raises(ValueError):
        ch.bal_iterate(np.ones(4, bool))
    assert ch.bal_iterate(np.ones(5, bool), max_iters=3)[:2] == (3, False) and len(ch.bal_weights()) == 5 and len(ch.bal_cells_get(2, 3)) == 3
    ch.mat_cells(100, fold=True)
    with pytest.raises(RuntimeError):
        ch.bal_marginals_get()


# ---- the walk down the device state, the options and the clean-up that the four commands share --------------------------------
def test_the_calls_on_the_device_and_no_more():
    ch = MC.Recording(BC.OracleChrom(*MC.twelve()))
    balance.balance_chrom(ch, "chr1", 100, ignore_diags=2, min_nnz=1)
    assert ch.log == [("mat_cells", (100,), {"cut": 0, "fold": True}), ("bal_marginals", (2,), {}), ("bal_marginals_get", (0, 5), {}),
                      ("bal_iterate", ("b[5]",), {"max_iters": 200, "tol": 1e-5}), ("bal_weights", (0, 5), {}),
                      ("mat_cells_get", (0, 10), {}), ("bal_cells_get", (0, 10), {}), ("mat_free", (), {})]
    ch = MC.Recording(BC.OracleChrom(*MC.twelve()))
    balance.balance_chrom(ch, "chr1", 100, ignore_diags=2, min_nnz=1, chunk=7, region=("chr1", 100, 400))
    assert ch.log[5:] == [("mat_cells_get", (0, 7), {}), ("bal_cells_get", (0, 7), {}), ("mat_cells_get", (7, 3), {}), ("bal_cells_get", (7, 3), {}),
                          ("mat_window", (100, 1, 1, 3, 3), {"cut": 0, "mirror": True}), ("mat_free", (), {})]


def test_main_hands_every_option_on(standin, tmp_path):
    out = os.path.join(str(tmp_path), "o")
    kw = dict(res=100, cut=20, ignore_diags=1, min_nnz=1, min_count=1, mad_max=2.5, tol=1e-8, max_iters=30, region="chr1:100-400")
    js = balance.jd2balance("jd", out + "k", chroms={"chr1", "chr2"}, **kw)
    assert js["args"] == kw
    assert balance.main(["-d", "jd", "-o", out + "m", "-res", "100", "-cut", "20", "-c", "chr1,chr2", "-ignorediags", "1", "-minnnz", "1",
                         "-mincount", "1", "-mad", "2.5", "-tol", "1e-8", "-maxiters", "30", "-r", "chr1:100-400"]) == 0
    assert _read(out + "m", balance.SUFFIXES) == _read(out + "k", balance.SUFFIXES)
    assert balance.check_args(**{k: kw[k] for k in balance.BalanceArgs._fields})._asdict() == {k: kw[k] for k in balance.BalanceArgs._fields}


@pytest.mark.parametrize("step", ["bal_marginals", "bal_iterate", "bal_weights", "mat_cells_get", "mat_window"])
def test_a_failing_step_frees_the_cells_once_and_writes_nothing(step, standin, tmp_path):
    standin["chr1"].chrom = ch = MC.Recording(standin["chr1"].chrom, fail=step)
    with pytest.raises(RuntimeError):
        balance.jd2balance("jd", os.path.join(str(tmp_path), "f"), region="chr1:100-400", **ARGS)
    assert [c[0] for c in ch.log].count("mat_free") == 1 and ch.log[-1][0] == "mat_free" and ch.log[-2][0] == step
    assert os.listdir(str(tmp_path)) == [] and standin["chr2"].chrom.calls == []
