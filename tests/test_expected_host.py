"""CPU: the oracle of K26 on the hand-written rows and on a planted case, the smoothing's group edges, the host side of
cloops_amd.expected -- the five texts byte for byte through the oracle's stand-in chromosome, the command line, and that a refused
argument writes nothing."""
import json
import os
import threading

import numpy as np
import pytest

import balance_cases as BC
import expected_cases as EC
import matrix_cases as MC
from cloops_amd import balance, expected, matrix


class Record(object):
    def __init__(self, X, Y):
        self.chrom, self.lock = EC.OracleChrom(X, Y), threading.Lock()


@pytest.fixture
def standin(monkeypatch):
    """matrix._records (which expected reads) served by stand-in chromosomes: chr1 = the twelve rows, chr2 = 300 scattered ones"""
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
def test_oracle_on_the_twelve_rows():
    bx, by, cnt, _ = MC.cells_oracle(*MC.twelve(), 0, 100, True)
    one = np.ones(5)
    # cells: (0,0,1) (0,1,1) (0,4,2) (1,1,1) (1,3,2) (1,4,1) (2,2,1) (2,4,1) (3,3,1) (3,4,1)
    p, c, v, nu = EC.diagonals_oracle(bx, by, cnt, 0, 5, 0, np.ones(5, bool), one)
    assert (p.tolist(), c.tolist(), v.tolist(), nu) == ([5, 4, 3, 2, 1], [4, 2, 3, 1, 2], [4.0, 2.0, 3.0, 1.0, 2.0], 10)
    assert (p.dtype, c.dtype, v.dtype) == (np.int64, np.uint64, np.float64)
    p, c, v, nu = EC.diagonals_oracle(bx, by, cnt, 0, 5, 2, np.ones(5, bool), one)
    assert (p.tolist(), c.tolist(), v.tolist(), nu) == ([0, 0, 3, 2, 1], [0, 0, 3, 1, 2], [0.0, 0.0, 3.0, 1.0, 2.0], 4)
    masked = np.array([1, 1, 0, 1, 1], bool)                                 # bin 2 out: its three cells and four of the pairs go
    p, c, v, nu = EC.diagonals_oracle(bx, by, cnt, 0, 5, 0, masked, one)
    assert (p.tolist(), c.tolist(), nu) == ([4, 2, 1, 2, 1], [3, 2, 2, 1, 2], 8)
    p, c, v, nu = EC.diagonals_oracle(bx, by, cnt, 0, 5, 7, masked, one)      # ignore_diags above nb
    assert not p.any() and not c.any() and nu == 0
    # weights: (w[bx] cnt) w[by]; a weight on a masked bin is never read
    w = np.array([2.0, 0.5, np.nan, 1.0, 4.0])
    p, c, v, nu = EC.diagonals_oracle(bx, by, cnt, 0, 5, 2, masked, w)
    assert v.tolist() == [0.0, 0.0, 0.5 * 2 * 1.0, 0.5 * 1 * 4.0, 2.0 * 2 * 4.0] and c.tolist() == [0, 0, 2, 1, 2]
    e = np.array([1.0, 1.0, 0.5, 0.0, np.nan])
    oe = EC.oe_oracle(bx, by, cnt, 0, 5, 2, masked, w, e)
    assert np.array_equal(oe, [np.nan, np.nan, np.nan, np.nan, 2.0, np.nan, np.nan, np.nan, np.nan, np.nan], equal_nan=True)
    oe = EC.oe_oracle(bx, by, cnt, 0, 5, 0, masked, w, np.full(5, 2.0))
    assert np.array_equal(oe, [2.0, 0.5, 8.0, 0.125, 0.5, 1.0, np.nan, np.nan, 0.5, 2.0], equal_nan=True)
    # the pairs: the correlation against the definition's loop, and an empty input
    rng = np.random.default_rng(3)
    for nb in (1, 2, 5, 64, 65, 130):
        for ign in (0, 2, nb + 1):
            m = rng.random(nb) < 0.6
            assert np.array_equal(EC.pairs_oracle(m, ign), EC.pairs_by_loop(m, ign))
        assert EC.pairs_oracle(np.ones(nb, bool), 0).tolist() == list(range(nb, 0, -1))
    z = np.zeros(0, np.int32)
    p, c, v, nu = EC.diagonals_oracle(z, z, z, 0, 0, 2, np.zeros(0, bool), np.zeros(0))
    assert len(p) == len(c) == len(v) == 0 and nu == 0


def test_oracle_on_a_planted_circulant():
    """A = d_i d_j M, M a symmetric circulant: the balanced matrix is a multiple of M, so value_avg[d] = K M[0][d] for one K"""
    bx, by, cnt, dd = BC.planted()
    n = 24
    o = BC.ice_oracle(bx, by, cnt, 0, np.ones(n, bool), 200, 1e-12)
    assert o["converged"]
    p, c, v, nu = EC.diagonals_oracle(bx, by, cnt, 0, n, 0, np.ones(n, bool), o["weight"])
    assert p.tolist() == list(range(n, 0, -1)) and nu == n * (n + 1) // 2
    first = bx == 0
    row = cnt[first].astype(np.float64) / (dd[0] * dd[by[first]])             # M[0][k]
    k = (v / p) / row
    assert np.ptp(k) / k.mean() < 4 * np.sqrt(n * 1e-12)                     # (weight d is constant within sqrt(nb tol): BC's planted test)
    # another order of the cells moves the sums within their bound, and the integers not at all
    q = EC.diagonals_oracle(bx, by, cnt, 0, n, 0, np.ones(n, bool), o["weight"], perm=BC.cell_perm(len(bx), 1))
    bound, L = EC.sum_bound(bx, by, 0, n, 0, np.ones(n, bool))
    assert L.tolist() == p.tolist() and np.array_equal(q[1], c) and (np.abs(q[2] - v) <= bound * v).all()
    # O/E over the per-diagonal average: M is constant along a diagonal, so every O/E is 1 within the convergence
    oe = EC.oe_oracle(bx, by, cnt, 0, n, 0, np.ones(n, bool), o["weight"], v / p)
    assert np.abs(oe - 1).max() < 1e-4


# ---- the smoothing ---------------------------------------------------------------------------------------------------
def test_group_edges():
    P1 = [0, 1, 10, 100, 1000, 10000]
    P3 = [0, 1, 3, 5, 10, 22, 47, 100, 216, 465, 1000, 2155, 4642, 10000]
    P10 = [0, 1, 2, 3, 4, 6, 7, 8, 10, 13, 16, 20, 26, 32, 40, 51, 64, 80, 100, 126, 159, 200, 252, 317, 399, 502, 631, 795, 1000]
    for P, edges, nd in ((1, P1, 10001), (3, P3, 10001), (10, P10, 1001)):
        got = expected.group_bounds(nd, P).tolist()
        assert got == edges + [nd] == EC.edges_oracle(nd, P)
        assert all(a < b for a, b in zip(got, got[1:]))                       # strictly increasing: no duplicate
        for e in edges[2:]:                                                   # nd below, at and one past an edge
            assert expected.group_bounds(e - 1, P).tolist() == [x for x in edges if x < e - 1] + [e - 1]
            assert expected.group_bounds(e, P).tolist() == [x for x in edges if x < e] + [e]
            assert expected.group_bounds(e + 1, P).tolist() == [x for x in edges if x <= e] + [e + 1]
    for P in (1, 2, 3, 7, 10, 25):
        for nd in (0, 1, 2, 3, 11, 99, 100, 101, 3000):
            assert expected.group_bounds(nd, P).tolist() == EC.edges_oracle(nd, P), (P, nd)
    assert expected.group_bounds(0, 10).tolist() == [0] and expected.group_bounds(1, 10).tolist() == [0, 1]
    assert expected.group_bounds(2, 1).tolist() == [0, 1, 2]                  # diagonal 0 is a group of its own
    for bad in (0, -1, 2.5, "x", None, True):
        with pytest.raises(ValueError):
            expected.group_bounds(100, bad)


def test_smoothing_against_the_loops():
    rng = np.random.default_rng(0)
    for nd, P in ((300, 10), (300, 1), (57, 3), (1, 10), (0, 10), (2, 4)):
        p = rng.integers(0, 50, nd)
        p[:2] = 0
        if nd > 40:
            p[30:40] = 0                                                     # a whole group without pairs (P = 10: [32, 40))
        v = rng.random(nd) * p
        sm, groups = expected.smooth(p, v, P)
        want, wg = EC.smooth_oracle(p, v, P)
        assert len(sm) == nd and np.array_equal(np.isnan(sm), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.allclose(sm[ok], want[ok], rtol=1e-13, atol=0)
        assert [g[:3] for g in groups] == [g[:3] for g in wg] and np.allclose([g[3] for g in groups], [g[3] for g in wg], rtol=1e-13, atol=0)
        assert all((np.isnan(g[4]) and g[2] == 0) or g[4] == g[3] / g[2] for g in groups)
    p, v = np.array([0, 0, 4, 2, 0, 6]), np.array([0.0, 0.0, 2.0, 3.0, 0.0, 3.0])
    sm, groups = expected.smooth(p, v, 1)                                    # groups [0, 1) and [1, 6)
    assert np.array_equal(sm, [np.nan] + [8.0 / 12] * 5, equal_nan=True) and groups[1] == (1, 6, 12, 8.0, 8.0 / 12)
    e, _ = expected.expected_of(p, v, 2, 1)
    assert np.array_equal(e, [np.nan, np.nan] + [8.0 / 12] * 4, equal_nan=True)          # NaN below ignore_diags
    e, _ = expected.expected_of(p, v, 2, 1, nosmooth=True)
    assert np.array_equal(e, [np.nan, np.nan, 0.5, 1.5, np.nan, 0.5], equal_nan=True)


# ---- the texts -------------------------------------------------------------------------------------------------------
EXPECTED_TXT = ("chr1\t0\t0\t5\t4\t1.582033115\t0.316406623\t0.316406623\nchr1\t1\t100\t4\t2\t0.433614116\t0.108403529\t0.108403529\n"
                "chr1\t2\t200\t3\t3\t0.7468908977\t0.2489636326\t0.2489636326\nchr1\t3\t300\t2\t1\t0.1318709331\t0.06593546655\t0.06593546655\n"
                "chr1\t4\t400\t1\t2\t0.3966207659\t0.3966207659\t0.3966207659\n")
PS_TXT = ("chr1\t0\t100\t5\t1.582033115\t0.316406623\nchr1\t100\t200\t4\t0.433614116\t0.108403529\nchr1\t200\t300\t3\t0.7468908977\t0.2489636326\n"
          "chr1\t300\t400\t2\t0.1318709331\t0.06593546655\nchr1\t400\t500\t1\t0.3966207659\t0.3966207659\n")
CELLS_TXT = ("chr1\t0\t100\tchr1\t0\t100\t1\t0.3628185459\t1.146684423\nchr1\t0\t100\tchr1\t100\t200\t1\t0.2412643225\t2.225613176\n"
             "chr1\t0\t100\tchr1\t400\t500\t2\t0.3966207659\t1\nchr1\t100\t200\tchr1\t100\t200\t1\t0.1604341177\t0.5070504411\n"
             "chr1\t100\t200\tchr1\t300\t400\t2\t0.468025344\t1.879894421\nchr1\t100\t200\tchr1\t400\t500\t1\t0.1318709331\t2\n"
             "chr1\t200\t300\tchr1\t200\t300\t1\t0.7174445096\t2.267476271\nchr1\t200\t300\tchr1\t400\t500\t1\t0.2788655537\t1.120105579\n"
             "chr1\t300\t400\tchr1\t300\t400\t1\t0.3413359417\t1.078788865\nchr1\t300\t400\tchr1\t400\t500\t1\t0.1923497935\t1.774386824\n")
MATRIX_TXT = ("\tchr1:100-200\tchr1:200-300\tchr1:300-400\nchr1:100-200\t0.5070504411\t0\t1.879894421\n"
              "chr1:200-300\t0\t2.267476271\t0\nchr1:300-400\t1.879894421\t0\t1.078788865\n")
# -raw -perdecade 1: the groups are diagonal 0 (4 / 5) and the diagonals 1 .. 4 (8 contacts over 10 pairs)
RAW_EXPECTED_TXT = ("chr1\t0\t0\t5\t4\t4\t0.8\t0.8\nchr1\t1\t100\t4\t2\t2\t0.5\t0.8\nchr1\t2\t200\t3\t3\t3\t1\t0.8\n"
                    "chr1\t3\t300\t2\t1\t1\t0.5\t0.8\nchr1\t4\t400\t1\t2\t2\t2\t0.8\n")
RAW_PS_TXT = "chr1\t0\t100\t5\t4\t0.8\nchr1\t100\t500\t10\t8\t0.8\n"
RAW_CELLS_TXT = "".join("chr1\t%d\t%d\tchr1\t%d\t%d\t%d\t%d\t%s\n" % (x * 100, x * 100 + 100, y * 100, y * 100 + 100, c, c, "2.5" if c == 2 else "1.25")
                        for x, y, c in ((0, 0, 1), (0, 1, 1), (0, 4, 2), (1, 1, 1), (1, 3, 2), (1, 4, 1), (2, 2, 1), (2, 4, 1), (3, 3, 1), (3, 4, 1)))
RAW_MATRIX_TXT = "\tchr1:100-200\tchr1:200-300\tchr1:300-400\nchr1:100-200\t1.25\t0\t2.5\nchr1:200-300\t0\t1.25\t0\nchr1:300-400\t2.5\t0\t1.25\n"
ARGS = dict(res=100, ignore_diags=0, min_nnz=1)


def test_the_five_texts(standin, tmp_path):
    out = os.path.join(str(tmp_path), "e")
    js = expected.jd2expected("jd", out, chroms={"chr1"}, region="chr1:100-400", **ARGS)
    got = _read(out, expected.SUFFIXES)
    assert (got["_expected.txt"], got["_ps.txt"], got["_oe_cells.txt"], got["_oe_matrix.txt"]) == (EXPECTED_TXT, PS_TXT, CELLS_TXT, MATRIX_TXT)
    st = js["chroms"]["chr1"]
    assert {k: st[k] for k in ("b0", "nb", "nd", "n_used", "n_valid", "iters", "converged")} == \
        {"b0": 0, "nb": 5, "nd": 5, "n_used": 10, "n_valid": 5, "iters": 16, "converged": True}
    assert abs(st["var"] - 7.1631827641550376e-06) < 1e-15 and abs(st["scale"] - 4.352666867779687) < 1e-9
    assert js["args"] == {"res": 100, "cut": 0, "raw": False, "per_decade": 10, "nosmooth": False, "ignore_diags": 0, "min_nnz": 1, "min_count": 0,
                          "mad_max": 5.0, "tol": 1e-5, "max_iters": 200, "region": "chr1:100-400"}
    assert got["_expected.json"] == json.dumps(js, indent=1, sort_keys=True) + "\n" and json.loads(got["_expected.json"]) == js
    assert sorted(os.listdir(str(tmp_path))) == sorted("e" + s for s in expected.SUFFIXES)
    ch = standin["chr1"].chrom
    assert ch.cells is None and ch.bal is None and ch.exp is None             # freed
    # the value column is balance's own
    balance.jd2balance("jd", out, chroms={"chr1"}, **ARGS)
    with open(out + "_balanced_cells.txt") as fh:
        assert fh.read().splitlines() == ["\t".join(line.split("\t")[:8]) for line in got["_oe_cells.txt"].splitlines()]


def test_the_raw_texts(standin, tmp_path):
    out = os.path.join(str(tmp_path), "r")
    js = expected.jd2expected("jd", out, chroms={"chr1"}, region="chr1:100-400", raw=True, per_decade=1, **ARGS)
    got = _read(out, expected.SUFFIXES)
    assert (got["_expected.txt"], got["_ps.txt"], got["_oe_cells.txt"], got["_oe_matrix.txt"]) == \
        (RAW_EXPECTED_TXT, RAW_PS_TXT, RAW_CELLS_TXT, RAW_MATRIX_TXT)
    st = js["chroms"]["chr1"]
    assert (st["iters"], st["converged"], st["var"], st["scale"], st["n_used"], st["n_valid"]) == (0, False, None, None, 10, 5)
    # -nosmooth: every diagonal over its own average
    js = expected.jd2expected("jd", out, chroms={"chr1"}, raw=True, nosmooth=True, **ARGS)
    got = _read(out, expected.SUFFIXES[:4])
    assert [line.split("\t")[6:] for line in got["_expected.txt"].splitlines()] == [[a, a] for a in ("0.8", "0.5", "1", "0.5", "2")]
    assert [line.split("\t")[8] for line in got["_oe_cells.txt"].splitlines()] == ["1.25", "2", "1", "1.25", "2", "2", "1.25", "1", "1.25", "2"]


def test_chromosomes_in_name_order_chunks_and_nan(standin, tmp_path):
    out = os.path.join(str(tmp_path), "c")
    js = expected.jd2expected("jd", out, **ARGS)
    got = _read(out, expected.SUFFIXES[:4])
    assert not os.path.exists(out + expected.SUFFIXES[4])                    # no region: four files
    names = [line.split("\t")[0] for line in got["_expected.txt"].splitlines()]
    assert names == sorted(names) and set(names) == {"chr1", "chr2"} and sorted(js["chroms"]) == ["chr1", "chr2"]
    assert got["_expected.txt"].startswith(EXPECTED_TXT) and got["_oe_cells.txt"].startswith(CELLS_TXT) and got["_ps.txt"].startswith(PS_TXT)
    assert all(len(line.split("\t")) == 9 for line in got["_oe_cells.txt"].splitlines())
    assert all(len(line.split("\t")) == 8 and int(line.split("\t")[3]) > 0 for line in got["_expected.txt"].splitlines())
    # the seven bg2 columns are those of matrix.jd2cells
    matrix.jd2cells("jd", out, res=100)
    with open(out + "_cells.txt") as fh:
        assert fh.read().splitlines() == ["\t".join(line.split("\t")[:7]) for line in got["_oe_cells.txt"].splitlines()]
    ch = standin["chr2"].chrom
    whole = expected.expected_chrom(ch, "chr2", 250, ignore_diags=1, min_nnz=2)
    assert expected.expected_chrom(ch, "chr2", 250, ignore_diags=1, min_nnz=2, chunk=7) == whole and whole["cells"].count("\n") > 7
    assert "\tnan\n" in whole["cells"] and "\tnan\tnan\n" in whole["cells"] and whole["stats"]["n_valid"] < whole["stats"]["nb"]
    assert "\tnan\t" not in whole["expected"] and "\t0\t0\tnan\n" in whole["ps"]        # the group of diagonal 0 has no pairs
    lines = whole["cells"].splitlines()
    assert all(line.endswith("\tnan") for line in lines if line.split("\t")[1] == line.split("\t")[4])   # the diagonal is ignored
    # nothing used: every O/E is NaN, no diagonal has pairs
    js = expected.jd2expected("jd", out, chroms={"chr1"}, res=100, ignore_diags=5, min_nnz=0)
    st = js["chroms"]["chr1"]
    assert (st["iters"], st["n_used"], st["n_valid"], st["nd"]) == (0, 0, 0, 5)
    got = _read(out, expected.SUFFIXES[:3])
    assert got["_expected.txt"] == "" and all(line.endswith("\tnan\tnan") for line in got["_oe_cells.txt"].splitlines())


def test_formats_and_the_region_matrix():
    e = np.array([np.nan, 2.0, 0.0])
    m = expected.oe_matrix(np.array([[4, 2, 6], [2, 0, 8], [6, 8, 2]]), np.array([1.0, 0.5, np.nan]), e)
    assert np.array_equal(m, [[np.nan, 0.5, np.nan], [0.5, np.nan, np.nan], [np.nan, np.nan, np.nan]], equal_nan=True)
    m = expected.oe_matrix(np.ones((2, 2)), np.ones(2), np.array([4.0]))                            # |i - j| beyond the diagonals
    assert np.array_equal(m, [[0.25, np.nan], [np.nan, 0.25]], equal_nan=True)
    assert expected.format_expected("c", 10, [0, 3], [0, 7], [0.0, 1.5], [np.nan, 0.25]) == "c\t1\t10\t3\t7\t1.5\t0.5\t0.25\n"
    assert expected.format_ps("c", 10, [(0, 1, 0, 0.0, float("nan")), (1, 4, 6, 3.0, 0.5)]) == "c\t0\t10\t0\t0\tnan\nc\t10\t40\t6\t3\t0.5\n"
    assert expected.format_cells("c", 10, [-1], [4], [3], [np.nan], [0.125]) == "c\t-10\t0\tc\t40\t50\t3\tnan\t0.125\n"
    assert np.array_equal(expected.raw_values([3, 4], [4, 5], [2, 7], 3, [1.0, 1.0, np.nan]), [2.0, np.nan], equal_nan=True)


# ---- refusals and the command line -------------------------------------------------------------------------------------
def test_nothing_is_written_when_an_argument_is_refused(standin, tmp_path):
    out = os.path.join(str(tmp_path), "r")
    J = expected.jd2expected
    bad = [lambda: J("jd", out, res=0), lambda: J("jd", out, res="x"), lambda: J("jd", out, ignore_diags=-1), lambda: J("jd", out, min_nnz=-1),
           lambda: J("jd", out, mad_max=float("nan")), lambda: J("jd", out, tol=-1e-9), lambda: J("jd", out, max_iters=-1),
           lambda: J("jd", out, per_decade=0), lambda: J("jd", out, per_decade=-3), lambda: J("jd", out, per_decade=2.5),
           lambda: J("jd", out, per_decade="ten"), lambda: J("jd", out, per_decade=None),
           lambda: J("jd", out, region="chr1:500-0"), lambda: J("jd", out, region="chr9:0-500"),
           lambda: J("jd", out, chroms={"chr2"}, region="chr1:0-500"), lambda: J("jd", out, region="chr1:0-100000", res=10)]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    assert os.listdir(str(tmp_path)) == []
    assert all(r.chrom.calls == [] for r in standin.values())                # ... and before any work on a chromosome


def test_a_missing_directory_is_refused(tmp_path):
    with pytest.raises(ValueError):
        expected.jd2expected("/nonexistent/jd", os.path.join(str(tmp_path), "x"))
    assert os.listdir(str(tmp_path)) == []


def test_help_defaults_and_overrides():
    op = expected.help(["-d", "jd", "-o", "out"])
    assert (op.d, op.output, op.res, op.cut, op.chroms, op.raw, op.perdecade, op.nosmooth, op.region, op.ignorediags, op.minnnz, op.mincount, op.mad,
            op.tol, op.maxiters) == ("jd", "out", 10000, 0, "", False, 10, False, None, 2, 10, 0, 5.0, 1e-5, 200)
    op = expected.help(["-d", "jd", "-o", "out", "-res", "2500", "-cut", "3", "-c", "chr1,chr2", "-raw", "-perdecade", "4", "-nosmooth", "-r",
                        "chr1:0-100000", "-ignorediags", "1", "-minnnz", "4", "-mincount", "7", "-mad", "2.5", "-tol", "1e-8", "-maxiters", "500"])
    assert (op.res, op.cut, op.chroms, op.raw, op.perdecade, op.nosmooth, op.region, op.ignorediags, op.minnnz, op.mincount, op.mad, op.tol,
            op.maxiters) == (2500, 3, "chr1,chr2", True, 4, True, "chr1:0-100000", 1, 4, 7, 2.5, 1e-8, 500)
    for bad in ([], ["-d", "jd"], ["-o", "out"], ["-d", "jd", "-o", "out", "-res", "x"], ["-d", "jd", "-o", "out", "-perdecade", "2.5"],
                ["-d", "jd", "-o", "out", "-raw", "1"]):
        with pytest.raises(SystemExit):
            expected.help(bad)


def test_main_writes_the_files(standin, tmp_path):
    out = os.path.join(str(tmp_path), "m")
    assert expected.main(["-d", "jd", "-o", out, "-res", "100", "-c", "chr1", "-ignorediags", "0", "-minnnz", "1", "-r", "chr1:100-400"]) == 0
    got = _read(out, expected.SUFFIXES)
    assert (got["_expected.txt"], got["_ps.txt"], got["_oe_cells.txt"], got["_oe_matrix.txt"]) == (EXPECTED_TXT, PS_TXT, CELLS_TXT, MATRIX_TXT)
    assert expected.main(["-d", "jd", "-o", out, "-res", "100", "-c", "chr1", "-ignorediags", "0", "-minnnz", "1", "-raw", "-perdecade", "1"]) == 0
    assert _read(out, expected.SUFFIXES[:1])["_expected.txt"] == RAW_EXPECTED_TXT
    with pytest.raises(ValueError):
        expected.main(["-d", "jd", "-o", os.path.join(str(tmp_path), "z"), "-perdecade", "0"])
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("z")]


def test_suffixes_are_its_own():
    assert expected.SUFFIXES == ("_expected.txt", "_ps.txt", "_oe_cells.txt", "_expected.json", "_oe_matrix.txt")
    assert set(expected.SUFFIXES).isdisjoint(matrix.SUFFIXES) and set(expected.SUFFIXES).isdisjoint(balance.SUFFIXES)
    assert len(set(expected.SUFFIXES)) == 5


def test_the_stand_in_keeps_the_order_of_calls():
    ch = EC.OracleChrom(*MC.twelve())
    ch.mat_cells(100, fold=True)
    with pytest.raises(RuntimeError):
        ch.exp_diagonals(balanced=False)                                     # no marginals
    assert ch.bal_marginals(2) == (0, 5, 4)
    with pytest.raises(RuntimeError):
        ch.exp_diagonals()                                                   # balanced before bal_iterate
    with pytest.raises(RuntimeError):
        ch.exp_diagonals_get()
    assert ch.exp_diagonals(balanced=False) == (5, 4)
    with pytest.raises(RuntimeError):
        ch.exp_cells_get()                                                   # before exp_set
    with pytest.raises(RuntimeError):
        ch.exp_set(np.ones(4))
    ch.exp_set(np.ones(5))
    assert len(ch.exp_cells_get(2, 3)) == 3 and [len(a) for a in ch.exp_diagonals_get(1, 2)] == [2, 2, 2]
    ch.bal_iterate(np.ones(5, bool), max_iters=3)
    with pytest.raises(RuntimeError):
        ch.exp_diagonals_get()                                               # dropped with the earlier weights
    with pytest.raises(RuntimeError):
        ch.exp_diagonals(valid=np.ones(5, bool))                             # the balanced mode takes no mask
    assert ch.exp_diagonals() == (5, 4)
    for drop in (ch.exp_free, ch.bal_free, lambda: ch.mat_cells(100, fold=True)):
        drop()
        with pytest.raises(RuntimeError):
            ch.exp_diagonals_get()


# ---- the walk down the device state, the options and the clean-up that the commands share -------------------------------------
CELLS = ("mat_cells", (100,), {"cut": 0, "fold": True})
MARGINALS = [("bal_marginals", (2,), {}), ("bal_marginals_get", (0, 5), {})]
ITERATE = ("bal_iterate", ("b[5]",), {"max_iters": 200, "tol": 1e-5})
DIAGONALS = [("exp_diagonals_get", (0, 5), {}), ("exp_set", ("f[5]",), {})]


def test_the_calls_on_the_device_and_no_more():
    ch = MC.Recording(EC.OracleChrom(*MC.twelve()))
    expected.expected_chrom(ch, "chr1", 100, ignore_diags=2, min_nnz=1)
    assert ch.log == [CELLS] + MARGINALS + [ITERATE, ("bal_weights", (0, 5), {}), ("exp_diagonals", (), {})] + DIAGONALS + \
        [("mat_cells_get", (0, 10), {}), ("bal_cells_get", (0, 10), {}), ("exp_cells_get", (0, 10), {}), ("mat_free", (), {})]
    ch = MC.Recording(EC.OracleChrom(*MC.twelve()))
    expected.expected_chrom(ch, "chr1", 100, ignore_diags=2, min_nnz=1, raw=True, chunk=7, region=("chr1", 100, 400))
    assert ch.log == [CELLS] + MARGINALS + [("exp_diagonals", (), {"valid": "b[5]", "balanced": False})] + DIAGONALS + \
        [("mat_cells_get", (0, 7), {}), ("exp_cells_get", (0, 7), {}), ("mat_cells_get", (7, 3), {}), ("exp_cells_get", (7, 3), {}),
         ("mat_window", (100, 1, 1, 3, 3), {"cut": 0, "mirror": True}), ("mat_free", (), {})]


def test_main_hands_every_option_on(standin, tmp_path):
    out = os.path.join(str(tmp_path), "o")
    kw = dict(res=100, cut=20, raw=True, per_decade=4, nosmooth=True, ignore_diags=1, min_nnz=1, min_count=1, mad_max=2.5, tol=1e-8, max_iters=30,
              region="chr1:100-400")
    js = expected.jd2expected("jd", out + "k", chroms={"chr1", "chr2"}, **kw)
    assert js["args"] == kw
    assert expected.main(["-d", "jd", "-o", out + "m", "-res", "100", "-cut", "20", "-c", "chr1,chr2", "-raw", "-perdecade", "4", "-nosmooth",
                          "-ignorediags", "1", "-minnnz", "1", "-mincount", "1", "-mad", "2.5", "-tol", "1e-8", "-maxiters", "30", "-r",
                          "chr1:100-400"]) == 0
    assert _read(out + "m", expected.SUFFIXES) == _read(out + "k", expected.SUFFIXES)
    # the records as keywords of the per-chromosome function, and as records
    nine = {k: kw[k] for k in balance.BalanceArgs._fields + expected.ExpectedArgs._fields}
    bal, exp = expected.options_of(**nine)
    assert dict(bal._asdict(), **exp._asdict()) == nine and expected.options_of(bal=bal, exp=exp) == (bal, exp)
    ch = standin["chr2"].chrom
    assert expected.expected_chrom(ch, "chr2", 100, cut=20, **nine) == expected.expected_chrom(ch, "chr2", 100, cut=20, bal=bal, exp=exp)
    with pytest.raises(TypeError):
        expected.options_of(perdecade=4)


@pytest.mark.parametrize("step", ["bal_iterate", "bal_weights", "exp_diagonals", "exp_set", "exp_cells_get"])
def test_a_failing_step_frees_the_cells_once_and_writes_nothing(step, standin, tmp_path):
    standin["chr1"].chrom = ch = MC.Recording(standin["chr1"].chrom, fail=step)
    with pytest.raises(RuntimeError):
        expected.jd2expected("jd", os.path.join(str(tmp_path), "f"), **ARGS)
    assert [c[0] for c in ch.log].count("mat_free") == 1 and ch.log[-1][0] == "mat_free" and ch.log[-2][0] == step
    assert os.listdir(str(tmp_path)) == [] and standin["chr2"].chrom.calls == []
