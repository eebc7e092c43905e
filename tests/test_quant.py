"""CPU: loop re-quantification (cloops_amd.quant, scripts/quantifyLoops.py) and differential loops (cloops_amd.deloops,
scripts/deLoops).  The K11 count table is replaced by a numpy brute force over the PETs (`brute_counts`, also the
yardstick of the GPU tests in test_gpu_quant.py); fed through the host functions it must reproduce the goldens that the
real scripts wrote (tests/golden/make_golden_quant.py) text for text."""
import os

import joblib
import numpy as np
import pytest

import golden_util as G
import refload

GOLD = G.GOLD
QUANT_GOLD = (("chr21_quantLoops.txt", "A", 0, "chr21"), ("chr21_dis4601_quantLoops.txt", "B", 4601, "chr21_dis4601"))


def brute_counts(X, Y, windows, cut=0):
    """numpy restatement of cl_quant_counts: (int32 [R, 123], N).  [0] |S(A_0)|, [1] |S(B_0)| with S(W) = {X in W} | {Y in W};
    [2 + 11 k + l] |{X in A_k} & {Y in B_l}|; windows inclusive, PETs with Y - X < cut dropped when cut > 0."""
    X = np.asarray(X, np.int64)
    Y = np.asarray(Y, np.int64)
    if cut > 0:
        keep = (Y - X) >= cut
        X, Y = X[keep], Y[keep]
    w = np.asarray(windows, np.int64).reshape(-1, 44)
    lo, hi = w[:, :22], w[:, 22:]
    order = np.argsort(X, kind="stable")
    xs, ys = X[order], Y[order]
    out = np.zeros((len(w), 123), np.int32)
    for r in range(len(w)):
        inside = lambda v, k: (v >= lo[r, k]) & (v <= hi[r, k])
        out[r, 0] = np.count_nonzero(inside(X, 0) | inside(Y, 0))
        out[r, 1] = np.count_nonzero(inside(X, 11) | inside(Y, 11))
        a, b = np.searchsorted(xs, lo[r, :11].min(), "left"), np.searchsorted(xs, hi[r, :11].max(), "right")
        x, y = xs[a:b], ys[a:b]
        ma = np.stack([inside(x, k) for k in range(11)], 1).astype(np.int64)
        mb = np.stack([inside(y, 11 + k) for k in range(11)], 1).astype(np.int64)
        out[r, 2:] = (ma.T @ mb).reshape(-1)
    return out, len(X)


def _brute_backend(monkeypatch):
    """route quant._counts (K11 on the resident chromosome) to brute_counts on the .jd file"""
    from cloops_amd import pipe, quant

    def counts(f, wins, dis):
        _, mat = pipe.parseJd(f, 0)
        mat = np.asarray(mat).reshape(-1, 3)
        return brute_counts(mat[:, 1], mat[:, 2], wins, dis)
    monkeypatch.setattr(quant, "_counts", counts)


def write_datasets(root):
    """.jd directories of dataset A (the chr21 example) and B (its subsample of make_golden_quant.py) -> (dirA, dirB)"""
    X, Y = G.chr21_xy()
    z = np.load(os.path.join(GOLD, "chr21_quant_subsample.npz"))
    rows = np.flatnonzero(np.unpackbits(z["mask"])[:int(z["n"])])
    out = []
    for name, sel in (("chr21_A", np.arange(len(X))), ("chr21_B", rows)):
        d = os.path.join(str(root), name)
        os.makedirs(d)
        joblib.dump(np.stack([sel, X[sel], Y[sel]], 1).astype(np.int64), os.path.join(d, "chr21-chr21.jd"))
        out.append(d)
    return out


def _read(path):
    with open(path) as fh:
        return fh.read()


def test_quantify_cli_matches_golden(tmp_path, monkeypatch):
    from cloops_amd import quant
    _brute_backend(monkeypatch)
    dirs = dict(zip("AB", write_datasets(tmp_path)))
    for fname, ds, dis, prefix in QUANT_GOLD:
        out = os.path.join(str(tmp_path), prefix)
        assert quant.main(["-f", os.path.join(GOLD, "chr21_v2.loop"), "-d", dirs[ds], "-o", out, "-dis", str(dis)]) == 0
        assert _read(out + "_quantLoops.txt") == _read(os.path.join(GOLD, fname)), fname


def test_deloops_cli_matches_golden(tmp_path, monkeypatch):
    from cloops_amd import deloops
    _brute_backend(monkeypatch)
    da, db = write_datasets(tmp_path)
    monkeypatch.chdir(tmp_path)
    assert deloops.main(["-fa", os.path.join(GOLD, "chr21_v2.loop"), "-fb", os.path.join(GOLD, "chr21_v1.loop"),
                         "-da", da, "-db", db, "-p", "4"]) == 0
    for name in ("chr21_A.deloop", "chr21_B.deloop"):
        assert _read(os.path.join(str(tmp_path), name)) == _read(os.path.join(GOLD, name)), name


def test_chroms_option_same_rows(tmp_path, monkeypatch):
    """-c seeds the records from a set (row order follows the hash seed): compared as sets of rows"""
    from cloops_amd import quant
    _brute_backend(monkeypatch)
    da, _ = write_datasets(tmp_path)
    out = os.path.join(str(tmp_path), "c")
    quant.main(["-f", os.path.join(GOLD, "chr21_v2.loop"), "-d", da, "-o", out, "-c", "chr21,chr22"])
    got = _read(out + "_quantLoops.txt").split("\n")
    want = _read(os.path.join(GOLD, "chr21_quantLoops.txt")).split("\n")
    assert got[0] == want[0] and sorted(got[1:]) == sorted(want[1:])


def test_brute_counts_by_sets():
    """the brute force against the reference's set semantics (getCounts / getPETsforRegions) on a small case"""
    rng = np.random.default_rng(3)
    X = rng.integers(0, 400, 300)
    Y = X + rng.integers(0, 300, 300)
    w = np.zeros((3, 44), np.int64)
    for r in range(3):
        lo = rng.integers(0, 600, 22)
        w[r, :22], w[r, 22:] = lo, lo + rng.integers(-5, 80, 22)
    got, n = brute_counts(X, Y, w)
    assert n == 300
    ids = np.arange(300)
    region = lambda v, a, b: set(ids[(v >= a) & (v <= b)].tolist())
    for r in range(3):
        A = [(w[r, k], w[r, 22 + k]) for k in range(11)]
        B = [(w[r, 11 + k], w[r, 33 + k]) for k in range(11)]
        assert got[r, 0] == len(region(X, *A[0]) | region(Y, *A[0]))
        assert got[r, 1] == len(region(X, *B[0]) | region(Y, *B[0]))
        for k in range(11):
            for l in range(11):
                assert got[r, 2 + 11 * k + l] == len(region(X, *A[k]) & region(Y, *B[l]))


def test_windows_equal_reference_nearby_regions():
    """quant's windows (cModel._windows) == the converted reference getNearbyPairRegions, incl. windows clamped at 0"""
    if not refload.available():
        pytest.skip("reference checkout not present")
    from cloops_amd import quant
    ns = refload.ref_cmodel_namespace()
    rs = {"a": ["chr1", 100, 900, "chr1", 5000, 5300], "b": ["chr1", 10, 20, "chr1", 30, 41],
          "c": ["chr1", 44800894, 44801696, "chr1", 44911732, 44912078], "d": ["chr1", 0, 1, "chr1", 7, 7]}
    w = quant._loop_windows(rs)
    for q, r in enumerate(rs.values()):
        ivas, ivbs = ns["getNearbyPairRegions"]([r[1], r[2]], [r[4], r[5]], win=5)
        assert [[int(w[q, k]), int(w[q, 22 + k])] for k in range(1, 11)] == [[int(a), int(b)] for a, b in ivas]
        assert [[int(w[q, 11 + k]), int(w[q, 33 + k])] for k in range(1, 11)] == [[int(a), int(b)] for a, b in ivbs]
        assert [w[q, 0], w[q, 22], w[q, 11], w[q, 33]] == [r[1], r[2], r[4], r[5]]
    assert (w >= 0).all() and (w[1, 1:11] == 0).any()                     # some windows of "b" clamped by max([0, ...])


def test_cli_parsing():
    from cloops_amd import deloops, quant
    op = quant.help(["-f", "a.loop", "-d", "A", "-o", "out", "-p", "3", "-c", "chr1,chr2", "-dis", "500"])
    assert (op.f, op.d, op.output, op.cpu, op.chroms, op.dis) == ("a.loop", "A", "out", 3, "chr1,chr2", 500)
    op = quant.help(["-f", "a.loop", "-d", "A", "-o", "out"])
    assert (op.cpu, op.chroms, op.dis) == (1, "", 0)
    op = deloops.deloopHelp(["-fa", "a.loop", "-fb", "b.loop", "-da", "A", "-db", "B", "-dis", "7"])
    assert (op.fa, op.fb, op.da, op.db, op.cpu, op.chroms, op.dis) == ("a.loop", "b.loop", "A", "B", 1, "", 7)
    with pytest.raises(SystemExit):
        quant.help(["-f", "a.loop", "-o", "out"])                          # -d is required
    with pytest.raises(SystemExit):
        deloops.deloopHelp(["-fa", "a.loop", "-da", "A", "-db", "B"])      # -fb is required


def _write_loop(path, header, rows):
    with open(path, "w") as fh:
        if header is not None:
            fh.write("\t".join(header) + "\n")
        for r in rows:
            fh.write("\t".join(r) + "\n")


def test_anchor_columns_by_header_and_fallback(tmp_path):
    from cloops_amd import quant
    d = str(tmp_path)
    open(os.path.join(d, "chr1-chr1.jd"), "w").close()
    # insertion-order header (cModel.runStat): iva / ivb at 10 / 11, columns 6 / 7 hold numbers
    hdr = ["loopId", "distance", "ra", "rb", "rab", "ES", "FDR", "hypergeometric_p-value", "poisson_p-value", "binomial_p-value",
           "iva", "ivb", "significant"]
    row = ["L1", "1.0", "1", "1", "1", "1.0", "0.0", "1e-20", "1e-20", "1e-20", "chr1:100-200", "chr1:900-1000", "1.0"]
    low = ["L2"] + row[1:-1] + ["0.0"]
    _write_loop(os.path.join(d, "a.loop"), hdr, [row, low])
    rec = quant.preDs(os.path.join(d, "a.loop"), d)
    assert list(rec) == ["chr1"] and rec["chr1"]["rs"] == {"L1": ["chr1", 100, 200, "chr1", 900, 1000]}
    assert rec["chr1"]["f"] == os.path.join(d, "chr1-chr1.jd")
    # alphabetical header of old pandas: iva / ivb at 6 / 7, found by name as well
    alpha = ["loopId", "ES", "FDR", "binomial_p-value", "distance", "hypergeometric_p-value", "iva", "ivb", "significant"]
    _write_loop(os.path.join(d, "b.loop"), alpha, [["L9", "1", "0", "0", "5", "0", "chr1:1-2", "chr1:30-40", "1"]])
    assert quant.preDs(os.path.join(d, "b.loop"), d)["chr1"]["rs"] == {"L9": ["chr1", 1, 2, "chr1", 30, 40]}
    # no header naming the anchors: the first line is skipped like the script's, columns 6 / 7
    first = ["L0", "1", "0", "0", "5", "0", "chr1:5-6", "chr1:70-80", "1"]
    _write_loop(os.path.join(d, "c.loop"), None, [first, ["L8", "1", "0", "0", "5", "0", "chr1:3-4", "chr1:50-60", "1"]])
    assert quant.preDs(os.path.join(d, "c.loop"), d)["chr1"]["rs"] == {"L8": ["chr1", 3, 4, "chr1", 50, 60]}
    # explicit columns win; a chromosome without its .jd is dropped
    assert quant.preDs(os.path.join(d, "a.loop"), d, ivac=10, ivbc=11)["chr1"]["rs"]["L1"][1] == 100
    _write_loop(os.path.join(d, "e.loop"), hdr, [row[:10] + ["chr2:1-2", "chr2:5-9", "1.0"]])
    assert quant.preDs(os.path.join(d, "e.loop"), d) == {}


def test_error_cases(tmp_path, monkeypatch):
    """where the scripts fail, the port raises: no chromosome in common (pd.concat of nothing), a model of < 2 PETs"""
    from cloops_amd import deloops, quant
    _brute_backend(monkeypatch)
    d = str(tmp_path)
    for name, n in (("one", 1), ("two", 2)):
        os.makedirs(os.path.join(d, name))
        mat = np.stack([np.arange(n), np.arange(n) * 10 + 100, np.arange(n) * 10 + 950], 1).astype(np.int64)
        joblib.dump(mat, os.path.join(d, name, "chr1-chr1.jd"))
    hdr = ["loopId", "iva", "ivb", "significant"]
    _write_loop(os.path.join(d, "a.loop"), hdr, [["L1", "chr1:100-200", "chr1:900-1000", "1"]])
    _write_loop(os.path.join(d, "b.loop"), hdr, [["L1", "chr2:100-200", "chr2:900-1000", "1"]])
    with pytest.raises(ValueError, match="fewer than 2 PETs"):
        quant.main(["-f", os.path.join(d, "a.loop"), "-d", os.path.join(d, "one"), "-o", os.path.join(d, "x")])
    ds = quant.main(["-f", os.path.join(d, "a.loop"), "-d", os.path.join(d, "two"), "-o", os.path.join(d, "x")])
    assert ds == 0 and _read(os.path.join(d, "x_quantLoops.txt")).split("\n")[1].split("\t")[3:6] == ["2", "2", "2"]
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="no chromosome"):
        deloops.main(["-fa", os.path.join(d, "a.loop"), "-fb", os.path.join(d, "b.loop"), "-da", os.path.join(d, "two"),
                      "-db", os.path.join(d, "two")])
    with pytest.raises(ValueError, match="fewer than 2 PETs"):
        deloops.main(["-fa", os.path.join(d, "a.loop"), "-fb", os.path.join(d, "a.loop"), "-da", os.path.join(d, "two"),
                      "-db", os.path.join(d, "one")])


def test_deloops_background_is_zero():
    """lam = (rabc + 1) * Nt / Nc whatever the shifted windows hold (the script's getPermutatedBg always fails)"""
    from cloops_amd import deloops
    rs = {"x": ["chr1", 10, 20, "chr1", 50, 60], "y": ["chr1", 10, 20, "chr1", 50, 60]}
    ds = deloops.estSigFromCounts(rs, [5, 0], 100, [2, 0], 50)
    from scipy.stats import poisson
    lam = 3 * 2.0
    assert float(ds.loc["x", "FoldEnrichment"]) == 5 / lam
    assert float(ds.loc["x", "poisson_p-value"]) == max([poisson.sf(4.0, lam), 1e-300])
    w = deloops._anchor_windows(rs)
    assert (w[:, 1:11] == 10).all() and (w[:, 23:33] == 9).all() and (w[:, 12:22] == 50).all() and (w[:, 34:44] == 49).all()
