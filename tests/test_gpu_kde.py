"""GPU: the kernel density sums of K17 (k_sweep.hip: cl_kde_array, cl_dist_collect, cl_dist_kde) against float64 direct sums
and scipy.stats.gaussian_kde -- the array front end over the whole distance domain, the run front end on every source form
of the distance groups, and the pictures of a sweep (`plot`) end to end.

Tolerance of the raw sums: |S - S_ref| <= 4e-5 S_ref + n 2^-100 (n = sum of weights).  The terms that matter have |t| <= 120
(t = -log2(e) z^2 / 2); four float32 roundings on the way to t give |dt| <= 120 * 4 * 2^-24 = 2.9e-5, i.e. 2e-5 relative after
exp2; one or two ulps of exp2 come on top, and a factor 2 covers an exp2 that is a few ulps off.  The absolute floor covers
the terms below float32's normal range (they add up to less than n 2^-126).  So that the floor hides nothing, every case
asserts that at least 2/3 of its grid points have S_ref > 1e3 n 2^-100."""
import os
import threading

import numpy as np
import pytest
from scipy.stats import gaussian_kde

import golden_util as G
import pipe_checks
from cloops_amd import _lib, api, pipe, plots
from cloops_amd.synth import synth_chrom

pytestmark = pytest.mark.gpu

RTOL = 4e-5
FLOOR = 2.0 ** -100
WORST = {"ratio": 0.0}                  # largest err / tol seen (printed by the last test of the module)


def direct_sums(x, lo, step, inv_h, gridsize, w=None):
    """S[j] = sum_i w_i exp(-((x_i - grid_j) inv_h)^2 / 2) in float64, in blocks of entries"""
    grid = lo + np.arange(gridsize, dtype=np.float64) * step
    x = np.asarray(x, np.float64)
    S = np.zeros(gridsize)
    for a in range(0, len(x), 4096):
        e = np.exp(-0.5 * ((x[a:a + 4096, None] - grid[None, :]) * inv_h) ** 2)
        S += (e if w is None else e * np.asarray(w[a:a + 4096], np.float64)[:, None]).sum(0)
    return S


def check_sums(S, ref, n, what):
    tol = RTOL * ref + n * FLOOR
    assert np.count_nonzero(ref > 1e3 * n * FLOOR) * 3 >= 2 * len(ref), (what, "the floor would hide errors")
    err = np.abs(S - ref)
    ratio = float(np.max(err / tol))
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print("%s: worst err / tol = %.4f" % (what, ratio))
    assert ratio <= 1.0, (what, ratio, int(np.argmax(err / tol)))


# ---- 1. the array front end ---------------------------------------------------------------------------------------
EDGE = [1, 2, 3, 4, 5, 7, 8, 9] + [2 ** k + o for k in range(4, 31) for o in (-1, 0, 1)] + [2 ** 31 - 1]
SIZES = [(0, 0), (100, 70), (600, 400), (3000, 2000)]
_INPUTS = {}


def array_input(k):
    """edge values + n1 short + n2 log-uniform distances, a third negated, 50 zeros mixed in -> int64 array (shared, read-only)"""
    if k not in _INPUTS:
        n1, n2 = SIZES[k]
        rng = np.random.default_rng(100 + k)
        d = np.concatenate([np.array(EDGE, np.int64), rng.integers(1, 800, n1), np.floor(2 ** rng.uniform(10, 27, n2)).astype(np.int64)])
        d[rng.random(len(d)) < 1 / 3] *= -1
        d = np.concatenate([d, np.zeros(50, np.int64)])
        d = d[rng.permutation(len(d))]
        d.setflags(write=False)
        _INPUTS[k] = d
    return _INPUTS[k]


def setup_of(d, h, gridsize):
    """-> (x, n, h, lo, step): h None = Scott; the grid as plots.support makes it"""
    ad = np.abs(d[d != 0])
    x = np.log2(ad.astype(np.float64))
    n = len(x)
    if h is None:
        h = float(x.std(ddof=1)) * n ** -0.2
    lo, step = plots.support(int(ad.min()), int(ad.max()), h, gridsize)
    return x, n, h, lo, step


CASES = [(k, h) for k in range(4) for h in ((None, 0.02, 0.005) if k >= 2 else (None,))]


@pytest.mark.parametrize("gridsize", [2, 100, 200, 257, 1024])
@pytest.mark.parametrize("k,h", CASES)
def test_array_sums(k, h, gridsize):
    d = array_input(k)
    assert len(d) == 90 + sum(SIZES[k]) + 50
    x, n, h, lo, step = setup_of(d, h, gridsize)
    S = api.kde_array(d, lo, step, 1.0 / h, gridsize)
    assert S.shape == (gridsize,) and S.dtype == np.float64
    check_sums(S, direct_sums(x, lo, step, 1.0 / h, gridsize), n, "array %d h=%.4g G=%d" % (k, h, gridsize))


@pytest.mark.parametrize("zeros", [0, 50])
@pytest.mark.parametrize("n", [1024, 1025])
def test_array_tile_edge(n, zeros):
    """exactly one full tile of non-zero entries, and one entry more (with and without zeros between them)"""
    d = array_input(2)
    d = d[d != 0][:n]
    assert len(d) == n
    if zeros:
        d = np.insert(d, np.arange(0, n, n // zeros)[:zeros], 0)
        assert len(d) == n + zeros
    for h in (None, 0.02):
        x, nn, hh, lo, step = setup_of(d, h, 200)
        assert nn == n
        S = api.kde_array(d, lo, step, 1.0 / hh, 200)
        check_sums(S, direct_sums(x, lo, step, 1.0 / hh, 200), n, "tile edge n=%d zeros=%d h=%.4g" % (n, zeros, hh))


def test_array_edge_cases():
    assert np.array_equal(api.kde_array(np.zeros(0, np.int32), 0.0, 0.1, 2.0, 200), np.zeros(200))
    assert np.array_equal(api.kde_array(np.zeros(7, np.int32), 0.0, 0.1, 2.0, 200), np.zeros(200))      # zeros only
    d = array_input(1)
    for bad in (1, 1025, 0, -3):
        with pytest.raises(_lib.CloopsHipError) as ei:
            api.kde_array(d, 0.0, 0.1, 2.0, bad)
        assert ei.value.code == _lib.CL_ERR_ARG
    with pytest.raises(_lib.CloopsHipError):
        api.kde_array(d, 0.0, 0.1, 0.0, 200)                              # 1 / h must be positive
    # |d| alone counts: the negated array gives the very same sums; and a call repeated gives the same bits
    x, n, h, lo, step = setup_of(d, None, 257)
    a = api.kde_array(d, lo, step, 1.0 / h, 257)
    assert np.array_equal(a, api.kde_array(d, lo, step, 1.0 / h, 257))
    assert np.array_equal(a, api.kde_array(-d, lo, step, 1.0 / h, 257))
    big = array_input(3)
    x, n, h, lo, step = setup_of(big, 0.02, 1024)
    assert np.array_equal(api.kde_array(big, lo, step, 1.0 / h, 1024), api.kde_array(big, lo, step, 1.0 / h, 1024))


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_kde_curve_is_gaussian_kde(k):
    d = array_input(k)
    grid, dens = plots.kde_curve(d)
    x = np.log2(np.abs(d[d != 0]).astype(np.float64))
    h = x.std(ddof=1) * len(x) ** -0.2
    assert np.allclose(grid, np.linspace(x.min() - 3 * h, x.max() + 3 * h, 200), rtol=0, atol=1e-11)
    assert np.allclose(dens, gaussian_kde(x)(grid), rtol=1e-4, atol=0)


def test_plot_int_sel_cut_frag_on_arrays(tmp_path):
    """the reference's signature on two distance lists -> <prefix>.pdf; a list without a density leaves its curve out"""
    d = array_input(2)
    prefix = str(tmp_path / "arrays")
    plots.plotIntSelCutFrag(list(np.abs(d[:600])), d[600:].astype(np.float64), 4601, 120, prefix=prefix)
    with open(prefix + ".pdf", "rb") as fh:
        assert fh.read(4) == b"%PDF"
    said = []
    plots.plotIntSelCutFrag([64, 64, 0], d, 4601, 120, prefix=prefix + "1", warn=said.append)
    assert os.path.getsize(prefix + "1.pdf") > 1000 and len(said) == 1


# ---- 2. the run front end -----------------------------------------------------------------------------------------
EPS, MINPTS = 2000, 5
_RUN = {}


class _Res(object):
    """what pipe._cluster_arrays needs of a cache resident"""

    def __init__(self, X, Y):
        self.chrom, self.d, self.lock = api.Chromosome(X, Y), Y - X, threading.RLock()


def run_data():
    if "xy" not in _RUN:
        X, Y = synth_chrom(20000, 20000000, 77)
        _RUN["xy"] = (X.astype(np.int64), Y.astype(np.int64))
    return _RUN["xy"]


def run_lists(variant, cut):
    """the `dis` / `dss` lists of the host-list route (pipe.py:63,106-109) for the run, as |d| > 0 (shared, made once)"""
    if (variant, cut) not in _RUN:
        X, Y = run_data()
        r = _Res(X, Y)
        parts = pipe._cluster_arrays(r, EPS, MINPTS, cut, variant)
        r.chrom.close()
        out = []
        for d in (parts[2], parts[3]):
            a = np.abs(d[d != 0]).astype(np.int64)
            a.setflags(write=False)
            out.append(a)
        _RUN[variant, cut] = out
    return _RUN[variant, cut]


@pytest.mark.parametrize("how", ["step", "cluster"])
@pytest.mark.parametrize("cut", [0, 1000])
@pytest.mark.parametrize("variant", ["v1", "v2", "block"])
def test_run_collect_and_sums(variant, cut, how):
    X, Y = run_data()
    lists = run_lists(variant, cut)
    assert len(lists[0]) > 100 and len(lists[1]) > 100                    # both inter- and self-ligation clusters
    ch = api.Chromosome(X, Y)
    if how == "step":
        ch.cand_reset()
        ch.sweep_plan([EPS], [MINPTS])
        ch.step_async(variant, EPS, MINPTS, cut, 0, -1)
        ch.wait()
        st = ch.step_result()[2]
    else:
        ch.cluster(variant, EPS, MINPTS, cut, want_labels=False)
        st = ch.dist_summary(cut)
    col = ch.dist_collect(cut)
    assert col["n_pos"] == [len(a) for a in lists] == st["n_pos"]
    assert col["dmin"] == [int(a.min()) for a in lists] and col["dmax"] == [int(a.max()) for a in lists]
    for g in (0, 1):
        x = np.log2(lists[g].astype(np.float64))
        n = len(x)
        h = plots.scott_bandwidth(n, st["sumx"][g], st["sumxx"][g], st["xshift"])
        assert h == pytest.approx(x.std(ddof=1) * n ** -0.2, rel=1e-9)
        lo, step = plots.support(col["dmin"][g], col["dmax"][g], h, 200)
        S = ch.dist_kde(g, lo, step, 1.0 / h, 200)
        check_sums(S, direct_sums(x, lo, step, 1.0 / h, 200), n, "run %s cut=%d %s group %d" % (variant, cut, how, g))
        assert np.array_equal(S, ch.dist_kde(g, lo, step, 1.0 / h, 200))  # same lists: same bits
        col2 = ch.dist_collect(cut)                                       # collected again (another append order): same bits
        assert col2 == col and np.array_equal(S, ch.dist_kde(g, lo, step, 1.0 / h, 200))
    ch.close()


def test_run_error_cases():
    X, Y = run_data()
    ch = api.Chromosome(X, Y)
    with pytest.raises(_lib.CloopsHipError) as e0:
        ch.dist_summary(0)
    for call in (lambda: ch.dist_kde(0, 0.0, 0.1, 2.0, 200), lambda: ch.dist_collect(0)):
        with pytest.raises(_lib.CloopsHipError) as e1:                    # before any run: what dist_summary says there
            call()
        assert (e1.value.code, str(e1.value)) == (e0.value.code, str(e0.value))
    ch.cluster("v2", EPS, MINPTS, 0, want_labels=False)
    with pytest.raises(_lib.CloopsHipError) as e2:                        # a run, but nothing collected from it
        ch.dist_kde(0, 0.0, 0.1, 2.0, 200)
    assert e2.value.code == _lib.CL_ERR_ARG and "cl_dist_collect" in str(e2.value)
    ch.dist_collect(0)
    ch.dist_kde(0, 5.0, 0.1, 2.0, 200)
    for bad in (1, 1025):
        with pytest.raises(_lib.CloopsHipError) as e3:
            ch.dist_kde(0, 5.0, 0.1, 2.0, bad)
        assert e3.value.code == _lib.CL_ERR_ARG
    with pytest.raises(_lib.CloopsHipError):
        ch.dist_kde(2, 5.0, 0.1, 2.0, 200)                                # no such group
    ch.cluster("v2", EPS, MINPTS, 1000, want_labels=False)                # another run: the collected lists are stale
    with pytest.raises(_lib.CloopsHipError) as e4:
        ch.dist_kde(1, 5.0, 0.1, 2.0, 200)
    assert "cl_dist_collect" in str(e4.value)
    ch.close()


# ---- 3. the pipeline ------------------------------------------------------------------------------------------------
def test_pipe_plot_end_to_end(tmp_path):
    """test_end_to_end_bedpe_to_loop_file's input with plot=1: one picture per step, everything else as without"""
    import gzip
    X, Y = G.chr21_xy()
    bed = os.path.join(str(tmp_path), "in.bedpe.gz")
    with gzip.open(bed, "wt") as fh:
        for x, y in zip(X.tolist(), Y.tolist()):
            fh.write("chr21\t%d\t%d\tchr21\t%d\t%d\tid\t1\t+\t-\n" % (x, x, y, y))
    fout = os.path.join(str(tmp_path), "run")
    pipe.CACHE.clear()
    steps = pipe.pipe([bed], fout, [500, 1000, 2000], [5], tmp=0, hic=0, plot=1)
    for eps in (500, 1000, 2000):
        p = "%s_eps%d_minPts5_disCutoff.pdf" % (fout, eps)
        assert os.path.exists(p) and os.path.getsize(p) > 1000
        with open(p, "rb") as fh:
            assert fh.read(4) == b"%PDF"
    assert [s.get("cut_out") for s in steps] == [4601, 13532, 11103]
    assert open(fout + ".loop").read() == open(os.path.join(G.GOLD, "chr21_v2.loop")).read()


def test_sweep_plot_curves_are_gaussian_kde(tmp_path):
    pipe.CACHE.clear()
    f = pipe_checks.write_chr21_jd(tmp_path)
    prefix = os.path.join(str(tmp_path), "pic")
    dataI, cut, cuts, steps = pipe.runSweepFast([f], [500, 1000, 2000], [5], cut=0, plot=prefix)
    assert [s.get("cut_out") for s in steps] == [4601, 13532, 11103]
    for st in steps:
        k = st["kde"]
        assert st["plot_s"] > 0 and k["grid"].shape == (2, 200) and k["density"].shape == (2, 200)
        assert os.path.getsize("%s_eps%d_minPts5_disCutoff.pdf" % (prefix, st["eps"])) > 1000
        parts = pipe._cluster_arrays(pipe.CACHE.get(f), st["eps"], st["minPts"], st["cut_in"])
        for g, col in ((0, 2), (1, 3)):
            d = parts[col]
            x = np.log2(np.abs(d[d != 0]))
            n = len(x)
            h = x.std(ddof=1) * n ** -0.2
            assert k["n"][g] == n and k["h"][g] == pytest.approx(h, rel=1e-9)
            assert np.allclose(k["grid"][g], np.linspace(x.min() - 3 * h, x.max() + 3 * h, 200), rtol=0, atol=1e-9)
            want = gaussian_kde(x)(k["grid"][g])
            assert np.allclose(k["density"][g], want, rtol=1e-4, atol=n * FLOOR / (n * h * np.sqrt(2 * np.pi)))
    plain = pipe.runSweepFast([f], [500, 1000, 2000], [5], cut=0, plot=None)
    assert all("kde" not in st and "plot_s" not in st for st in plain[3])
    assert (plain[1], plain[2]) == (cut, cuts)
    assert list(plain[0]) == list(dataI) and all(np.array_equal(plain[0][key]["boxes"], dataI[key]["boxes"]) for key in dataI)
    pipe.CACHE.clear()


def test_worst_ratio_report():
    """(last: the largest err / tol of this module's sums, for DESIGN.md)"""
    print("K17 worst err / tol over the module: %.4f" % WORST["ratio"])
    assert WORST["ratio"] <= 1.0
