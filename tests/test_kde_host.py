"""CPU: the host side of the distance-cutoff pictures (cloops_amd.plots, the `plot` keyword of pipe.runSweepFast) -- Scott's
bandwidth from shifted sums, grid and normalisation against scipy.stats.gaussian_kde, the PDF writer, and the sweep driver over
a stand-in chromosome whose dist_collect / dist_kde are numpy (no GPU, no library)."""
import os

import joblib
import numpy as np
import pytest
from scipy.stats import gaussian_kde

import fake_backend
from cloops_amd import api, pipe, plots
from cloops_amd.synth import synth_chrom


def numpy_sums(x, lo, step, inv_h, gridsize, w=None):
    """S[j] = sum_i w_i exp(-((x_i - grid_j) inv_h)^2 / 2) in float64"""
    grid = lo + np.arange(gridsize, dtype=np.float64) * step
    e = np.exp(-0.5 * ((np.asarray(x, np.float64)[:, None] - grid[None, :]) * inv_h) ** 2)
    return (e if w is None else e * np.asarray(w, np.float64)[:, None]).sum(0)


def test_scott_bandwidth_from_shifted_sums():
    rng = np.random.default_rng(17)
    for n, shift in ((2, 0.0), (50, 11.0), (4000, 11.0), (100000, 7.5)):
        x = rng.normal(12.0, 2.5, n)
        s = x - shift
        h = plots.scott_bandwidth(n, s.sum(), (s * s).sum(), shift)
        assert h == pytest.approx(x.std(ddof=1) * n ** -0.2, rel=1e-10)
    assert np.isnan(plots.scott_bandwidth(1, 3.0, 9.0)) and np.isnan(plots.scott_bandwidth(0, 0.0, 0.0))
    assert plots.scott_bandwidth(5, 10.0, 20.0) == 0.0                  # five equal values: no spread
    assert not plots.drawable(1, float("nan")) and not plots.drawable(5, 0.0) and plots.drawable(2, 0.3)


@pytest.mark.parametrize("n,gridsize", [(2, 200), (300, 200), (5000, 64)])
def test_support_and_density_against_gaussian_kde(n, gridsize):
    rng = np.random.default_rng(n)
    d = np.floor(2 ** rng.uniform(3, 27, n)).astype(np.int64)
    x = np.log2(d)
    h = plots.scott_bandwidth(n, x.sum(), (x * x).sum())
    lo, step = plots.support(int(d.min()), int(d.max()), h, gridsize)
    grid = plots.grid_points(lo, step, gridsize)
    want_grid = np.linspace(x.min() - 3 * h, x.max() + 3 * h, gridsize)
    assert np.allclose(grid, want_grid, rtol=0, atol=1e-12)
    dens = plots.density(numpy_sums(x, lo, step, 1.0 / h, gridsize), n, h)
    assert np.allclose(dens, gaussian_kde(x, bw_method="scott")(grid), rtol=1e-9, atol=0)


def _curve(seed, n=500):
    rng = np.random.default_rng(seed)
    x = rng.normal(10 + seed, 1.5, n)
    grid = np.linspace(x.min() - 1, x.max() + 1, 200)
    return grid, gaussian_kde(x)(grid), n


def _is_pdf(path):
    with open(path, "rb") as fh:
        head = fh.read(4)
    return head == b"%PDF" and os.path.getsize(path) > 1000


def test_plot_cut_curves_writes_a_pdf(tmp_path):
    prefix = str(tmp_path / "both")
    said = []
    plots.plot_cut_curves([_curve(1), _curve(4)], 4601, prefix, warn=said.append)
    assert _is_pdf(prefix + ".pdf") and said == []
    for k in (0, 1):                                                    # one group without a density: the other is drawn
        prefix = str(tmp_path / ("one%d" % k))
        curves = [_curve(1), _curve(4)]
        curves[k] = None
        said = []
        plots.plot_cut_curves(curves, 4601, prefix, warn=said.append)
        assert _is_pdf(prefix + ".pdf")
        assert len(said) == 1 and ("inter" if k == 0 else "self") in said[0]


def test_plot_int_sel_cut_frag_log0_is_not_ported(tmp_path):
    with pytest.raises(NotImplementedError):
        plots.plotIntSelCutFrag([100, 200, 300], [10, 20, 30], 50, 120, log=0, prefix=str(tmp_path / "x"))
    assert not os.path.exists(str(tmp_path / "x.pdf"))


# ---- the sweep driver over a numpy chromosome ---------------------------------------------------------------------
class KdeFake(fake_backend.FakeChromosome):
    """FakeChromosome + numpy versions of Chromosome.dist_collect / dist_kde, counting their calls"""
    calls = {"collect": 0, "kde": 0}

    def dist_collect(self, cut=0):
        type(self).calls["collect"] += 1
        g, ad = self._groups(cut)
        self._kde = [ad[(g == k) & (ad > 0)] for k in (0, 1)]
        return {"n_pos": [len(a) for a in self._kde], "dmin": [int(a.min()) if len(a) else 0 for a in self._kde],
                "dmax": [int(a.max()) if len(a) else 0 for a in self._kde]}

    def dist_kde(self, group, lo, step, inv_h, gridsize):
        type(self).calls["kde"] += 1
        return numpy_sums(np.log2(self._kde[group].astype(np.float64)), lo, step, inv_h, gridsize)


@pytest.fixture()
def kde_pipe(monkeypatch, tmp_path):
    monkeypatch.setattr(api, "Chromosome", KdeFake)
    monkeypatch.setattr(api, "device_count", lambda: 1)
    pipe.CACHE.clear()
    KdeFake.calls = {"collect": 0, "kde": 0}
    fs = []
    for k in range(2):
        X, Y = synth_chrom(1500, 4000000, 40 + k)
        f = str(tmp_path / ("c%d-c%d.jd" % (k, k)))
        joblib.dump(np.stack([np.arange(len(X)), X, Y], 1).astype(np.int64), f)
        fs.append(f)
    yield fs, tmp_path
    pipe.CACHE.clear()


def test_sweep_with_plot_adds_curves_and_files(kde_pipe):
    fs, tmp = kde_pipe
    plain = pipe.runSweepFast(fs, [1000, 2000], [5], cut=0)
    assert KdeFake.calls == {"collect": 0, "kde": 0}                     # plot=None: not one extra call
    assert all("kde" not in st and "plot_s" not in st for st in plain[3])
    prefix = str(tmp / "pic")
    dataI, cut, cuts, steps = pipe.runSweepFast(fs, [1000, 2000], [5], cut=0, plot=prefix)
    with_cut = [st for st in steps if "cut_out" in st]
    assert len(with_cut) == 2                                           # (the data gives both groups in both steps)
    assert KdeFake.calls["collect"] == 2 * len(fs) and 0 < KdeFake.calls["kde"] <= 2 * 2 * len(fs)
    for st in steps:
        assert ("kde" in st) == ("cut_out" in st) == ("plot_s" in st)
    for st in with_cut:
        k = st["kde"]
        assert k["grid"].shape == (2, 200) and k["density"].shape == (2, 200) and k["grid"].dtype == np.float64
        assert _is_pdf("%s_eps%d_minPts%d_disCutoff.pdf" % (prefix, st["eps"], st["minPts"]))
        assert st["plot_s"] > 0
        # the curves are those of the distance lists of the host-list route (pipe.py:106-109) at this step's cut
        parts = [pipe._cluster_arrays(pipe.CACHE.get(f), st["eps"], st["minPts"], st["cut_in"]) for f in fs]
        for g, col in ((0, 2), (1, 3)):
            d = np.concatenate([p[col] for p in parts])
            x = np.log2(np.abs(d[d != 0]))
            assert k["n"][g] == len(x)
            assert k["h"][g] == pytest.approx(x.std(ddof=1) * len(x) ** -0.2, rel=1e-9)
            assert k["grid"][g][0] == pytest.approx(x.min() - 3 * k["h"][g], rel=1e-12)
            assert np.allclose(k["density"][g], gaussian_kde(x)(k["grid"][g]), rtol=1e-8, atol=0)
    # nothing else moved
    assert (cut, cuts) == (plain[1], plain[2])
    assert [{k: v for k, v in st.items() if k not in ("kde", "plot_s", "wall_s")} for st in steps] == \
           [{k: v for k, v in st.items() if k != "wall_s"} for st in plain[3]]
    assert list(dataI) == list(plain[0]) and all(np.array_equal(dataI[k]["boxes"], plain[0][k]["boxes"]) for k in dataI)


def test_sweep_plot_with_allsum_raises(kde_pipe):
    fs, tmp = kde_pipe
    with pytest.raises(ValueError):
        pipe.runSweepFast(fs, [1000], [5], cut=0, allsum=lambda a: a, plot=str(tmp / "pic"))
    assert KdeFake.calls == {"collect": 0, "kde": 0}
    assert not [n for n in os.listdir(str(tmp)) if n.endswith(".pdf")]


def test_a_group_without_spread_is_left_out(tmp_path):
    """_step_kde on a group of equal distances: NaN rows, and the picture is still written with the other group"""
    class R(object):
        def __init__(self, chrom):
            import threading
            self.chrom, self.lock = chrom, threading.Lock()

    ch = KdeFake(np.zeros(1), np.ones(1))
    ch._kde = [np.array([64, 64, 64]), np.array([10, 20, 40, 80, 160])]
    ch.dist_collect = lambda cut=0: {"n_pos": [3, 5], "dmin": [64, 10], "dmax": [64, 160]}
    x = [np.log2(a.astype(np.float64)) for a in ch._kde]
    kde = pipe._step_kde([R(ch)], 0, [3, 5], [v.sum() for v in x], [(v * v).sum() for v in x], 0.0)
    assert np.isnan(kde["density"][0]).all() and kde["n"] == [3, 5]
    assert np.allclose(kde["density"][1], gaussian_kde(x[1])(kde["grid"][1]), rtol=1e-9, atol=0)
    said = []
    pipe._plot_step(kde, 50, str(tmp_path / "p"), said.append)
    assert _is_pdf(str(tmp_path / "p.pdf")) and len(said) == 1
