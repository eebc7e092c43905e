"""GPU: the distance statistics of a sweep step (K7, k_sweep.hip) against plain high-precision references --
numpy longdouble log2 summed with math.fsum, exact integer histograms, np.sort -- over the whole distance
domain (all 30 octaves, all 128 entries of the log2 tables), every source form of k7_summary, the fine
histogram fused into a sweep step, cl_dist_bin_hist, the exact median's refinement and the sweep chain
on groups of (nearly) equal distances."""
import math

import numpy as np
import pytest

import dist_stats_cases as C
import oracle
from cloops_amd import _lib, api, ests, pipe
from cloops_amd.synth import synth_chrom

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
#: bound on one term x = log2 d - 11 of k7_log2 against the exact value: a few ulp of log2 d < 32 (2^-48 each), the shift
TERM_ERR = 6 * 2.0 ** -48
TOP = 2 ** 30 - 2                     # the largest |d|: X = -(2^29 - 1), Y = 2^29 - 1 (v1 / block)


def _xy_of_dist(d):
    """PETs of the given distances inside the coordinate domain (|X|, |Y| < 2^29): X = -(d // 2)"""
    d = np.asarray(d, np.int64)
    X = -(d // 2)
    return X, X + d


def _exact_terms(a):
    """x = log2 a - 11 in longdouble (64-bit mantissa: ~2^-11 ulp of a double), as exact float64 pairs"""
    x = np.log2(np.asarray(a, np.longdouble)) - 11
    hi = x.astype(np.float64)
    lo = (x - hi).astype(np.float64)
    return x, hi, lo


def _check_sums(st, g, a, threads=65536):
    """sum x and sum x^2 of group g against fsum of the exact terms, within (per term) TERM_ERR and (summation) the
    depth of the reduction -- ceil(n / threads) terms in order per thread, then at most 64 levels -- times u sum |t|"""
    a = np.abs(np.asarray(a, np.int64))
    a = a[a > 0]
    n = len(a)
    assert st["n_pos"][g] == n
    if n == 0:
        assert st["sumx"][g] == 0.0 and st["sumxx"][g] == 0.0
        return
    x, hi, lo = _exact_terms(a)
    sx = math.fsum(np.concatenate([hi, lo]).tolist())
    xx = x * x
    xxh = xx.astype(np.float64)
    sxx = math.fsum(np.concatenate([xxh, (xx - xxh).astype(np.float64)]).tolist())
    ax = float(np.abs(hi).sum())
    depth = -(-n // threads) + 64
    tol_x = n * TERM_ERR + depth * U * ax
    tol_xx = 2 * TERM_ERR * ax + (depth + 1) * U * sxx
    assert abs(st["sumx"][g] - sx) <= tol_x, (g, st["sumx"][g], sx, tol_x)
    assert abs(st["sumxx"][g] - sxx) <= tol_xx, (g, st["sumxx"][g], sxx, tol_xx)


def _loghist(a):
    a = np.abs(np.asarray(a, np.int64))
    a = a[a > 0]
    return np.bincount(np.array([ests.logbin(v) for v in a.tolist()], np.int64), minlength=3840)


def _check_summary(st, ref):
    """a summary against the oracle's lists (pipe.py:63,106-109): counts and histogram exact, sums within the bound"""
    assert st["n_all"] == [len(ref["dis"]), len(ref["dss"])]
    _check_sums(st, 0, ref["dis"])
    _check_sums(st, 1, ref["dss"])
    assert np.array_equal(st["loghist"], _loghist(ref["dss"]))


# ---- the whole distance domain ------------------------------------------------------------------
def _domain_distances():
    """lower edge, middle and upper edge of every reachable log bin of the 30 octaves, the largest distance, and d = 0"""
    d = set()
    for b in range(3840):
        lo, hi = ests.logbin_range(b)
        if ests.logbin(lo) == b:
            d.update((lo, (lo + hi - 1) // 2, hi - 1))
    d.discard(2 ** 30 - 1)
    d.add(TOP)
    return np.array(sorted(d) + [0, 0, 0], np.int64)


@pytest.mark.parametrize("variant", ["v1", "block"])
def test_summary_over_the_whole_distance_domain(variant):
    """every PET below the cut: all in the self group, read by the pass over the rows (cut >= 65536)"""
    d = _domain_distances()
    X, Y = _xy_of_dist(d)
    ch = api.Chromosome(X, Y)
    cut = 2 ** 30 - 1
    ch.cluster(variant, 500, 5, cut, want_labels=False)
    st = ch.dist_summary(cut)
    assert st["xshift"] == 11.0
    assert st["n_all"] == [0, len(d)] and st["n_pos"] == [0, len(d) - 3]          # d = 0 counts in n_all only
    h = _loghist(d)
    assert h[3839] > 0 and np.array_equal(st["loghist"], h)
    _check_sums(st, 1, d)
    ch.close()


@pytest.mark.parametrize("octave", [7, 17, 29])
def test_log2_every_table_entry_alone(octave):
    """k7_log2 term by term: one PET per handle, so that sum x IS the term.  All 128 table entries of a low, a middle
    and the top octave, at the entry's lower edge, centre or upper edge"""
    worst = 0.0
    for k in range(128):
        lo = (128 + k) << (octave - 7)
        w = 1 << (octave - 7)
        dd = [lo, lo + w // 2, lo + w - 1][k % 3]
        dd = min(dd, TOP)
        X, Y = _xy_of_dist([dd])
        ch = api.Chromosome(X, Y)
        ch.cluster("v1", 500, 5, dd + 1, want_labels=False)
        st = ch.dist_summary(dd + 1)
        ch.close()
        assert st["n_pos"] == [0, 1]
        L = np.log2(np.longdouble(dd))
        got = np.longdouble(st["sumx"][1]) + 11
        err = abs(float(got - L))
        tol = 4 * np.spacing(float(L)) + 0.5 * np.spacing(abs(st["sumx"][1]))
        assert err <= tol, (k, dd, err, tol)
        worst = max(worst, err / np.spacing(float(L)))
        assert st["loghist"][ests.logbin(dd)] == 1
    assert worst <= 4


# ---- every source form of k7_summary --------------------------------------------------------------
def _synth(n, seed, swapped=0.0):
    X, Y = synth_chrom(n, 20000000, seed)
    X, Y = X.astype(np.int64), Y.astype(np.int64)
    if swapped:
        m = np.random.RandomState(seed).rand(n) < swapped
        X[m], Y[m] = Y[m].copy(), X[m].copy()                  # rows with Y < X (v1 / block): |d| (ests.py:42-43)
    return X, Y


@pytest.mark.parametrize("variant,device_labels,swapped", [("v2", True, 0.0), ("v2", False, 0.0), ("v1", True, 0.0),
                                                            ("v1", False, 0.05), ("block", True, 0.05)])
def test_summary_source_forms(variant, device_labels, swapped):
    """sorted arrays (v2, v1), row-order labels (set_device_labels(False)), block; PETs below the cut from the upload
    histogram (cut < 65536) or from a pass over the rows (cut >= 65536, rows with Y < X); a cut that removes every PET"""
    X, Y = _synth(120000, 31 + int(swapped * 100), swapped)
    ch = api.Chromosome(X, Y)
    ch.set_device_labels(device_labels)
    for eps, minPts, cut in ((500, 5, 0), (1000, 5, 3000), (1000, 4, 100000), (500, 5, 2 ** 30 - 1)):
        ch.cluster(variant, eps, minPts, cut, want_labels=False)
        ref = oracle.single_dbscan(variant, X, Y, eps, minPts, cut)
        st = ch.dist_summary(cut)
        _check_summary(st, ref)
        if cut == 2 ** 30 - 1:
            assert st["n_all"] == [0, len(X)]                  # pipe.py:59-65: every PET in dss
    ch.close()


# ---- the fine histogram fused into a sweep step ---------------------------------------------------
def _step(ch, variant, eps, minPts, cut, fine_lo, step=0):
    ch.cand_reset()
    ch.sweep_plan([eps], [minPts])
    ch.step_async(variant, eps, minPts, cut, step, fine_lo)
    ch.wait()
    return ch.step_result()


@pytest.mark.parametrize("variant,fine_lo", [("v2", 0), ("v2", 1), ("v2", 16384 - 1000), ("v1", 2 ** 30 - 2048),
                                             ("v1", 2 ** 30), ("block", 2 ** 29 - 100)])
def test_step_fine_histogram(variant, fine_lo):
    """step_result()["fine"] == numpy's histogram of the self group's |d| in [fine_lo, fine_lo + 2048); the rest of the
    step's summary == dist_summary of the same run (counts, histogram exactly; sums within the bound); the step repeated
    gives bitwise the same statistics"""
    X, Y = _synth(80000, 7)
    if variant != "v2":                                     # distances up to 2^30 - 2 (octave 29), below the cut
        Xb, Yb = _xy_of_dist(np.linspace(2 ** 29 - 3000, TOP, 3000).astype(np.int64))
        X, Y = np.concatenate([X, Xb]), np.concatenate([Y, Yb])
        Xc, Yc = _xy_of_dist(2 ** 30 - 2048 + np.arange(0, 2046, 3))
        X, Y = np.concatenate([X, Xc]), np.concatenate([Y, Yc])
        cut = 2 ** 30 - 1                                   # (>= 65536: the pass over the rows; nothing left to cluster)
    else:
        Xc = np.arange(3000) * 7 + 1000
        X, Y = np.concatenate([X, Xc, Xc]), np.concatenate([Y, Xc, Xc + (np.arange(3000) % 40)])   # d = 0 .. 39
        cut = 3000
    ch = api.Chromosome(X, Y)
    ni, ns, s = _step(ch, variant, 1000, 5, cut, fine_lo)
    ref = oracle.single_dbscan(variant, X, Y, 1000, 5, cut)
    a = np.abs(ref["dss"]).astype(np.int64)
    a = a[(a > 0) & (a >= fine_lo) & (a < fine_lo + 2048)]
    assert s["fine_lo"] == fine_lo
    want = np.bincount(a - fine_lo, minlength=2048)
    assert np.array_equal(s["fine"], want)
    if fine_lo == 0:
        assert s["fine"][0] == 0 and s["n_all"][1] > s["n_pos"][1]     # d = 0: no log2, no bin, not counted here either
    _check_summary(s, ref)
    st = ch.dist_summary(cut)
    for k in ("n_all", "n_pos"):
        assert st[k] == s[k]
    assert np.array_equal(st["loghist"], s["loghist"])
    _, _, s2 = _step(ch, variant, 1000, 5, cut, fine_lo)
    assert s2["sumx"] == s["sumx"] and s2["sumxx"] == s["sumxx"]          # bitwise: fixed reduction order
    assert np.array_equal(s2["fine"], s["fine"]) and np.array_equal(s2["loghist"], s["loghist"])
    ch.close()


# ---- cl_dist_bin_hist -------------------------------------------------------------------------------
def test_bin_hist_octave_edges_and_shifts():
    """(|d| - lo) >> shift over lo <= |d| < hi for shift 0 .. 20, [lo, hi) one whole octave (2048 bins exactly: the top
    bin is the last one) or a part of one ending inside a bin, against numpy on the oracle's dss"""
    rng = np.random.RandomState(3)
    d = np.concatenate([np.arange(1, 4096), rng.randint(1, TOP + 1, 200000), [2 ** e + k for e in range(1, 30) for k in (-1, 0, 1)]])
    d = d[(d >= 1) & (d <= TOP)]
    X, Y = _xy_of_dist(d)
    ch = api.Chromosome(X, Y)
    cut = 2 ** 30 - 1
    ch.cluster("v1", 500, 5, cut, want_labels=False)
    a = np.asarray(d, np.int64)
    for shift in range(0, 21):
        e = min(shift + 11, 29)
        for lo, hi in ((2 ** e, 2 ** (e + 1)), (2 ** e, 2 ** e + (2047 << shift) + 1), (2 ** e + 3, 2 ** e + 3 + (100 << shift))):
            hi = min(hi, 2 ** 30)
            got = ch.dist_bin_hist(cut, lo, hi, shift)
            s = a[(a >= lo) & (a < hi)]
            want = np.bincount((s - lo) >> shift, minlength=2048)
            assert len(want) == 2048 and np.array_equal(got, want), (shift, lo, hi)
    got = ch.dist_bin_hist(cut, 5, 5, 0)                       # empty range
    assert not got.any()
    ch.close()


def test_bin_hist_argument_errors():
    X, Y = _xy_of_dist(np.arange(1, 5000))
    ch = api.Chromosome(X, Y)
    ch.cluster("v1", 500, 5, 10000, want_labels=False)
    for lo, hi, shift in ((0, 100, -1), (0, 100, 32), (100, 99, 0), (0, 2049, 0), (0, (2048 << 5) + 1, 5)):
        with pytest.raises(_lib.CloopsHipError) as ei:
            ch.dist_bin_hist(10000, lo, hi, shift)
        assert ei.value.code == _lib.CL_ERR_ARG
    assert ch.dist_bin_hist(10000, 0, 2048, 0).sum() == 2047        # the widest range that fits
    ch.close()


# ---- the exact median's refinement (pipe._select_kth) ---------------------------------------------------
class _R(object):
    def __init__(self, ch):
        self.chrom = ch


def test_select_kth_over_several_chromosomes():
    """every rank of a small self group summed over three chromosomes; ranks inside octave-29 bins (2^22 wide: two
    refinement passes) -- against np.sort of the oracle's dss"""
    rng = np.random.RandomState(9)
    for cut, make in ((3000, lambda k: _synth(300, 50 + k)),
                      (2 ** 30 - 1, lambda k: _xy_of_dist(np.concatenate([rng.randint(1, TOP + 1, 3000), rng.randint(2 ** 29, TOP + 1, 2000)])))):
        chroms, dss, loghist = [], [], np.zeros(3840, np.int64)
        for k in range(3):
            X, Y = make(k)
            ch = api.Chromosome(X, Y)
            ch.cluster("v1", 500, 5, cut, want_labels=False)
            ref = oracle.single_dbscan("v1", X, Y, 500, 5, cut)
            dss.append(np.abs(ref["dss"]))
            loghist += ch.dist_summary(cut)["loghist"]
            chroms.append(_R(ch))
        srt = np.sort(np.concatenate(dss)).astype(np.int64)
        srt = srt[srt > 0]
        if cut == 3000:
            ranks = list(range(len(srt)))
        else:
            ranks = [int(r) for r in np.flatnonzero(srt >= 2 ** 29)[::97]] + [len(srt) - 1]
        got = pipe._select_kth(chroms, cut, loghist, ranks)
        assert got == [int(srt[r]) for r in ranks]
        for r in chroms:
            r.chrom.close()


# ---- end to end: the sweep chain ------------------------------------------------------------------------
def _oracle_chain(xys, eps, minPts, cut, variant="v2"):
    """the chain of cut_2 values built from the oracle's dis / dss lists with ests.estIntSelCutFrag (pipe.py:247-275;
    a chromosome without inter-ligation clusters is skipped, pipe.py:121-122)"""
    cuts = [cut]
    for ep in eps:
        for m in minPts:
            dis, dss = [], []
            for X, Y in xys:
                r = oracle.single_dbscan(variant, X, Y, ep, m, cut)
                if len(r["dataI"]):
                    dis.append(r["dis"])
                    dss.append(r["dss"])
            if not dis:
                continue
            dis, dss = np.concatenate(dis), np.concatenate(dss)
            if len(dis) and len(dss):
                cut = ests.estIntSelCutFrag(dis, dss)[0]
                cuts.append(cut)
    return cuts


@pytest.fixture()
def gpu_cache():
    pipe.CACHE.clear()
    yield
    pipe.CACHE.clear()


@pytest.mark.parametrize("name", C.NAMES)
def test_sweep_chain_on_degenerate_groups(gpu_cache, tmp_path, name):
    X, Y = C.case(name)
    f = C.write_jd(tmp_path, "chrA", X, Y)
    _, _, cuts, steps = pipe.runSweepFast([f], [500, 1000], [5], cut=C.CUT)
    assert cuts == _oracle_chain([(X, Y)], [500, 1000], [5], C.CUT)


def test_sweep_chain_two_chromosomes(gpu_cache, tmp_path):
    xys = [_synth(60000, 71), C.case("self_equal", seed=2)]
    fs = [C.write_jd(tmp_path, "chr%d" % k, X, Y) for k, (X, Y) in enumerate(xys)]
    _, _, cuts, steps = pipe.runSweepFast(fs, [500, 1000, 2000], [5], cut=0)
    assert cuts == _oracle_chain(xys, [500, 1000, 2000], [5], 0)
