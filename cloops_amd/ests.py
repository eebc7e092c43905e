"""Distance-cutoff estimation between self-ligation and inter-ligation PETs.

Host-side restatement of cLoops/ests.py:36-61 (`estIntSelCutFrag`) -- the tiny float step
that closes the (eps, minPts) sweep chain of cLoops/pipe.py:247-275.  numpy float64, same
operations in the same order as the reference (abs, drop NaN, drop <= 0, log2, median +
3 sigma vs the sigma-weighted mean of the two means, take the smaller, 2**cut truncated)."""
import math

import numpy as np


def estFragSize(ds, top=500):
    """cLoops/ests.py:23-33: the fragment size behind `eps = 0` (pipe.py:237-239: eps = [2 * frags]) -- the median of the
    `top` most frequent distances between PETs mapped to different strands.  Same pandas calls as the reference (a
    Series of the distance counts, `sort_values(ascending=False)` with its default sort, the first `top` index values):
    which of several equally frequent distances make the cut is whatever pandas' sort does, here as there."""
    from collections import Counter
    import pandas as pd
    ds = pd.Series(Counter(ds))
    ds.sort_values(inplace=True, ascending=False)
    ds = ds[:top]
    return int(np.median(ds.index))


def estIntSelCutFrag(di, ds, log=1):
    """di: distances of PETs in inter-ligation clusters; ds: of self-ligation PETs.
    Returns (rcut, rfrags) as Python ints (ests.py:57,60)."""
    di = np.abs(np.asarray(di, dtype=np.float64))
    ds = np.abs(np.asarray(ds, dtype=np.float64))
    di = di[~np.isnan(di)]
    ds = ds[~np.isnan(ds)]
    di = di[di > 0]
    ds = ds[ds > 0]
    if log:
        di = np.log2(di)
        ds = np.log2(ds)
    ds_std, di_std = ds.std(), di.std()
    cut1 = np.median(ds) + 3 * ds_std
    cut2 = (ds.mean() * ds_std + di.mean() * di_std) / (ds_std + di_std)
    cut = min([cut1, cut2])
    rcut = int(2 ** cut)
    frags = np.median(ds)
    rfrags = int(2 ** frags)
    return rcut, rfrags


def estIntSelCutFrag_from_stats(n_pos, sumlog, sqdev, median_pair, with_margin=False):
    """The same estimator from pre-reduced statistics (cl_dist_summary / cl_dist_bin_hist
    of the GPU library) instead of the raw distance lists:
      n_pos      [inter, self]  number of non-zero distances
      sumlog     [inter, self]  sum of log2|d|
      sqdev      [inter, self]  sum of (log2|d| - mean)^2
      median_pair (lo, hi)      the two middle order statistics of the self-group |d| (equal for odd n)
    Same formulas, same order of operations as ests.py:49-60; only the summation order inside
    mean / std differs from numpy's pairwise sums (the result is truncated to int)."""
    di_mean = sumlog[0] / n_pos[0]
    ds_mean = sumlog[1] / n_pos[1]
    # (a one-pass sqdev of a group of (nearly) equal distances cancels to rounding noise, which can be negative: the
    #  reference's std is then 0 or tiny, never NaN)
    di_std = np.sqrt(max(float(sqdev[0]), 0.0) / n_pos[0])
    ds_std = np.sqrt(max(float(sqdev[1]), 0.0) / n_pos[1])
    ds_median = _median_log2(median_pair)
    cut = _cut_of(ds_median, ds_mean, ds_std, di_mean, di_std)
    rcut = int(2 ** cut)
    rfrags = int(2 ** ds_median)
    if with_margin:
        # distance of 2**cut from the nearest integer: the sums behind `cut` are reduced in a different order
        # than numpy's pairwise sums, so a value this close to an integer could truncate differently
        raw = float(2 ** cut)
        return rcut, rfrags, abs(raw - round(raw))
    return rcut, rfrags


def _median_log2(median_pair):
    lo, hi = median_pair
    return (np.log2(np.float64(lo)) + np.log2(np.float64(hi))) / 2 if lo != hi else np.log2(np.float64(lo))


def _cut_of(ds_median, ds_mean, ds_std, di_mean, di_std):
    """ests.py:53-55 on scalars.  Both stds 0 make cut2 0/0 = NaN; min([cut1, nan]) is cut1, as in the reference"""
    with np.errstate(invalid="ignore", divide="ignore"):
        cut1 = ds_median + 3 * ds_std
        cut2 = (ds_mean * ds_std + di_mean * di_std) / (ds_std + di_std)
    return min([cut1, cut2])


#: unit roundoff of float64
_U = 2.0 ** -53
#: bound on the error of one term x = log2|d| - xshift, against the exact value, of the library's k7_log2 (a few ulp of
#: log2 d < 31) and of numpy's log2 alike: 16 ulp of a number in [16, 32)
LOG2_TERM_ERR = 16 * 2.0 ** -48
#: every K7 reduction spreads its terms over at least this many threads, each summing its share in order (cl_chrom.h:
#: the step's k7_summary runs K7_STEP_BLOCKS x K7_STEP_THREADS = 262144, cl_dist_summary K7_BLOCKS x TPB = 524288;
#: 4x below the smaller as a margin)
K7_MIN_THREADS = 65536
#: additions behind one thread's partial sum that do not depend on n: 6 wave shuffles, 16 waves, 8 partials per thread
#: of k7_reduce_parts, its 8-level tree -- and numpy's pairwise sums (at most ~64 levels)
K7_FIXED_DEPTH = 64


def stats_error_bounds(n_terms, n_pos, sumx, sumxx, n_parts=1):
    """Bounds on the error of what the cut is made of, for ONE group: (mean, std) of log2|d| from the reduced sums
    sum x, sum x^2 (x = log2|d| - xshift) against the values numpy computes from the lists.

    The error of a recursive sum of m terms is at most (m - 1) u sum|t| (u = 2^-53); a K7 reduction adds a thread's
    ceil(n_terms / K7_MIN_THREADS) terms in order, then K7_FIXED_DEPTH levels of partials, then the host adds
    `n_parts` partials (chromosomes, ranks).  sum |x| <= sqrt(n sum x^2).  The per-term error of the log2 itself
    (ours and numpy's, LOG2_TERM_ERR each) moves a mean and a standard deviation by at most that much (centring is a
    projection: |std(x) - std(x')| <= max |x_i - x'_i|).  numpy's own mean / std carry at most ~64 u relative.

    -> (err_sumlog, sq_lo, sq_hi, err_std_abs): |sum log2 - sum_ref| <= err_sumlog, the sum of squared deviations of the
    computed terms lies in [sq_lo, sq_hi] (sq_lo >= 0), and std_ref is within err_std_abs + 64 u std of sqrt(sq / n)."""
    n = float(n_pos)
    depth = -(-int(n_terms) // K7_MIN_THREADS) + K7_FIXED_DEPTH + int(n_parts)
    g = depth * _U / (1.0 - depth * _U)
    sxx = max(float(sumxx), 0.0)
    ax = math.sqrt(n * sxx) * (1 + 1e-6)                     # >= sum |x|
    e_sx = g * ax
    e_sxx = (g + _U) * sxx                                   # (+ the rounding of each w x * x)
    sx = float(sumx)
    sq = sxx - sx * sx / n
    e_sq = e_sxx + (2 * abs(sx) * e_sx + e_sx * e_sx) / n + 4 * _U * (sxx + sx * sx / n)
    return e_sx, max(sq - e_sq, 0.0), max(sq + e_sq, 0.0), 2 * LOG2_TERM_ERR


def estIntSelCutFrag_bounded(n_all, n_pos, sumx, sumxx, xshift, median_pair, n_parts=1):
    """estIntSelCutFrag_from_stats on the raw reduced sums (cl_dist_summary / the sweep step), with a guaranteed range:
    -> (rcut, rfrags, (rcut_lo, rcut_hi), margin), where int(2 ** cut) of the reference's estIntSelCutFrag on the same
    distance lists lies in [rcut_lo, rcut_hi] (stats_error_bounds, carried through ests.py:53-57 by evaluating the
    formula at the corners of the box of possible (means, stds) -- it is monotone in each of them).  rcut_lo == rcut_hi:
    the statistics settle the cut; otherwise only the lists can (pipe.runSweepFast's recheck).  margin = |2**cut - nearest
    integer| of the point estimate (estIntSelCutFrag_from_stats).
    n_all / n_pos / sumx / sumxx: [inter, self] as in cl_dsummary."""
    n_terms = int(n_all[0]) + int(n_all[1])
    mean_c, mean_r, std_r = [], [], []
    for g in (0, 1):
        n = float(n_pos[g])
        sumlog = float(sumx[g]) + xshift * n_pos[g]
        e_sx, sq_lo, sq_hi, e_t = stats_error_bounds(n_terms, n_pos[g], sumx[g], sumxx[g], n_parts)
        e_m = (e_sx + 2 * _U * abs(sumlog)) / n + e_t + 64 * _U * abs(sumlog) / n
        m = sumlog / n
        mean_c.append(m)
        mean_r.append((m - e_m, m + e_m))
        s_lo, s_hi = math.sqrt(sq_lo / n), math.sqrt(sq_hi / n)
        std_r.append((max(s_lo * (1 - 64 * _U) - e_t - e_m, 0.0), s_hi * (1 + 64 * _U) + e_t + e_m))
    sq_c = [float(sumxx[g]) - float(sumx[g]) ** 2 / n_pos[g] for g in (0, 1)]
    rcut, rfrags, margin = estIntSelCutFrag_from_stats(n_pos, [float(sumx[g]) + xshift * n_pos[g] for g in (0, 1)], sq_c, median_pair,
                                                       with_margin=True)
    med = float(_median_log2(median_pair))
    e_med = 4 * _U * abs(med)
    # cut = min(cut1, cut2): cut1 rises with ds_std; cut2 is a weighted mean of the two means -- linear in each mean,
    # monotone in each std.  The lower bound is the least of both over the corners, the upper the smaller of their maxima
    # (cut2 = NaN where both stds are 0: the reference then takes cut1)
    c1 = [med + s * 3 + e for s in std_r[1] for e in (-e_med, e_med)]
    c2, c2_nan = [], False
    for ms in mean_r[1]:
        for mi in mean_r[0]:
            for ss in std_r[1]:
                for si in std_r[0]:
                    if ss + si > 0:
                        c2.append((ms * ss + mi * si) / (ss + si))
                    else:
                        c2_nan = True
                        c2 += [min(ms, mi), max(ms, mi)]               # (both stds tiny: any weighting of the means)
    lo = min(min(c1), min(c2))
    hi = max(c1) if c2_nan else min(max(c1), max(c2))
    lo -= 8 * _U * abs(lo) + 1e-300
    hi += 8 * _U * abs(hi) + 1e-300
    return rcut, rfrags, (int(2 ** lo), int(2 ** hi)), margin


# ---- the log-binned first level of the exact median (cl_dist_summary of include/cloops_hip.h) -----------------
def logbin(d):
    """bin of a distance d >= 1: floor(log2 d) * 128 + the 7 bits below the leading one (monotone in d)"""
    d = int(d)
    e = d.bit_length() - 1
    m = ((d >> (e - 7)) if e >= 7 else (d << (7 - e))) & 127
    return e * 128 + m


def logbin_range(b):
    """[lo, hi) of the distances that fall into log bin b"""
    e, m = divmod(int(b), 128)
    if e >= 7:
        return (128 + m) << (e - 7), (128 + m + 1) << (e - 7)
    lo = (128 + m) >> (7 - e)
    return lo, lo + 1
