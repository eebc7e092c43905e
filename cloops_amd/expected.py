"""Expected contacts by distance and observed / expected: per diagonal of a chromosome's contact matrix the number of valid bin pairs
and the sum of the (balanced) values of its cells -- the P(s) curve, what `cooltools expected-cis` computes -- the expected value of
every diagonal, the O/E value of every cell, and the O/E matrix of a region.

The reference has nothing of the kind.  The cells are K24's (`cl_mat_cells`, folded), the mask and the weights K25's (`balance.valid_bins`,
`cl_bal_iterate`); the pairs per diagonal, the sums per diagonal and the O/E of the cells run in kernel K26 over the cells resident in
HBM (`cl_exp_diagonals` / `cl_exp_diagonals_get` / `cl_exp_set` / `cl_exp_cells_get`).  The smoothing of the curve, the texts and the
files stay on the host.

Definitions (include/cloops_hip.h, cl_exp_diagonals):
- A bin is valid iff its ICE weight is a number (with `-raw`: iff the mask of `balance.valid_bins` holds it; its weight is then 1).  A
  cell is used iff by - bx >= ignore_diags and both of its bins are valid; its value is (w[bx] cnt) w[by].
- Per diagonal d: n_pairs = the valid bin pairs at that distance (0 below ignore_diags), count_sum / value_sum = the counts / the
  values of its used cells, value_avg = value_sum / n_pairs.
- Smoothing: the diagonals are grouped between the distinct integers ceil(10 ** (k / P)), k = 0, 1, .., P = `-perdecade`; diagonal 0
  is a group of its own.  A group's value is the sum of its value_sum over the sum of its n_pairs (NaN without pairs); expected[d] is
  its group's value, or value_avg[d] itself with `-nosmooth`; NaN below ignore_diags.
- O/E of a cell = value / expected[by - bx], NaN where the cell is not used or the expected value is NaN or 0.
- `<o>_expected.txt`: `chrom diag dist n_pairs count_sum value_sum value_avg expected` per diagonal with n_pairs > 0; `<o>_ps.txt`:
  `chrom dist_start dist_end n_pairs value_sum value_avg` per group; `<o>_oe_cells.txt`: K24's bg2 columns, the balanced value (with
  `-raw` the count where both bins are valid) and O/E; `<o>_expected.json`: per chromosome b0, nb, nd, n_used, n_valid and the
  balance statistics, and the arguments; with `-r` `<o>_oe_matrix.txt`: the mirrored window of the region times outer(w, w) over
  expected[|i - j|].  Floats as %.10g, NaN as nan.
"""
import argparse
import json
import logging
import sys

import numpy as np

from . import matrix
from .balance import _num, check_args, fmt, format_balanced_matrix, valid_bins, weights_over
from .matrix import CHUNK, check_res, parse_region, region_bins, window_fits
from .peaks import write_outputs

logger = logging.getLogger("cloops_amd.expected")

SUFFIXES = ("_expected.txt", "_ps.txt", "_oe_cells.txt", "_expected.json", "_oe_matrix.txt")


def check_perdecade(per_decade):
    """-> the groups per decade as an integer; ValueError unless it is one at or above 1"""
    if isinstance(per_decade, bool) or not isinstance(per_decade, (int, np.integer)) or per_decade < 1:
        raise ValueError("perdecade must be an integer at or above 1, got %r" % (per_decade,))
    return int(per_decade)


def group_bounds(nd, per_decade):
    """the bounds of the diagonal groups over [0, nd) -> int64, ascending: 0, then the distinct ceil(10 ** (k / P)) below nd, then nd;
    group g is [bounds[g], bounds[g + 1])"""
    nd, p = int(nd), check_perdecade(per_decade)
    if nd <= 0:
        return np.zeros(1, np.int64)
    out, k = [0], 0
    while True:
        e = 10 ** (k // p) if k % p == 0 else int(np.ceil(10.0 ** (k / float(p))))
        if e >= nd:
            break
        if e > out[-1]:
            out.append(e)
        k += 1
    out.append(nd)
    return np.array(out, np.int64)


def smooth(n_pairs, val_sum, per_decade):
    """-> (smoothed float64[nd]: the value of each diagonal's group, groups: (start, end, n_pairs, value_sum, value_avg) per group)"""
    n_pairs, val_sum = np.asarray(n_pairs, np.int64), np.asarray(val_sum, np.float64)
    nd = len(n_pairs)
    bounds = group_bounds(nd, per_decade)
    which = np.searchsorted(bounds, np.arange(nd, dtype=np.int64), side="right") - 1
    ng = len(bounds) - 1
    gp = np.zeros(ng, np.int64)
    np.add.at(gp, which, n_pairs)
    gv = np.bincount(which, val_sum, ng) if nd else np.zeros(0)
    avg = np.full(ng, np.nan)
    avg[gp > 0] = gv[gp > 0] / gp[gp > 0]
    groups = [(int(bounds[g]), int(bounds[g + 1]), int(gp[g]), float(gv[g]), float(avg[g])) for g in range(ng)]
    return (avg[which] if nd else np.zeros(0)), groups


def per_diagonal(n_pairs, val_sum):
    """value_avg: val_sum / n_pairs, NaN without pairs"""
    n_pairs, val_sum = np.asarray(n_pairs, np.int64), np.asarray(val_sum, np.float64)
    out = np.full(len(n_pairs), np.nan)
    has = n_pairs > 0
    out[has] = val_sum[has] / n_pairs[has]
    return out


def expected_of(n_pairs, val_sum, ignore_diags, per_decade=10, nosmooth=False):
    """-> (expected float64[nd], the groups of `smooth`): NaN below ignore_diags"""
    smoothed, groups = smooth(n_pairs, val_sum, per_decade)
    exp = per_diagonal(n_pairs, val_sum) if nosmooth else smoothed.copy()
    exp[:int(ignore_diags)] = np.nan
    return exp, groups


def format_expected(chrom, res, n_pairs, cnt_sum, val_sum, expected):
    """`<o>_expected.txt` of one chromosome: one line per diagonal with n_pairs > 0"""
    avg = per_diagonal(n_pairs, val_sum)
    return "".join("%s\t%d\t%d\t%d\t%d\t%s\t%s\t%s\n" % (chrom, d, d * res, p, c, fmt(v), fmt(a), fmt(e))
                   for d, (p, c, v, a, e) in enumerate(zip(np.asarray(n_pairs).tolist(), np.asarray(cnt_sum).tolist(), np.asarray(val_sum).tolist(),
                                                           avg.tolist(), np.asarray(expected).tolist())) if p > 0)


def format_ps(chrom, res, groups):
    """`<o>_ps.txt` of one chromosome: `chrom dist_start dist_end n_pairs value_sum value_avg` per group"""
    return "".join("%s\t%d\t%d\t%d\t%s\t%s\n" % (chrom, s * res, e * res, p, fmt(v), fmt(a)) for s, e, p, v, a in groups)


def format_cells(chrom, res, bx, by, cnt, val, oe):
    """`<o>_oe_cells.txt` of one chunk: the bg2 columns of matrix.format_cells, then the value and O/E"""
    bx, by = np.asarray(bx, np.int64), np.asarray(by, np.int64)
    return "".join("%s\t%d\t%d\t%s\t%d\t%d\t%d\t%s\t%s\n" % (chrom, x * res, (x + 1) * res, chrom, y * res, (y + 1) * res, c, fmt(v), fmt(q))
                   for x, y, c, v, q in zip(bx.tolist(), by.tolist(), np.asarray(cnt, np.int64).tolist(), np.asarray(val, np.float64).tolist(),
                                            np.asarray(oe, np.float64).tolist()))


def raw_values(bx, by, cnt, b0, ew):
    """the value of a cell without balancing: its count where both bins are valid (ew: 1 or NaN per bin), NaN elsewhere"""
    ew = np.asarray(ew, np.float64)
    return (ew[np.asarray(bx, np.int64) - b0] * np.asarray(cnt, np.float64)) * ew[np.asarray(by, np.int64) - b0]


def oe_matrix(mat, wr, expected):
    """the mirrored window `mat` (n x n) times outer(wr, wr) over expected[|i - j|]: NaN where the expected
    value is NaN, 0 or beyond the diagonals"""
    n = len(wr)
    d = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    e = np.full((n, n), np.nan)
    ok = d < len(expected)
    e[ok] = np.asarray(expected, np.float64)[d[ok]]
    e[e == 0] = np.nan
    return np.asarray(mat, np.float64) * np.outer(wr, wr) / e


def expected_chrom(ch, chrom, res, cut=0, ignore_diags=2, min_nnz=10, min_count=0, mad_max=5, tol=1e-5, max_iters=200, raw=False,
                   per_decade=10, nosmooth=False, region=None, chunk=CHUNK):
    """One chromosome on the device: `ch` has the mat_*, bal_* and exp_* methods of api.Chromosome; region = (chrom, start, end) or None
    -> dict(expected: text, ps: text, cells: text, stats: the json's entry, matrix: text or None)"""
    try:
        n_cells = ch.mat_cells(res, cut=cut, fold=True)[0]
        b0, nb, _ = ch.bal_marginals(ignore_diags)
        sum_, nnz = ch.bal_marginals_get(0, nb)
        valid = valid_bins(sum_, nnz, min_nnz, min_count, mad_max)
        if raw:
            iters, converged, var, scale = 0, False, float("nan"), float("nan")
            ew = np.where(valid, 1.0, np.nan)
            nd, n_used = ch.exp_diagonals(valid=valid, balanced=False)
        else:
            iters, converged, var, scale = ch.bal_iterate(valid, max_iters=max_iters, tol=tol)
            ew = ch.bal_weights(0, nb)
            nd, n_used = ch.exp_diagonals()
        n_pairs, cnt_sum, val_sum = ch.exp_diagonals_get(0, nd)
        exp, groups = expected_of(n_pairs, val_sum, ignore_diags, per_decade, nosmooth)
        ch.exp_set(exp)
        cells = []
        for first in range(0, int(n_cells), int(chunk)):
            k = min(int(chunk), int(n_cells) - first)
            bx, by, cnt = ch.mat_cells_get(first, k)
            val = raw_values(bx, by, cnt, b0, ew) if raw else ch.bal_cells_get(first, k)
            cells.append(format_cells(chrom, res, bx, by, cnt, val, ch.exp_cells_get(first, k)))
        mat_text = None
        if region is not None:
            rb0, rn = region_bins(region[1], region[2], res)
            mat = ch.mat_window(res, rb0, rb0, rn, rn, cut=cut, mirror=True)[0]
            mat_text = format_balanced_matrix(chrom, res, rb0, rb0, oe_matrix(mat, weights_over(b0, ew, rb0, rn), exp))
    finally:
        ch.mat_free()
    if not raw and nb > 0 and not converged:
        logger.warning("WARNING: %s did not converge in %d iterations (variance %s, tol %s)" % (chrom, iters, fmt(var), fmt(tol)))
    stats = {"b0": int(b0), "nb": int(nb), "nd": int(nd), "n_used": int(n_used), "n_valid": int(np.count_nonzero(~np.isnan(ew))),
             "iters": int(iters), "converged": bool(converged), "var": _num(var), "scale": _num(scale)}
    return {"expected": format_expected(chrom, res, n_pairs, cnt_sum, val_sum, exp), "ps": format_ps(chrom, res, groups),
            "cells": "".join(cells), "stats": stats, "matrix": mat_text}


def expected_outputs(per_chrom, args):
    """{suffix: text} of the files from {chrom: expected_chrom's dict}, and the json's content"""
    names = sorted(per_chrom)
    js = {"args": args, "chroms": {n: per_chrom[n]["stats"] for n in names}}
    texts = {SUFFIXES[0]: "".join(per_chrom[n]["expected"] for n in names), SUFFIXES[1]: "".join(per_chrom[n]["ps"] for n in names),
             SUFFIXES[2]: "".join(per_chrom[n]["cells"] for n in names), SUFFIXES[3]: json.dumps(js, indent=1, sort_keys=True) + "\n"}
    mats = [per_chrom[n]["matrix"] for n in names if per_chrom[n]["matrix"] is not None]
    if mats:
        texts[SUFFIXES[4]] = mats[0]
    return texts, js


def jd2expected(jd, fout, res=10000, cut=0, chroms=(), raw=False, per_decade=10, nosmooth=False, region=None, ignore_diags=2, min_nnz=10,
                min_count=0, mad_max=5, tol=1e-5, max_iters=200):
    """The expected values by distance and the O/E cells of every cis chromosome of `jd` -> `<fout>_expected.txt`, `<fout>_ps.txt`,
    `<fout>_oe_cells.txt`, `<fout>_expected.json` and, with `region`, `<fout>_oe_matrix.txt`; returns the json's content."""
    res, cut = check_res(res), int(cut)
    ignore_diags, min_nnz, min_count, mad_max, tol, max_iters = check_args(ignore_diags, min_nnz, min_count, mad_max, tol, max_iters)
    per_decade = check_perdecade(per_decade)
    rg = None if region is None else parse_region(region)
    if rg is not None and not window_fits(rg, rg, res):
        raise ValueError("the region needs more than %d bins a side or %d cells at -res %d; the smallest -res that fits is %d"
                         % (matrix.WMAX, matrix.CELLS_MAX, res, matrix.smallest_res(rg, rg)))
    recs = matrix._records(jd, chroms)
    if rg is not None and rg[0] not in [c for c, _ in recs]:
        raise ValueError("no cis .jd file of chromosome %s among those to process" % rg[0])
    per_chrom = {}
    for chrom, r in recs:
        logger.info("expected contacts by distance of %s" % chrom)
        with r.lock:
            per_chrom[chrom] = expected_chrom(r.chrom, chrom, res, cut, ignore_diags, min_nnz, min_count, mad_max, tol, max_iters, bool(raw),
                                              per_decade, bool(nosmooth), region=rg if rg is not None and rg[0] == chrom else None)
    args = {"res": res, "cut": cut, "raw": bool(raw), "per_decade": per_decade, "nosmooth": bool(nosmooth), "ignore_diags": ignore_diags,
            "min_nnz": min_nnz, "min_count": min_count, "mad_max": mad_max, "tol": tol, "max_iters": max_iters,
            "region": None if rg is None else "%s:%d-%d" % rg}
    texts, js = expected_outputs(per_chrom, args)
    write_outputs(fout, texts)
    return js


def help(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cloops_amd.expected",
                                 description="Expected contacts by distance (P(s)) and observed / expected cells on MI355X. "
                                             "For example: python -m cloops_amd.expected -d hic -o hic -res 10000")
    ap.add_argument("-d", dest="d", required=True, type=str, help="The directory of cis .jd files.")
    ap.add_argument("-o", dest="output", required=True, type=str, help="Output prefix.")
    ap.add_argument("-res", dest="res", required=False, default=10000, type=int, help="Bin size in bp, default 10000.")
    ap.add_argument("-cut", dest="cut", required=False, default=0, type=int, help="Distance cutoff to filter PETs, default 0.")
    ap.add_argument("-c", dest="chroms", required=False, default="", type=str,
                    help="Whether to process limited chroms, specify it as chr1,chr2,chr3, default is all.")
    ap.add_argument("-raw", dest="raw", required=False, action="store_true",
                    help="Expected values of the raw counts over the valid bins, without balancing.")
    ap.add_argument("-perdecade", dest="perdecade", required=False, default=10, type=int,
                    help="Groups of diagonals per decade of distance the expected value is averaged over, default 10.")
    ap.add_argument("-nosmooth", dest="nosmooth", required=False, action="store_true",
                    help="The expected value of a diagonal is its own average, not its group's.")
    ap.add_argument("-r", dest="region", required=False, default=None, type=str,
                    help="Also write the O/E matrix of this region, chrom:start-end, into <o>_oe_matrix.txt.")
    ap.add_argument("-ignorediags", dest="ignorediags", required=False, default=2, type=int,
                    help="Cells nearer the diagonal than this many bins take no part, default 2.")
    ap.add_argument("-minnnz", dest="minnnz", required=False, default=10, type=int, help="A bin needs this many non-empty cells, default 10.")
    ap.add_argument("-mincount", dest="mincount", required=False, default=0, type=int, help="A bin needs this many contacts, default 0.")
    ap.add_argument("-mad", dest="mad", required=False, default=5.0, type=float,
                    help="Bins whose log marginal lies more than this many median absolute deviations below the median are left out; "
                         "0 switches the filter off. Default 5.")
    ap.add_argument("-tol", dest="tol", required=False, default=1e-5, type=float, help="Variance of the marginals to stop at, default 1e-5.")
    ap.add_argument("-maxiters", dest="maxiters", required=False, default=200, type=int, help="Most iterations, default 200.")
    return ap.parse_args(argv)


def main(argv=None):
    op = help(argv)
    jd2expected(op.d, op.output, res=op.res, cut=op.cut, chroms=[] if op.chroms == "" else set(op.chroms.split(",")), raw=op.raw,
                per_decade=op.perdecade, nosmooth=op.nosmooth, region=op.region, ignore_diags=op.ignorediags, min_nnz=op.minnnz,
                min_count=op.mincount, mad_max=op.mad, tol=op.tol, max_iters=op.maxiters)
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())
