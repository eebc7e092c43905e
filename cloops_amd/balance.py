"""Matrix balancing: one weight per bin of a chromosome's contact matrix (iterative correction, ICE, Imakaev 2012 -- what `cooler
balance` does), the balanced value of every cell, and the balanced matrix of a region.

The reference has nothing of the kind.  The cells are K24's (`cl_mat_cells`, folded); the marginals and the iteration run in kernel
K25 over the cells resident in HBM (`cl_bal_marginals` / `cl_bal_iterate` / `cl_bal_weights_get` / `cl_bal_cells_get`).  The mask of
the bins, the texts and the files stay on the host.

Definitions (include/cloops_hip.h, cl_bal_marginals):
- Bins b0 .. b0 + nb - 1: from the first cell's bx to the largest by.  A cell is used iff by - bx >= ignore_diags.
- sum / nnz of a bin: the counts / the number of the used cells that touch it (the full symmetric matrix's row).
- A bin is valid iff nnz >= min_nnz, sum >= max(1, min_count) and, with mad_max > 0, log(sum) >= med - mad_max mad over the bins with
  sum > 0 (med: the median of log(sum), mad: the median of |log(sum) - med|).
- w = 1 on the valid bins; each iteration divides w by the bin's weighted marginal over their mean, until the variance of those
  ratios falls below tol.  weight = w / sqrt(the last mean), NaN on the other bins; balanced = count weight[bx] weight[by].
- `<o>_balance.txt`: `chrom start end sum nnz weight` per bin; `<o>_balanced_cells.txt`: K24's bg2 columns and the balanced value;
  `<o>_balance.json`: per chromosome b0, nb, n_used, n_valid, iters, converged, var, scale, and the arguments; with `-r`
  `<o>_balanced_matrix.txt`: the mirrored window of the region times outer(weight, weight).  Floats as %.10g, NaN as nan.
- A chromosome that does not converge within max_iters is reported with a warning and `converged: false`, not dropped.
"""
import argparse
import json
import logging
import sys

import numpy as np

from . import matrix
from .matrix import CHUNK, bin_label, check_res, parse_region, region_bins, window_fits
from .peaks import write_outputs

logger = logging.getLogger("cloops_amd.balance")

SUFFIXES = ("_balance.txt", "_balanced_cells.txt", "_balance.json", "_balanced_matrix.txt")
FLOAT = "%.10g"


def fmt(v):
    v = float(v)
    return "nan" if v != v else FLOAT % v


def valid_bins(sum_, nnz, min_nnz=10, min_count=0, mad_max=5):
    """the bins that take part in the iteration -> bool[nb]"""
    s, z = np.asarray(sum_).astype(np.float64), np.asarray(nnz).astype(np.int64)
    ok = (z >= int(min_nnz)) & (s >= max(1, int(min_count)))
    pos = s > 0
    if mad_max > 0 and pos.any():
        ls = np.log(s[pos])
        med = np.median(ls)
        mad = np.median(np.abs(ls - med))
        keep = np.zeros(len(s), bool)
        keep[pos] = ls >= med - float(mad_max) * mad
        ok &= keep
    return ok


def check_args(ignore_diags, min_nnz, min_count, mad_max, tol, max_iters):
    """-> the six as numbers; ValueError for one that cl_bal_* or the mask would refuse"""
    try:
        ignore_diags, min_nnz, min_count, max_iters = int(ignore_diags), int(min_nnz), int(min_count), int(max_iters)
        mad_max, tol = float(mad_max), float(tol)
    except (TypeError, ValueError):
        raise ValueError("ignorediags, minnnz, mincount and maxiters must be integers, mad and tol numbers")
    if ignore_diags < 0 or ignore_diags >= (1 << 31):
        raise ValueError("ignorediags must lie in [0, 2^31), got %d" % ignore_diags)
    if min_nnz < 0 or min_count < 0:
        raise ValueError("minnnz and mincount must not be negative, got %d and %d" % (min_nnz, min_count))
    if not mad_max >= 0:
        raise ValueError("mad must be a number at or above 0 (0: no such filter), got %r" % mad_max)
    if not tol >= 0:
        raise ValueError("tol must be a number at or above 0, got %r" % tol)
    if max_iters < 0 or max_iters >= (1 << 31):
        raise ValueError("maxiters must lie in [0, 2^31), got %d" % max_iters)
    return ignore_diags, min_nnz, min_count, mad_max, tol, max_iters


def format_bins(chrom, res, b0, sum_, nnz, weight):
    """`<o>_balance.txt` of one chromosome: `chrom start end sum nnz weight`"""
    return "".join("%s\t%d\t%d\t%d\t%d\t%s\n" % (chrom, (b0 + k) * res, (b0 + k + 1) * res, s, z, fmt(w))
                   for k, (s, z, w) in enumerate(zip(np.asarray(sum_).tolist(), np.asarray(nnz).tolist(), np.asarray(weight).tolist())))


def format_cells(chrom, res, bx, by, cnt, bal):
    """`<o>_balanced_cells.txt` of one chunk: the bg2 columns of matrix.format_cells, then the balanced value"""
    bx, by = np.asarray(bx, np.int64), np.asarray(by, np.int64)
    return "".join("%s\t%d\t%d\t%s\t%d\t%d\t%d\t%s\n" % (chrom, x * res, (x + 1) * res, chrom, y * res, (y + 1) * res, c, fmt(v))
                   for x, y, c, v in zip(bx.tolist(), by.tolist(), np.asarray(cnt, np.int64).tolist(), np.asarray(bal, np.float64).tolist()))


def format_balanced_matrix(chrom, res, bx0, by0, mat):
    """`<o>_balanced_matrix.txt`: the labels of matrix.format_matrix around floats"""
    mat = np.asarray(mat, np.float64)
    lines = ["\t" + "\t".join(bin_label(chrom, by0 + j, res) for j in range(mat.shape[1]))]
    for i in range(mat.shape[0]):
        lines.append(bin_label(chrom, bx0 + i, res) + "\t" + "\t".join(fmt(v) for v in mat[i].tolist()))
    return "\n".join(lines) + "\n"


def weights_over(b0, weight, first, n):
    """the weights of the bins [first, first + n): NaN outside [b0, b0 + len(weight))"""
    out = np.full(int(n), np.nan)
    lo, hi = max(int(first), int(b0)), min(int(first) + int(n), int(b0) + len(weight))
    if lo < hi:
        out[lo - first:hi - first] = np.asarray(weight)[lo - b0:hi - b0]
    return out


def _num(v):
    """a float of the json: the ten digits of the texts, None for NaN"""
    v = float(v)
    return None if v != v else float(FLOAT % v)


def balance_chrom(ch, chrom, res, cut=0, ignore_diags=2, min_nnz=10, min_count=0, mad_max=5, tol=1e-5, max_iters=200, region=None,
                  chunk=CHUNK):
    """One chromosome on the device: `ch` has the mat_* and bal_* methods of api.Chromosome; region = (chrom, start, end) or None
    -> dict(bins: text, cells: text, stats: the json's entry, matrix: text or None)"""
    try:
        n_cells = ch.mat_cells(res, cut=cut, fold=True)[0]
        b0, nb, n_used = ch.bal_marginals(ignore_diags)
        sum_, nnz = ch.bal_marginals_get(0, nb)
        valid = valid_bins(sum_, nnz, min_nnz, min_count, mad_max)
        iters, converged, var, scale = ch.bal_iterate(valid, max_iters=max_iters, tol=tol)
        weight = ch.bal_weights(0, nb)
        cells = []
        for first in range(0, int(n_cells), int(chunk)):
            k = min(int(chunk), int(n_cells) - first)
            bx, by, cnt = ch.mat_cells_get(first, k)
            cells.append(format_cells(chrom, res, bx, by, cnt, ch.bal_cells_get(first, k)))
        mat_text = None
        if region is not None:
            rb0, rn = region_bins(region[1], region[2], res)
            mat = ch.mat_window(res, rb0, rb0, rn, rn, cut=cut, mirror=True)[0]
            wr = weights_over(b0, weight, rb0, rn)
            mat_text = format_balanced_matrix(chrom, res, rb0, rb0, np.asarray(mat, np.float64) * np.outer(wr, wr))
    finally:
        ch.mat_free()
    if nb > 0 and not converged:
        logger.warning("WARNING: %s did not converge in %d iterations (variance %s, tol %s)" % (chrom, iters, fmt(var), fmt(tol)))
    stats = {"b0": int(b0), "nb": int(nb), "n_used": int(n_used), "n_valid": int(np.count_nonzero(valid)), "iters": int(iters),
             "converged": bool(converged), "var": _num(var), "scale": _num(scale)}
    return {"bins": format_bins(chrom, res, b0, sum_, nnz, weight), "cells": "".join(cells), "stats": stats, "matrix": mat_text}


def balance_outputs(per_chrom, args):
    """{suffix: text} of the files from {chrom: balance_chrom's dict}, and the json's content"""
    names = sorted(per_chrom)
    js = {"args": args, "chroms": {n: per_chrom[n]["stats"] for n in names}}
    texts = {SUFFIXES[0]: "".join(per_chrom[n]["bins"] for n in names), SUFFIXES[1]: "".join(per_chrom[n]["cells"] for n in names),
             SUFFIXES[2]: json.dumps(js, indent=1, sort_keys=True) + "\n"}
    mats = [per_chrom[n]["matrix"] for n in names if per_chrom[n]["matrix"] is not None]
    if mats:
        texts[SUFFIXES[3]] = mats[0]
    return texts, js


def jd2balance(jd, fout, res=10000, cut=0, chroms=(), ignore_diags=2, min_nnz=10, min_count=0, mad_max=5, tol=1e-5, max_iters=200,
               region=None):
    """The weights and balanced cells of every cis chromosome of `jd` -> `<fout>_balance.txt`, `<fout>_balanced_cells.txt`,
    `<fout>_balance.json` and, with `region`, `<fout>_balanced_matrix.txt`; returns the json's content."""
    res, cut = check_res(res), int(cut)
    ignore_diags, min_nnz, min_count, mad_max, tol, max_iters = check_args(ignore_diags, min_nnz, min_count, mad_max, tol, max_iters)
    rg = None if region is None else parse_region(region)
    if rg is not None and not window_fits(rg, rg, res):
        raise ValueError("the region needs more than %d bins a side or %d cells at -res %d; the smallest -res that fits is %d"
                         % (matrix.WMAX, matrix.CELLS_MAX, res, matrix.smallest_res(rg, rg)))
    recs = matrix._records(jd, chroms)
    if rg is not None and rg[0] not in [c for c, _ in recs]:
        raise ValueError("no cis .jd file of chromosome %s among those to balance" % rg[0])
    per_chrom = {}
    for chrom, r in recs:
        logger.info("balancing the contact matrix of %s" % chrom)
        with r.lock:
            per_chrom[chrom] = balance_chrom(r.chrom, chrom, res, cut, ignore_diags, min_nnz, min_count, mad_max, tol, max_iters,
                                             region=rg if rg is not None and rg[0] == chrom else None)
    args = {"res": res, "cut": cut, "ignore_diags": ignore_diags, "min_nnz": min_nnz, "min_count": min_count, "mad_max": mad_max, "tol": tol,
            "max_iters": max_iters, "region": None if rg is None else "%s:%d-%d" % rg}
    texts, js = balance_outputs(per_chrom, args)
    write_outputs(fout, texts)
    return js


def help(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cloops_amd.balance",
                                 description="Balanced contact matrices (iterative correction) on MI355X. "
                                             "For example: python -m cloops_amd.balance -d hic -o hic -res 10000")
    ap.add_argument("-d", dest="d", required=True, type=str, help="The directory of cis .jd files.")
    ap.add_argument("-o", dest="output", required=True, type=str, help="Output prefix.")
    ap.add_argument("-res", dest="res", required=False, default=10000, type=int, help="Bin size in bp, default 10000.")
    ap.add_argument("-cut", dest="cut", required=False, default=0, type=int, help="Distance cutoff to filter PETs, default 0.")
    ap.add_argument("-c", dest="chroms", required=False, default="", type=str,
                    help="Whether to process limited chroms, specify it as chr1,chr2,chr3, default is all.")
    ap.add_argument("-ignorediags", dest="ignorediags", required=False, default=2, type=int,
                    help="Cells nearer the diagonal than this many bins take no part in the balancing, default 2.")
    ap.add_argument("-minnnz", dest="minnnz", required=False, default=10, type=int, help="A bin needs this many non-empty cells, default 10.")
    ap.add_argument("-mincount", dest="mincount", required=False, default=0, type=int, help="A bin needs this many contacts, default 0.")
    ap.add_argument("-mad", dest="mad", required=False, default=5.0, type=float,
                    help="Bins whose log marginal lies more than this many median absolute deviations below the median are left out; "
                         "0 switches the filter off. Default 5.")
    ap.add_argument("-tol", dest="tol", required=False, default=1e-5, type=float, help="Variance of the marginals to stop at, default 1e-5.")
    ap.add_argument("-maxiters", dest="maxiters", required=False, default=200, type=int, help="Most iterations, default 200.")
    ap.add_argument("-r", dest="region", required=False, default=None, type=str,
                    help="Also write the balanced matrix of this region, chrom:start-end, into <o>_balanced_matrix.txt.")
    return ap.parse_args(argv)


def main(argv=None):
    op = help(argv)
    jd2balance(op.d, op.output, res=op.res, cut=op.cut, chroms=[] if op.chroms == "" else set(op.chroms.split(",")),
               ignore_diags=op.ignorediags, min_nnz=op.minnnz, min_count=op.mincount, mad_max=op.mad, tol=op.tol, max_iters=op.maxiters,
               region=op.region)
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())
