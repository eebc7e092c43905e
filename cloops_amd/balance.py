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
import collections
import logging
import sys

import numpy as np

from .matrix import CHUNK, bin_label, cell_chunks, check_res, chrom_outputs, chroms_of, common, each_chrom, region_bins, region_records
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


class BalanceArgs(collections.namedtuple("BalanceArgs", "ignore_diags min_nnz min_count mad_max tol max_iters")):
    """the six balancing options; the fields are the keywords of the jd2* and the keys of the json's `args` (`_asdict`)"""
    __slots__ = ()

    @classmethod
    def parsed(cls, op):
        """of a namespace with the options of add_options, unchecked"""
        return cls(op.ignorediags, op.minnnz, op.mincount, op.mad, op.tol, op.maxiters)


def check_args(ignore_diags=2, min_nnz=10, min_count=0, mad_max=5, tol=1e-5, max_iters=200):
    """-> BalanceArgs of the six as numbers; ValueError for one that cl_bal_* or the mask would refuse"""
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
    return BalanceArgs(ignore_diags, min_nnz, min_count, mad_max, tol, max_iters)


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


Balanced = collections.namedtuple("Balanced", "n_cells b0 nb n_used sum nnz mask iters converged var scale")


def balanced_state(ch, res, cut, bal, raw=False):
    """The folded cells of a chromosome, their marginals, the mask of the bins and -- unless `raw` -- the iteration, left on the device
    -> Balanced.  `bal`: BalanceArgs.  The weights are not fetched (bal_weights); the caller's `finally` has the mat_free."""
    n_cells = ch.mat_cells(res, cut=cut, fold=True)[0]
    b0, nb, n_used = ch.bal_marginals(bal.ignore_diags)
    sum_, nnz = ch.bal_marginals_get(0, nb)
    mask = valid_bins(sum_, nnz, bal.min_nnz, bal.min_count, bal.mad_max)
    result = (0, False, float("nan"), float("nan")) if raw else ch.bal_iterate(mask, max_iters=bal.max_iters, tol=bal.tol)
    return Balanced(n_cells, b0, nb, n_used, sum_, nnz, mask, *result)


def not_converged(chrom, st, tol, raw=False, num=fmt):
    """the warning of a chromosome whose iteration stopped at max_iters, None for any other; `num` writes its two floats"""
    if raw or st.nb == 0 or st.converged:
        return None
    return "%s did not converge in %d iterations (variance %s, tol %s)" % (chrom, st.iters, num(st.var), num(tol))


def balance_stats(st):
    """the four statistics of the iteration in a chromosome's entry of the json"""
    return {"iters": int(st.iters), "converged": bool(st.converged), "var": _num(st.var), "scale": _num(st.scale)}


def balance_chrom(ch, chrom, res, cut=0, region=None, chunk=CHUNK, bal=None, **options):
    """One chromosome on the device: `ch` has the mat_* and bal_* methods of api.Chromosome; region = (chrom, start, end) or None;
    `bal`: BalanceArgs, or its fields as keywords -> dict(bins: text, cells: text, stats: the json's entry, matrix: text or None)"""
    bal = check_args(**options) if bal is None else bal
    try:
        st = balanced_state(ch, res, cut, bal)
        weight = ch.bal_weights(0, st.nb)
        cells, first = [], 0
        for bx, by, cnt in cell_chunks(ch, st.n_cells, chunk):
            cells.append(format_cells(chrom, res, bx, by, cnt, ch.bal_cells_get(first, len(bx))))
            first += len(bx)
        mat_text = None
        if region is not None:
            rb0, rn = region_bins(region[1], region[2], res)
            mat = ch.mat_window(res, rb0, rb0, rn, rn, cut=cut, mirror=True)[0]
            wr = weights_over(st.b0, weight, rb0, rn)
            mat_text = format_balanced_matrix(chrom, res, rb0, rb0, np.asarray(mat, np.float64) * np.outer(wr, wr))
    finally:
        ch.mat_free()
    msg = not_converged(chrom, st, bal.tol)
    if msg is not None:
        logger.warning("WARNING: " + msg)
    stats = dict(balance_stats(st), b0=int(st.b0), nb=int(st.nb), n_used=int(st.n_used), n_valid=int(np.count_nonzero(st.mask)))
    return {"bins": format_bins(chrom, res, st.b0, st.sum, st.nnz, weight), "cells": "".join(cells), "stats": stats, "matrix": mat_text}


def balance_outputs(per_chrom, args):
    """{suffix: text} of the files from {chrom: balance_chrom's dict}, and the json's content"""
    return chrom_outputs(per_chrom, ((SUFFIXES[0], "bins"), (SUFFIXES[1], "cells")), SUFFIXES[2], {"args": args}, SUFFIXES[3])


def jd2balance(jd, fout, res=10000, cut=0, chroms=(), ignore_diags=2, min_nnz=10, min_count=0, mad_max=5, tol=1e-5, max_iters=200,
               region=None):
    """The weights and balanced cells of every cis chromosome of `jd` -> `<fout>_balance.txt`, `<fout>_balanced_cells.txt`,
    `<fout>_balance.json` and, with `region`, `<fout>_balanced_matrix.txt`; returns the json's content."""
    res, cut = check_res(res), int(cut)
    bal = check_args(ignore_diags, min_nnz, min_count, mad_max, tol, max_iters)
    rg, recs = region_records(jd, chroms, region, res, "balance")
    per_chrom = each_chrom(recs, logger, "balancing the contact matrix of %s",
                           lambda ch, chrom: balance_chrom(ch, chrom, res, cut, region=rg if rg is not None and rg[0] == chrom else None, bal=bal))
    args = dict(bal._asdict(), res=res, cut=cut, region=None if rg is None else "%s:%d-%d" % rg)
    texts, js = balance_outputs(per_chrom, args)
    write_outputs(fout, texts)
    return js


def add_options(ap):
    """the six options of BalanceArgs.parsed"""
    ap.add_argument("-ignorediags", dest="ignorediags", required=False, default=2, type=int,
                    help="Cells nearer the diagonal than this many bins take no part, default 2.")
    ap.add_argument("-minnnz", dest="minnnz", required=False, default=10, type=int, help="A bin needs this many non-empty cells, default 10.")
    ap.add_argument("-mincount", dest="mincount", required=False, default=0, type=int, help="A bin needs this many contacts, default 0.")
    ap.add_argument("-mad", dest="mad", required=False, default=5.0, type=float,
                    help="Bins whose log marginal lies more than this many median absolute deviations below the median are left out; "
                         "0 switches the filter off. Default 5.")
    ap.add_argument("-tol", dest="tol", required=False, default=1e-5, type=float, help="Variance of the marginals to stop at, default 1e-5.")
    ap.add_argument("-maxiters", dest="maxiters", required=False, default=200, type=int, help="Most iterations of the balancing, default 200.")


def help(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cloops_amd.balance",
                                 description="Balanced contact matrices (iterative correction) on MI355X. "
                                             "For example: python -m cloops_amd.balance -d hic -o hic -res 10000")
    common(ap, 10000, chroms=True)
    add_options(ap)
    ap.add_argument("-r", dest="region", required=False, default=None, type=str,
                    help="Also write the balanced matrix of this region, chrom:start-end, into <o>_balanced_matrix.txt.")
    return ap.parse_args(argv)


def main(argv=None):
    op = help(argv)
    jd2balance(op.d, op.output, res=op.res, cut=op.cut, chroms=chroms_of(op), region=op.region, **BalanceArgs.parsed(op)._asdict())
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())
