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
import collections
import logging
import sys

import numpy as np

from . import balance
from .balance import BalanceArgs, balance_stats, balanced_state, check_args, fmt, format_balanced_matrix, not_converged, weights_over
from .matrix import CHUNK, cell_chunks, check_res, chrom_outputs, chroms_of, common, each_chrom, region_bins, region_records
from .peaks import write_outputs

logger = logging.getLogger("cloops_amd.expected")

SUFFIXES = ("_expected.txt", "_ps.txt", "_oe_cells.txt", "_expected.json", "_oe_matrix.txt")


class ExpectedArgs(collections.namedtuple("ExpectedArgs", "raw per_decade nosmooth")):
    """the three options of the expected values; the fields are the keywords of the jd2* and the keys of the json's `args` (`_asdict`)"""
    __slots__ = ()

    @classmethod
    def parsed(cls, op):
        """of a namespace with the options of add_options, unchecked"""
        return cls(op.raw, op.perdecade, op.nosmooth)


def check_perdecade(per_decade):
    """-> the groups per decade as an integer; ValueError unless it is one at or above 1"""
    if isinstance(per_decade, bool) or not isinstance(per_decade, (int, np.integer)) or per_decade < 1:
        raise ValueError("perdecade must be an integer at or above 1, got %r" % (per_decade,))
    return int(per_decade)


def check_exp_args(raw=False, per_decade=10, nosmooth=False):
    """-> ExpectedArgs of the three, checked by check_perdecade"""
    return ExpectedArgs(bool(raw), check_perdecade(per_decade), bool(nosmooth))


def options_of(bal=None, exp=None, **options):
    """the two records of a *_chrom -> (BalanceArgs, ExpectedArgs): those given, or made of their fields among the keywords"""
    if bal is None:
        bal = check_args(**{k: options.pop(k) for k in BalanceArgs._fields if k in options})
    if exp is None:
        exp = check_exp_args(**{k: options.pop(k) for k in ExpectedArgs._fields if k in options})
    if options:
        raise TypeError("unexpected keywords %s" % ", ".join(sorted(options)))
    return bal, exp


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


Expected = collections.namedtuple("Expected", "nd n_used n_pairs cnt_sum val_sum expected groups")


def expected_state(ch, st, bal, exp):
    """The sums per diagonal of the state `st` of balance.balanced_state (with `exp.raw`: of the counts over its mask), the expected
    values of them, set on the device -> Expected.  `bal`: BalanceArgs, `exp`: ExpectedArgs."""
    nd, n_used = ch.exp_diagonals(valid=st.mask, balanced=False) if exp.raw else ch.exp_diagonals()
    n_pairs, cnt_sum, val_sum = ch.exp_diagonals_get(0, nd)
    expected, groups = expected_of(n_pairs, val_sum, bal.ignore_diags, exp.per_decade, exp.nosmooth)
    ch.exp_set(expected)
    return Expected(nd, n_used, n_pairs, cnt_sum, val_sum, expected, groups)


def expected_chrom(ch, chrom, res, cut=0, region=None, chunk=CHUNK, **options):
    """One chromosome on the device: `ch` has the mat_*, bal_* and exp_* methods of api.Chromosome; region = (chrom, start, end) or None;
    `options`: the records bal= and exp= (options_of), or their fields as keywords
    -> dict(expected: text, ps: text, cells: text, stats: the json's entry, matrix: text or None)"""
    bal, exp = options_of(**options)
    try:
        st = balanced_state(ch, res, cut, bal, exp.raw)
        ew = np.where(st.mask, 1.0, np.nan) if exp.raw else ch.bal_weights(0, st.nb)
        ex = expected_state(ch, st, bal, exp)
        cells, first = [], 0
        for bx, by, cnt in cell_chunks(ch, st.n_cells, chunk):
            val = raw_values(bx, by, cnt, st.b0, ew) if exp.raw else ch.bal_cells_get(first, len(bx))
            cells.append(format_cells(chrom, res, bx, by, cnt, val, ch.exp_cells_get(first, len(bx))))
            first += len(bx)
        mat_text = None
        if region is not None:
            rb0, rn = region_bins(region[1], region[2], res)
            mat = ch.mat_window(res, rb0, rb0, rn, rn, cut=cut, mirror=True)[0]
            mat_text = format_balanced_matrix(chrom, res, rb0, rb0, oe_matrix(mat, weights_over(st.b0, ew, rb0, rn), ex.expected))
    finally:
        ch.mat_free()
    msg = not_converged(chrom, st, bal.tol, exp.raw)
    if msg is not None:
        logger.warning("WARNING: " + msg)
    stats = dict(balance_stats(st), b0=int(st.b0), nb=int(st.nb), nd=int(ex.nd), n_used=int(ex.n_used), n_valid=int(np.count_nonzero(~np.isnan(ew))))
    return {"expected": format_expected(chrom, res, ex.n_pairs, ex.cnt_sum, ex.val_sum, ex.expected), "ps": format_ps(chrom, res, ex.groups),
            "cells": "".join(cells), "stats": stats, "matrix": mat_text}


def expected_outputs(per_chrom, args):
    """{suffix: text} of the files from {chrom: expected_chrom's dict}, and the json's content"""
    return chrom_outputs(per_chrom, ((SUFFIXES[0], "expected"), (SUFFIXES[1], "ps"), (SUFFIXES[2], "cells")), SUFFIXES[3], {"args": args},
                         SUFFIXES[4])


def jd2expected(jd, fout, res=10000, cut=0, chroms=(), raw=False, per_decade=10, nosmooth=False, region=None, ignore_diags=2, min_nnz=10,
                min_count=0, mad_max=5, tol=1e-5, max_iters=200):
    """The expected values by distance and the O/E cells of every cis chromosome of `jd` -> `<fout>_expected.txt`, `<fout>_ps.txt`,
    `<fout>_oe_cells.txt`, `<fout>_expected.json` and, with `region`, `<fout>_oe_matrix.txt`; returns the json's content."""
    res, cut = check_res(res), int(cut)
    bal, exp = check_args(ignore_diags, min_nnz, min_count, mad_max, tol, max_iters), check_exp_args(raw, per_decade, nosmooth)
    rg, recs = region_records(jd, chroms, region, res, "process")
    per_chrom = each_chrom(recs, logger, "expected contacts by distance of %s",
                           lambda ch, chrom: expected_chrom(ch, chrom, res, cut, region=rg if rg is not None and rg[0] == chrom else None,
                                                            bal=bal, exp=exp))
    args = dict(bal._asdict(), res=res, cut=cut, region=None if rg is None else "%s:%d-%d" % rg, **exp._asdict())
    texts, js = expected_outputs(per_chrom, args)
    write_outputs(fout, texts)
    return js


def add_options(ap):
    """the three options of ExpectedArgs.parsed, then the six of balance.add_options"""
    ap.add_argument("-raw", dest="raw", required=False, action="store_true", help="The raw counts over the valid bins, without balancing.")
    ap.add_argument("-perdecade", dest="perdecade", required=False, default=10, type=int,
                    help="Groups of diagonals per decade of distance the expected value is averaged over, default 10.")
    ap.add_argument("-nosmooth", dest="nosmooth", required=False, action="store_true",
                    help="The expected value of a diagonal is its own average, not its group's.")
    balance.add_options(ap)


def parsed_options(op):
    """the nine keywords of a jd2* from a namespace with the options of add_options: the fields of the two records"""
    return dict(BalanceArgs.parsed(op)._asdict(), **ExpectedArgs.parsed(op)._asdict())


def help(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cloops_amd.expected",
                                 description="Expected contacts by distance (P(s)) and observed / expected cells on MI355X. "
                                             "For example: python -m cloops_amd.expected -d hic -o hic -res 10000")
    common(ap, 10000, chroms=True)
    ap.add_argument("-r", dest="region", required=False, default=None, type=str,
                    help="Also write the O/E matrix of this region, chrom:start-end, into <o>_oe_matrix.txt.")
    add_options(ap)
    return ap.parse_args(argv)


def main(argv=None):
    op = help(argv)
    jd2expected(op.d, op.output, res=op.res, cut=op.cut, chroms=chroms_of(op), region=op.region, **parsed_options(op))
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())


