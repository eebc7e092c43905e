"""PETs at loop anchors for browser tracks: scripts/jd2cleanWashuPETs.py, function for function.

The script merges the anchors of the loops pairwise until nothing merges (quadratic in the anchor count), builds dicts of
row lists for every coordinate and collects the rows with an end in a merged anchor in a Python set.  Here the merge is a
sort and a sweep, and the membership test of every PET is kernel K13 on the chromosome resident in HBM
(`cl_anchor_mask`): it returns one bit per row, and the rows come from the mask in ascending order.  Each output
`<o>/<chrA>-<chrB>.jd` holds those rows of the chromosome's `parseJd` matrix, same columns and dtype, written with
`joblib.dump`, so `pipe.parseJd`, `pipe.CACHE` and the other modules read it back unchanged.

Semantics pinned:
- `preDs` reads the anchors from the columns named `iva` / `ivb` of the header, else 6 / 7 (quant._anchor_columns; the
  script reads 6 / 7, which hold `FDR` and the hypergeometric p-value in the `.loop` files this project writes).
- A loop is skipped when float(last column) < 1 unless `sig` is False (`-s`); a repeated loopId replaces the earlier one;
  loops are filed under iva's chromosome; a chromosome without loops, or whose `.jd` is missing (a warning), is dropped.
- Both anchors of every loop of a chromosome go into one pool, merged where they overlap or share an endpoint; a PET is
  kept when X or Y lies in a merged anchor, closed on both ends.
- Deviation: rows are written in ascending row order.  The script writes `mat[list(ps)]`, in CPython's set-table order
  (ascending whenever the table is larger than the largest row index).  The row set is the same.
- No chromosome left: the summary's ratio m / n raises ZeroDivisionError, as the script does (after `-o` was created).
"""
import argparse
import logging
import os
import sys

import numpy as np

from .cModel import parseIv
from .quant import _anchor_columns

logger = logging.getLogger("cloops_amd.cleanpets")


def preDs(f, d, sig=True, chroms=[], ivac=None, ivbc=None):
    """scripts/jd2cleanWashuPETs.py:92-126: the loops of the `.loop` file `f` (only the significant ones when `sig`) per
    chromosome of iva, with the `<chrom>-<chrom>.jd` of directory `d` -> {chrom: {"rs": {loopId: [c, s, e, c, s, e]}, "f": path}}.
    `ivac` / `ivbc` None: the anchor columns are found by header name (module docstring)."""
    ivac, ivbc = _anchor_columns(f, ivac, ivbc)
    records = {}
    if len(chroms) > 0:
        for c in chroms:
            records[c] = {"rs": {}, "f": ""}
    for i, line in enumerate(open(f)):
        if i == 0:
            continue
        line = line.split("\n")[0].split("\t")
        if sig and float(line[-1]) < 1:
            continue
        iva = parseIv(line[ivac])
        ivb = parseIv(line[ivbc])
        if len(chroms) > 0 and iva[0] not in chroms:
            continue
        if iva[0] not in records:
            records[iva[0]] = {"rs": {}, "f": ""}
        records[iva[0]]["rs"][line[0]] = iva + ivb
    for chrom in list(records.keys()):
        if len(records[chrom]["rs"]) == 0:
            del records[chrom]
            continue
        jd = os.path.join(d, "%s-%s.jd" % (chrom, chrom))
        if os.path.isfile(jd):
            records[chrom]["f"] = jd
        else:
            logger.warning("%s not found, however there are loops in that chromosome." % jd)
            del records[chrom]
    return records


def _anchor_pool(loops):
    """both anchors of every loop -> (starts, ends) int64"""
    rs = list(loops.values())
    starts = np.array([r[1] for r in rs] + [r[4] for r in rs], dtype=np.int64)
    ends = np.array([r[2] for r in rs] + [r[5] for r in rs], dtype=np.int64)
    return starts, ends


def getAnchors(loops):
    """scripts/jd2cleanWashuPETs.py:183-197: the anchors of `loops` merged until none overlap or share an endpoint -> [[s, e], ...],
    ascending (the script's list holds the same intervals in the order of its pairwise merge)"""
    starts, ends = _anchor_pool(loops)
    if len(starts) == 0:
        return []
    o = np.lexsort((ends, starts))
    starts, ends = starts[o], ends[o]
    reach = np.maximum.accumulate(ends)
    new = np.ones(len(starts), dtype=bool)
    new[1:] = starts[1:] > reach[:-1]                  # a new anchor starts beyond everything before it
    first = np.flatnonzero(new)
    last = np.append(first[1:], len(starts)) - 1
    return [[int(s), int(e)] for s, e in zip(starts[first], reach[last])]


def _anchor_rows(jdf, starts, ends):
    """K13 on the resident chromosome of `jdf` (a .jd path or a 'mem://' name of pipe.CACHE) -> (key, its parseJd matrix's rows
    with an end in an anchor (int64 [M, 3] for .jd files), number of rows, merged anchors)"""
    from .pipe import CACHE
    r = CACHE.get(jdf)
    with r.lock:
        mask, n_merged, n_kept = r.chrom.anchor_mask(starts, ends)
        rows = r.chrom.rows_of_mask(mask)
    assert len(rows) == n_kept
    ids = r.ids if r.ids is not None else np.arange(len(r.X), dtype=np.int64)
    return r.key, np.stack([ids[rows], r.X[rows], r.Y[rows]], 1), len(r.X), n_merged


def getAnchorPETs(jdf, loops, pre):
    """scripts/jd2cleanWashuPETs.py:200-227: the PETs of `jdf` with an end in a merged anchor of `loops` -> `<pre>/<chrA>-<chrB>.jd`;
    returns (loops, merged anchors, raw PETs, PETs in anchors)"""
    import joblib
    starts, ends = _anchor_pool(loops)
    key, nmat, n, n_merged = _anchor_rows(jdf, starts, ends)
    logger.info("%s:%s & %s loops,merged %s anchors" % (key, jdf, len(loops), n_merged))
    joblib.dump(nmat, os.path.join(pre, "-".join(key) + ".jd"))
    logger.info("%s:%s raw PETs %s PETs in anchors" % (key, n, nmat.shape[0]))
    return len(loops), n_merged, n, nmat.shape[0]


def jd2cleanWashuPETs(f, dir, sig, pre, chroms=[], cpu=1):
    """scripts/jd2cleanWashuPETs.py:230-242 -> (loops, merged anchors, raw PETs, PETs in anchors, ratio).  `cpu` is accepted for
    the script's signature: the chromosomes run one after the other, each as one kernel launch."""
    records = preDs(f, dir, sig, chroms=chroms)
    ds = [getAnchorPETs(records[key]["f"], records[key]["rs"], pre) for key in records.keys()]
    l, a, n, m = 0, 0, 0, 0
    for d in ds:
        l += d[0]
        a += d[1]
        n += d[2]
        m += d[3]
    r = m / 1.0 / n                                    # ZeroDivisionError without a chromosome, as in the script
    logger.info("%s\t%s,loops:%s, anchors:%s,raw PETs: %s, PETs in anchors:%s, ratio:%s" % (f, dir, l, a, n, m, r))
    return l, a, n, m, r


def help(argv=None):
    """the flags of scripts/jd2cleanWashuPETs.py:33-89"""
    ap = argparse.ArgumentParser(description="Filtering raw PET to keep only PET located in loop anchors "
                                             "(scripts/jd2cleanWashuPETs.py) on MI355X. "
                                             "For example: python -m cloops_amd.cleanpets -d trac -f trac.loop -o trac_clean")
    ap.add_argument("-d", dest="d", required=True, type=str, help="The directory of cis .jd file.")
    ap.add_argument("-f", dest="f", required=True, type=str, help="Loops file called by cLoops.")
    ap.add_argument("-p", dest="cpu", required=False, default=1, type=int,
                    help="Accepted for compatibility; the filtering runs on the GPU.")
    ap.add_argument("-s", dest="significant", required=False, action="store_false",
                    help="Whether to only using the PETs located at loop anchors. Default is yes, set this flag to use all potential "
                         "anchors called in the loop file.")
    ap.add_argument("-c", dest="chroms", required=False, default="", type=str,
                    help="Whether to process limited chroms, specify it as chr1,chr2,chr3, default is processed all chroms.")
    ap.add_argument("-o", dest="output", required=True, type=str, help="Output prefix.")
    return ap.parse_args(argv)


def main(argv=None):
    """scripts/jd2cleanWashuPETs.py:244-255"""
    op = help(argv)
    chroms = [] if op.chroms == "" else set(op.chroms.split(","))
    if not os.path.exists(op.output):
        os.mkdir(op.output)
    jd2cleanWashuPETs(op.f, op.d, op.significant, op.output, chroms=chroms, cpu=op.cpu)
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())
