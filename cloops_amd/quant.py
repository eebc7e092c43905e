"""Re-quantification of a loop set on another dataset: scripts/quantifyLoops.py, function for function.

The reference counts each loop's PETs with Python sets (cModel.getPETsforRegions, cModel.py:73-80) for the anchor pair
and for the 10 x 10 shifted window pairs of getNearbyPairRegions (cModel.py:83-105), once per loop.  Here the counting is
kernel K11 on the chromosome resident in HBM (`cl_quant_counts`): for every loop ra, rb and the directed counts
|{X in A_k} & {Y in B_l}| of the 11 x 11 window pairs, all loops of a chromosome in one launch.  The statistics are
evaluated on that table with the same numpy / scipy calls on the same integers, and the rows carry the same Python
types as the script's, so `<prefix>_quantLoops.txt` is text-identical to the converted reference.

Semantics pinned:
- `preDs` reads the anchors from the columns named `iva` / `ivb` of the header.  The script reads columns 6 and 7, their
  place when pandas sorted a `.loop` file's columns alphabetically; in the `.loop` files written in insertion order
  (cModel.runStat) those are `FDR` and `hypergeometric_p-value`.  Without such a header the columns are 6 and 7.
- Only loops whose last column is >= 1 are used; rows come in the chromosome order of the loop file, then loop order.
- With `-c` the script seeds its records from a Python set: the chromosome order then follows the hash seed.
- The local background is the mean of the 100 shifted pair counts; ES = 100 (an int) when it is 0.
"""
import argparse
import logging
import os
import sys

import numpy as np

from .cModel import parseIv, _windows

logger = logging.getLogger("cloops_amd.quant")

#: the count table of cl_quant_counts: [0] ra, [1] rb, [2 + 11 k + l] |{X in A_k} & {Y in B_l}|
QUANT_COLS = 123


def _anchor_columns(f, ivac, ivbc):
    """the columns of iva / ivb: explicit ones, else by header name, else 6 / 7 (the script's defaults)"""
    if ivac is not None and ivbc is not None:
        return ivac, ivbc
    with open(f) as fh:
        head = fh.readline().split("\n")[0].split("\t")
    if "iva" in head and "ivb" in head:
        return head.index("iva") if ivac is None else ivac, head.index("ivb") if ivbc is None else ivbc
    return 6 if ivac is None else ivac, 7 if ivbc is None else ivbc


def preDs(f, d, chroms=[], ivac=None, ivbc=None):
    """scripts/quantifyLoops.py:100-132 (= scripts/deLoops:35-67): the significant loops of the `.loop` file `f`, per
    chromosome, with the `<chrom>-<chrom>.jd` of directory `d` -> {chrom: {"rs": {loopId: [c, s, e, c, s, e]}, "f": path}}.
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
        if float(line[-1]) < 1:                     # only the significant loops
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


def _counts(f, wins, dis):
    """K11 on the resident chromosome of `f` (a .jd path or a 'mem://' name of pipe.CACHE) -> (int32 [R, 123], N)"""
    from .pipe import CACHE
    r = CACHE.get(f)
    with r.lock:
        return r.chrom.quant_counts(wins, dis)


def _loop_windows(rs, win=5):
    """the 44 window bounds of every loop of `rs` (cModel._windows: the windows of cModel.getNearbyPairRegions)"""
    if win != 5:
        raise ValueError("K11 counts the 10 + 10 windows of getNearbyPairRegions(win=5); win=%s is not supported" % win)
    return _windows(list(rs.values()))[3]


def _need_model(N, f):
    # getGenomeCoverage returns (None, 0) below 2 PETs and getPETsforRegions then fails on the None model
    if N < 2:
        raise ValueError("%s: fewer than 2 PETs (after the distance cutoff), no coverage model to count loops on" % f)


def quantFromCounts(rs, counts):
    """the rows of scripts/quantifyLoops.py:estSigOneChr (:137-179) from the K11 table of `rs` -> DataFrame or None"""
    import pandas as pd
    from scipy.stats import poisson
    if len(rs) == 0:
        return None
    c = np.asarray(counts, dtype=np.int64).reshape(-1, QUANT_COLS)
    rab = c[:, 2]
    # getPermutatedBg (:124-134): float(np.mean(rabs)) of the 100 shifted pairs, A windows outer; integer sums are exact
    mrab = c[:, 2:].reshape(-1, 11, 11)[:, 1:, 1:].reshape(-1, 100).mean(axis=1)
    sf = poisson.sf(rab - 1.0, mrab)
    pop = np.where(sf > 1e-300, sf, 1e-300)                          # max([1e-300, sf])
    ds = {}
    for q, (key, r) in enumerate(rs.items()):
        m = float(mrab[q])
        ds[key] = {
            "iva": "%s:%s-%s" % (r[0], r[1], r[2]),
            "ivb": "%s:%s-%s" % (r[0], r[4], r[5]),
            "ra": int(c[q, 0]),
            "rb": int(c[q, 1]),
            "rab": int(rab[q]),
            "ES": int(rab[q]) / m if m > 0 else 100,
            "poisson_p-value": float(pop[q]),
        }
    return pd.DataFrame(ds).T


def estSigOneChr(rs, jdf, pre, dis=0, win=5):
    """scripts/quantifyLoops.py:137-179: the loops of one chromosome quantified on the PETs of `jdf` (Y - X >= dis)"""
    if len(rs) == 0:
        return None
    counts, N = _counts(jdf, _loop_windows(rs, win), dis)
    _need_model(N, jdf)
    return quantFromCounts(rs, counts)


def quantifyLoops(ra, prea, dis=0, cpu=1):
    """scripts/quantifyLoops.py:182-187 -> `<prea>_quantLoops.txt`.  `cpu` is accepted for the script's signature: the
    chromosomes run one after the other, each as one kernel launch."""
    import pandas as pd
    ds = [estSigOneChr(ra[key]["rs"], ra[key]["f"], key, dis) for key in ra.keys()]
    ds = [d for d in ds if d is not None]
    if len(ds) == 0:
        raise ValueError("no significant loop with a matching .jd file to quantify")      # pd.concat([]) in the script
    ds = pd.concat(ds)
    ds.to_csv(prea + "_quantLoops.txt", sep="\t", index_label="loopId")
    return ds


def help(argv=None):
    """the flags of scripts/quantifyLoops.py:36-97"""
    ap = argparse.ArgumentParser(description="Quantify loops from cLoops called (scripts/quantifyLoops.py) on MI355X. "
                                             "For example: python -m cloops_amd.quant -f a.loop -d A -o fout")
    ap.add_argument("-f", dest="f", required=True, type=str,
                    help="Loops file called by cLoops. Only using significant loops as mark 1, you can change this in the .loop file.")
    ap.add_argument("-d", dest="d", required=True, type=str,
                    help="Directory for .jd files of loop file a, generated by cLoops with option -s 1.")
    ap.add_argument("-o", dest="output", required=True, type=str, help="Output file name prefix. ")
    ap.add_argument("-p", dest="cpu", required=False, default=1, type=int,
                    help="Accepted for compatibility; the counting runs on the GPU.")
    ap.add_argument("-c", dest="chroms", required=False, default="", type=str,
                    help="Whether to process limited chroms, specify it as chr1,chr2,chr3, default is not.")
    ap.add_argument("-dis", dest="dis", required=False, default=0, type=int,
                    help="Set a distance cutoff to filter PETs, could be the inter-ligation and self-ligation cutoff, default is 0.")
    return ap.parse_args(argv)


def main(argv=None):
    """scripts/quantifyLoops.py:190-204"""
    op = help(argv)
    chroms = [] if op.chroms == "" else set(op.chroms.split(","))
    ra = preDs(op.f, op.d, chroms)
    quantifyLoops(ra, op.output, op.dis, op.cpu)
    return 0


if __name__ == "__main__":
    sys.exit(main())
