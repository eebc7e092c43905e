"""Differentially enriched loops between two conditions: scripts/deLoops, function for function.

Per chromosome the treatment and the control are two chromosomes resident in HBM (pipe.CACHE); kernel K11
(`cl_quant_counts`) gives every loop's rab = |{X in iva} & {Y in ivb}| on both, all loops of a side in one launch.

Semantics pinned: the script's local background is always 0.  deLoops:getPermutatedBg (:70-97) calls
`getCounts(na, model)` with the whole two-sided model instead of `model[0]`; under Python 3 numpy,
`np.searchsorted([xs_keys, xs], v)` raises ValueError (inhomogeneous shape), the bare `except: continue` skips every
window, and mrabt = mrabc = 0.0.  So lam = max((0 + 1), (rabc + 1)) * Nt / Nc = (rabc + 1) * Nt / Nc, and only the anchor
pair is counted: the shifted windows go to K11 empty.  Anchor columns, significant-loop filter and row order: `quant.preDs`.
"""
import argparse
import logging
import os
import sys

import numpy as np

from . import quant
from .cModel import getBonPvalues
from .quant import preDs  # noqa: F401  (scripts/deLoops:35-67)

logger = logging.getLogger("cloops_amd.deloops")


def _anchor_windows(rs):
    """the K11 windows of the anchor pair alone: windows 1..10 of each side empty (lo = the anchor's lo, hi = lo - 1), so
    they neither widen the slice K11 scans nor hold any PET -> int32 [R, 44]"""
    w = quant._loop_windows(rs).astype(np.int64)
    for side in (0, 11):
        w[:, side + 1:side + 11] = w[:, side:side + 1]
        w[:, 22 + side + 1:22 + side + 11] = w[:, side:side + 1] - 1
    return w.astype(np.int32)


def estSigFromCounts(rs, rabt, Nt, rabc, Nc):
    """scripts/deLoops:estSigOneLoop (:100-116) for all loops of `rs` and the rows of estSigTvsC (:119-147) -> DataFrame or
    None.  rabt / rabc: rab of every loop on the treatment / control; mrabt = mrabc = 0.0 (module docstring)."""
    import pandas as pd
    from scipy.stats import poisson
    if len(rs) == 0:
        return None
    normratio = float(Nt) / float(Nc)
    rabt = np.asarray(rabt, dtype=np.int64)
    rabc = np.asarray(rabc, dtype=np.int64)
    lams = (np.stack([np.zeros(len(rabc)), rabc], 1) + 1.0) * normratio
    lam = np.max(lams, axis=1)
    pop = poisson.sf(rabt - 1.0, lam)
    fc = rabt / lam
    pop = np.where(1e-300 > pop, 1e-300, pop)                          # max([pop, 1e-300])
    ds = {}
    for q, (key, r) in enumerate(rs.items()):
        ds[key] = {
            "iva": "%s:%s-%s" % (r[0], r[1], r[2]),
            "ivb": "%s:%s-%s" % (r[0], r[4], r[5]),
            "poisson_p-value": float(pop[q]),
            "FoldEnrichment": float(fc[q]),
        }
    ds = pd.DataFrame(ds).T
    ds["poisson_p-value_corrected"] = getBonPvalues(ds["poisson_p-value"])
    return ds


def _rab(rs, f, dis):
    """rab of every loop of `rs` on the resident chromosome of `f`, and its N"""
    if len(rs) == 0:
        return np.zeros(0, np.int64), quant._counts(f, np.zeros((0, 44), np.int32), dis)[1]
    counts, N = quant._counts(f, _anchor_windows(rs), dis)
    return counts[:, 2].astype(np.int64), N


def estSigTvsC(rs, ft, fc, pre, dis=0):
    """scripts/deLoops:119-147: the loops `rs` with `ft` as treatment and `fc` as control (.jd paths or 'mem://' names)"""
    rabt, Nt = _rab(rs, ft, dis)
    rabc, Nc = _rab(rs, fc, dis)
    quant._need_model(Nt, ft)
    quant._need_model(Nc, fc)
    return estSigFromCounts(rs, rabt, Nt, rabc, Nc)


def estSigOneChr(rst, bedpet, rsc, bedpec, pre, dis=0):
    """scripts/deLoops:150-165: both loop sets of one chromosome, each against the other condition"""
    dst = estSigTvsC(rst, bedpet, bedpec, pre, dis)
    dsc = estSigTvsC(rsc, bedpec, bedpet, pre, dis)
    return dst, dsc


def callDeLoops(ra, rb, prea, preb, dis=0, cpu=1):
    """scripts/deLoops:168-180 -> `<prea>.deloop`, `<preb>.deloop`.  `cpu` is accepted for the script's signature."""
    import pandas as pd
    logger.info("Calling differentially enriched loops for %s vs %s" % (prea, preb))
    ds = [estSigOneChr(ra[key]["rs"], ra[key]["f"], rb[key]["rs"], rb[key]["f"], key, dis) for key in ra.keys()]
    dsa = [t[0] for t in ds if t[0] is not None]
    dsb = [t[1] for t in ds if t[1] is not None]
    if len(dsa) == 0 or len(dsb) == 0:
        raise ValueError("no chromosome with significant loops in both %s and %s" % (prea, preb))    # pd.concat([])
    dsa, dsb = pd.concat(dsa), pd.concat(dsb)
    dsa.to_csv(prea + ".deloop", sep="\t", index_label="loopId")
    dsb.to_csv(preb + ".deloop", sep="\t", index_label="loopId")
    return dsa, dsb


def deloopHelp(argv=None):
    """the flags of cLoops/utils.py:deloopHelp (:207-276)"""
    ap = argparse.ArgumentParser(description="Differentially enriched loops calling based on loops called by cLoops "
                                             "(scripts/deLoops) on MI355X. For example: "
                                             "python -m cloops_amd.deloops -fa a.loop -fb b.loop -da A -db B")
    ap.add_argument("-fa", dest="fa", required=True, type=str,
                    help="Loops file called by cLoops. Only using significant loops as mark 1, you can change this in the .loop file.")
    ap.add_argument("-fb", dest="fb", required=True, type=str, help="Loops file called by cLoops.")
    ap.add_argument("-da", dest="da", required=True, type=str,
                    help="Directory for .jd files of loop file a, generated by cLoops with option -s 1.")
    ap.add_argument("-db", dest="db", required=True, type=str,
                    help="Directory for .jd files of loop file b, generated by cLoops with option -s 1.")
    ap.add_argument("-p", dest="cpu", required=False, default=1, type=int,
                    help="Accepted for compatibility; the counting runs on the GPU.")
    ap.add_argument("-c", dest="chroms", required=False, default="", type=str,
                    help="Whether to process limited chroms, specify it as chr1,chr2,chr3, default is not.")
    ap.add_argument("-dis", dest="dis", required=False, default=0, type=int,
                    help="Set a distance cutoff to filter PETs, could be the inter-ligation and self-ligation cutoff, default is 0.")
    return ap.parse_args(argv)


def main(argv=None):
    """scripts/deLoops:183-206: writes `<basename of -da>.deloop` and `<basename of -db>.deloop` in the working directory"""
    op = deloopHelp(argv)
    chroms = [] if op.chroms == "" else set(op.chroms.split(","))
    ra = preDs(op.fa, op.da, chroms)
    rb = preDs(op.fb, op.db, chroms)
    prea = os.path.split(op.da)[1]
    preb = os.path.split(op.db)[1]
    keys = set(ra.keys()).intersection(set(rb.keys()))
    for key in list(ra.keys()):
        if key not in keys:
            del ra[key]
            logger.info("No match of %s in %s or %s" % (key, op.fa, op.da))
    for key in list(rb.keys()):
        if key not in keys:
            del rb[key]
            logger.info("No match of %s in %s or %s" % (key, op.fb, op.db))
    if len(keys) == 0:
        raise ValueError("no chromosome has significant loops and a .jd file in both conditions")
    callDeLoops(ra, rb, prea, preb, op.dis, op.cpu)
    return 0


if __name__ == "__main__":
    sys.exit(main())
