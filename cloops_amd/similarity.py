"""How alike are two samples' contact maps: the stratum-adjusted correlation coefficient (SCC) of HiCRep (Yang et al. 2017) for every
pair of samples, per chromosome and genome-wide.

The reference has nothing of the kind (its successor ships `estSim`; users export cells and run a CPU tool).  The cells are K24's
(`cl_mat_cells`, folded) of both samples resident in HBM; the box smoothing and the six integer moments of every diagonal come from kernel
K28 (`cl_scc_moments`).  The coefficients, the weights, the texts and the files stay on the host.

Definitions (include/cloops_hip.h, cl_scc_moments):
- Both matrices are smoothed by a (2h+1)^2 box SUM over the window of bins that both samples' cells span together; a stratum d holds the
  positions (i, i + d) where either smoothed value is non-zero; D = min(nb, dmax // res + 1) strata are taken.
- The device returns n, sx, sy, sxx, syy, sxy of every stratum as exact integers.  With Python ints, for a stratum with n >= 2:
  num = n sxy - sx sy, va = n sxx - sx^2, vb = n syy - sy^2, rho = float(num) / (sqrt(float(va)) sqrt(float(vb))) when va > 0 and
  vb > 0, else NaN.  The weight is HiCRep's analytic one, n (1 + 1 / n) / 12; 0 where rho is NaN or d < ignore_diags.
- scc = sum(w rho) / sum(w), NaN when no stratum has weight.  pcc is the plain Pearson coefficient over all counted pixels of the strata
  d >= ignore_diags, from the summed moments by the same formula.
- The genome value of a pair is the plain mean of its chromosomes' finite scc (pcc likewise).  Chromosomes present in only one sample
  are skipped and listed in the json.  SCC depends on sequencing depth: a pair whose kept PETs differ by more than a factor of two is
  warned about; equalising depth by down-sampling is not done here.
- `<o>_scc.txt`: `sampleA sampleB chrom bins diags h pixels scc pcc keptA keptB`, one row per pair and chromosome and a `genome` row
  per pair; `<o>_scc_strata.txt`: `sampleA sampleB chrom d n rho weight`; `<o>_scc_matrix.txt`: the symmetric samples x samples table
  of genome values, diagonal 1; `<o>_scc.json`: the arguments, the records, the skipped chromosomes and the warnings.  Floats are
  written with repr (they read back to the same bits), NaN as nan.
"""
import argparse
import json
import logging
import math
import os
import sys

from . import _lib
from .coverage import chrom_files
from .matrix import check_res
from .peaks import write_outputs

logger = logging.getLogger("cloops_amd.similarity")

SUFFIXES = ("_scc.txt", "_scc_strata.txt", "_scc_matrix.txt", "_scc.json")
HMAX, BAND_MAX = _lib.CL_SCC_HMAX, _lib.CL_SCC_BAND_MAX
DEPTH_FACTOR = 2                                                            # kept counts further apart than this are warned about


def check_args(n_samples, res, h, dmax, ignore_diags, names=None):
    """-> (res, h, dmax, ignore_diags) checked; ValueError otherwise"""
    if n_samples < 2:
        raise ValueError("a comparison needs at least two samples, got %d" % n_samples)
    res = check_res(res)
    for name, v in (("h", h), ("dmax", dmax), ("ignorediags", ignore_diags)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError("%s must be an integer, got %r" % (name, v))
    if not 0 <= h <= HMAX:
        raise ValueError("h must lie in [0, %d], got %d" % (HMAX, h))
    if dmax < 0:
        raise ValueError("dmax must be at or above 0, got %d" % dmax)
    if ignore_diags < 0:
        raise ValueError("ignorediags must be at or above 0, got %d" % ignore_diags)
    if names is not None and (len(names) != n_samples or len(set(names)) != len(names) or any(not n or any(c.isspace() for c in n) for n in names)):
        raise ValueError("names must be %d distinct words, one per sample, got %r" % (n_samples, list(names)))
    return res, h, dmax, ignore_diags


def smax_of(h, max_count, n_kept):
    """the largest box sum a sample can have: a box holds (2h+1)^2 entries, and a kept PET stands in at most two entries"""
    return min((2 * int(h) + 1) ** 2 * int(max_count), 2 * int(n_kept))


def scc_fits(smax_a, smax_b, nb):
    """the overflow rule of cl_scc_moments: no sum of squares over a diagonal of nb positions can reach 2^64"""
    return max(int(smax_a), int(smax_b)) ** 2 * int(nb) < (1 << 64)


def pearson_of(n, sx, sy, sxx, syy, sxy):
    """Pearson's coefficient from exact integer moments; NaN with fewer than two points or without spread on either side"""
    n, sx, sy, sxx, syy, sxy = int(n), int(sx), int(sy), int(sxx), int(syy), int(sxy)
    if n < 2:
        return float("nan")
    num, va, vb = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
    if va <= 0 or vb <= 0:
        return float("nan")
    return float(num) / (math.sqrt(float(va)) * math.sqrt(float(vb)))


def combine(moments, ignore_diags=0):
    """the six arrays of scc_moments -> dict(n, rho, weight: lists per stratum; pixels, scc, pcc)"""
    cols = [[int(v) for v in a] for a in moments]
    D = len(cols[0])
    rho, weight = [], []
    for d in range(D):
        r = pearson_of(*(c[d] for c in cols))
        n = cols[0][d]
        w = 0.0 if (math.isnan(r) or d < ignore_diags) else n * (1.0 + 1.0 / n) / 12.0
        rho.append(r)
        weight.append(w)
    sw = sum(weight)
    scc = sum(w * r for w, r in zip(weight, rho) if w > 0.0) / sw if sw > 0.0 else float("nan")
    total = [sum(c[ignore_diags:]) for c in cols]
    return {"n": cols[0], "rho": rho, "weight": weight, "pixels": total[0], "scc": scc, "pcc": pearson_of(*total)}


def cells_span(ch):
    """the bins the cells of the last mat_cells(fold=True) span -> (lowest, highest), None without cells.  The span is K25's (the first
    cell's bx .. the largest by, taken on the device): no cell is copied to the host; the marginals made on the way are dropped"""
    b0, nb, _ = ch.bal_marginals(0)
    ch.bal_free()
    return (b0, b0 + nb - 1) if nb > 0 else None


def band_check(nb, D, h):
    if nb * (D + 4 * h) > BAND_MAX:
        raise ValueError("%d bins x (%d diagonals + 4 h) passes the %d entries of a band array: give a larger -res or a smaller -dmax or -h"
                         % (nb, D, BAND_MAX))


def pair_chrom(cha, chb, res, h=1, dmax=5000000, cut=0, ignore_diags=0):
    """One chromosome of two samples on the device: `cha` / `chb` have the mat_* and scc_* methods of api.Chromosome -> the record
    dict(b0, bins, diags, h, keptA, keptB, n, rho, weight, pixels, scc, pcc)"""
    try:
        ka = kb = cha.mat_cells(res, cut=cut, fold=True)[1]
        if chb is not cha:                                                  # (a sample against itself: one handle, a == b in the C call)
            kb = chb.mat_cells(res, cut=cut, fold=True)[1]
        spans = [s for s in (cells_span(cha), cells_span(chb)) if s is not None]
        b0 = min(s[0] for s in spans) if spans else 0
        nb = max(s[1] for s in spans) - b0 + 1 if spans else 0
        D = min(nb, dmax // res + 1)
        band_check(nb, D, h)
        moments = cha.scc_moments(chb, b0, nb, h=h, n_diags=D)
    finally:
        try:
            cha.mat_free()
        finally:
            if chb is not cha:
                chb.mat_free()
    rec = combine(moments, ignore_diags)
    rec.update({"b0": int(b0), "bins": int(nb), "diags": int(D), "h": int(h), "keptA": int(ka), "keptB": int(kb)})
    return rec


def fnum(x):
    """a float as the files hold it: repr (reads back to the same bits), NaN as nan"""
    return "nan" if math.isnan(x) else repr(float(x))


def _jnum(x):
    return None if math.isnan(x) else float(x)


def finite_mean(values):
    v = [x for x in values if not math.isnan(x) and not math.isinf(x)]
    return sum(v) / len(v) if v else float("nan")


def genome_of(per_chrom):
    """{chrom: record} of a pair -> its genome row: sums of the integers, plain means of the finite scc and pcc"""
    recs = list(per_chrom.values())
    return {"bins": sum(r["bins"] for r in recs), "pixels": sum(r["pixels"] for r in recs), "keptA": sum(r["keptA"] for r in recs),
            "keptB": sum(r["keptB"] for r in recs), "scc": finite_mean([r["scc"] for r in recs]), "pcc": finite_mean([r["pcc"] for r in recs])}


def depth_warning(a, b, g):
    lo, hi = sorted((g["keptA"], g["keptB"]))
    if hi > DEPTH_FACTOR * lo:
        return ("%s and %s differ in depth by more than a factor of %d (%d and %d kept PETs): SCC depends on depth, down-sample the deeper one"
                % (a, b, DEPTH_FACTOR, g["keptA"], g["keptB"]))
    return None


def similarity_outputs(names, pairs, args):
    """{suffix: text} of the four files and the json's content.  pairs: [dict(a, b: sample names, chroms: {chrom: record}, skipped:
    [chrom])] for every a before b in `names`"""
    head = "# genome rows: the plain mean of the chromosomes' finite scc (pcc likewise); integers summed\n"
    rows = [head, "sampleA\tsampleB\tchrom\tbins\tdiags\th\tpixels\tscc\tpcc\tkeptA\tkeptB\n"]
    strata = ["sampleA\tsampleB\tchrom\td\tn\trho\tweight\n"]
    value, js_pairs, warnings = {}, [], []
    for p in pairs:
        a, b, per = p["a"], p["b"], p["chroms"]
        for chrom in sorted(per):
            r = per[chrom]
            rows.append("%s\t%s\t%s\t%d\t%d\t%d\t%d\t%s\t%s\t%d\t%d\n" % (a, b, chrom, r["bins"], r["diags"], r["h"], r["pixels"], fnum(r["scc"]),
                                                                    fnum(r["pcc"]), r["keptA"], r["keptB"]))
            strata.extend("%s\t%s\t%s\t%d\t%d\t%s\t%s\n" % (a, b, chrom, d, r["n"][d], fnum(r["rho"][d]), fnum(r["weight"][d])) for d in range(r["diags"]))
        g = genome_of(per)
        rows.append("%s\t%s\tgenome\t%d\t.\t%d\t%d\t%s\t%s\t%d\t%d\n" % (a, b, g["bins"], args["h"], g["pixels"], fnum(g["scc"]), fnum(g["pcc"]),
                                                                   g["keptA"], g["keptB"]))
        value[(a, b)] = value[(b, a)] = g["scc"]
        w = depth_warning(a, b, g)
        if w:
            warnings.append(w)
        js_pairs.append({"a": a, "b": b, "skipped": sorted(p["skipped"]), "genome": {k: (_jnum(v) if isinstance(v, float) else v) for k, v in g.items()},
                         "chroms": {c: {k: (_jnum(v) if isinstance(v, float) else v) for k, v in per[c].items() if k not in ("n", "rho", "weight")}
                                    for c in sorted(per)}})
    matrix = ["\t" + "\t".join(names) + "\n"]
    for a in names:
        matrix.append(a + "\t" + "\t".join("1" if a == b else fnum(value[(a, b)]) for b in names) + "\n")
    js = {"args": args, "samples": list(names), "pairs": js_pairs, "warnings": warnings}
    return {SUFFIXES[0]: "".join(rows), SUFFIXES[1]: "".join(strata), SUFFIXES[2]: "".join(matrix),
            SUFFIXES[3]: json.dumps(js, indent=1, sort_keys=True) + "\n"}, js


def default_names(dirs):
    names = [os.path.basename(os.path.normpath(d)) or d for d in dirs]
    return names if len(set(names)) == len(names) else ["s%d" % (k + 1) for k in range(len(dirs))]


def jds2similarity(dirs, fout, res=100000, h=1, dmax=5000000, cut=0, ignore_diags=0, chroms=(), names=None):
    """The SCC of every pair of the samples `dirs` (directories of cis .jd files) -> `<fout>_scc.txt`, `<fout>_scc_strata.txt`,
    `<fout>_scc_matrix.txt` and `<fout>_scc.json`; returns the json's content."""
    dirs = list(dirs)
    res, h, dmax, ignore_diags = check_args(len(dirs), res, h, dmax, ignore_diags, names)
    cut = int(cut)
    names = default_names(dirs) if names is None else list(names)
    from .pipe import CACHE
    files = [dict(chrom_files(d, chroms)) for d in dirs]
    pairs = []
    for i in range(len(dirs)):
        for j in range(i + 1, len(dirs)):
            shared = sorted(set(files[i]) & set(files[j]))
            per = {}
            for chrom in shared:
                logger.info("similarity of %s and %s on %s" % (names[i], names[j], chrom))
                # both residents pinned against eviction while either is in use; two spellings of one file are ONE resident, whose
                # lock is taken once; two residents are locked in the order of their files' names, the same in every thread
                with CACHE.pinned([files[i][chrom], files[j][chrom]]) as (ra, rb):
                    if ra is rb:
                        with ra.lock:
                            per[chrom] = pair_chrom(ra.chrom, ra.chrom, res, h, dmax, cut, ignore_diags)
                    else:
                        first, second = (ra, rb) if os.path.realpath(files[i][chrom]) <= os.path.realpath(files[j][chrom]) else (rb, ra)
                        with first.lock:
                            with second.lock:
                                per[chrom] = pair_chrom(ra.chrom, rb.chrom, res, h, dmax, cut, ignore_diags)
            pairs.append({"a": names[i], "b": names[j], "chroms": per, "skipped": sorted(set(files[i]) ^ set(files[j]))})
    args = {"res": res, "h": h, "dmax": dmax, "cut": cut, "ignore_diags": ignore_diags, "samples": dirs}
    texts, js = similarity_outputs(names, pairs, args)
    for w in js["warnings"]:
        logger.warning("WARNING: " + w)
    write_outputs(fout, texts)
    return js


def help(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cloops_amd.similarity", add_help=False,
                                 description="Similarity of samples' contact maps on MI355X: the stratum-adjusted correlation coefficient. "
                                             "For example: python -m cloops_amd.similarity -d rep1,rep2 -o reps -res 100000 -h 1")
    ap.add_argument("--help", action="help", help="Show this message and exit.")
    ap.add_argument("-d", dest="d", required=True, type=str, help="The directories of cis .jd files of the samples, as dirA,dirB[,dirC..].")
    ap.add_argument("-o", dest="output", required=True, type=str, help="Output prefix.")
    ap.add_argument("-res", dest="res", required=False, default=100000, type=int, help="Bin size in bp, default 100000.")
    ap.add_argument("-h", dest="h", required=False, default=1, type=int, help="Half-width of the smoothing box in bins, 0 to %d, default 1." % HMAX)
    ap.add_argument("-dmax", dest="dmax", required=False, default=5000000, type=int, help="Largest distance in bp whose stratum takes part, default 5000000.")
    ap.add_argument("-cut", dest="cut", required=False, default=0, type=int, help="Distance cutoff to filter PETs, default 0.")
    ap.add_argument("-ignorediags", dest="ignorediags", required=False, default=0, type=int, help="Strata nearer the diagonal than this get no weight, default 0.")
    ap.add_argument("-c", dest="chroms", required=False, default="", type=str,
                    help="Whether to process limited chroms, specify it as chr1,chr2,chr3, default is all.")
    ap.add_argument("-names", dest="names", required=False, default="", type=str, help="Names of the samples, as A,B[,C..]; default: the directories' names.")
    return ap.parse_args(argv)


def main(argv=None):
    op = help(argv)
    jds2similarity([d for d in op.d.split(",") if d], op.output, res=op.res, h=op.h, dmax=op.dmax, cut=op.cut, ignore_diags=op.ignorediags,
                   chroms=[] if op.chroms == "" else set(op.chroms.split(",")), names=None if op.names == "" else op.names.split(","))
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())
