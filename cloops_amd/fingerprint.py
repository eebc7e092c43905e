"""Contact-matrix fingerprints for quality control: scripts/jd2fingerprint, function for function.

The script bins every PET of a dataset into the cells of the upper contact matrix with a Python dict of dicts, one
iteration per PET, sorts the counts of the non-empty cells and writes the cumulative PET share of 100 rank groups.  Here
the counting is kernel K12 on the chromosome resident in HBM (`cl_contact_hist`): it returns the HISTOGRAM of the cell
counts (distinct count, number of cells holding it), which determines the sorted counts.  The rank groups are formed from
the merged genome-wide histogram with exact int64 prefix sums; `np.cumsum` and the division are then the script's own,
so the values are bit-identical to the converted reference and `<prefix>_fingerprint.txt` is text-identical.

Semantics pinned.  The script cannot run under Python 3 (`xrange`; `/` is true division, so the bin size
would have no effect): its Python-2 integer arithmetic is pinned, and the Python-3 dict / pandas order for the table.
- jd2contactMatrixUpper: rows with Y - X >= cut when cut > 0; minC = min over BOTH coordinate columns of those rows; the
  cell is ((x - minC) // binSize, (y - minC) // binSize).  No rows: ValueError (np.min of an empty array).
- contactMatrixUpper2Bins: step = cells // bins; groups are consecutive step-slices of the ascending counts, a partial
  tail is dropped, so there are cells // step groups -- possibly MORE than bins.  step == 0: ValueError (range step 0).
- jds2FingerPrint: the counts of every input are concatenated; no input: ValueError (np.concatenate of nothing).
- getFingerPrint / CLI: `-cut` is accepted and has NO effect (getFingerPrint does not pass it on); every `*.jd` of a
  directory counts; the label is dir.split("/")[-1] (a trailing slash gives ""), an empty entry of -labels falls back to
  it, a label count that differs from the directory count logs an error and writes nothing; columns are `random` then the
  datasets in -d order, a repeated label replaces the earlier column's values in its place; a dataset whose group count
  is not `bins` makes pandas raise ValueError before any file is written; `-p` has no effect; `-plot` is type=bool, so
  any non-empty value plots (`0` included) -> `<prefix>_fingerprint.pdf`.
- binSize < 1: ValueError before any GPU work (the script divides by zero at 0 and mirrors cells for negative sizes).
"""
import argparse
import logging
import os
import sys
from glob import glob

import numpy as np

logger = logging.getLogger("cloops_amd.fingerprint")


def _check_bin_size(binSize):
    if int(binSize) < 1:
        raise ValueError("binSize must be >= 1, got %s" % binSize)


def _cell_hist(f, cut, binSize):
    """K12 on the resident chromosome of `f` (a .jd path or a 'mem://' name of pipe.CACHE) -> (values, mult, n_kept)"""
    from .pipe import CACHE
    r = CACHE.get(f)
    with r.lock:
        values, mult, kept, _ = r.chrom.contact_hist(binSize, cut)
    return values, mult, kept


def _as_hist(ds):
    """(values, mult) as given, or the histogram of a plain array of cell counts"""
    if isinstance(ds, tuple):
        values, mult = ds
        return np.asarray(values, dtype=np.int64), np.asarray(mult, dtype=np.int64)
    values, mult = np.unique(np.asarray(ds, dtype=np.int64), return_counts=True)
    return values, mult.astype(np.int64)


def merge_hists(hists):
    """genome-wide histogram of several (values, mult) histograms (the counts of np.concatenate, as a histogram)"""
    if len(hists) == 0:
        raise ValueError("need at least one array to concatenate")
    v = np.concatenate([np.asarray(h[0], dtype=np.int64) for h in hists])
    m = np.concatenate([np.asarray(h[1], dtype=np.int64) for h in hists])
    values, inv = np.unique(v, return_inverse=True)
    mult = np.zeros(len(values), dtype=np.int64)
    np.add.at(mult, inv, m)
    keep = mult > 0
    return values[keep], mult[keep]


def group_sums(values, mult, bins=100):
    """the sums of the script's rank groups (scripts/jd2fingerprint:53-65, before the cumsum) from a histogram of cell counts:
    the ascending counts cut into consecutive slices of step = cells // bins, the partial tail dropped -> int64 [cells // step]"""
    values = np.asarray(values, dtype=np.int64)
    mult = np.asarray(mult, dtype=np.int64)
    order = np.argsort(values, kind="stable")
    values, mult = values[order], mult[order]
    cells = int(mult.sum())
    step = cells // bins
    if step == 0:
        raise ValueError("range() arg 3 must not be zero")              # range(0, len(ds), 0) in the script
    ngroups = cells // step
    c0 = np.concatenate([[0], np.cumsum(mult)])                          # cells before bin j
    p0 = np.concatenate([[0], np.cumsum(values * mult)])                 # PETs in those cells
    k = np.arange(ngroups + 1, dtype=np.int64) * step                    # the first k sorted counts ...
    j = np.searchsorted(c0, k, side="right") - 1                         # ... end inside bin j (c0[j] <= k < c0[j + 1])
    vj = np.concatenate([values, [0]])[j]
    s = p0[j] + (k - c0[j]) * vj                                         # ... and sum to s
    return np.diff(s)


def jd2contactMatrixUpper(jd, cut=0, binSize=2000):
    """scripts/jd2fingerprint:32-50: the counts of the non-empty cells of `jd` (a .jd path or a 'mem://' name), returned as
    their histogram (values ascending, mult) -- the script's array up to order"""
    _check_bin_size(binSize)
    values, mult, kept = _cell_hist(jd, cut, binSize)
    if kept == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")     # np.min(mat)
    return values, mult


def contactMatrixUpper2Bins(ds, bins=100):
    """scripts/jd2fingerprint:53-65.  `ds`: a histogram (values, mult) or a plain array of cell counts"""
    values, mult = _as_hist(ds)
    nn = group_sums(values, mult, bins)
    nn = np.cumsum(nn) / float(nn.sum())
    return nn


def jds2FingerPrint(jds, cut=0, binSize=2000, cpu=10, bins=100):
    """scripts/jd2fingerprint:68-73.  `cpu` is accepted for the script's signature: the inputs run one after the other."""
    _check_bin_size(binSize)
    if len(jds) == 0:
        raise ValueError("need at least one array to concatenate")
    ds = merge_hists([jd2contactMatrixUpper(jd, cut, binSize) for jd in jds])
    return contactMatrixUpper2Bins(ds, bins)


def plotFingerPrint(data, prefix="test"):
    """cLoops/cPlots.py:78-90 with matplotlib's Agg canvas -> `<prefix>_fingerprint.pdf`"""
    from matplotlib.figure import Figure
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    fig = Figure()
    FigureCanvasAgg(fig)
    ax = fig.add_subplot(1, 1, 1)
    x = data.index
    for c in data.columns:
        ax.plot(x, data[c], label=c)
    ax.legend()
    ax.set_xlabel("bins of contact matrix rank from low to high")
    ax.set_ylabel("PETs ratio")
    fig.savefig("%s_fingerprint.pdf" % prefix)


def getFingerPrint(dirs, labels, fout, cut=0, binSize=2000, cpu=10, plot=1, bins=100):
    """scripts/jd2fingerprint:76-103 -> `<fout>_fingerprint.txt` (and .pdf); the DataFrame written, or None when the
    label count does not match.  `cut` has no effect, as in the script."""
    import pandas as pd
    _check_bin_size(binSize)
    dirs = dirs.split(",")
    if labels != "" and len(dirs) != len(labels.split(",")):
        logger.error("Numbers of directories and labels are not equal! Return.")
        return None
    if labels != "":
        labels = labels.split(",")
    data = {}
    x = np.linspace(0, 1, bins)
    y = np.linspace(0, 1, bins)
    data["random"] = y
    for i in range(len(dirs)):
        logger.info("Getting finger print for %s" % dirs[i])
        nlabel = dirs[i].split("/")[-1]
        s = jds2FingerPrint(sorted(glob(os.path.join(dirs[i], "*.jd"))), binSize=binSize, cpu=cpu, bins=bins)
        if labels != "" and labels[i] != "":
            data[labels[i]] = s
        else:
            data[nlabel] = s
    data = pd.DataFrame(data)
    data.index = x
    data.to_csv("%s_fingerprint.txt" % fout)
    if plot:
        plotFingerPrint(data, fout)
    return data


def help(argv=None):
    """the flags of cLoops.utils.jd2fingerprintHelp (cLoops/utils.py:442-499)"""
    ap = argparse.ArgumentParser(description="Get the finger print for the datasets using contact matrix with specific bin size "
                                             "(scripts/jd2fingerprint) on MI355X. For example: python -m cloops_amd.fingerprint "
                                             "-d CTCF_ChIA-PET,cohesin_HiChIP,HiC -o test -bs 2000 -plot 1 -labels CTCF_ChIA-PET,cohesin_HiChIP,HiC")
    ap.add_argument("-d", dest="d", required=True, type=str,
                    help="The directories of cis .jd files, created by cLoops with option -s 1. Multiple datasets as -d a,b,c")
    ap.add_argument("-o", dest="output", required=True, type=str, help="Output prefix.")
    ap.add_argument("-bs", dest="binSize", default=2000, type=int, help="Bin size of the contact matrix, default is 2000.")
    ap.add_argument("-labels", dest="labels", default="", help="Labels of the datasets, default is the directory name.")
    ap.add_argument("-plot", dest="plot", default=0, type=bool,
                    help="Any non-empty value plots the finger print (type=bool, as in the script: 0 plots too); default is not.")
    ap.add_argument("-p", dest="cpu", required=False, default=1, type=int,
                    help="Accepted for compatibility; the counting runs on the GPU.")
    ap.add_argument("-cut", dest="cut", type=int, default=0,
                    help="Accepted for compatibility; as in the script it has no effect.")
    return ap.parse_args(argv)


def main(argv=None):
    """scripts/jd2fingerprint:106-124"""
    op = help(argv)
    getFingerPrint(op.d, op.labels, op.output, cut=op.cut, binSize=op.binSize, cpu=op.cpu, plot=op.plot)
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())
