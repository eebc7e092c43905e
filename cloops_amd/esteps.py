"""Estimate eps from the data: the k-distance curve of the PETs, the classic way to choose the eps of DBSCAN.

The reference has nothing of the kind (its -eps 0 means "twice the estimated fragment size", a property of the library, not of the
density; an exact k-NN over millions of PETs is out of reach in Python).  Here the integers come from kernel K23 on the chromosome
resident in HBM (`cl_kdis_build` / `cl_kdis_hist`): per asked k the distance d_k of every PET to its k-th nearest other PET under
|dx| + |dy|, binned into the project's integer log bins (`ests.logbin`, 128 per octave).  The floating point (quantiles, Otsu's
threshold) stays on the host in numpy, as in peaks.py and domains.py.

Definitions (include/cloops_hip.h, cl_kdis_build):
- Rows with Y - X >= cut take part (all rows for cut <= 0).  k = minPts - 1: a PET is a core of (eps, minPts) iff d_k <= eps.
- Per k the histograms of the chromosomes add: hist[b] rows with d_k >= 1 in log bin b, n_zero rows with d_k == 0, n_none rows of
  chromosomes with no k other rows.  n = all kept rows; the rows with a distance are n - n_none.
- Quantile q (1, 5, 10, 25, 50, 75, 90, 95, 99 %): rank = ceil(q (n - n_none) / 100), at least 1; zeros come first in the cumulative
  count; the value is 0 when the zeros reach the rank, else the lower bound (`ests.logbin_range`) of the bin in which the cumulative
  count first reaches it.  Without a row that has a distance: None.
- Suggested eps_k: Otsu's threshold on the histogram over the bin index, zeros excluded.  With w0(t), s0(t) the cumulative counts and
  index sums over bins <= t and W, S their totals, t maximises (w0 S - s0 W)^2 / (w0 (W - w0)) over the t with 0 < w0 < W (float64, the
  first maximum); eps_k = the lower bound of bin t + 1, so the rows below eps_k are exactly the zeros and the bins <= t.
  share_below = (n_zero + w0(t)) / (n - n_none).  eta = the between-class variance at t over the total variance of the bin index, in
  0 .. 1: low when the curve is not bimodal, and then eps_k says little.  Fewer than two occupied bins: eps_k, share_below and eta are
  None.
- Chromosomes are taken in plain string order of their names; a `.jd` whose key names two chromosomes is left out.
"""
import argparse
import json
import logging
import sys

import numpy as np

from . import _lib
from .coverage import chrom_files
from .ests import logbin_range
from .peaks import int_list, write_outputs

logger = logging.getLogger("cloops_amd.esteps")

QUANTILES = (1, 5, 10, 25, 50, 75, 90, 95, 99)                  # per cent
HEAD = ("k", "minPts", "n", "n_zero", "n_none") + tuple("q%d" % q for q in QUANTILES) + ("eps", "share_below", "eta")
SUFFIXES = ("_kdis.txt", "_kdis.json")
KMAX, BINS, NK_MAX = _lib.CL_KDIS_KMAX, _lib.CL_KDIS_BINS, 8
DEFAULT_K = (4, 9, 19)                                          # minPts 5, 10, 20


def k_list(v):
    """`-k`: a comma list ("4,9,19"), one number or an iterable -> the ascending list of the distinct k, 1 .. 8 of them in [1, 64]"""
    ks = int_list(v, "k")
    if len(ks) > NK_MAX or ks[-1] > KMAX:
        raise ValueError("k takes 1 to %d values in [1, %d], got %r" % (NK_MAX, KMAX, v))
    return ks


def _hist(hist):
    h = np.asarray(hist)
    if h.shape != (BINS,) or h.dtype.kind not in "iu":
        raise ValueError("a histogram of %d integer counts required" % BINS)
    return h.astype(np.int64)


def quantiles_of(hist, n_zero, qs=QUANTILES):
    """the quantiles (per cent, integers) of the d_k behind a histogram and its zero count -> [int] (None each without any row)"""
    h = _hist(hist)
    n = int(n_zero) + int(h.sum())
    if n == 0:
        return [None] * len(qs)
    cum = int(n_zero) + np.cumsum(h)
    out = []
    for q in qs:
        rank = max(1, -((-int(q) * n) // 100))                  # ceil(q n / 100) in integers
        out.append(0 if rank <= int(n_zero) else int(logbin_range(int(np.searchsorted(cum, rank, side="left")))[0]))
    return out


def otsu_of(hist, n_zero=0):
    """Otsu's threshold over the bin index -> dict(eps, share_below, eta, bin): bin = t, eps = the lower bound of bin t + 1 (all None
    with fewer than two occupied bins)"""
    h = _hist(hist)
    none = {"eps": None, "share_below": None, "eta": None, "bin": None}
    if np.count_nonzero(h) < 2:
        return none
    idx = np.arange(BINS, dtype=np.float64)
    hf = h.astype(np.float64)
    w0, s0 = np.cumsum(hf), np.cumsum(hf * idx)
    W, S = w0[-1], s0[-1]
    ok = (w0 > 0) & (w0 < W)
    crit = np.full(BINS, -1.0)
    crit[ok] = (w0[ok] * S - s0[ok] * W) ** 2 / (w0[ok] * (W - w0[ok]))
    t = int(np.argmax(crit))                                    # (the first maximum)
    total = W * float((hf * idx * idx).sum()) - S * S           # W^2 times the variance of the bin index
    eta = float(min(1.0, max(0.0, crit[t] / total))) if total > 0 else 0.0
    below = int(n_zero) + int(h[:t + 1].sum())
    return {"eps": int(logbin_range(t + 1)[0]), "share_below": below / float(int(n_zero) + int(h.sum())), "eta": eta, "bin": t}


def estimate_of(hist, n_zero, n_none):
    """one k: the line of `<o>_kdis.txt` without k -> dict(n, n_zero, n_none, quantiles {q: value}, eps, share_below, eta)"""
    h = _hist(hist)
    o = otsu_of(h, n_zero)
    return {"n": int(n_zero) + int(n_none) + int(h.sum()), "n_zero": int(n_zero), "n_none": int(n_none),
            "quantiles": {"q%d" % q: v for q, v in zip(QUANTILES, quantiles_of(h, n_zero))},
            "eps": o["eps"], "share_below": o["share_below"], "eta": o["eta"]}


def chrom_kdis(ch, ks, cut):
    """One chromosome on the device: `ch` has the kdis_* methods of api.Chromosome -> dict(n_kept, hist {k: int64[BINS]}, n_zero {k:},
    n_none {k:})"""
    out = {"hist": {}, "n_zero": {}, "n_none": {}}
    try:
        out["n_kept"] = int(ch.kdis_build(ks, cut))
        for w, k in enumerate(ks):
            hist, nz, nn = ch.kdis_hist(w)
            out["hist"][k], out["n_zero"][k], out["n_none"][k] = np.asarray(hist).astype(np.int64), int(nz), int(nn)
    finally:
        ch.kdis_free()
    return out


def sum_chroms(per_chrom, ks):
    """{k: (hist, n_zero, n_none)} over the chromosomes"""
    out = {}
    for k in ks:
        h = np.zeros(BINS, np.int64)
        for d in per_chrom.values():
            h += d["hist"][k]
        out[k] = (h, sum(d["n_zero"][k] for d in per_chrom.values()), sum(d["n_none"][k] for d in per_chrom.values()))
    return out


def _txt(v):
    return "NA" if v is None else str(v)


def format_table(ests):
    """`<o>_kdis.txt`: a header, then one tab-separated line per k (floats as Python prints them, NA for None)"""
    lines = ["\t".join(HEAD)]
    for k in sorted(ests):
        e = ests[k]
        row = [k, k + 1, e["n"], e["n_zero"], e["n_none"]] + [e["quantiles"]["q%d" % q] for q in QUANTILES] + [e["eps"], e["share_below"], e["eta"]]
        lines.append("\t".join(_txt(v) for v in row))
    return "\n".join(lines) + "\n"


def outputs_of(per_chrom, ks, cut):
    """{suffix: text} of the two files from the per-chromosome histograms, and the json's content"""
    sums = sum_chroms(per_chrom, ks)
    ests = {k: estimate_of(*sums[k]) for k in ks}
    js = {"k": list(ks), "cut": int(cut), "quantiles": list(QUANTILES), "bins": BINS,
          "chroms": {name: {"n": int(d["n_kept"])} for name, d in per_chrom.items()},
          "total": {"n": int(sum(d["n_kept"] for d in per_chrom.values()))},
          "estimates": {str(k): dict(ests[k], k=k, minPts=k + 1) for k in ks}}
    return {SUFFIXES[0]: format_table(ests), SUFFIXES[1]: json.dumps(js, indent=1, sort_keys=True) + "\n"}, js, sums


def plot_kdis(sums, ests, prefix):
    """`<prefix>_kdis.pdf`: per k the histogram over log2 d with eps_k drawn in; no matplotlib: a warning and False"""
    try:
        from matplotlib.figure import Figure
        from matplotlib.backends.backend_agg import FigureCanvasAgg
    except ImportError as e:
        logger.warning("WARNING: no picture drawn for %s_kdis.pdf (%s)" % (prefix, e))
        return False
    fig = Figure()
    FigureCanvasAgg(fig)
    ax = fig.add_subplot(1, 1, 1)
    x = np.log2([logbin_range(b)[0] for b in range(BINS)])
    for k in sorted(sums):
        h = sums[k][0]
        occ = np.flatnonzero(h)
        if len(occ) == 0:
            continue
        sl = slice(occ[0], occ[-1] + 1)
        eps = ests[str(k)]["eps"]
        line, = ax.plot(x[sl], h[sl], label="k = %d%s" % (k, "" if eps is None else ", eps = %d" % eps), linewidth=0.8)
        if eps is not None:
            ax.axvline(np.log2(eps), color=line.get_color(), linestyle="--", linewidth=0.8)
    ax.set_xlabel("log2(distance to the k-th nearest PET, bp)")
    ax.set_ylabel("PETs per log bin")
    ax.legend(fontsize=8)
    fig.savefig(prefix + "_kdis.pdf")
    return True


def check_args(ks, cut):
    """-> (ks, cut) as the kernel takes them; ValueError otherwise"""
    ks = k_list(ks)
    try:
        cut = int(cut)
    except (TypeError, ValueError):
        raise ValueError("cut must be an integer, got %r" % (cut,))
    return ks, cut


def jd2esteps(jd, fout, ks=DEFAULT_K, cut=0, chroms=(), plot=False):
    """The k-distance curves of `jd` (a directory of `.jd` files, or a list of .jd paths / 'mem://' names of pipe.CACHE, so the
    chromosomes of a finished sweep serve without files) -> `<fout>_kdis.txt`, `<fout>_kdis.json` and, with `plot`,
    `<fout>_kdis.pdf`; returns the json's content."""
    ks, cut = check_args(ks, cut)
    from .pipe import CACHE
    per_chrom = {}
    for chrom, f in chrom_files(jd, chroms):
        logger.info("k-distances of %s" % f)
        r = CACHE.get(f)
        with r.lock:
            per_chrom[chrom] = chrom_kdis(r.chrom, ks, cut)
    texts, js, sums = outputs_of(per_chrom, ks, cut)
    write_outputs(fout, texts)
    if plot:
        plot_kdis(sums, js["estimates"], fout)
    return js


def help(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cloops_amd.esteps",
                                 description="Estimate eps from the k-distance curve of the PETs on MI355X. "
                                             "For example: python -m cloops_amd.esteps -d out -o out -k 4,9,19")
    ap.add_argument("-d", dest="d", required=True, type=str, help="The directory of cis .jd files.")
    ap.add_argument("-o", dest="output", required=True, type=str, help="Output prefix.")
    ap.add_argument("-k", dest="k", required=False, default=",".join(str(k) for k in DEFAULT_K), type=str,
                    help="Neighbour ranks k = minPts - 1, a comma list of up to 8 values in [1, 64], default is 4,9,19.")
    ap.add_argument("-cut", dest="cut", required=False, default=0, type=int, help="Distance cutoff to filter PETs, default 0.")
    ap.add_argument("-c", dest="chroms", required=False, default="", type=str,
                    help="Whether to process limited chroms, specify it as chr1,chr2,chr3, default is all.")
    ap.add_argument("-plot", dest="plot", required=False, action="store_true", help="Draw the histograms into <o>_kdis.pdf.")
    return ap.parse_args(argv)


def main(argv=None):
    op = help(argv)
    chroms = [] if op.chroms == "" else set(op.chroms.split(","))
    jd2esteps(op.d, op.output, ks=op.k, cut=op.cut, chroms=chroms, plot=op.plot)
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())
