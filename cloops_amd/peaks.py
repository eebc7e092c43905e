"""Peaks of the PET ends: where the ends themselves pile up -- the binding sites or anchors looked at next to the loops.

The reference has nothing of the kind (its successor calls peaks by 1D density clustering of the ends and a Poisson test against the
local background).  Here the integers come from kernel K21 on the chromosome resident in HBM (`cl_peak_sort` / `cl_peak_call` /
`cl_peak_get` / `cl_peak_count` / `cl_peak_summits`): the end points sorted once, every (eps, minPts) called on the sorted array, then
one count call and one summit call over the merged peaks.  The floating point (Poisson) stays on the host in scipy, as in cModel.py.

Definitions (include/cloops_hip.h, cl_peak_sort):
- Rows with Y - X >= cut take part (all rows for cut <= 0).  `ends`: "left" takes every row's X, "right" its Y, "both" both.
- The candidate peaks of a setting (eps, minPts) are the clusters of sequential 1D DBSCAN over the ascending end points, as half-open
  intervals [first member, last member + 1).
- The candidates of every setting are merged into their interval union: intervals that overlap merge, abutting ones stay apart.
- Of a merged peak [start, end), L = end - start and c = its end points.  Genome rate: lambda_g = N L / G, N = the end points of every
  chromosome written, G = the sum of (largest - smallest end point + 1) over them.  For every fold f of `flank` the window
  [max(0, start - f L), end + f L) gives lambda_f = (count(window) - c) L / (window length - L).  lambda = the largest of them,
  ES = c / lambda, p = poisson.sf(c - 1, lambda), corrected by cModel.getBonPvalues over the peaks of all chromosomes.  A peak is
  significant iff p_corrected <= pcut and ES >= escut.
- The summit of a peak is its end point with the most end points within min(eps) bp, the smallest position on ties.
- Chromosomes are written in plain string order of their names; a `.jd` whose key names two chromosomes is left out.
"""
import argparse
import json
import logging
import os
import sys

import numpy as np

from .coverage import chrom_files, ends_code

logger = logging.getLogger("cloops_amd.peaks")

SETTING_KEYS = ("n_peaks", "n_cores", "n_clustered")           # per chromosome and setting, in cl_peak_call's order
HEAD = ("peakId", "chrom", "start", "end", "length", "count", "summit", "summitCount")
TAIL = ("lambda", "ES", "poisson_p-value", "poisson_p-value_corrected", "significant")
SUFFIXES = ("_peaks.txt", "_peaks.bed", "_peaks.json")
WIDTH_MAX = 1 << 29                                            # eps lies in [1, 2^29) (cl_peak_call)


def int_list(v, what):
    """a comma list ("100,200"), one number or an iterable of numbers -> the sorted list of the distinct ints, all >= 1"""
    if isinstance(v, str):
        v = [x for x in v.split(",") if x != ""]
    elif isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        v = [v]
    try:
        out = sorted(set(int(x) for x in v))
    except (TypeError, ValueError):
        raise ValueError("%s must be a list of integers, got %r" % (what, v))
    if len(out) == 0 or out[0] < 1:
        raise ValueError("%s needs at least one value, all >= 1, got %r" % (what, v))
    return out


def merge_intervals(starts, ends):
    """the union of half-open intervals: intervals that overlap merge, abutting ones stay apart (a new one begins where the next start
    reaches the running maximum of the ends) -> (start, end) int64, ascending and disjoint"""
    s, e = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    if len(s) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    o = np.lexsort((e, s))
    s, e = s[o], e[o]
    top = np.maximum.accumulate(e)
    first = np.ones(len(s), bool)
    first[1:] = s[1:] >= top[:-1]
    idx = np.flatnonzero(first)
    return s[idx], np.maximum.reduceat(e, idx)


def flank_windows(start, end, flank):
    """for every fold f of `flank` the window [max(0, start - f L), end + f L) around [start, end), L = end - start
    -> [(window start, window end)] int64"""
    s, e = np.asarray(start, np.int64), np.asarray(end, np.int64)
    L = e - s
    return [(np.maximum(0, s - f * L), e + f * L) for f in flank]


def significance(start, end, count, windows, bg, N, G):
    """lambda, ES and the Poisson p-value of the peaks [start, end) holding `count` end points; windows / bg: the flank windows and the
    end points in each; N, G: the end points and the covered span of the genome -> (lambda, ES, p) float64"""
    s, e = np.asarray(start, np.int64), np.asarray(end, np.int64)
    c = np.asarray(count, np.int64)
    if len(s) == 0:
        z = np.zeros(0, float)
        return z, z.copy(), z.copy()
    from scipy.stats import poisson
    L = e - s
    lam = int(N) * L / int(G)
    for (ws, we), b in zip(windows, bg):
        lam = np.maximum(lam, (np.asarray(b, np.int64) - c) * L / ((we - ws) - L))
    return lam, c / lam, poisson.sf(c - 1, lam)


def correct_and_mark(p, ES, pcut, escut):
    """Bonferroni over all peaks (cModel.getBonPvalues) and the two cuts -> (p_corrected, significant bool)"""
    from .cModel import getBonPvalues
    pc = getBonPvalues(p) if len(p) else np.zeros(0, float)
    return pc, (pc <= pcut) & (np.asarray(ES) >= escut)


def chrom_peaks(ch, eps, minPts, cut, ends, flank):
    """One chromosome on the device: `ch` has the peaks_* methods of api.Chromosome.  Sort once, call every (eps, minPts), merge the
    candidates on the host, then one count call over the merged peaks and their flank windows and one summit call with w = min(eps)
    -> dict(n_ends, vmin, vmax, settings {"eps,minPts": dict(n_peaks, n_cores, n_clustered)}, candidates, start, end, count, bg
    [one array per fold], summit, summit_count)"""
    n_ends, vmin, vmax = ch.peaks_sort(cut, ends)
    try:
        settings, cs, ce = {}, [], []
        for e in eps:
            for m in minPts:
                stat = ch.peaks_call(e, m)
                s, en, _, _ = ch.peaks_get()
                settings["%d,%d" % (e, m)] = dict(zip(SETTING_KEYS, (int(x) for x in stat)))
                cs.append(s.astype(np.int64))
                ce.append(en.astype(np.int64))
        cs, ce = np.concatenate(cs), np.concatenate(ce)
        ms, me = merge_intervals(cs, ce)
        wins = flank_windows(ms, me, flank)
        counts = ch.peaks_count(np.concatenate([ms] + [w[0] for w in wins]), np.concatenate([me] + [w[1] for w in wins])).astype(np.int64)
        P = len(ms)
        pos, cnt = ch.peaks_summits(ms, me, min(eps))
    finally:
        ch.peaks_free()
    return {"n_ends": int(n_ends), "vmin": int(vmin), "vmax": int(vmax), "settings": settings, "candidates": int(len(cs)),
            "start": ms, "end": me, "count": counts[:P], "bg": [counts[(k + 1) * P:(k + 2) * P] for k in range(len(flank))],
            "summit": pos.astype(np.int64), "summit_count": cnt.astype(np.int64)}


def genome_of(per_chrom):
    """-> (N, G): the end points of all chromosomes and the sum of their covered spans (a chromosome without end points adds nothing)"""
    N = sum(d["n_ends"] for d in per_chrom.values())
    G = sum(d["vmax"] - d["vmin"] + 1 for d in per_chrom.values() if d["n_ends"] > 0)
    return N, G


def table_of(per_chrom, flank, pcut, escut):
    """the rows of `<o>_peaks.txt` of every chromosome in plain string order, the significance computed over all of them
    -> (rows [tuple], significant bool array, {chrom: number of significant peaks})"""
    N, G = genome_of(per_chrom)
    names = sorted(per_chrom)
    lam, ES, p = [], [], []
    for name in names:
        d = per_chrom[name]
        l, es, pv = significance(d["start"], d["end"], d["count"], flank_windows(d["start"], d["end"], flank), d["bg"], N, G)
        lam.append(l); ES.append(es); p.append(pv)
    lam, ES, p = (np.concatenate(a) if a else np.zeros(0, float) for a in (lam, ES, p))
    pc, sig = correct_and_mark(p, ES, pcut, escut)
    rows, k, nsig = [], 0, {}
    for name in names:
        d = per_chrom[name]
        P = len(d["start"])
        nsig[name] = int(sig[k:k + P].sum())
        for j in range(P):
            s, e = int(d["start"][j]), int(d["end"][j])
            rows.append(("peak-%s-%d" % (name, j), name, s, e, e - s, int(d["count"][j]), int(d["summit"][j]), int(d["summit_count"][j]))
                        + tuple(int(b[j]) for b in d["bg"])
                        + (float(lam[k + j]), float(ES[k + j]), float(p[k + j]), float(pc[k + j]), int(sig[k + j])))
        k += P
    return rows, sig, nsig


def format_table(rows, flank):
    """`<o>_peaks.txt` as text: a header, then one tab-separated line per merged peak (floats as Python prints them: the shortest text
    that reads back to the same number)"""
    head = HEAD + tuple("flank%dCount" % f for f in flank) + TAIL
    return "".join("\t".join(str(v) for v in r) + "\n" for r in [head] + list(rows))


def format_bed(rows):
    """`<o>_peaks.bed`: the significant peaks, `chrom start end peakId count`"""
    return "".join("%s\t%d\t%d\t%s\t%d\n" % (r[1], r[2], r[3], r[0], r[5]) for r in rows if r[-1] == 1)


def summary_of(per_chrom, nsig, eps, minPts, cut, ends, flank, pcut, escut):
    """the content of `<o>_peaks.json`: the parameters, per chromosome the end points, every setting's statistics, the candidates, the
    merged and the significant peaks, and the totals"""
    N, G = genome_of(per_chrom)
    chroms = {name: {"n_ends": d["n_ends"], "vmin": d["vmin"], "vmax": d["vmax"], "settings": d["settings"], "candidates": d["candidates"],
                     "merged": int(len(d["start"])), "significant": int(nsig[name])} for name, d in per_chrom.items()}
    total = {"n_ends": int(N), "span": int(G)}
    for k in ("candidates", "merged", "significant"):
        total[k] = sum(c[k] for c in chroms.values())
    return {"eps": list(eps), "minPts": list(minPts), "cut": int(cut), "ends": ends_code(ends), "flank": list(flank), "pcut": float(pcut),
            "escut": float(escut), "w": int(min(eps)), "chroms": chroms, "total": total}


def write_outputs(fout, texts):
    """the files `fout + suffix` of `texts` {suffix: str}, each written under a temporary name and renamed when all are complete: a
    failure leaves no half-written file"""
    tmp = []
    try:
        for suffix, text in texts.items():
            t = fout + suffix + ".tmp"
            tmp.append(t)
            with open(t, "w") as fh:
                fh.write(text)
        for suffix in texts:
            os.replace(fout + suffix + ".tmp", fout + suffix)
    except BaseException:
        for t in tmp:
            if os.path.exists(t):
                os.remove(t)
        raise


def outputs_of(per_chrom, eps, minPts, cut, ends, flank, pcut, escut):
    """{suffix: text} of the three files from the per-chromosome integers, and the per-chromosome summary"""
    rows, _, nsig = table_of(per_chrom, flank, pcut, escut)
    js = summary_of(per_chrom, nsig, eps, minPts, cut, ends, flank, pcut, escut)
    return {SUFFIXES[0]: format_table(rows, flank), SUFFIXES[1]: format_bed(rows),
            SUFFIXES[2]: json.dumps(js, indent=1, sort_keys=True) + "\n"}, js


def check_args(eps, minPts, cut, ends, flank, pcut, escut):
    """-> (eps, minPts, cut, ends code, flank, pcut, escut) as the kernels and the test take them; ValueError otherwise"""
    eps, minPts, flank = int_list(eps, "eps"), int_list(minPts, "minPts"), int_list(flank, "flank")
    if eps[-1] >= WIDTH_MAX:
        raise ValueError("eps must lie below 2^29, got %s" % eps[-1])
    code = ends_code(ends)
    pcut, escut = float(pcut), float(escut)
    if not (0.0 <= pcut <= 1.0):
        raise ValueError("pcut must lie in [0, 1], got %s" % pcut)
    if not escut >= 0.0:
        raise ValueError("escut must be >= 0, got %s" % escut)
    return eps, minPts, int(cut), code, flank, pcut, escut


def jd2peaks(jd, fout, eps=(100, 200), minPts=(5, 10), cut=0, ends="both", flank=(5, 10), pcut=1e-2, escut=2.0, chroms=()):
    """The peaks of the PET ends of `jd` (a directory of `.jd` files, or a list of .jd paths / 'mem://' names of pipe.CACHE, so the
    chromosomes of a finished sweep serve without files) -> `<fout>_peaks.txt` (every merged peak), `<fout>_peaks.bed` (the significant
    ones) and `<fout>_peaks.json`; returns the json's content.  Every chromosome is sorted and counted before the first peak is
    tested: the genome rate needs the end points of all of them."""
    eps, minPts, cut, code, flank, pcut, escut = check_args(eps, minPts, cut, ends, flank, pcut, escut)
    from .pipe import CACHE
    per_chrom = {}
    for chrom, f in chrom_files(jd, chroms):
        logger.info("calling peaks of %s" % f)
        r = CACHE.get(f)
        with r.lock:
            per_chrom[chrom] = chrom_peaks(r.chrom, eps, minPts, cut, code, flank)
    texts, js = outputs_of(per_chrom, eps, minPts, cut, ends, flank, pcut, escut)
    write_outputs(fout, texts)
    return js


def help(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cloops_amd.peaks",
                                 description="Peaks of the PET ends on MI355X. "
                                             "For example: python -m cloops_amd.peaks -d trac -o trac")
    ap.add_argument("-d", dest="d", required=True, type=str, help="The directory of cis .jd files.")
    ap.add_argument("-o", dest="output", required=True, type=str, help="Output prefix.")
    ap.add_argument("-eps", dest="eps", required=False, default="100,200", type=str,
                    help="Distances that define two end points as neighbours, a comma list, default is 100,200.")
    ap.add_argument("-minPts", dest="minPts", required=False, default="5,10", type=str,
                    help="Points required within eps of a core point (itself included), a comma list, default is 5,10.")
    ap.add_argument("-cut", dest="cut", required=False, default=0, type=int, help="Distance cutoff to filter PETs, default 0.")
    ap.add_argument("-ends", dest="ends", required=False, default="both", choices=["both", "left", "right"],
                    help="Which PET ends count, default both.")
    ap.add_argument("-flank", dest="flank", required=False, default="5,10", type=str,
                    help="Folds of a peak's length to either side that make its local background windows, a comma list, default is 5,10.")
    ap.add_argument("-pcut", dest="pcut", required=False, default=1e-2, type=float,
                    help="Bonferroni-corrected Poisson p-value cutoff of a significant peak, default 1e-2.")
    ap.add_argument("-escut", dest="escut", required=False, default=2.0, type=float,
                    help="Enrichment score cutoff of a significant peak, default 2.0.")
    ap.add_argument("-c", dest="chroms", required=False, default="", type=str,
                    help="Whether to process limited chroms, specify it as chr1,chr2,chr3, default is all.")
    return ap.parse_args(argv)


def main(argv=None):
    op = help(argv)
    chroms = [] if op.chroms == "" else set(op.chroms.split(","))
    jd2peaks(op.d, op.output, eps=op.eps, minPts=op.minPts, cut=op.cut, ends=op.ends, flank=op.flank, pcut=op.pcut, escut=op.escut,
             chroms=chroms)
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())
