"""Domains: the contiguous stretches of a chromosome whose PETs stay among themselves, and the boundaries between them.

The reference has nothing of the kind (users bin the chromosome into a matrix elsewhere and run an insulation tool).  Here the integers
come from kernel K22 on the chromosome resident in HBM (`cl_dom_tracks` / `cl_dom_get` / `cl_dom_count`): the kept rows sorted by X
once, three tracks over the bins for every window w, then one count call over the called domains.  The floating point (scores,
thresholds) stays on the host in numpy, as in peaks.py and cModel.py.

Definitions (include/cloops_hip.h, cl_dom_tracks):
- Rows with Y - X >= cut take part (all rows for cut <= 0).  Bins of `res` bp; entry b of a track describes the boundary at the start of
  bin b, at b res, for b = bmin .. bmax + 1: cross(b) = the rows of the 2 w bins around it that cross it, up(b) / down(b) = those that
  stay before / behind it.
- cov(b) = cross + up + down; b is valid iff cov(b) >= mincov; s(b) = cross(b) / cov(b), the share of the window's PETs that cross the
  boundary.  It normalises itself: no pseudo-count, no chromosome mean, no log.
- A valid b is a boundary iff, with L the valid bins of [b - w, b) and R the valid bins of (b, b + w]: L and R are not both empty,
  s(j) > s(b) for every j in L, s(j) >= s(b) for every j in R (the leftmost of a tie wins), and strength(b) = the smallest over the
  non-empty sides of (max s on that side) - s(b) >= delta.  The two ends of a track have cross = 0 by construction, so the first and
  the last domain close without a special case wherever the chromosome's ends are covered.
- A domain is the stretch between two consecutive boundaries a < b, [a res, b res), kept iff b - a <= maxbins and at least half of the
  bins a .. b - 1 are valid.  ES = intra / max(1, nx + ny - 2 intra): the PETs inside over the PETs with exactly one end inside;
  density = intra / (end - start); a domain is significant iff ES >= escut.
- Every w of `-w` is called on its own; its rows carry w, in ascending w.
- Chromosomes are written in plain string order of their names; a `.jd` whose key names two chromosomes is left out.
The defaults (res 10000, w 10, mincov 20, delta 0.05, maxbins 500, escut 1.0, cut 0) are starting points from a CPU prototype on the
chr21 example and on planted data, not tuned on real Hi-C.
"""
import argparse
import json
import logging
import sys

import numpy as np

from .coverage import chrom_files
from .peaks import int_list, write_outputs

logger = logging.getLogger("cloops_amd.domains")

DOMAIN_HEAD = ("domainId", "chrom", "start", "end", "length", "w", "intra", "nx", "ny", "ES", "density", "significant")
BOUNDARY_HEAD = ("chrom", "pos", "w", "cross", "up", "down", "score", "strength")
SUFFIXES = ("_domains.txt", "_domains.bed", "_boundaries.txt", "_domains.json")
RES_MAX = 1 << 29                                               # res and w res lie below 2^29, w in [1, 1024] (cl_dom_tracks)
W_MAX = 1024


def score_of(cross, up, down, mincov):
    """-> (s float64, valid bool): s(b) = cross / (cross + up + down) where that sum reaches mincov, 0.0 elsewhere"""
    c = np.asarray(cross, np.int64)
    cov = c + np.asarray(up, np.int64) + np.asarray(down, np.int64)
    valid = cov >= max(1, int(mincov))
    return np.where(valid, c / np.maximum(cov, 1), 0.0), valid


def boundaries_of(s, valid, w, delta):
    """the boundaries among the entries of one track -> (indices int64 ascending, strength float64)"""
    s, valid = np.asarray(s, float), np.asarray(valid, bool)
    n = len(s)
    lo, hi = np.where(valid, s, np.inf), np.where(valid, s, -np.inf)
    minL, minR = np.full(n, np.inf), np.full(n, np.inf)
    maxL, maxR = np.full(n, -np.inf), np.full(n, -np.inf)
    for d in range(1, min(int(w), n - 1) + 1):
        minL[d:] = np.minimum(minL[d:], lo[:-d]); maxL[d:] = np.maximum(maxL[d:], hi[:-d])
        minR[:-d] = np.minimum(minR[:-d], lo[d:]); maxR[:-d] = np.maximum(maxR[:-d], hi[d:])
    hasL, hasR = maxL > -np.inf, maxR > -np.inf
    strength = np.minimum(np.where(hasL, maxL, np.inf), np.where(hasR, maxR, np.inf)) - s
    ok = valid & (hasL | hasR) & (minL > s) & (minR >= s)
    ok[ok] = strength[ok] >= delta
    idx = np.flatnonzero(ok)
    return idx.astype(np.int64), strength[idx]


def domains_of(bidx, valid, maxbins):
    """the kept domains between consecutive boundaries (indices into a track) -> (a, b) int64: entries a .. b - 1"""
    bidx, valid = np.asarray(bidx, np.int64), np.asarray(valid, bool)
    if len(bidx) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    a, b = bidx[:-1], bidx[1:]
    nv = np.concatenate([[0], np.cumsum(valid)])
    keep = ((b - a) <= maxbins) & (2 * (nv[b] - nv[a]) >= (b - a))
    return a[keep], b[keep]


def chrom_domains(ch, res, ws, cut, mincov=20, delta=0.05, maxbins=500):
    """One chromosome on the device: `ch` has the domains_* methods of api.Chromosome.  Per w (ascending): the tracks, the host rules,
    one count call over the kept domains -> {w: dict(n_bins, bin0, n_kept, cross, up, down, score, valid, boundary [track indices],
    strength, start, end [bp], intra, nx, ny)}"""
    out = {}
    try:
        for w in ws:
            n_bins, bin0, n_kept = ch.domains_tracks(cut, res, w)
            cross, up, down = (np.asarray(a, np.int64) for a in ch.domains_get())
            s, valid = score_of(cross, up, down, mincov)
            bidx, strength = boundaries_of(s, valid, w, delta)
            a, b = domains_of(bidx, valid, maxbins)
            start, end = (a + bin0) * res, (b + bin0) * res
            intra, nx, ny = (np.asarray(v, np.int64) for v in ch.domains_count(start, end))
            out[int(w)] = {"n_bins": int(n_bins), "bin0": int(bin0), "n_kept": int(n_kept), "cross": cross, "up": up, "down": down,
                           "score": s, "valid": valid, "boundary": bidx, "strength": strength, "start": start, "end": end,
                           "intra": intra, "nx": nx, "ny": ny}
    finally:
        ch.domains_free()
    return out


def enrichment(intra, nx, ny, start, end):
    """-> (ES, density) float64"""
    intra = np.asarray(intra, np.int64)
    one = np.asarray(nx, np.int64) + np.asarray(ny, np.int64) - 2 * intra
    return intra / np.maximum(1, one), intra / np.maximum(1, np.asarray(end, np.int64) - np.asarray(start, np.int64))


def domain_rows(per_chrom, escut):
    """the rows of `<o>_domains.txt`: chromosomes in plain string order, ascending w, ascending position"""
    rows = []
    for name in sorted(per_chrom):
        for w in sorted(per_chrom[name]):
            d = per_chrom[name][w]
            ES, dens = enrichment(d["intra"], d["nx"], d["ny"], d["start"], d["end"])
            for j in range(len(d["start"])):
                s, e = int(d["start"][j]), int(d["end"][j])
                rows.append(("domain-%s-w%d-%d" % (name, w, j), name, s, e, e - s, w, int(d["intra"][j]), int(d["nx"][j]), int(d["ny"][j]),
                             float(ES[j]), float(dens[j]), int(ES[j] >= escut)))
    return rows


def boundary_rows(per_chrom, res):
    rows = []
    for name in sorted(per_chrom):
        for w in sorted(per_chrom[name]):
            d = per_chrom[name][w]
            for k, st in zip(d["boundary"], d["strength"]):
                k = int(k)
                rows.append((name, (k + d["bin0"]) * res, w, int(d["cross"][k]), int(d["up"][k]), int(d["down"][k]), float(d["score"][k]),
                             float(st)))
    return rows


def format_rows(head, rows):
    """a header, then one tab-separated line per row (floats as Python prints them: the shortest text that reads back to the same
    number)"""
    return "".join("\t".join(str(v) for v in r) + "\n" for r in [head] + list(rows))


def format_bed(rows):
    """`<o>_domains.bed`: the significant domains, `chrom start end domainId intra`"""
    return "".join("%s\t%d\t%d\t%s\t%d\n" % (r[1], r[2], r[3], r[0], r[6]) for r in rows if r[-1] == 1)


def format_bedgraph(per_chrom, res, w):
    """`<o>_insulation_w<W>.bedGraph`: `chrom b res (b + 1) res score` for the valid b >= 0"""
    out = []
    for name in sorted(per_chrom):
        d = per_chrom[name].get(w)
        if d is None:
            continue
        for k in np.flatnonzero(d["valid"]):
            b = int(k) + d["bin0"]
            if b >= 0:
                out.append("%s\t%d\t%d\t%s\n" % (name, b * res, (b + 1) * res, float(d["score"][k])))
    return "".join(out)


def summary_of(per_chrom, rows, res, ws, cut, mincov, delta, maxbins, escut):
    """the content of `<o>_domains.json`: the parameters, per chromosome and w the bins, valid bins, boundaries, domains and significant
    domains, and the totals"""
    sig = {}
    for r in rows:
        sig[(r[1], r[5])] = sig.get((r[1], r[5]), 0) + r[-1]
    chroms = {}
    for name, by_w in per_chrom.items():
        chroms[name] = {str(w): {"n_kept": d["n_kept"], "bins": d["n_bins"], "bin0": d["bin0"], "valid": int(d["valid"].sum()),
                                 "boundaries": int(len(d["boundary"])), "domains": int(len(d["start"])),
                                 "significant": int(sig.get((name, w), 0))} for w, d in by_w.items()}
    total = {k: sum(c[k] for by_w in chroms.values() for c in by_w.values()) for k in ("bins", "valid", "boundaries", "domains", "significant")}
    return {"res": int(res), "w": list(ws), "cut": int(cut), "mincov": int(mincov), "delta": float(delta), "maxbins": int(maxbins),
            "escut": float(escut), "chroms": chroms, "total": total}


def suffixes_of(ws):
    return SUFFIXES[:3] + tuple("_insulation_w%d.bedGraph" % w for w in ws) + SUFFIXES[3:]


def outputs_of(per_chrom, res, ws, cut, mincov, delta, maxbins, escut):
    """{suffix: text} of the files from the per-chromosome integers, and the summary"""
    rows = domain_rows(per_chrom, escut)
    js = summary_of(per_chrom, rows, res, ws, cut, mincov, delta, maxbins, escut)
    texts = {SUFFIXES[0]: format_rows(DOMAIN_HEAD, rows), SUFFIXES[1]: format_bed(rows),
             SUFFIXES[2]: format_rows(BOUNDARY_HEAD, boundary_rows(per_chrom, res))}
    for w in ws:
        texts["_insulation_w%d.bedGraph" % w] = format_bedgraph(per_chrom, res, w)
    texts[SUFFIXES[3]] = json.dumps(js, indent=1, sort_keys=True) + "\n"
    return texts, js


def check_args(res, w, cut, mincov, delta, maxbins, escut):
    """-> (res, ws, cut, mincov, delta, maxbins, escut) as the kernels and the rules take them; ValueError otherwise"""
    try:
        res, mincov, maxbins = int(res), int(mincov), int(maxbins)
    except (TypeError, ValueError):
        raise ValueError("res, mincov and maxbins must be integers, got %r, %r, %r" % (res, mincov, maxbins))
    ws = int_list(w, "w")
    if not (1 <= res < RES_MAX):
        raise ValueError("res must lie in [1, 2^29), got %s" % res)
    if ws[-1] > W_MAX or ws[-1] * res >= RES_MAX:
        raise ValueError("w must lie in [1, %d] with w res below 2^29, got %s at res %s" % (W_MAX, ws[-1], res))
    if mincov < 1:
        raise ValueError("mincov must be >= 1, got %s" % mincov)
    if maxbins < 1:
        raise ValueError("maxbins must be >= 1, got %s" % maxbins)
    delta, escut = float(delta), float(escut)
    if not delta >= 0.0:
        raise ValueError("delta must be >= 0, got %s" % delta)
    if not escut >= 0.0:
        raise ValueError("escut must be >= 0, got %s" % escut)
    return res, ws, int(cut), mincov, delta, maxbins, escut


def jd2domains(jd, fout, res=10000, w=(10,), cut=0, mincov=20, delta=0.05, maxbins=500, escut=1.0, chroms=()):
    """The domains of `jd` (a directory of `.jd` files, or a list of .jd paths / 'mem://' names of pipe.CACHE, so the chromosomes of a
    finished sweep serve without files) -> `<fout>_domains.txt` (every kept domain), `<fout>_domains.bed` (the significant ones),
    `<fout>_boundaries.txt`, `<fout>_insulation_w<W>.bedGraph` per w and `<fout>_domains.json`; returns the json's content."""
    res, ws, cut, mincov, delta, maxbins, escut = check_args(res, w, cut, mincov, delta, maxbins, escut)
    from .pipe import CACHE
    per_chrom = {}
    for chrom, f in chrom_files(jd, chroms):
        logger.info("calling domains of %s" % f)
        r = CACHE.get(f)
        with r.lock:
            per_chrom[chrom] = chrom_domains(r.chrom, res, ws, cut, mincov, delta, maxbins)
    texts, js = outputs_of(per_chrom, res, ws, cut, mincov, delta, maxbins, escut)
    write_outputs(fout, texts)
    return js


def help(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cloops_amd.domains",
                                 description="Domains and their boundaries on MI355X. "
                                             "For example: python -m cloops_amd.domains -d hic -o hic")
    ap.add_argument("-d", dest="d", required=True, type=str, help="The directory of cis .jd files.")
    ap.add_argument("-o", dest="output", required=True, type=str, help="Output prefix.")
    ap.add_argument("-res", dest="res", required=False, default=10000, type=int, help="Bin size in bp, default 10000.")
    ap.add_argument("-w", dest="w", required=False, default="10", type=str,
                    help="Windows in bins to either side of a boundary, a comma list, each called on its own, default is 10.")
    ap.add_argument("-cut", dest="cut", required=False, default=0, type=int, help="Distance cutoff to filter PETs, default 0.")
    ap.add_argument("-mincov", dest="mincov", required=False, default=20, type=int,
                    help="PETs a boundary's window must hold for its score to count, default 20.")
    ap.add_argument("-delta", dest="delta", required=False, default=0.05, type=float,
                    help="Least rise of the score to either side of a boundary, default 0.05.")
    ap.add_argument("-maxbins", dest="maxbins", required=False, default=500, type=int, help="Most bins of a domain, default 500.")
    ap.add_argument("-escut", dest="escut", required=False, default=1.0, type=float,
                    help="Enrichment score cutoff of a significant domain, default 1.0.")
    ap.add_argument("-c", dest="chroms", required=False, default="", type=str,
                    help="Whether to process limited chroms, specify it as chr1,chr2,chr3, default is all.")
    return ap.parse_args(argv)


def main(argv=None):
    op = help(argv)
    chroms = [] if op.chroms == "" else set(op.chroms.split(","))
    jd2domains(op.d, op.output, res=op.res, w=op.w, cut=op.cut, mincov=op.mincov, delta=op.delta, maxbins=op.maxbins, escut=op.escut,
               chroms=chroms)
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())
