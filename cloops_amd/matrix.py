"""Contact matrices: a binned window for a heatmap, the non-empty cells of whole chromosomes, and the profile of one viewpoint.

The reference has nothing of the kind (users dump `.jd` files and bin them elsewhere).  Here the integers come from kernel K24 on the
chromosome resident in HBM (`cl_mat_window` / `cl_mat_cells` / `cl_mat_cells_get` / `cl_mat_v4c`) over the rows sorted by X once
(K19's table, shared with agg, domains and esteps).  Labels, text and scaling stay on the host.

Definitions (include/cloops_hip.h, cl_mat_window):
- Rows with Y - X >= cut take part (all rows for cut <= 0).  The bin of a coordinate p is floor(p / res).
- A region `chr:start-end` is the half-open interval [start, end) with 0 <= start < end; its bins are those that overlap it:
  start // res .. (end - 1) // res.  A bin is labelled `chr:b res-(b + 1) res`.
- window: the counts of region x region2 (rows: the bins of X, columns: the bins of Y).  Without a second region the window is the
  diagonal one and mirrored: a PET with bx != by also counts at its transposed cell, so the matrix is symmetric with its diagonal
  counted once.
- cells: the distinct (bx, by) of a chromosome with their counts, ascending, folded onto bx <= by unless `-nofold`, as `bg2` lines
  `chrom start1 end1 chrom start2 end2 count` (what `cooler load -f bg2` reads), fetched in chunks of CHUNK cells.
- v4c: a PET adds 1 at the bin of its Y when its X lies in the viewpoint and 1 at the bin of its X when its Y does.  One bedGraph line
  per non-zero bin.  norm "cpm": counts per million of the viewpoint's n_x + n_y contacts, three decimals (coverage.fixed_point).
- Chromosomes are written in plain string order of their names; a `.jd` whose key names two chromosomes is left out, and a second
  region on another chromosome is refused (trans matrices are not made).
"""
import argparse
import json
import logging
import re
import sys

import numpy as np

from . import _lib
from .coverage import CPM_NUM, NORMS, chrom_files, fixed_point
from .peaks import write_outputs

logger = logging.getLogger("cloops_amd.matrix")

SUFFIXES = ("_matrix.txt", "_matrix.json", "_cells.txt", "_cells.json", "_v4c.bedGraph", "_v4c.json")
WMAX, CELLS_MAX = _lib.CL_MAT_WMAX, _lib.CL_MAT_CELLS_MAX
RES_MAX = 1 << 29                                               # res lies in [1, 2^29) (cl_mat_window)
NB_MAX = 1 << 24                                                # bins of a virtual 4C (cl_mat_v4c)
CHUNK = 1 << 20                                                 # cells per mat_cells_get
_REGION = re.compile(r"^([^\s:]+):(-?[0-9]+)-(-?[0-9]+)$")


def parse_region(text):
    """`chr21:20000000-21000000` -> ("chr21", 20000000, 21000000): the half-open [start, end), 0 <= start < end"""
    m = _REGION.match(text) if isinstance(text, str) else None
    if m is None:
        raise ValueError("a region is written chrom:start-end, got %r" % (text,))
    chrom, start, end = m.group(1), int(m.group(2)), int(m.group(3))
    if start < 0:
        raise ValueError("a region starts at or above 0, got %r" % (text,))
    if start >= end:
        raise ValueError("a region needs start < end, got %r" % (text,))
    return chrom, start, end


def check_res(res):
    try:
        res = int(res)
    except (TypeError, ValueError):
        raise ValueError("res must be an integer, got %r" % (res,))
    if not (1 <= res < RES_MAX):
        raise ValueError("res must lie in [1, 2^29), got %s" % res)
    return res


def region_bins(start, end, res):
    """the bins of `res` bp that overlap [start, end) -> (first bin, number of bins)"""
    b0 = int(start) // int(res)
    return b0, (int(end) - 1) // int(res) - b0 + 1


def bin_label(chrom, b, res):
    return "%s:%d-%d" % (chrom, b * res, (b + 1) * res)


def window_fits(r1, r2, res):
    nx, ny = region_bins(r1[1], r1[2], res)[1], region_bins(r2[1], r2[2], res)[1]
    return nx <= WMAX and ny <= WMAX and nx * ny <= CELLS_MAX


def smallest_res(r1, r2):
    """the smallest res at which region x region2 is a window cl_mat_window takes"""
    l1, l2 = r1[2] - r1[1], r2[2] - r2[1]
    # n bins cover at most n res bp, so a fitting res is at least len / WMAX and at least sqrt(l1 l2 / CELLS_MAX)
    res = max(1, -(-max(l1, l2) // WMAX), int(np.sqrt(float(l1) * float(l2) / CELLS_MAX)))
    while not window_fits(r1, r2, res):
        res += 1
    return res


def format_matrix(chrom, res, bx0, by0, mat):
    """`<o>_matrix.txt`: a tab and the column labels, then per row its label and its counts"""
    mat = np.asarray(mat)
    lines = ["\t" + "\t".join(bin_label(chrom, by0 + j, res) for j in range(mat.shape[1]))]
    for i in range(mat.shape[0]):
        lines.append(bin_label(chrom, bx0 + i, res) + "\t" + "\t".join(str(int(v)) for v in mat[i]))
    return "\n".join(lines) + "\n"


def window_of(ch, r1, r2, res, cut, mirror):
    """One window on the device: `ch` has the mat_* methods of api.Chromosome; r1 / r2 = (chrom, start, end) of the rows / columns
    -> (texts {suffix: text}, the json's content, the matrix)"""
    (bx0, nx), (by0, ny) = region_bins(r1[1], r1[2], res), region_bins(r2[1], r2[2], res)
    mat, n_in, n_kept = ch.mat_window(res, bx0, by0, nx, ny, cut=cut, mirror=mirror)
    js = {"region": "%s:%d-%d" % r1, "region2": "%s:%d-%d" % r2, "res": int(res), "nx": int(nx), "ny": int(ny), "cut": int(cut),
          "mirror": bool(mirror), "n_in": int(n_in), "n_kept": int(n_kept), "max": int(np.asarray(mat).max())}
    return {SUFFIXES[0]: format_matrix(r1[0], res, bx0, by0, mat), SUFFIXES[1]: json.dumps(js, indent=1, sort_keys=True) + "\n"}, js, mat


def cell_chunks(ch, n_cells, chunk=CHUNK):
    """the cells of the last mat_cells, at most `chunk` at a time -> (bx, by, cnt) per chunk"""
    for first in range(0, int(n_cells), int(chunk)):
        yield ch.mat_cells_get(first, min(int(chunk), int(n_cells) - first))


def format_cells(chrom, res, bx, by, cnt):
    """bg2 lines of one chunk: `chrom start1 end1 chrom start2 end2 count`"""
    bx, by = np.asarray(bx, np.int64), np.asarray(by, np.int64)
    return "".join("%s\t%d\t%d\t%s\t%d\t%d\t%d\n" % (chrom, x * res, (x + 1) * res, chrom, y * res, (y + 1) * res, c)
                   for x, y, c in zip(bx.tolist(), by.tolist(), np.asarray(cnt, np.int64).tolist()))


def chrom_cells(ch, chrom, res, cut, fold, chunk=CHUNK):
    """One chromosome on the device -> (its bg2 text, dict(n_cells, n_kept, max_count))"""
    try:
        n_cells, n_kept, max_count = ch.mat_cells(res, cut=cut, fold=fold)
        text = "".join(format_cells(chrom, res, *c) for c in cell_chunks(ch, n_cells, chunk))
    finally:
        ch.mat_free()
    return text, {"n_cells": int(n_cells), "n_kept": int(n_kept), "max_count": int(max_count)}


def cells_outputs(per_chrom, res, cut, fold):
    """{suffix: text} of the two files from {chrom: (text, stats)}, and the json's content"""
    names = sorted(per_chrom)
    stats = {n: per_chrom[n][1] for n in names}
    total = {"n_cells": sum(s["n_cells"] for s in stats.values()), "n_kept": sum(s["n_kept"] for s in stats.values()),
             "max_count": max([s["max_count"] for s in stats.values()] or [0])}
    js = {"res": int(res), "cut": int(cut), "fold": bool(fold), "chroms": stats, "total": total}
    return {SUFFIXES[2]: "".join(per_chrom[n][0] for n in names), SUFFIXES[3]: json.dumps(js, indent=1, sort_keys=True) + "\n"}, js


def cpm_scale(norm, n_contacts):
    """the (numerator, denominator) of coverage.fixed_point for `norm`; None for raw counts, and for a viewpoint without contacts"""
    if norm not in NORMS:
        raise ValueError("norm must be one of %s, got %r" % (", ".join(NORMS), norm))
    if norm == "none" or int(n_contacts) <= 0:
        return None
    return (CPM_NUM, int(n_contacts))


def format_v4c(chrom, res, b0, out, view, scale=None):
    """`<o>_v4c.bedGraph`: a track line, then `chrom start end value` per non-zero bin"""
    out = np.asarray(out, np.int64)
    lines = ['track type=bedGraph name="v4c %s:%d-%d"\n' % view]
    for k in np.flatnonzero(out).tolist():
        v = str(int(out[k])) if scale is None else fixed_point(out[k], scale[0], scale[1])
        lines.append("%s\t%d\t%d\t%s\n" % (chrom, (b0 + k) * res, (b0 + k + 1) * res, v))
    return "".join(lines)


def kept_span(ch, res, cut, chunk=CHUNK):
    """the bins the kept rows of a chromosome span at `res` -> (first bin, number of bins), (0, 0) without rows: the folded cells
    ascend by their smaller bin, and the largest bin is the largest by"""
    try:
        n_cells = ch.mat_cells(res, cut=cut, fold=True)[0]
        if n_cells == 0:
            return 0, 0
        lo = int(ch.mat_cells_get(0, 1)[0][0])
        hi = max(int(c[1].max()) for c in cell_chunks(ch, n_cells, chunk))
    finally:
        ch.mat_free()
    return lo, hi - lo + 1


def v4c_of(ch, view, rng, res, cut, norm):
    """One viewpoint on the device: view = (chrom, v0, v1), rng = (chrom, start, end) or None for the span of the kept rows
    -> (texts, the json's content, the profile)"""
    b0, nb = kept_span(ch, res, cut) if rng is None else region_bins(rng[1], rng[2], res)
    if nb > NB_MAX:
        raise ValueError("the profile has %d bins at res %d, more than 2^24: give a larger -res or a region -r" % (nb, res))
    out, n_x, n_y, n_kept = ch.mat_v4c(res, view[1], view[2], b0, nb, cut=cut)
    js = {"viewpoint": "%s:%d-%d" % view, "res": int(res), "cut": int(cut), "norm": norm, "n_x": int(n_x), "n_y": int(n_y),
          "n_kept": int(n_kept), "bin0": int(b0), "n_bins": int(nb), "max": int(np.asarray(out).max()) if nb > 0 else 0}
    text = format_v4c(view[0], res, b0, out, view, cpm_scale(norm, n_x + n_y))
    return {SUFFIXES[4]: text, SUFFIXES[5]: json.dumps(js, indent=1, sort_keys=True) + "\n"}, js, out


def plot_matrix(mat, js, prefix):
    """`<prefix>_matrix.pdf`: log1p of the counts as a heatmap; no matplotlib: a warning and False"""
    try:
        from matplotlib.figure import Figure
        from matplotlib.backends.backend_agg import FigureCanvasAgg
    except ImportError as e:
        logger.warning("WARNING: no picture drawn for %s_matrix.pdf (%s)" % (prefix, e))
        return False
    fig = Figure()
    FigureCanvasAgg(fig)
    ax = fig.add_subplot(1, 1, 1)
    im = ax.imshow(np.log1p(np.asarray(mat, np.float64)), cmap="Reds", interpolation="nearest", aspect="auto")
    ax.set_xlabel(js["region2"])
    ax.set_ylabel(js["region"])
    ax.set_title("log(1 + PETs), %d bp bins" % js["res"], fontsize=9)
    fig.colorbar(im)
    fig.savefig(prefix + "_matrix.pdf")
    return True


def _records(jd, chroms=()):
    """`jd` (a directory of `.jd` files, or a list of .jd paths / 'mem://' names of pipe.CACHE) -> [(chrom, resident record)] of the
    cis ones, only those of `chroms` if given, in plain string order"""
    from .pipe import CACHE
    return [(chrom, CACHE.get(f)) for chrom, f in chrom_files(jd, chroms)]


def region_records(jd, chroms, region, res, verb):
    """-> (`region` as (chrom, start, end) or None, _records(jd, chroms)); ValueError for a region that is no window at `res`, or whose
    chromosome is not among those records (`verb`: what the caller does to them)"""
    rg = None if region is None else parse_region(region)
    if rg is not None and not window_fits(rg, rg, res):
        raise ValueError("the region needs more than %d bins a side or %d cells at -res %d; the smallest -res that fits is %d"
                         % (WMAX, CELLS_MAX, res, smallest_res(rg, rg)))
    recs = _records(jd, chroms)
    if rg is not None and rg[0] not in [c for c, _ in recs]:
        raise ValueError("no cis .jd file of chromosome %s among those to %s" % (rg[0], verb))
    return rg, recs


def each_chrom(recs, log, what, fn):
    """{chrom: fn(the record's chromosome, chrom)} over the records of _records, each under its lock, after the line `what` % chrom
    on the logger `log`"""
    per_chrom = {}
    for chrom, r in recs:
        log.info(what % chrom)
        with r.lock:
            per_chrom[chrom] = fn(r.chrom, chrom)
    return per_chrom


def chrom_outputs(per_chrom, parts, json_suffix, js, matrix_suffix=None):
    """{suffix: text} of a command's files from {chrom: dict of texts}: per (suffix, key) of `parts` the texts of that key joined in
    name order, the json `js` (given "chroms": the "stats" of each) under `json_suffix`, and under `matrix_suffix` the "matrix" text of
    the chromosome that has one; and the json's content"""
    names = sorted(per_chrom)
    js = dict(js, chroms={n: per_chrom[n]["stats"] for n in names})
    texts = {suffix: "".join(per_chrom[n][key] for n in names) for suffix, key in parts}
    texts[json_suffix] = json.dumps(js, indent=1, sort_keys=True) + "\n"
    mats = [] if matrix_suffix is None else [per_chrom[n]["matrix"] for n in names if per_chrom[n]["matrix"] is not None]
    if mats:
        texts[matrix_suffix] = mats[0]
    return texts, js


def _one_record(jd, chrom):
    recs = _records(jd, {chrom})
    if len(recs) != 1:
        raise ValueError("no cis .jd file of chromosome %s" % chrom)
    return recs[0][1]


def jd2window(jd, fout, region, region2=None, res=5000, cut=0, mirror=None, plot=False):
    """The contact matrix of `region` x `region2` (the diagonal window of `region`, mirrored, without a second one) ->
    `<fout>_matrix.txt`, `<fout>_matrix.json` and, with `plot`, `<fout>_matrix.pdf`; returns the json's content."""
    res, cut = check_res(res), int(cut)
    r1 = parse_region(region)
    r2 = r1 if region2 is None else parse_region(region2)
    if r2[0] != r1[0]:
        raise ValueError("both regions must lie on one chromosome (no trans matrices), got %s and %s" % (r1[0], r2[0]))
    if not window_fits(r1, r2, res):
        raise ValueError("the window needs more than %d bins a side or %d cells at -res %d; the smallest -res that fits is %d"
                         % (WMAX, CELLS_MAX, res, smallest_res(r1, r2)))
    mirror = region2 is None if mirror is None else bool(mirror)
    r = _one_record(jd, r1[0])
    logger.info("contact matrix of %s x %s" % (region, region2 or region))
    with r.lock:
        try:
            texts, js, mat = window_of(r.chrom, r1, r2, res, cut, mirror)
        finally:
            r.chrom.mat_free()
    write_outputs(fout, texts)
    if plot:
        plot_matrix(mat, js, fout)
    return js


def jd2cells(jd, fout, res=10000, cut=0, chroms=(), fold=True):
    """The non-empty cells of every cis chromosome of `jd` -> `<fout>_cells.txt` (bg2) and `<fout>_cells.json`; returns the json's
    content."""
    res, cut = check_res(res), int(cut)
    per_chrom = each_chrom(_records(jd, chroms), logger, "contact-matrix cells of %s", lambda ch, chrom: chrom_cells(ch, chrom, res, cut, bool(fold)))
    texts, js = cells_outputs(per_chrom, res, cut, bool(fold))
    write_outputs(fout, texts)
    return js


def jd2v4c(jd, fout, view, region=None, res=1000, cut=0, norm="none"):
    """The virtual-4C profile of the viewpoint `view` over `region` (the span of the chromosome's kept rows without one) ->
    `<fout>_v4c.bedGraph` and `<fout>_v4c.json`; returns the json's content."""
    res, cut = check_res(res), int(cut)
    if norm not in NORMS:
        raise ValueError("norm must be one of %s, got %r" % (", ".join(NORMS), norm))
    v = parse_region(view)
    rng = None if region is None else parse_region(region)
    if rng is not None and rng[0] != v[0]:
        raise ValueError("the viewpoint and the region must lie on one chromosome, got %s and %s" % (v[0], rng[0]))
    if rng is not None and region_bins(rng[1], rng[2], res)[1] > NB_MAX:
        raise ValueError("the region has more than 2^24 bins at -res %d" % res)
    r = _one_record(jd, v[0])
    logger.info("virtual 4C of %s" % view)
    with r.lock:
        try:
            texts, js, _ = v4c_of(r.chrom, v, rng, res, cut, norm)
        finally:
            r.chrom.mat_free()
    write_outputs(fout, texts)
    return js


def common(p, res, chroms=False):
    """-d -o -res -cut and, for a command over all chromosomes, -c; `res`: the command's default"""
    p.add_argument("-d", dest="d", required=True, type=str, help="The directory of cis .jd files.")
    p.add_argument("-o", dest="output", required=True, type=str, help="Output prefix.")
    p.add_argument("-res", dest="res", required=False, default=res, type=int, help="Bin size in bp, default %d." % res)
    p.add_argument("-cut", dest="cut", required=False, default=0, type=int, help="Distance cutoff to filter PETs, default 0.")
    if chroms:
        p.add_argument("-c", dest="chroms", required=False, default="", type=str,
                       help="Whether to process limited chroms, specify it as chr1,chr2,chr3, default is all.")


def chroms_of(op):
    """the `chroms` of a jd2* from the -c of `common`"""
    return [] if op.chroms == "" else set(op.chroms.split(","))


def help(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cloops_amd.matrix",
                                 description="Contact matrices on MI355X. "
                                             "For example: python -m cloops_amd.matrix window -d hic -o hic -r chr21:20000000-21000000")
    sub = ap.add_subparsers(dest="cmd")
    sub.required = True
    w = sub.add_parser("window", help="The dense contact matrix of a region, as text for a heatmap.")
    common(w, 5000)
    w.add_argument("-r", dest="region", required=True, type=str, help="The region of the rows, chrom:start-end.")
    w.add_argument("-r2", dest="region2", required=False, default=None, type=str,
                   help="The region of the columns, default the region of the rows (the diagonal window, mirrored).")
    w.add_argument("-mirror", dest="mirror", required=False, action="store_true",
                   help="Count every PET at its transposed cell too (default with one region).")
    w.add_argument("-plot", dest="plot", required=False, action="store_true", help="Draw the matrix into <o>_matrix.pdf.")
    c = sub.add_parser("cells", help="The non-empty cells of every chromosome, as bg2 text.")
    common(c, 10000, chroms=True)
    c.add_argument("-nofold", dest="nofold", required=False, action="store_true",
                   help="Keep a PET with Y bin below X bin in its own cell instead of the upper triangle's.")
    v = sub.add_parser("v4c", help="The interaction profile of one viewpoint, as a bedGraph.")
    common(v, 1000)
    v.add_argument("-v", dest="view", required=True, type=str, help="The viewpoint, chrom:start-end.")
    v.add_argument("-r", dest="region", required=False, default=None, type=str,
                   help="The region of the profile, default the span of the chromosome's PETs.")
    v.add_argument("-norm", dest="norm", required=False, default="none", choices=list(NORMS),
                   help="none: raw counts; cpm: counts per million contacts of the viewpoint, three decimals. Default none.")
    return ap.parse_args(argv)


def main(argv=None):
    op = help(argv)
    if op.cmd == "window":
        jd2window(op.d, op.output, op.region, region2=op.region2, res=op.res, cut=op.cut, mirror=True if op.mirror else None, plot=op.plot)
    elif op.cmd == "cells":
        jd2cells(op.d, op.output, res=op.res, cut=op.cut, chroms=chroms_of(op), fold=not op.nofold)
    else:
        jd2v4c(op.d, op.output, op.view, region=op.region, res=op.res, cut=op.cut, norm=op.norm)
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())
