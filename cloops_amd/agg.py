"""Aggregate pile-up of the PETs around called loops: is a loop set any good?

The aggregate peak analysis of Rao et al. 2014 (`agg` of later cLoops versions; the reference itself has nothing of the kind): cut a
window of W x W bins of `res` bp, W = 2 w + 1, around every loop centre, pile the PETs of all loops into one matrix S and compare
its centre bin with its corners.  The counting is kernel K19 on the chromosome resident in HBM (`cl_agg_loops`): per loop the window's
matrix M, its total, centre and four corner sums, and S = the sum of M over the loops, all integers.  Everything else here is host
arithmetic on those integers in float64.

Definitions (include/cloops_hip.h, cl_agg_loops):
- A loop's centre is cx = (x1 + x2) // 2, cy = (y1 + y2) // 2 of its anchors `iva = chr:x1-x2`, `ivb = chr:y1-y2`; its window starts at
  ox = cx - w res - res // 2, oy likewise; a PET falls into cell ((X - ox) // res, (Y - oy) // res) when both differences lie in
  [0, W res).  Row index = the X bin.
- Corners are corner x corner cells: ll = M[W - corner:, :corner] (nearest the diagonal, the lower left of a Juicer plot), ul, ur, lr.
- A loop is used iff cy - cx >= min_dist, by default (2 w + 2) res: the whole window then lies strictly above the diagonal.  Skipped
  loops are counted and reported, as are loops between two chromosomes and loops on chromosomes without PETs.
- APA = S[w, w] / (S_ll / corner^2), P2UL / P2UR / P2LR likewise; ZscoreLL = (S[w, w] - mean(LL cells of S)) / std(the same, ddof 0);
  per loop P2LL = centre / (ll / corner^2); x / 0 is inf and 0 / 0 nan, as in numpy.
- Loops are read like quantifyLoops reads them (quant._anchor_columns, cModel.parseIv): the significant ones unless `-s`.
"""
import argparse
import json
import logging
import os
import sys

import numpy as np

from .cModel import parseIv
from .quant import _anchor_columns

logger = logging.getLogger("cloops_amd.agg")

STAT_COLS = ("total", "centre", "ll", "ul", "ur", "lr")         # the six per-loop integers of cl_agg_loops, in its order


def read_loops(f, sig=True, chroms=(), ivac=None, ivbc=None):
    """the loops of the `.loop` file `f` -> (loops in the file, loops taken, loops between two chromosomes, {chrom: {loopId:
    [c, x1, x2, c, y1, y2]}}): only the significant ones (last column >= 1) when `sig`, only those of `chroms` if given; a loop whose
    anchors lie on two chromosomes is counted and left out; chromosomes and loops keep the file's order"""
    ivac, ivbc = _anchor_columns(f, ivac, ivbc)
    n_file, n_taken, n_trans, out = 0, 0, 0, {}
    for i, line in enumerate(open(f)):
        if i == 0:
            continue
        line = line.split("\n")[0].split("\t")
        if len(line) <= max(ivac, ivbc):
            continue
        n_file += 1
        if sig and float(line[-1]) < 1:
            continue
        iva, ivb = parseIv(line[ivac]), parseIv(line[ivbc])
        if len(chroms) > 0 and iva[0] not in chroms:
            continue
        n_taken += 1
        if iva[0] != ivb[0]:
            n_trans += 1
            continue
        out.setdefault(iva[0], {})[line[0]] = iva + ivb
    return n_file, n_taken, n_trans, out


def loop_centres(rs):
    """records [c, x1, x2, c, y1, y2] (a list, or the dict loopId -> record) -> (cx, cy) int64: the anchors' mid-points, floored"""
    rs = list(rs.values()) if isinstance(rs, dict) else list(rs)
    a = np.asarray([[r[1], r[2], r[4], r[5]] for r in rs], dtype=np.int64).reshape(-1, 4)
    return (a[:, 0] + a[:, 1]) // 2, (a[:, 2] + a[:, 3]) // 2


def default_min_dist(res, w):
    """the smallest cy - cx whose window lies strictly above the diagonal: its nearest cell starts (2 w + 1) res above it"""
    return (2 * int(w) + 2) * int(res)


def select_loops(cx, cy, res, w, min_dist=None):
    """-> (keep bool [n], number skipped): a loop is used iff cy - cx >= min_dist (None: default_min_dist)"""
    cx, cy = np.asarray(cx, dtype=np.int64), np.asarray(cy, dtype=np.int64)
    md = default_min_dist(res, w) if min_dist is None else int(min_dist)
    keep = (cy - cx) >= md
    return keep, int((~keep).sum())


def window_origin(c, res, w):
    """the first coordinate of the window around centre `c`: the centre bin is [c - res // 2, c - res // 2 + res)"""
    return c - int(w) * int(res) - int(res) // 2


def corner_blocks(M, corner):
    """-> the (ll, ul, ur, lr) corner x corner blocks of a matrix (or of a stack of matrices, last two axes)"""
    M = np.asarray(M)
    k, W = int(corner), M.shape[-1]
    return M[..., W - k:, :k], M[..., :k, :k], M[..., :k, W - k:], M[..., W - k:, W - k:]


def scores(S, corner):
    """the aggregate's five scores from S (W x W integers) -> dict(APA, P2UL, P2UR, P2LR, ZscoreLL), float64 with numpy's x / 0 = inf
    and 0 / 0 = nan"""
    S = np.asarray(S, dtype=np.float64)
    w = (S.shape[0] - 1) // 2
    k2 = float(int(corner) ** 2)
    c = S[w, w]
    ll, ul, ur, lr = corner_blocks(S, corner)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {name: float(np.float64(c) / (np.float64(b.sum()) / k2)) for name, b in (("APA", ll), ("P2UL", ul), ("P2UR", ur), ("P2LR", lr))}
        out["ZscoreLL"] = float((np.float64(c) - ll.mean()) / ll.std(ddof=0))
    return out


def p2ll(stats, corner):
    """per loop centre / (ll / corner^2) from the stats table of cl_agg_loops -> float64 [n]"""
    st = np.asarray(stats, dtype=np.float64).reshape(-1, 6)
    with np.errstate(divide="ignore", invalid="ignore"):
        return st[:, 1] / (st[:, 2] / float(int(corner) ** 2))


def _chrom_files(jd, chroms):
    """`jd`: a directory of `<chrom>-<chrom>.jd` files, or a list of .jd paths / 'mem://' names of pipe.CACHE -> {chrom: name}"""
    from .pipe import CACHE
    out = {}
    if isinstance(jd, str):
        for c in chroms:
            f = os.path.join(jd, "%s-%s.jd" % (c, c))
            if os.path.isfile(f):
                out[c] = f
        return out
    for f in jd:
        if f.startswith("mem://"):
            key = CACHE.get(f).key
        else:
            key = tuple(os.path.splitext(os.path.split(f)[-1])[0].split("-"))
        if len(key) == 2 and key[0] == key[1]:
            out[key[0]] = f
    return out


def plot_agg(S, sc, n_used, res, prefix):
    """heat map of S -> `<prefix>_agg.pdf` (row = X bin, drawn downwards, so that the corner nearest the diagonal is the lower left as
    in a Juicer plot); no matplotlib: a warning and False"""
    try:
        from matplotlib.figure import Figure
        from matplotlib.backends.backend_agg import FigureCanvasAgg
    except ImportError as e:
        logger.warning("WARNING: no heat map drawn for %s_agg.pdf (%s)" % (prefix, e))
        return False
    S = np.asarray(S, dtype=np.float64)
    w = (S.shape[0] - 1) // 2
    fig = Figure(figsize=(5, 4.4))
    FigureCanvasAgg(fig)
    ax = fig.add_subplot(1, 1, 1)
    ext = (w + 0.5) * res / 1000.0
    im = ax.imshow(S, origin="upper", cmap="Reds", interpolation="nearest", extent=(-ext, ext, ext, -ext))
    fig.colorbar(im, ax=ax, label="PETs")
    ax.set_xlabel("distance from the loop's second anchor (kb)")
    ax.set_ylabel("distance from the loop's first anchor (kb)")
    ax.set_title("%d loops, APA %.3f, Z-score LL %.3f" % (n_used, sc["APA"], sc["ZscoreLL"]))
    fig.savefig("%s_agg.pdf" % prefix)
    return True


def aggLoops(loop_file, jd, out=None, res=1000, w=10, corner=3, cut=0, min_dist=None, sig=True, chroms=(), plot=False):
    """The aggregate of the loops of `loop_file` on the PETs of `jd` (a directory of `<chrom>-<chrom>.jd` files, or a list of .jd
    paths / 'mem://' names of pipe.CACHE, so the chromosomes of a finished sweep serve without files) -> dict(S int64 [W, W],
    rows = [(loopId, cx, cy, total, centre, ll, ul, ur, lr, P2LL)], summary = the content of `<out>_agg.json`).  With `out` it writes
    `<out>_agg.txt` (S, W tab-separated rows), `<out>_agg_loops.txt` (one row per used loop) and `<out>_agg.json`; `plot` adds
    `<out>_agg.pdf`."""
    from .pipe import CACHE
    res, w, corner = int(res), int(w), int(corner)
    W = 2 * w + 1
    n_file, n_taken, n_trans, loops = read_loops(loop_file, sig, chroms)
    files = _chrom_files(jd, list(loops.keys()))
    S = np.zeros((W, W), dtype=np.int64)
    rows, used, near, no_pets, n_pets = [], 0, 0, 0, 0
    for chrom, rs in loops.items():
        r = CACHE.get(files[chrom]) if chrom in files else None
        if r is None or len(r.X) == 0:
            logger.warning("WARNING: no PETs for %s, its %d loops are left out of the aggregate" % (chrom, len(rs)))
            no_pets += len(rs)
            continue
        cx, cy = loop_centres(rs)
        keep, skipped = select_loops(cx, cy, res, w, min_dist)
        near += skipped
        ids = [k for k, ok in zip(rs.keys(), keep.tolist()) if ok]
        cx, cy = cx[keep], cy[keep]
        with r.lock:
            s, stats, _, kept = r.chrom.agg_loops(cx, cy, res, w, corner, cut)
        S += s
        n_pets += kept
        used += len(ids)
        ratio = p2ll(stats, corner)
        rows += [(i, int(a), int(b)) + tuple(int(v) for v in st) + (float(p),) for i, a, b, st, p in zip(ids, cx, cy, stats, ratio)]
    sc = scores(S, corner)
    summary = {"loop_file": loop_file, "loops_in_file": n_file, "loops_read": n_taken, "loops_used": used,
               "loops_skipped_near_diagonal": near, "loops_without_pets": no_pets, "loops_between_chromosomes": n_trans,
               "pets": n_pets, "significant_only": bool(sig),
               "res": res, "w": w, "corner": corner, "cut": int(cut), "min_dist": default_min_dist(res, w) if min_dist is None else int(min_dist),
               "scores": sc}
    logger.info("%s: %d loops read, %d used, %d skipped near the diagonal, %d without PETs; APA %s, ZscoreLL %s"
                % (loop_file, n_taken, used, near, no_pets, sc["APA"], sc["ZscoreLL"]))
    if out is not None:
        with open(out + "_agg.txt", "w") as fh:
            for row in S.tolist():
                fh.write("\t".join(str(v) for v in row) + "\n")
        with open(out + "_agg_loops.txt", "w") as fh:
            fh.write("\t".join(("loopId", "cx", "cy") + STAT_COLS + ("P2LL",)) + "\n")
            for row in rows:
                fh.write("\t".join(str(v) for v in row) + "\n")
        with open(out + "_agg.json", "w") as fh:
            json.dump(summary, fh, indent=1, sort_keys=True)
            fh.write("\n")
        if plot:
            plot_agg(S, sc, used, res, out)
    return {"S": S, "rows": rows, "summary": summary}


def help(argv=None):
    ap = argparse.ArgumentParser(description="Aggregate pile-up of PETs around called loops on MI355X. "
                                             "For example: python -m cloops_amd.agg -d trac -f trac.loop -o trac")
    ap.add_argument("-d", dest="d", required=True, type=str, help="The directory of cis .jd files.")
    ap.add_argument("-f", dest="f", required=True, type=str, help="Loops file called by cLoops.")
    ap.add_argument("-o", dest="output", required=True, type=str, help="Output prefix.")
    ap.add_argument("-res", dest="res", required=False, default=1000, type=int, help="Bin size in bp, default 1000.")
    ap.add_argument("-w", dest="w", required=False, default=10, type=int, help="Half width of the window in bins (1..20), default 10.")
    ap.add_argument("-corner", dest="corner", required=False, default=3, type=int, help="Side of the corner blocks in bins, default 3.")
    ap.add_argument("-cut", dest="cut", required=False, default=0, type=int, help="Distance cutoff to filter PETs, default 0.")
    ap.add_argument("-minDist", dest="minDist", required=False, default=None, type=int,
                    help="Smallest distance between a loop's anchor centres, default (2 w + 2) res.")
    ap.add_argument("-s", dest="significant", required=False, action="store_false",
                    help="Use every loop of the file. Default is the significant ones only.")
    ap.add_argument("-c", dest="chroms", required=False, default="", type=str,
                    help="Whether to process limited chroms, specify it as chr1,chr2,chr3, default is all.")
    ap.add_argument("-plot", dest="plot", required=False, action="store_true", help="Draw the heat map of the aggregate.")
    return ap.parse_args(argv)


def main(argv=None):
    op = help(argv)
    chroms = [] if op.chroms == "" else set(op.chroms.split(","))
    aggLoops(op.f, op.d, op.output, res=op.res, w=op.w, corner=op.corner, cut=op.cut, min_dist=op.minDist, sig=op.significant,
             chroms=chroms, plot=op.plot)
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())
