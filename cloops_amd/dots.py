"""Loops called from the contact matrix itself: the local-enrichment ("donut") test of HiCCUPS (Rao et al. 2014; `cooltools dots`
restates it) on every pixel of a band of a chromosome's matrix, the thresholds of an FDR per chunk of the local expected count, the
enrichment filter, and the merging of the significant pixels into loops.

The reference has nothing of the kind: it calls loops by clustering PETs (cDBSCAN), which suits ChIA-PET and HiChIP; on Hi-C people run
this test.  The cells are K24's (`cl_mat_cells`, folded), the mask and the weights K25's, the expected values K26's
(`expected.expected_of`, `cl_exp_set`); the four neighbourhood sums of observed and expected around every pixel, the histogram and the
call run in kernel K29 over the state resident in HBM (`cl_dot_lambdas` / `cl_dot_hist` / `cl_dot_call` and their gets).  The
thresholds, the filter, the merging, the texts and the files stay on the host.

Definitions (include/cloops_hip.h, cl_dot_lambdas):
- Around a pixel (i, j) the device sums the balanced values V and the expected values E over four neighbourhoods -- donut, lower-left,
  horizontal, vertical, of inner half-width `-p` and outer half-width `-w` -- and gives la_k = ((NO_k / NE_k) expected[j - i]) / (w[i]
  w[j]): the raw count the pixel would have if it were as enriched as its neighbourhood.  A pixel takes part when all four are numbers.
- The diagonals are dmin = max(ignore_diags, p + 2, mindist // res) <= d < dmax = min(nb, maxdist // res + 1).
- Chunks of la: edges[l] = 2 ** (l / 3), l < `-chunks`; a pixel with a la above the last edge is left out (a warning says how many).
- Thresholds: per neighbourhood k and chunk l, with n the pixels of the chunk and ge[t] those with a count >= t, thr[k][l] is the
  smallest t in 1 .. 4095 with ge[t] > 0 and n poisson.sf(t - 1, edges[l]) <= fdr ge[t] -- the expected false positives at the chunk's
  upper edge over the observed ones; no such t: the chunk calls nothing.  A pixel is significant when its count reaches the threshold
  of its chunk in all four neighbourhoods.
- Enrichment filter, per significant pixel: cnt / la_donut >= e0, cnt / la_ll >= e1, cnt / la_h >= e2, cnt / la_v >= e3 and
  max(cnt / la_donut, cnt / la_ll) >= e4 (`-enrich e0,e1,e2,e3,e4`).
- Loops: the kept pixels are merged into connected components under Chebyshev distance <= max(1, merge // res) bins; a loop is its
  component's pixel of largest count (ties: the lowest (bx, by)), with the component's size and centroid (bp, the bins' centres);
  components of fewer than `-minpix` pixels are dropped.
- Deviations from HiCCUPS: w does not grow where the neighbourhood is sparse; there is no q-value rule for singletons, `-minpix` stands
  in for it; the enrichment filter runs per pixel before the merging, not on the merged loop.
- `<o>_dots.bedpe`: `chrom start1 end1 chrom start2 end2 count la_donut la_ll la_h la_v size cx cy` per loop; `<o>_dots_pixels.txt`:
  `chrom start1 end1 chrom start2 end2 count la_donut la_ll la_h la_v passed` per significant pixel; `<o>_dots_thresholds.txt`: `chrom
  kernel chunk edge pixels threshold` per neighbourhood and chunk (threshold `none` where the chunk calls nothing); `<o>_dots.json`:
  the arguments, per chromosome the statistics, and the warnings.  Floats are written with repr (they read back to the same bits), NaN
  as nan.
"""
import argparse
import logging
import sys

import numpy as np

from . import _lib, matrix
from .balance import balance_stats, balanced_state, check_args, not_converged
from .expected import add_options, check_exp_args, expected_state, options_of, parsed_options
from .matrix import CHUNK, check_res, chrom_outputs, chroms_of, common, each_chrom
from .peaks import write_outputs
from .similarity import fnum

logger = logging.getLogger("cloops_amd.dots")

SUFFIXES = ("_dots.bedpe", "_dots_pixels.txt", "_dots_thresholds.txt", "_dots.json")
KERNELS = ("donut", "ll", "h", "v")
WMAX, CHUNKS_MAX, CMAX = _lib.CL_DOT_WMAX, _lib.CL_DOT_CHUNKS_MAX, _lib.CL_DOT_CMAX
NO_THRESHOLD = 0xFFFFFFFF
DEFAULT_ENRICH = (1.75, 1.75, 1.5, 1.5, 2.0)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_dot_args(p, w, mindist, maxdist, fdr, chunks, merge, minpix, enrich):
    """-> (p, w, mindist, maxdist, fdr, chunks, merge, minpix, enrich: five floats) checked; ValueError otherwise"""
    for name, v in (("p", p), ("w", w), ("mindist", mindist), ("maxdist", maxdist), ("chunks", chunks), ("merge", merge), ("minpix", minpix)):
        if not _is_int(v):
            raise ValueError("%s must be an integer, got %r" % (name, v))
    if not 0 <= p < w <= WMAX:
        raise ValueError("needs 0 <= p < w <= %d, got p %d, w %d" % (WMAX, p, w))
    if mindist < 0 or maxdist < 0:
        raise ValueError("mindist and maxdist must be at or above 0, got %d and %d" % (mindist, maxdist))
    fdr = float(fdr)
    if not 0.0 < fdr <= 1.0:
        raise ValueError("fdr must lie in (0, 1], got %r" % (fdr,))
    if not 1 <= chunks <= CHUNKS_MAX:
        raise ValueError("chunks must lie in [1, %d], got %d" % (CHUNKS_MAX, chunks))
    if merge < 0:
        raise ValueError("merge must be at or above 0, got %d" % merge)
    if minpix < 1:
        raise ValueError("minpix must be at or above 1, got %d" % minpix)
    if isinstance(enrich, str):
        try:
            enrich = [float(x) for x in enrich.split(",")]
        except ValueError:
            raise ValueError("enrich is five numbers e0,e1,e2,e3,e4, got %r" % (enrich,))
    enrich = tuple(float(x) for x in enrich)
    if len(enrich) != 5 or not all(x >= 0.0 for x in enrich):
        raise ValueError("enrich is five numbers at or above 0, got %r" % (enrich,))
    return int(p), int(w), int(mindist), int(maxdist), fdr, int(chunks), int(merge), int(minpix), enrich


def default_edges(n_chunks):
    """edges[l] = 2 ** (l / 3), l < n_chunks: 1, then a doubling every three chunks"""
    return np.array([2.0 ** (l / 3.0) for l in range(int(n_chunks))], np.float64)


def band_of(nb, ign, p, res, mindist, maxdist):
    """-> (dmin, dmax) of the defaults: max(ign, p + 2, mindist // res), min(nb, maxdist // res + 1)"""
    return max(int(ign), int(p) + 2, int(mindist) // int(res)), min(int(nb), int(maxdist) // int(res) + 1)


def thresholds(hist, edges, fdr):
    """hist: uint64 [4, n_chunks, CMAX + 1] of cl_dot_hist -> (thr uint32 [4, n_chunks], n int64 [4, n_chunks]: the chunk's pixels).
    thr[k][l] is the smallest t in 1 .. CMAX with ge[t] > 0 and n poisson.sf(t - 1, edges[l]) <= fdr ge[t]; NO_THRESHOLD without one"""
    from scipy.stats import poisson
    hist, edges = np.asarray(hist), np.asarray(edges, np.float64)
    nk, nch, nc = hist.shape
    thr = np.full((nk, nch), NO_THRESHOLD, np.uint32)
    n = hist.astype(np.int64).sum(axis=2)
    t = np.arange(1, nc, dtype=np.int64)
    for l in range(nch):
        sf = poisson.sf(t - 1, float(edges[l]))
        for k in range(nk):
            if n[k, l] == 0:
                continue
            ge = np.cumsum(hist[k, l, ::-1].astype(np.int64))[::-1][1:]     # ge[t], t = 1 .. CMAX
            ok = np.flatnonzero((ge > 0) & (float(n[k, l]) * sf <= fdr * ge.astype(np.float64)))
            if len(ok):
                thr[k, l] = int(t[ok[0]])
    return thr, n


def enrichment_pass(cnt, la4, enrich):
    """-> bool per pixel: the five ratios of the filter hold (a la of 0 gives an infinite ratio, a NaN fails)"""
    cnt, la4 = np.asarray(cnt, np.float64), np.asarray(la4, np.float64).reshape(-1, 4)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = cnt[:, None] / la4
        return ((r[:, 0] >= enrich[0]) & (r[:, 1] >= enrich[1]) & (r[:, 2] >= enrich[2]) & (r[:, 3] >= enrich[3])
                & (np.maximum(r[:, 0], r[:, 1]) >= enrich[4]))


def merge_pixels(bx, by, cnt, r, minpix=1):
    """the connected components of the pixels under Chebyshev distance <= r -> [(index of the loop's pixel: the largest cnt, ties to
    the lowest (bx, by); size; mean bx; mean by)] of the components with at least minpix pixels, ascending by the loop's (bx, by)"""
    bx, by, cnt = np.asarray(bx, np.int64), np.asarray(by, np.int64), np.asarray(cnt, np.int64)
    n = len(bx)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    order = np.lexsort((by, bx)).tolist()
    for ai, a in enumerate(order):
        for b in order[ai + 1:]:
            if bx[b] - bx[a] > r:
                break
            if abs(int(by[b] - by[a])) <= r:
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    comps = {}
    for a in order:
        comps.setdefault(find(a), []).append(a)
    out = []
    for members in comps.values():
        if len(members) < minpix:
            continue
        best = min(members, key=lambda a: (-int(cnt[a]), int(bx[a]), int(by[a])))
        out.append((best, len(members), float(np.mean(bx[members])), float(np.mean(by[members]))))
    out.sort(key=lambda t: (int(bx[t[0]]), int(by[t[0]])))
    return out


def _pixel_columns(chrom, res, x, y, c, la):
    return "%s\t%d\t%d\t%s\t%d\t%d\t%d\t%s" % (chrom, x * res, (x + 1) * res, chrom, y * res, (y + 1) * res, c, "\t".join(fnum(v) for v in la))


def format_loops(chrom, res, bx, by, cnt, la4, loops):
    """`<o>_dots.bedpe` of one chromosome: the loop's pixel, its count and four la, the component's size and centroid in bp"""
    la4 = np.asarray(la4, np.float64).reshape(-1, 4)
    return "".join("%s\t%d\t%s\t%s\n" % (_pixel_columns(chrom, res, int(bx[a]), int(by[a]), int(cnt[a]), la4[a].tolist()), size,
                                       fnum((cx + 0.5) * res), fnum((cy + 0.5) * res)) for a, size, cx, cy in loops)


def format_pixels(chrom, res, bx, by, cnt, la4, passed):
    """`<o>_dots_pixels.txt` of one chromosome: every significant pixel, its four la and whether it passed the filter"""
    la4 = np.asarray(la4, np.float64).reshape(-1, 4)
    return "".join("%s\t%d\n" % (_pixel_columns(chrom, res, int(bx[a]), int(by[a]), int(cnt[a]), la4[a].tolist()), 1 if passed[a] else 0)
                   for a in range(len(bx)))


def format_thresholds(chrom, edges, n, thr):
    """`<o>_dots_thresholds.txt` of one chromosome: `chrom kernel chunk edge pixels threshold` per neighbourhood and chunk"""
    return "".join("%s\t%s\t%d\t%s\t%d\t%s\n" % (chrom, KERNELS[k], l, fnum(float(edges[l])), int(n[k, l]),
                                               "none" if int(thr[k, l]) == NO_THRESHOLD else "%d" % int(thr[k, l]))
                   for k in range(len(KERNELS)) for l in range(len(edges)))


def dots_chrom(ch, chrom, res, cut=0, p=2, w=5, mindist=0, maxdist=2000000, fdr=0.1, chunks=40, merge=20000, minpix=1, enrich=DEFAULT_ENRICH,
               chunk=CHUNK, **options):
    """One chromosome on the device: `ch` has the mat_*, bal_*, exp_* and dot_* methods of api.Chromosome; `options`: the records bal=
    and exp= (expected.options_of), or their fields as keywords -> dict(loops: text, pixels: text, thresholds: text, stats: the json's
    entry, warnings: [str], called: [(bx, by)] of the loops)"""
    bal, exp = options_of(**options)
    try:
        st = balanced_state(ch, res, cut, bal, exp.raw)
        expected_state(ch, st, bal, exp)
        nb, n_cells = st.nb, int(st.n_cells)
        dmin, dmax = band_of(nb, bal.ignore_diags, p, res, mindist, maxdist)
        edges = default_edges(chunks)
        no_band = nb > 0 and dmin >= dmax                                   # fewer bins than the nearest tested diagonal
        thr, n_chunk = np.full((4, chunks), NO_THRESHOLD, np.uint32), np.zeros((4, chunks), np.int64)
        n_cand = n_full = n_beyond = 0
        sig = np.zeros(0, np.int64)
        if nb == 0:
            dmin = dmax = 0
        if not no_band:
            n_cand, n_full = ch.dot_lambdas(p, w, dmin, dmax)
            hist, n_beyond = ch.dot_hist(edges)
            thr, n_chunk = thresholds(hist, edges, fdr)
            n_sig = ch.dot_call(thr)
            sig = ch.dot_sig(0, n_sig)
        sx, sy, sc, sla = [], [], [], []
        for first in range(0, n_cells, int(chunk)):                         # the significant cells, chunk by chunk of the cells
            k = min(int(chunk), n_cells - first)
            mine = sig[(sig >= first) & (sig < first + k)] - first
            if len(mine) == 0:
                continue
            bx, by, cnt = ch.mat_cells_get(first, k)
            la = ch.dot_cells(first, k)
            sx.append(bx[mine]); sy.append(by[mine]); sc.append(cnt[mine]); sla.append(la[mine])
        cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
        sx, sy, sc = cat(sx, np.int64), cat(sy, np.int64), cat(sc, np.int64)
        sla = np.concatenate(sla) if sla else np.zeros((0, 4))
    finally:
        ch.mat_free()
    passed = enrichment_pass(sc, sla, enrich)
    keep = np.flatnonzero(passed)
    loops = merge_pixels(sx[keep], sy[keep], sc[keep], max(1, merge // res), minpix)
    msg = not_converged(chrom, st, bal.tol, exp.raw, num=fnum)
    warnings = [] if msg is None else [msg]
    if no_band:
        warnings.append("%s has %d bins, no diagonal in [%d, %d): no test" % (chrom, nb, dmin, dmax))
    if n_beyond > 0:
        warnings.append("%s: %d pixels have a local expected count above the last edge %s and were left out (more -chunks)"
                        % (chrom, n_beyond, fnum(float(edges[-1]))))
    if n_cells > 0 and n_full == 0 and not no_band:
        warnings.append("%s has cells but no pixel with all four neighbourhoods: no test" % chrom)
    for msg in warnings:
        logger.warning("WARNING: " + msg)
    stats = dict(balance_stats(st), b0=int(st.b0), nb=int(nb), dmin=int(dmin), dmax=int(dmax), n_cells=n_cells, n_cand=int(n_cand),
                 n_full=int(n_full), n_beyond=int(n_beyond), n_sig=int(len(sig)), n_kept=int(len(keep)), n_loops=len(loops))
    return {"loops": format_loops(chrom, res, sx[keep], sy[keep], sc[keep], sla[keep], loops),
            "pixels": format_pixels(chrom, res, sx, sy, sc, sla, passed), "thresholds": format_thresholds(chrom, edges, n_chunk, thr),
            "stats": stats, "warnings": warnings, "called": [(int(sx[keep][a]), int(sy[keep][a])) for a, _, _, _ in loops]}


def dots_outputs(per_chrom, args):
    """{suffix: text} of the files from {chrom: dots_chrom's dict}, and the json's content"""
    js = {"args": args, "warnings": [m for n in sorted(per_chrom) for m in per_chrom[n]["warnings"]]}
    return chrom_outputs(per_chrom, ((SUFFIXES[0], "loops"), (SUFFIXES[1], "pixels"), (SUFFIXES[2], "thresholds")), SUFFIXES[3], js)


def jd2dots(jd, fout, res=10000, cut=0, chroms=(), p=2, w=5, mindist=0, maxdist=2000000, fdr=0.1, chunks=40, merge=20000, minpix=1,
            enrich=DEFAULT_ENRICH, raw=False, per_decade=10, nosmooth=False, ignore_diags=2, min_nnz=10, min_count=0, mad_max=5, tol=1e-5,
            max_iters=200):
    """The loops of every cis chromosome of `jd` by the donut test -> `<fout>_dots.bedpe`, `<fout>_dots_pixels.txt`,
    `<fout>_dots_thresholds.txt` and `<fout>_dots.json`; returns the json's content."""
    res, cut = check_res(res), int(cut)
    bal, exp = check_args(ignore_diags, min_nnz, min_count, mad_max, tol, max_iters), check_exp_args(raw, per_decade, nosmooth)
    p, w, mindist, maxdist, fdr, chunks, merge, minpix, enrich = check_dot_args(p, w, mindist, maxdist, fdr, chunks, merge, minpix, enrich)
    per_chrom = each_chrom(matrix._records(jd, chroms), logger, "dots of %s",
                           lambda ch, chrom: dots_chrom(ch, chrom, res, cut, p, w, mindist, maxdist, fdr, chunks, merge, minpix, enrich,
                                                        bal=bal, exp=exp))
    args = dict(bal._asdict(), res=res, cut=cut, p=p, w=w, mindist=mindist, maxdist=maxdist, fdr=fdr, chunks=chunks, merge=merge,
                minpix=minpix, enrich=list(enrich), **exp._asdict())
    texts, js = dots_outputs(per_chrom, args)
    write_outputs(fout, texts)
    return js


def help(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cloops_amd.dots",
                                 description="Loops from the contact matrix by the donut enrichment test (HiCCUPS) on MI355X. "
                                             "For example: python -m cloops_amd.dots -d hic -o hic -res 10000")
    common(ap, 10000, chroms=True)
    ap.add_argument("-p", dest="p", required=False, default=2, type=int, help="Half-width of the inner square left out around a pixel, default 2.")
    ap.add_argument("-w", dest="w", required=False, default=5, type=int, help="Half-width of the neighbourhoods, at most 16, default 5.")
    ap.add_argument("-mindist", dest="mindist", required=False, default=0, type=int, help="Nearest tested distance in bp, default 0.")
    ap.add_argument("-maxdist", dest="maxdist", required=False, default=2000000, type=int, help="Farthest tested distance in bp, default 2000000.")
    ap.add_argument("-fdr", dest="fdr", required=False, default=0.1, type=float, help="False discovery rate of a chunk's threshold, default 0.1.")
    ap.add_argument("-chunks", dest="chunks", required=False, default=40, type=int,
                    help="Chunks of the local expected count, edges 2 ** (l / 3), at most 64, default 40.")
    ap.add_argument("-merge", dest="merge", required=False, default=20000, type=int,
                    help="Significant pixels within this many bp (Chebyshev, at least one bin) join one loop, default 20000.")
    ap.add_argument("-minpix", dest="minpix", required=False, default=1, type=int, help="A loop needs this many pixels, default 1.")
    ap.add_argument("-enrich", dest="enrich", required=False, default=",".join(repr(x) for x in DEFAULT_ENRICH), type=str,
                    help="Least count over la of the donut, lower-left, horizontal and vertical neighbourhoods, and of the larger of the "
                         "first two, default 1.75,1.75,1.5,1.5,2.0.")
    add_options(ap)
    return ap.parse_args(argv)


def main(argv=None):
    op = help(argv)
    jd2dots(op.d, op.output, res=op.res, cut=op.cut, chroms=chroms_of(op), p=op.p, w=op.w, mindist=op.mindist, maxdist=op.maxdist, fdr=op.fdr,
            chunks=op.chunks, merge=op.merge, minpix=op.minpix, enrich=op.enrich, **parsed_options(op))
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())
