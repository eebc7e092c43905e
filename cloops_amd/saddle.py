"""Saddle plots and compartment strength: the bins of every chromosome sorted into quantile classes of a per-bin track (the E1 of
`cloops_amd.compartments`), the mean observed / expected contact of every pair of classes, and one number for the plot -- the strength
(AA + BB) / (AB + BA) -- what `cooltools saddle` computes.

The reference has nothing of the kind.  The cells are K24's (`cl_mat_cells`, folded), the mask and the weights K25's, the expected values
K26's (`expected.expected_state`, `cl_exp_set`); the three tables per chromosome -- bin pairs, cells and O/E sums per pair of classes --
come from kernel K30 over the cells resident in HBM (`cl_sad_sums` / `cl_sad_get`).  The track, the edges, the classes, the band, the
symmetrising, the strength, the texts and the files stay on the host.

Definitions (include/cloops_hip.h, cl_sad_sums):
- The track per bin: `compartments.bin_track` of the `-track` bedGraph over the genome bins of `res` bp, bin 0 first; a bin of a
  chromosome beyond the track's last interval has no value.
- The edges: Q + 1 of them (`-q` Q, at most 62), the quantiles `linspace(qlo, qhi, Q + 1)` (`-qrange`) of all track values of the chosen
  chromosomes that the track names, taken once, genome-wide; `-vrange lo,hi` replaces them with Q + 1 equally spaced values.
- Classes: n_cls = Q + 2.  Class 0 is below the first edge, class Q + 1 above the last edge, and the classes 1 .. Q are
  `searchsorted(edges[1:-1], v, "right") + 1`: a value on an edge belongs to the class that starts there, a value equal to the last
  edge to class Q.  Class -1 -- the bin takes no part -- is for a NaN track value and for an invalid bin (K26's validity).
- The band: lo = max(ignore_diags, 1, ceil(mindist / res)) and hi = min(`compartments.pick_dmax`, nb), with `-maxdist` m > 0 also at
  most floor(m / res) + 1; lo is at most nb and hi at least lo (an empty band: zero tables).  A chromosome with fewer bins than
  max(ignore_diags, 1) has no band and no call.
- A chromosome without a track value is warned about and left out, before any call on it.
- Per chromosome K30's tables over the pairs i < j: sum, pairs, cells [n_cls, n_cls], row = the class of the lower bin.  The host
  symmetrises: S = sum + sum^T, N = pairs + pairs^T.  The genome-wide tables are the per-chromosome tables added in plain string order
  of the names (fp64 in that fixed order).
- Strength: k = max(1, round(corner Q)); A = the classes Q - k + 1 .. Q, B = the classes 1 .. k (the outer classes 0 and Q + 1 take
  no part); strength = ((S_AA + S_BB) / (N_AA + N_BB)) / ((S_AB + S_BA) / (N_AB + N_BA)), AA/AB = (S_AA / N_AA) / (that denominator),
  BB/AB likewise; per chromosome and genome-wide, NaN where a denominator is 0.
- `<o>_saddle.txt`: the genome-wide S / N, (Q + 2)^2, labelled by the classes' lower edges, NaN where N = 0; `<o>_saddle_sums.txt`:
  `chrom a b sum pairs cells` per chromosome and for `all`, before symmetrising; `<o>_saddle_bins.txt`: `class lo hi n_bins` per
  class; `<o>_saddle.json`: the arguments and the edges, per chromosome b0, nb, n_binned, n_pairs, n_in, lo, hi, the strengths and the
  balance statistics, and the genome-wide strengths; with `-plot` `<o>_saddle.pdf`, log-scaled.  Floats as %.10g, NaN as nan.
"""
import argparse
import logging
import sys

import numpy as np

from . import matrix
from .balance import _num, balance_stats, balanced_state, check_args, fmt, not_converged
from .compartments import bin_track, pick_dmax, read_bedgraph
from .expected import add_options, check_exp_args, expected_state, options_of, parsed_options
from .matrix import check_res, chrom_outputs, chroms_of, common, each_chrom
from .peaks import write_outputs

logger = logging.getLogger("cloops_amd.saddle")

SUFFIXES = ("_saddle.txt", "_saddle_sums.txt", "_saddle_bins.txt", "_saddle.json")
Q_MAX = 62                                                                  # CL_SAD_CLASSES_MAX - 2


def _pair(v, name):
    """`lo,hi` or a pair of numbers -> (float, float); ValueError otherwise"""
    try:
        a, b = (v.split(",") if isinstance(v, str) else v)
        return float(a), float(b)
    except (TypeError, ValueError):
        raise ValueError("%s is written lo,hi, got %r" % (name, v))


def check_saddle_args(q=50, qrange=(0.025, 0.975), vrange=None, mindist=0, maxdist=0, corner=0.2):
    """-> (Q, (qlo, qhi), (vlo, vhi) or None, mindist, maxdist, corner) checked; ValueError otherwise"""
    if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 1 <= q <= Q_MAX:
        raise ValueError("q must be an integer in [1, %d], got %r" % (Q_MAX, q))
    qlo, qhi = _pair(qrange, "qrange")
    if not 0.0 <= qlo < qhi <= 1.0:
        raise ValueError("qrange needs 0 <= lo < hi <= 1, got %r" % (qrange,))
    if vrange is not None:
        vrange = _pair(vrange, "vrange")
        if not (np.isfinite(vrange[0]) and np.isfinite(vrange[1]) and vrange[0] < vrange[1]):
            raise ValueError("vrange needs finite lo < hi, got %r" % (vrange,))
    try:
        mindist, maxdist = int(mindist), int(maxdist)
    except (TypeError, ValueError):
        raise ValueError("mindist and maxdist must be integers")
    if mindist < 0 or maxdist < 0 or (maxdist > 0 and maxdist < mindist):
        raise ValueError("mindist and maxdist must not be negative, and maxdist (0: none) not below mindist, got %d and %d" % (mindist, maxdist))
    corner = float(corner)
    if not 0.0 < corner <= 0.5:
        raise ValueError("corner must lie in (0, 0.5], got %r" % (corner,))
    return int(q), (qlo, qhi), vrange, mindist, maxdist, corner


def edges_of(values, q, qrange=(0.025, 0.975), vrange=None):
    """the Q + 1 edges: equally spaced over `vrange`, or the quantiles linspace(qlo, qhi, Q + 1) of the values that are numbers"""
    if vrange is not None:
        return np.linspace(vrange[0], vrange[1], q + 1)
    v = np.asarray(values, np.float64)
    v = v[~np.isnan(v)]
    if len(v) == 0:
        raise ValueError("the track has no value on the chosen chromosomes")
    return np.quantile(v, np.linspace(qrange[0], qrange[1], q + 1))


def classes_of(track, valid, edges):
    """the class of every bin -> int32: 0 below the first edge, Q + 1 above the last, 1 .. Q between (a value on an edge: the class that
    starts there; on the last edge: Q), -1 for a NaN value or an invalid bin"""
    v, e = np.asarray(track, np.float64), np.asarray(edges, np.float64)
    q = len(e) - 1
    ok = ~np.isnan(v) & np.asarray(valid, bool)
    cls = np.full(len(v), -1, np.int32)
    x = v[ok]
    k = (np.searchsorted(e[1:-1], x, "right") + 1).astype(np.int32)
    k[x < e[0]] = 0
    k[x > e[-1]] = q + 1
    cls[ok] = k
    return cls


def band_of(n_pairs, expected, ignore_diags, nb, res, mindist=0, maxdist=0):
    """the band (lo, hi) of a chromosome of nb bins, or None where it has fewer bins than max(ignore_diags, 1)"""
    near = max(int(ignore_diags), 1)
    if nb == 0:
        return 0, 0
    if nb < near:
        return None
    lo = min(max(near, -(-int(mindist) // int(res))), nb)
    hi = min(pick_dmax(n_pairs, expected, ignore_diags), nb)
    if maxdist > 0:
        hi = min(hi, int(maxdist) // int(res) + 1)
    return lo, max(hi, lo)


def corner_classes(q, corner):
    """-> (A, B): the k = max(1, round(corner Q)) highest and lowest of the classes 1 .. Q"""
    k = max(1, int(round(corner * q)))
    return np.arange(q - k + 1, q + 1), np.arange(1, k + 1)


def strength_of(sum_, pairs, corner):
    """the three strengths of the tables [Q + 2, Q + 2] before symmetrising -> dict(strength, aa_ab, bb_ab), NaN where a denominator is 0"""
    s, n = np.asarray(sum_, np.float64), np.asarray(pairs, np.int64)
    S, N = s + s.T, n + n.T
    A, B = corner_classes(len(S) - 2, corner)
    blk = lambda M, r, c: M[np.ix_(r, c)].sum()
    over = lambda a, b: float(a) / float(b) if b != 0 else float("nan")
    saa, sbb, sab = blk(S, A, A), blk(S, B, B), blk(S, A, B) + blk(S, B, A)
    naa, nbb, nab = int(blk(N, A, A)), int(blk(N, B, B)), int(blk(N, A, B) + blk(N, B, A))
    ab = over(sab, nab)
    ratio = lambda x: x / ab if ab == ab and ab != 0 else float("nan")
    return {"strength": ratio(over(saa + sbb, naa + nbb)), "aa_ab": ratio(over(saa, naa)), "bb_ab": ratio(over(sbb, nbb))}


def class_bounds(edges):
    """(lo, hi) of every class 0 .. Q + 1"""
    e = [float("-inf")] + np.asarray(edges, np.float64).tolist() + [float("inf")]
    return [(e[c], e[c + 1]) for c in range(len(e) - 1)]


def format_sums(chrom, sum_, pairs, cells):
    """`<o>_saddle_sums.txt` of one chromosome (or `all`): `chrom a b sum pairs cells` per pair of classes"""
    n = len(sum_)
    return "".join("%s\t%d\t%d\t%s\t%d\t%d\n" % (chrom, a, b, fmt(sum_[a][b]), pairs[a][b], cells[a][b]) for a in range(n) for b in range(n))


def format_saddle(edges, sum_, pairs):
    """`<o>_saddle.txt`: S / N of the symmetrised tables, labelled by the classes' lower edges, NaN where N = 0"""
    s, n = np.asarray(sum_, np.float64), np.asarray(pairs, np.int64)
    S, N = s + s.T, n + n.T
    mean = np.full(S.shape, np.nan)
    mean[N > 0] = S[N > 0] / N[N > 0]
    labels = [fmt(lo) for lo, _ in class_bounds(edges)]
    lines = ["\t" + "\t".join(labels)]
    for a in range(len(mean)):
        lines.append(labels[a] + "\t" + "\t".join(fmt(v) for v in mean[a].tolist()))
    return "\n".join(lines) + "\n", mean


def format_bins(edges, n_bins):
    """`<o>_saddle_bins.txt`: `class lo hi n_bins` per class"""
    return "".join("%d\t%s\t%s\t%d\n" % (c, fmt(lo), fmt(hi), n_bins[c]) for c, (lo, hi) in enumerate(class_bounds(edges)))


def saddle_chrom(ch, chrom, res, track, edges, cut=0, mindist=0, maxdist=0, corner=0.2, **options):
    """One chromosome on the device: `ch` has the mat_*, bal_*, exp_* and sad_* methods of api.Chromosome; track: the values of the
    genome bins 0 .. len - 1; `options`: the records bal= and exp= (expected.options_of), or their fields as keywords
    -> dict(sums: text, stats: the json's entry, tables: (sum, pairs, cells), n_bins: the binned bins per class)"""
    bal, exp = options_of(**options)
    n_cls = len(edges) + 1
    try:
        st = balanced_state(ch, res, cut, bal, exp.raw)
        nb = st.nb
        valid = np.asarray(st.mask, bool) if exp.raw else ~np.isnan(ch.bal_weights(0, nb))
        ex = expected_state(ch, st, bal, exp)
        mine = np.full(nb, np.nan)
        k0, k1 = max(int(st.b0), 0), min(int(st.b0) + nb, len(track))
        if k0 < k1:
            mine[k0 - st.b0:k1 - st.b0] = np.asarray(track, np.float64)[k0:k1]
        cls = classes_of(mine, valid, edges)
        band = band_of(ex.n_pairs, ex.expected, bal.ignore_diags, nb, res, mindist, maxdist)
        zeros = (np.zeros((n_cls, n_cls)), np.zeros((n_cls, n_cls), np.int64), np.zeros((n_cls, n_cls), np.int64))
        if band is None:
            n_binned, n_pairs, n_in, tables = int(np.count_nonzero(cls >= 0)), 0, 0, zeros
        else:
            n_binned, n_pairs, n_in = ch.sad_sums(cls, n_cls, band[0], band[1])
            tables = ch.sad_get()
    finally:
        ch.mat_free()
    msg = not_converged(chrom, st, bal.tol, exp.raw)
    if msg is not None:
        logger.warning("WARNING: " + msg)
    if band is None:
        logger.warning("WARNING: %s has %d bins, fewer than the %d nearest diagonals left out: no saddle" % (chrom, nb, max(bal.ignore_diags, 1)))
        band = (0, 0)
    stats = dict(balance_stats(st), b0=int(st.b0), nb=int(nb), n_binned=int(n_binned), n_pairs=int(n_pairs), n_in=int(n_in), lo=int(band[0]),
                 hi=int(band[1]), **{k: _num(v) for k, v in strength_of(tables[0], tables[1], corner).items()})
    return {"sums": format_sums(chrom, *tables), "stats": stats, "tables": tables, "n_bins": np.bincount(cls[cls >= 0], minlength=n_cls)}


def saddle_outputs(per_chrom, args, edges, corner):
    """{suffix: text} of the files from {chrom: saddle_chrom's dict}, the json's content and the genome-wide S / N"""
    n_cls = len(edges) + 1
    tot = [np.zeros((n_cls, n_cls)), np.zeros((n_cls, n_cls), np.int64), np.zeros((n_cls, n_cls), np.int64)]
    n_bins = np.zeros(n_cls, np.int64)
    for n in sorted(per_chrom):                                             # (fp64 in the fixed order of the names)
        for k in range(3):
            tot[k] = tot[k] + per_chrom[n]["tables"][k]
        n_bins += per_chrom[n]["n_bins"]
    strengths = {k: _num(v) for k, v in strength_of(tot[0], tot[1], corner).items()}
    texts, js = chrom_outputs(per_chrom, ((SUFFIXES[1], "sums"),), SUFFIXES[3],
                              {"args": args, "edges": [_num(e) for e in np.asarray(edges).tolist()], "all": strengths})
    texts[SUFFIXES[1]] += format_sums("all", *tot)
    texts[SUFFIXES[0]], mean = format_saddle(edges, tot[0], tot[1])
    texts[SUFFIXES[2]] = format_bins(edges, n_bins.tolist())
    return texts, js, mean


def plot_saddle(mean, js, prefix):
    """`<prefix>_saddle.pdf`: log10 of S / N as a heatmap; no matplotlib: a warning and False"""
    try:
        from matplotlib.figure import Figure
        from matplotlib.backends.backend_agg import FigureCanvasAgg
    except ImportError as e:
        logger.warning("WARNING: no picture drawn for %s_saddle.pdf (%s)" % (prefix, e))
        return False
    fig = Figure()
    FigureCanvasAgg(fig)
    ax = fig.add_subplot(1, 1, 1)
    m = np.asarray(mean, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        im = ax.imshow(np.log10(np.where(m > 0, m, np.nan)), cmap="coolwarm", interpolation="nearest", aspect="equal")
    ax.set_xlabel("class of the track (low to high)")
    ax.set_ylabel("class of the track (low to high)")
    ax.set_title("log10(observed / expected), strength %s" % fmt(float("nan") if js["all"]["strength"] is None else js["all"]["strength"]), fontsize=9)
    fig.colorbar(im)
    fig.savefig(prefix + "_saddle.pdf")
    return True


def genome_tracks(per, names, res):
    """the track over the genome bins of the chromosomes `names` that read_bedgraph's `per` holds -> {chrom: float64}"""
    out = {}
    for n in names:
        if n in per:
            s, e, v = per[n]
            out[n] = bin_track(s, e, v, 0, int((int(e.max()) - 1) // res + 1) if len(e) and e.max() > 0 else 0, res)
    return out


def jd2saddle(jd, fout, track, res=100000, cut=0, chroms=(), q=50, qrange=(0.025, 0.975), vrange=None, mindist=0, maxdist=0, corner=0.2,
              plot=False, raw=False, per_decade=10, nosmooth=False, ignore_diags=2, min_nnz=10, min_count=0, mad_max=5, tol=1e-5, max_iters=200):
    """The saddle tables and the compartment strength of every cis chromosome of `jd` that the bedGraph `track` has values for ->
    `<fout>_saddle.txt`, `<fout>_saddle_sums.txt`, `<fout>_saddle_bins.txt`, `<fout>_saddle.json` and, with `plot`,
    `<fout>_saddle.pdf`; returns the json's content."""
    res, cut = check_res(res), int(cut)
    bal, exp = check_args(ignore_diags, min_nnz, min_count, mad_max, tol, max_iters), check_exp_args(raw, per_decade, nosmooth)
    q, qrange, vrange, mindist, maxdist, corner = check_saddle_args(q, qrange, vrange, mindist, maxdist, corner)
    if track is None:
        raise ValueError("a track is needed (a bedGraph, such as the <o>_E1.bedGraph of cloops_amd.compartments)")
    recs = matrix._records(jd, chroms)
    tracks = genome_tracks(read_bedgraph(track), [c for c, _ in recs], res)
    have = {n for n, t in tracks.items() if np.count_nonzero(~np.isnan(t))}
    for c, _ in recs:
        if c not in have:
            logger.warning("WARNING: the track has no value on %s: left out" % c)
    recs = [(c, r) for c, r in recs if c in have]
    edges = edges_of(np.concatenate([tracks[c] for c, _ in recs]) if recs else np.zeros(0), q, qrange, vrange)
    per_chrom = each_chrom(recs, logger, "saddle tables of %s",
                           lambda ch, chrom: saddle_chrom(ch, chrom, res, tracks[chrom], edges, cut, mindist, maxdist, corner, bal=bal, exp=exp))
    args = dict(bal._asdict(), res=res, cut=cut, track=track, q=q, qrange=list(qrange), vrange=None if vrange is None else list(vrange),
                mindist=mindist, maxdist=maxdist, corner=corner, **exp._asdict())
    texts, js, mean = saddle_outputs(per_chrom, args, edges, corner)
    write_outputs(fout, texts)
    if plot:
        plot_saddle(mean, js, fout)
    return js


def help(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cloops_amd.saddle",
                                 description="Saddle plots and compartment strength on MI355X. "
                                             "For example: python -m cloops_amd.saddle -d hic -o hic -track hic_E1.bedGraph -res 100000")
    common(ap, 100000, chroms=True)
    ap.add_argument("-track", dest="track", required=True, type=str,
                    help="A bedGraph whose per-bin mean sorts the bins into classes, such as the <o>_E1.bedGraph of cloops_amd.compartments.")
    ap.add_argument("-q", dest="q", required=False, default=50, type=int, help="Quantile classes between the edges, 1 to 62, default 50.")
    ap.add_argument("-qrange", dest="qrange", required=False, default="0.025,0.975", type=str,
                    help="The quantiles of the first and the last edge, default 0.025,0.975.")
    ap.add_argument("-vrange", dest="vrange", required=False, default=None, type=str,
                    help="lo,hi: equally spaced edges between two track values instead of quantiles.")
    ap.add_argument("-mindist", dest="mindist", required=False, default=0, type=int, help="Smallest distance of a bin pair in bp, default 0.")
    ap.add_argument("-maxdist", dest="maxdist", required=False, default=0, type=int,
                    help="Largest distance of a bin pair in bp, default 0: as far as the expected values reach.")
    ap.add_argument("-corner", dest="corner", required=False, default=0.2, type=float,
                    help="Share of the classes at either end that make the strength's corners, default 0.2.")
    ap.add_argument("-plot", dest="plot", required=False, action="store_true", help="Draw the saddle into <o>_saddle.pdf.")
    add_options(ap)
    return ap.parse_args(argv)


def main(argv=None):
    op = help(argv)
    jd2saddle(op.d, op.output, op.track, res=op.res, cut=op.cut, chroms=chroms_of(op), q=op.q, qrange=op.qrange, vrange=op.vrange,
              mindist=op.mindist, maxdist=op.maxdist, corner=op.corner, plot=op.plot, **parsed_options(op))
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())
