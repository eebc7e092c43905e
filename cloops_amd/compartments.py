"""A/B compartments: the leading eigenvectors of a chromosome's observed / expected contact matrix minus one -- what `cooltools
eigs-cis` computes -- oriented by a per-bin track and written as a table, a bedGraph of the first vector and the compartment runs.

The reference has nothing of the kind.  The cells are K24's (`cl_mat_cells`, folded), the mask and the weights K25's, the expected values
K26's (`expected.expected_of`, `cl_exp_set`); the matrix-vector products and the subspace iteration run in kernel K27 over the cells
resident in HBM (`cl_eig_build` / `cl_eig_iterate` / `cl_eig_vectors_get`).  The choice of dmax and clip, the orientation, the texts and
the files stay on the host.

Definitions (include/cloops_hip.h, cl_eig_build):
- M[i][j] = min(oe(i, j), clip) - 1 where both bins are valid and ignore_diags <= |i - j| < dmax, 0 elsewhere; oe is 0 without a cell.
- dmax is the first diagonal d >= ignore_diags with valid pairs whose expected value is not a finite positive number, or nb.
- clip is the `-clip` percentile (np.percentile) of the non-NaN O/E of the cells; `-clip 100` (or no such cell) means no clip.
- The device's vectors have unit norm over the valid bins and their largest entry positive.  A vector is flipped when its Pearson
  correlation over the valid bins with a per-bin track is negative: the raw marginal of the bin (coverage), or with `-phase` the
  overlap-length-weighted mean of a bedGraph's intervals per bin (bins without overlap take no part).  A NaN or zero correlation
  leaves the device's sign.  The values written are v sqrt(|lambda|).
- `<o>_eigs.txt`: `chrom start end valid E1..En` per bin; `<o>_E1.bedGraph`: the valid bins; `<o>_compartments.bed`: the maximal runs
  of valid bins with E1 of one sign, named A (positive) or B, scored by the run's mean E1 (a zero or an invalid bin ends a run);
  `<o>_eigs.json`: per chromosome b0, nb, n_valid, n_in, dmax, clip, eigvals, resid, eig_iters, eig_converged, flipped, phase_corr
  (the correlations) and the balance statistics iters, converged, var, scale, and the arguments.  Floats as %.10g, NaN as nan.
"""
import argparse
import logging
import sys

import numpy as np

from . import matrix
from .balance import _num, balance_stats, balanced_state, check_args, fmt, not_converged
from .expected import add_options, check_exp_args, expected_state, options_of, parsed_options
from .matrix import CHUNK, check_res, chrom_outputs, chroms_of, common, each_chrom
from .peaks import write_outputs

logger = logging.getLogger("cloops_amd.compartments")

SUFFIXES = ("_eigs.txt", "_E1.bedGraph", "_compartments.bed", "_eigs.json")
N_EIGS_MAX = 6                                                              # CL_EIG_MAX


def check_eig_args(n_eigs, clip, eig_tol, eig_iters):
    """-> (n_eigs, clip percentile, tol, max_iters) checked; ValueError otherwise"""
    if isinstance(n_eigs, bool) or not isinstance(n_eigs, (int, np.integer)) or not 1 <= n_eigs <= N_EIGS_MAX:
        raise ValueError("neigs must be an integer in [1, %d], got %r" % (N_EIGS_MAX, n_eigs))
    clip = float(clip)
    if not 0.0 < clip <= 100.0:
        raise ValueError("clip must be a percentile in (0, 100], got %r" % (clip,))
    eig_tol = float(eig_tol)
    if not eig_tol >= 0.0:
        raise ValueError("eigtol must be at or above 0, got %r" % (eig_tol,))
    if isinstance(eig_iters, bool) or not isinstance(eig_iters, (int, np.integer)) or eig_iters < 0:
        raise ValueError("eigiters must be an integer at or above 0, got %r" % (eig_iters,))
    return int(n_eigs), clip, eig_tol, int(eig_iters)


def pick_dmax(n_pairs, expected, ignore_diags):
    """the first diagonal d >= ignore_diags with valid pairs whose expected value is not a finite positive number, or nb"""
    n_pairs, e = np.asarray(n_pairs, np.int64), np.asarray(expected, np.float64)
    nb = len(n_pairs)
    ok = np.isfinite(e) & (e > 0)
    bad = np.flatnonzero((n_pairs > 0) & ~ok & (np.arange(nb) >= int(ignore_diags)))
    return int(bad[0]) if len(bad) else nb


def clip_of(oe, percentile):
    """the clip of the O/E values: their `percentile` over the non-NaN ones; +inf at 100 or without a value"""
    oe = np.asarray(oe, np.float64)
    oe = oe[~np.isnan(oe)]
    if percentile >= 100.0 or len(oe) == 0:
        return float("inf")
    c = float(np.percentile(oe, percentile))
    return c if c > 0 else float("inf")


def read_bedgraph(path):
    """a bedGraph `chrom start end value` -> {chrom: (starts int64, ends int64, values float64)}; track and browser lines are skipped"""
    per = {}
    try:
        fh = open(path)
    except OSError as e:
        raise ValueError("the phase track %s cannot be read: %s" % (path, e))
    with fh:
        for ln, line in enumerate(fh, 1):
            f = line.split()
            if not f or f[0] in ("track", "browser") or f[0].startswith("#"):
                continue
            try:
                s, e, v = int(f[1]), int(f[2]), float(f[3])
            except (IndexError, ValueError):
                raise ValueError("%s line %d: not `chrom start end value`" % (path, ln))
            if e < s:
                raise ValueError("%s line %d: end before start" % (path, ln))
            per.setdefault(f[0], []).append((s, e, v))
    return {c: (np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int64), np.array([r[2] for r in rows], np.float64))
            for c, rows in per.items()}


def bin_track(starts, ends, values, b0, nb, res):
    """the overlap-length-weighted mean of the intervals [start, end) per bin b0 .. b0 + nb - 1 of `res` bp -> float64 [nb], NaN where
    no interval overlaps the bin"""
    num, den = np.zeros(nb), np.zeros(nb)
    for s, e, v in zip(np.asarray(starts, np.int64).tolist(), np.asarray(ends, np.int64).tolist(), np.asarray(values, np.float64).tolist()):
        if e <= s or np.isnan(v):
            continue
        for b in range(max(s // res, b0), min((e - 1) // res, b0 + nb - 1) + 1):
            ov = min(e, (b + 1) * res) - max(s, b * res)
            if ov > 0:
                num[b - b0] += ov * v
                den[b - b0] += ov
    out = np.full(nb, np.nan)
    out[den > 0] = num[den > 0] / den[den > 0]
    return out


def pearson(a, b):
    """the Pearson correlation of two arrays over the entries where both are numbers; NaN with fewer than two or without spread"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = ~np.isnan(a) & ~np.isnan(b)
    if ok.sum() < 2:
        return float("nan")
    a, b = a[ok] - a[ok].mean(), b[ok] - b[ok].mean()
    den = np.sqrt((a * a).sum() * (b * b).sum())
    return float((a * b).sum() / den) if den > 0 else float("nan")


def orient(v, track):
    """-> (the vector, flipped when its correlation with the track is negative; flipped; the correlation)"""
    r = pearson(v, track)
    flip = bool(r < 0)                                                      # (NaN and 0 leave the sign)
    return (-np.asarray(v, np.float64) if flip else np.asarray(v, np.float64)), flip, r


def format_eigs(chrom, res, b0, valid, E):
    """`<o>_eigs.txt` of one chromosome: `chrom start end valid E1..En` per bin; E: [n, nb]"""
    E = np.asarray(E, np.float64).reshape(-1, len(valid))
    return "".join("%s\t%d\t%d\t%d\t%s\n" % (chrom, (b0 + i) * res, (b0 + i + 1) * res, 1 if valid[i] else 0, "\t".join(fmt(x) for x in E[:, i].tolist()))
                   for i in range(len(valid)))


def format_bedgraph(chrom, res, b0, valid, e1):
    """`<o>_E1.bedGraph` of one chromosome: the valid bins"""
    return "".join("%s\t%d\t%d\t%s\n" % (chrom, (b0 + i) * res, (b0 + i + 1) * res, fmt(float(e1[i]))) for i in range(len(valid)) if valid[i])


def compartment_runs(valid, e1):
    """the maximal runs of valid bins with e1 of one sign -> [(first bin, end bin, "A" or "B", mean e1)]; a zero, a NaN or an invalid bin
    ends a run"""
    runs, start, sign = [], None, 0
    e1 = np.asarray(e1, np.float64)
    for i in range(len(valid) + 1):
        s = 0
        if i < len(valid) and valid[i] and not np.isnan(e1[i]):
            s = 1 if e1[i] > 0 else (-1 if e1[i] < 0 else 0)
        if s != sign:
            if sign != 0:
                runs.append((start, i, "A" if sign > 0 else "B", float(np.mean(e1[start:i]))))
            start, sign = i, s
    return runs


def format_runs(chrom, res, b0, valid, e1):
    """`<o>_compartments.bed` of one chromosome: `chrom start end A|B mean` per run"""
    return "".join("%s\t%d\t%d\t%s\t%s\n" % (chrom, (b0 + s) * res, (b0 + e) * res, name, fmt(m)) for s, e, name, m in compartment_runs(valid, e1))


def compartments_chrom(ch, chrom, res, cut=0, n_eigs=3, clip=99.9, eig_tol=1e-8, eig_iters=1000, phase=None, chunk=CHUNK, **options):
    """One chromosome on the device: `ch` has the mat_*, bal_*, exp_* and eig_* methods of api.Chromosome; phase = (starts, ends,
    values) of the chromosome's track or None; `options`: the records bal= and exp= (expected.options_of), or their fields as keywords
    -> dict(eigs: text, bedgraph: text, runs: text, stats: the json's entry, vectors: the oriented scaled vectors [n_eigs, nb])"""
    bal, exp = options_of(**options)
    try:
        st = balanced_state(ch, res, cut, bal, exp.raw)
        nb, n_cells = st.nb, int(st.n_cells)
        valid = np.asarray(st.mask, bool) if exp.raw else ~np.isnan(ch.bal_weights(0, nb))
        ex = expected_state(ch, st, bal, exp)
        oe = [ch.exp_cells_get(first, min(int(chunk), n_cells - first)) for first in range(0, n_cells, int(chunk))]
        clip_value = clip_of(np.concatenate(oe) if oe else np.zeros(0), clip)
        dmax = pick_dmax(ex.n_pairs, ex.expected, bal.ignore_diags)
        no_band = 0 < nb < bal.ignore_diags                                 # fewer bins than ignored diagonals: no band, no matrix
        if no_band:
            n_valid, n_in, eig_it, eig_cv = int(np.count_nonzero(valid)), 0, 0, False
            lam, resid, vecs = np.full(n_eigs, np.nan), np.full(n_eigs, np.nan), np.full((n_eigs, nb), np.nan)
        else:
            n_valid, n_in = ch.eig_build(clip_value, dmax)
            eig_it, eig_cv, lam, resid = ch.eig_iterate(n_eigs, max_iters=eig_iters, tol=eig_tol)
            vecs = np.stack([ch.eig_vectors(k, 0, nb) for k in range(n_eigs)]) if nb > 0 else np.zeros((n_eigs, 0))
    finally:
        ch.mat_free()
    msg = not_converged(chrom, st, bal.tol, exp.raw)
    if msg is not None:
        logger.warning("WARNING: " + msg)
    if no_band:
        logger.warning("WARNING: %s has %d bins, fewer than the %d ignored diagonals: no eigenvectors" % (chrom, nb, bal.ignore_diags))
    elif nb > 0 and not eig_cv:
        logger.warning("WARNING: the eigenvectors of %s did not converge in %d iterations (tol %s)" % (chrom, eig_it, fmt(eig_tol)))
    track = np.asarray(st.sum, np.float64) if phase is None else bin_track(phase[0], phase[1], phase[2], st.b0, nb, res)
    track = np.where(valid, track, np.nan) if nb > 0 else track
    E, flipped, corr = np.full((n_eigs, nb), np.nan), [], []
    for k in range(n_eigs):
        v, flip, r = orient(vecs[k], track)
        E[k] = v * np.sqrt(np.abs(lam[k]))
        flipped.append(flip)
        corr.append(_num(r))
    stats = dict(balance_stats(st), b0=int(st.b0), nb=int(nb), n_valid=int(n_valid), n_in=int(n_in), dmax=int(dmax), clip=_num(clip_value),
                 eigvals=[_num(x) for x in np.asarray(lam).tolist()], resid=[_num(x) for x in np.asarray(resid).tolist()],
                 eig_iters=int(eig_it), eig_converged=bool(eig_cv), flipped=flipped, phase_corr=corr)
    return {"eigs": format_eigs(chrom, res, st.b0, valid, E), "bedgraph": format_bedgraph(chrom, res, st.b0, valid, E[0]),
            "runs": format_runs(chrom, res, st.b0, valid, E[0]), "stats": stats, "vectors": E}


def compartments_outputs(per_chrom, args):
    """{suffix: text} of the files from {chrom: compartments_chrom's dict}, and the json's content"""
    return chrom_outputs(per_chrom, ((SUFFIXES[0], "eigs"), (SUFFIXES[1], "bedgraph"), (SUFFIXES[2], "runs")), SUFFIXES[3], {"args": args})


def jd2compartments(jd, fout, res=100000, cut=0, chroms=(), n_eigs=3, clip=99.9, eig_tol=1e-8, eig_iters=1000, phase=None, raw=False,
                    per_decade=10, nosmooth=False, ignore_diags=2, min_nnz=10, min_count=0, mad_max=5, tol=1e-5, max_iters=200):
    """The compartment vectors of every cis chromosome of `jd` -> `<fout>_eigs.txt`, `<fout>_E1.bedGraph`, `<fout>_compartments.bed`
    and `<fout>_eigs.json`; `phase`: the path of a bedGraph to orient the vectors by; returns the json's content."""
    res, cut = check_res(res), int(cut)
    bal, exp = check_args(ignore_diags, min_nnz, min_count, mad_max, tol, max_iters), check_exp_args(raw, per_decade, nosmooth)
    n_eigs, clip, eig_tol, eig_iters = check_eig_args(n_eigs, clip, eig_tol, eig_iters)
    tracks = None if phase is None else read_bedgraph(phase)
    no_track = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))
    per_chrom = each_chrom(matrix._records(jd, chroms), logger, "compartments of %s",
                           lambda ch, chrom: compartments_chrom(ch, chrom, res, cut, n_eigs, clip, eig_tol, eig_iters,
                                                                None if tracks is None else tracks.get(chrom, no_track), bal=bal, exp=exp))
    args = dict(bal._asdict(), res=res, cut=cut, n_eigs=n_eigs, clip=clip, eig_tol=eig_tol, eig_iters=eig_iters, phase=phase, **exp._asdict())
    texts, js = compartments_outputs(per_chrom, args)
    write_outputs(fout, texts)
    return js


def help(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cloops_amd.compartments",
                                 description="A/B compartments: the leading eigenvectors of the O/E contact matrix on MI355X. "
                                             "For example: python -m cloops_amd.compartments -d hic -o hic -res 100000")
    common(ap, 100000, chroms=True)
    ap.add_argument("-neigs", dest="neigs", required=False, default=3, type=int, help="Eigenvectors per chromosome, 1 to 6, default 3.")
    ap.add_argument("-clip", dest="clip", required=False, default=99.9, type=float,
                    help="Percentile of the O/E values the matrix is clipped at, default 99.9; 100 switches the clip off.")
    ap.add_argument("-eigtol", dest="eigtol", required=False, default=1e-8, type=float,
                    help="Residual of an eigenpair, relative to the largest eigenvalue, to stop at, default 1e-8.")
    ap.add_argument("-eigiters", dest="eigiters", required=False, default=1000, type=int, help="Most iterations of the eigensolver, default 1000.")
    ap.add_argument("-phase", dest="phase", required=False, default=None, type=str,
                    help="A bedGraph (GC content, gene density ..) whose per-bin mean orients the vectors; default: the bins' coverage.")
    add_options(ap)
    return ap.parse_args(argv)


def main(argv=None):
    op = help(argv)
    jd2compartments(op.d, op.output, res=op.res, cut=op.cut, chroms=chroms_of(op), n_eigs=op.neigs, clip=op.clip, eig_tol=op.eigtol,
                    eig_iters=op.eigiters, phase=op.phase, **parsed_options(op))
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())
