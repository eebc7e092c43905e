"""1D coverage tracks of the PET ends: the bedGraph that is loaded next to a loop track.

The reference has nothing of the kind; users dump `.jd` files and run `bedtools genomecov` on reshaped text.  Here the coverage of a
chromosome is made by kernel K20 on the chromosome resident in HBM (`cl_cov_build` / `cl_cov_text` / `cl_cov_chunks` /
`cl_cov_render`): the end points sorted once, the depth as a rank difference over the sorted array, the runs compacted and their
text rendered in chunks that never split a line, copied to two page-locked buffers in turn while the previous chunk is written.

Definitions (include/cloops_hip.h, cl_cov_build):
- Rows with Y - X >= cut take part (all rows for cut <= 0).  `ends`: "left" takes every row's X, "right" its Y, "both" both.
- An end point p stands for [max(0, p - ext), p + ext) -- the start / end of a washU record (cLoops/io.py:306-307) -- or, with
  res >= 1, for its bin [floor(p / res) res, floor(p / res) res + res) (ext is then ignored).
- The track is the maximal runs of constant depth > 0 in ascending order, one line `chrom\\tstart\\tend\\tvalue\\n` each.
- norm "none": value = the depth.  norm "cpm": counts per million end points with exactly three decimals, in integers:
  (depth * 10^9 + N // 2) // N thousandths, N = the end points of every chromosome written (fixed_point below prints the same).
- Chromosomes are written in plain string order of their names; a `.jd` whose key names two chromosomes is left out.
"""
import argparse
import glob
import json
import logging
import os
import sys

logger = logging.getLogger("cloops_amd.coverage")

ENDS = {"left": 1, "right": 2, "both": 3}                      # the `ends` bit set of cl_cov_build
NORMS = ("none", "cpm")
CPM_NUM = 10 ** 9                                              # thousandths of a count per million: depth * 10^6 * 1000 / N
STAT_KEYS = ("n_runs", "max_depth", "n_ends", "area")          # per chromosome, in cl_cov_build's order


def ends_code(ends):
    """"left" / "right" / "both" (or the bit set itself) -> 1 / 2 / 3"""
    if ends in ENDS:
        return ENDS[ends]
    if ends in (1, 2, 3) and not isinstance(ends, bool):
        return int(ends)
    raise ValueError("ends must be one of %s, got %r" % (", ".join(sorted(ENDS)), ends))


def scale_of(norm, n_ends_total):
    """the (numerator, denominator) of cl_cov_text for `norm`, None for raw counts; "cpm" of a track without end points has no
    line to scale: None too"""
    if norm not in NORMS:
        raise ValueError("norm must be one of %s, got %r" % (", ".join(NORMS), norm))
    if norm == "none" or int(n_ends_total) <= 0:
        return None
    return (CPM_NUM, int(n_ends_total))


def fixed_point(depth, num, den):
    """the value cl_cov_text prints for `depth` under the scale (num, den): (depth * num + den // 2) // den thousandths, with
    exactly three decimals"""
    q = (int(depth) * int(num) + int(den) // 2) // int(den)
    return "%d.%03d" % (q // 1000, q % 1000)


def format_runs(name, start, end, depth, scale=None):
    """the bedGraph text of runs as the device renders it (bytes): the host twin of cl_cov_text + cl_cov_render"""
    if scale is None:
        vals = [str(int(d)) for d in depth]
    else:
        vals = [fixed_point(d, scale[0], scale[1]) for d in depth]
    return "".join("%s\t%d\t%d\t%s\n" % (name, int(s), int(e), v) for s, e, v in zip(start, end, vals)).encode()


def chrom_files(jd, chroms=()):
    """`jd`: a directory of `.jd` files, or a list of .jd paths / 'mem://' names of pipe.CACHE -> [(chrom, name)] of the cis ones
    (key chrA == chrB, as cloops_amd.agg takes them), only those of `chroms` if given, in plain string order of the chromosome names"""
    if isinstance(jd, str):
        if not os.path.isdir(jd):
            raise ValueError("%s is not a directory of .jd files" % jd)
        jd = sorted(glob.glob(os.path.join(jd, "*.jd")))
    out = {}
    for f in jd:
        if f.startswith("mem://"):
            from .pipe import CACHE
            key = CACHE.get(f).key
        else:
            key = tuple(os.path.splitext(os.path.split(f)[-1])[0].split("-"))
        if len(key) == 2 and key[0] == key[1] and (len(chroms) == 0 or key[0] in chroms):
            out[key[0]] = f
    return sorted(out.items())


def summary_of(stats, ext, res, cut, ends, norm):
    """the content of `<fout>_bedGraph.json`: the parameters, the per-chromosome statistics and their totals"""
    total = {k: (max([s[k] for s in stats.values()] or [0]) if k == "max_depth" else sum(s[k] for s in stats.values())) for k in STAT_KEYS}
    return {"ext": int(ext), "res": int(res), "cut": int(cut), "ends": ends_code(ends), "norm": norm, "chroms": stats, "total": total}


def jd2bedgraph(jd, fout, ext=75, res=0, cut=0, ends="both", norm="none", chroms=(), budget=None):
    """The coverage of the PET ends of `jd` (a directory of `.jd` files, or a list of .jd paths / 'mem://' names of pipe.CACHE, so the
    chromosomes of a finished sweep serve without files) -> `<fout>.bedGraph` and `<fout>_bedGraph.json`; returns {chrom: dict(n_runs,
    max_depth, n_ends, area)}.  With norm "cpm" every chromosome is built first (its runs stay on the device) to get the genome-wide
    number of end points, then rendered."""
    code = ends_code(ends)
    if norm not in NORMS:
        raise ValueError("norm must be one of %s, got %r" % (", ".join(NORMS), norm))
    ext, res, cut = int(ext), int(res), int(cut)
    if res < 0 or (res == 0 and ext < 1):
        raise ValueError("needs res >= 1 (bins) or res = 0 and ext >= 1 (windows), got res=%s ext=%s" % (res, ext))
    from .pipe import CACHE
    files = chrom_files(jd, chroms)
    stats = {}

    def build(r, chrom):
        stats[chrom] = dict(zip(STAT_KEYS, r.chrom.coverage_build(cut, code, ext, res)))

    def render(r, fo, scale):
        ch = r.chrom
        ch.coverage_text(r.key[0], scale)
        for mv in ch.coverage_iter(budget or ch.TRACK_BUDGET):
            fo.write(mv)
        ch.coverage_free()

    try:
        with open(fout + ".bedGraph", "wb") as fo:
            if norm == "cpm":
                with CACHE.pinned([f for _, f in files]) as rs:
                    for (chrom, _), r in zip(files, rs):
                        with r.lock:
                            build(r, chrom)
                    scale = scale_of(norm, sum(s["n_ends"] for s in stats.values()))
                    for (chrom, f), r in zip(files, rs):
                        logger.info("converting %s" % f)
                        with r.lock:
                            render(r, fo, scale)
            else:
                for chrom, f in files:
                    logger.info("converting %s" % f)
                    r = CACHE.get(f)
                    with r.lock:
                        build(r, chrom)
                        render(r, fo, None)
    except BaseException:
        os.remove(fout + ".bedGraph")                                  # no half-written track stays behind
        raise
    with open(fout + "_bedGraph.json", "w") as fh:
        json.dump(summary_of(stats, ext, res, cut, ends, norm), fh, indent=1, sort_keys=True)
        fh.write("\n")
    return stats


def help(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cloops_amd.coverage",
                                 description="Coverage of the PET ends as a bedGraph on MI355X. "
                                             "For example: python -m cloops_amd.coverage -d trac -o trac")
    ap.add_argument("-d", dest="d", required=True, type=str, help="The directory of cis .jd files.")
    ap.add_argument("-o", dest="output", required=True, type=str, help="Output prefix.")
    ap.add_argument("-ext", dest="ext", required=False, default=75, type=int,
                    help="Extension from a PET end to both sides, default is 75 (ignored with -res).")
    ap.add_argument("-res", dest="res", required=False, default=0, type=int, help="Bin size in bp; default 0: windows of -ext.")
    ap.add_argument("-cut", dest="cut", required=False, default=0, type=int, help="Distance cutoff to filter PETs, default 0.")
    ap.add_argument("-ends", dest="ends", required=False, default="both", choices=sorted(ENDS), help="Which PET ends count, default both.")
    ap.add_argument("-norm", dest="norm", required=False, default="none", choices=list(NORMS),
                    help="none: raw depth; cpm: counts per million end points, three decimals. Default none.")
    ap.add_argument("-c", dest="chroms", required=False, default="", type=str,
                    help="Whether to process limited chroms, specify it as chr1,chr2,chr3, default is all.")
    return ap.parse_args(argv)


def main(argv=None):
    op = help(argv)
    chroms = [] if op.chroms == "" else set(op.chroms.split(","))
    jd2bedgraph(op.d, op.output, ext=op.ext, res=op.res, cut=op.cut, ends=op.ends, norm=op.norm, chroms=chroms)
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())
