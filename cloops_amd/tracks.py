"""Browser tracks of PETs and loops: cLoops/io.py:218-348 (loops2washU, loops2juice, jd2washU, jd2hic), function for function,
and the scripts jd2washU / jd2juice as `python -m cloops_amd.tracks washu|juice`.

The reference loops over every PET in Python, writes two lines per PET for washU and one for juicer into a temporary file, and
hands the washU text to `bedtools sort`.  Here the text of a chromosome is made by kernel K14 on the chromosome resident in HBM
(`cl_track_build` / `cl_track_chunks` / `cl_track_render`): filtered by parseJd's cut, in the final order, in chunks that never
split a line, copied to two page-locked buffers in turn while the previous chunk is written to the file.

Semantics pinned:
- washU lines are `chrA\tstart\tend\tchrB:pstart-pend,1\tid\t.\n`, two per PET (its X end first, then its Y end), start =
  max(0, p - ext) and end = p + ext in int64; the file is sorted by chromosome name (bytes), start, end, then generation order
  (row, then end) -- `bedtools sort` leaves that last tie open.  juice lines are `0\tchrA\tX\t0\t1\tchrB\tY\t1\n`, files in
  sorted name order, rows in row order.
- `.jd` files come from `pipe.CACHE` (so `mem://` names work; a resident without ids numbers its rows).  A key with chrA != chrB
  raises ValueError naming the file (neither project writes trans `.jd` files).
- bgzip / tabix and juicer_tools run when they are on PATH, as the reference runs them.  Deviation: without bgzip and tabix the
  sorted plain text stays in `fout` with one warning; the reference's `bedtools sort` step, when bedtools is missing, leaves an
  empty `fout` and removes its unsorted temp file.  Without juicer_tools the text stays and the command to run is logged.
- loops2washU / loops2juice find their columns by header name (iva, ivb, rab, loopId, FDR, ES, distance and the three
  p-values; the reference reads positions that match its Python-2 column order), falling back to the reference's positions when
  a name is missing; "significant" is the last column, as in the reference.
"""
import argparse
import glob
import logging
import os
import shutil
import subprocess
import sys

import numpy as np

from .cModel import parseIv

logger = logging.getLogger("cloops_amd.tracks")

# the columns the reference reads (cLoops/io.py:231-285, its Python-2 `.loop` column order) and their header names
LOOP_COLUMNS = {"loopId": 0, "ES": 1, "FDR": 2, "binomial_p-value": 3, "distance": 4, "hypergeometric_p-value": 5, "iva": 6,
                "ivb": 7, "poisson_p-value": 8, "rab": 10}


def _loop_columns(fin):
    """{name: column} of the `.loop` file `fin`: by header name when every name is there, else the reference's positions"""
    with open(fin) as fh:
        head = fh.readline().split("\n")[0].split("\t")
    if all(k in head for k in LOOP_COLUMNS):
        return {k: head.index(k) for k in LOOP_COLUMNS}
    return dict(LOOP_COLUMNS)


def _log(lg):
    return lg if lg is not None and hasattr(lg, "info") else logger


def loops2washU(fin, fout, logger=None, significant=1):
    """cLoops/io.py:220-241: the loops of `fin` (only the significant ones unless `significant` is 0) -> washU long-range lines
    `iva\tivb\t1`"""
    lg = _log(logger)
    lg.info("Converting %s to washU long range interaction track." % fin)
    col = _loop_columns(fin)
    with open(fout, "w") as f:
        for i, line in enumerate(open(fin)):
            if i == 0:
                continue
            line = line.split("\n")[0].split("\t")
            if significant and float(line[-1]) < 1:
                continue
            nline = [line[col["iva"]], line[col["ivb"]], "1"]
            f.write("\t".join(map(str, nline)) + "\n")
    lg.info("Converting %s to washU long range interaction track finished." % fin)


def loops2juice(fin, fout, logger=None, significant=1):
    """cLoops/io.py:253-289: the loops of `fin` -> Juicebox 2D annotation features, p-values as -log10(p) (Python-3 str of the
    float64: p = 0 gives inf); rows whose numbers do not parse are skipped, as in the reference"""
    lg = _log(logger)
    lg.info("Converting %s to Juicebox 2D annotation feature." % fin)
    col = _loop_columns(fin)
    with open(fout, "w") as f:
        line = ["chromosome1", "x1", "x2", "chromosome2", "y1", "y2", "color", "observed", "loopId", "FDR", "EnrichmentScore",
                "distance", "-log10(binomal_p-value)", "-log10(poisson_p-value)", "-log10(hypergeometric_p-value)"]
        f.write("\t".join(line) + "\n")
        for i, line in enumerate(open(fin)):
            if i == 0:
                continue
            line = line.split("\n")[0].split("\t")
            if significant and float(line[-1]) < 1:
                continue
            iva = parseIv(line[col["iva"]])
            ivb = parseIv(line[col["ivb"]])
            try:
                with np.errstate(divide="ignore"):
                    nline = [iva[0], iva[1], iva[2], ivb[0], ivb[1], ivb[2], '"0,255,255"', line[col["rab"]], line[col["loopId"]],
                             line[col["FDR"]], line[col["ES"]], line[col["distance"]],
                             -np.log10(float(line[col["binomial_p-value"]])), -np.log10(float(line[col["poisson_p-value"]])),
                             -np.log10(float(line[col["hypergeometric_p-value"]]))]
            except Exception:
                continue
            f.write("\t".join(map(str, nline)) + "\n")
    lg.info("Converting %s to Juicebox 2D annotation feature finished." % fin)


def _key(f):
    """parseJd's key of `f` (cLoops/io.py:210-211); a trans key raises"""
    key = tuple(os.path.split(f)[1].replace(".jd", "").split("-"))
    if len(key) < 2 or key[0] != key[1]:
        raise ValueError("%s: not a cis .jd file (key %s); trans .jd files are not supported" % (f, "-".join(key)))
    return key


def _chunks(f, kind, cut, ext, budget=None):
    """K14 on the resident chromosome of `f` (a .jd path or a 'mem://' name of pipe.CACHE): the chunks of its text, in order,
    as memoryviews valid until the next one is requested"""
    from .pipe import CACHE
    r = CACHE.get(f)
    key = _key(f)
    with r.lock:
        ch = r.chrom
        ch.track_build(kind, cut, ext, r._ids, key[0], key[1])
        try:
            for mv in ch.track_iter(budget or ch.TRACK_BUDGET):
                yield mv
        finally:
            ch.track_free()


def _write(fs, fout, kind, cut, ext):
    with open(fout, "wb") as fo:
        for f in fs:
            logger.info("converting %s" % f)
            for mv in _chunks(f, kind, cut, ext):
                fo.write(mv)


def jd2washU(fs, fout, cut, ext):
    """cLoops/io.py:292-323: the PETs of the `.jd` files `fs` -> washU long-range track `fout`, sorted (chromosome, start, end),
    then `bgzip fout` and `tabix -p bed fout.gz` when both are on PATH"""
    logger.info("Converting %s to washU track." % (",".join(fs)))
    if cut < 0:
        raise ValueError("cut < 0")
    fs = sorted(fs, key=lambda f: (_key(f)[0].encode(), f))          # bedtools sort: chromosome names in byte order
    _write(fs, fout, "washu", cut, ext)
    if shutil.which("bgzip") and shutil.which("tabix"):
        subprocess.run(["bgzip", fout], check=True)
        subprocess.run(["tabix", "-p", "bed", fout + ".gz"], check=True)
        logger.info("Converting %s to washU random accessed track finished." % fout)
    else:
        logger.warning("bgzip and tabix are not both on PATH: %s stays sorted plain text; to index it run `bgzip %s` and "
                       "`tabix -p bed %s.gz`" % (fout, fout, fout))


def jd2hic(fs, fout, cut, org, resolution):
    """cLoops/io.py:326-348: the PETs of the `.jd` files `fs` -> `juicer_tools pre` short-format text `<fout minus .hic>.txt`, then
    `juicer_tools pre -n -r <resolution> -d <txt> <fout> <org>` when juicer_tools is on PATH (the text is removed after it)"""
    logger.info("Converting %s to .hic file which could be loaded in juicebox" % (",".join(fs)))
    if cut < 0:
        raise ValueError("cut < 0")
    txt = (fout[:-4] if fout.endswith(".hic") else fout) + ".txt"
    fs = sorted(fs)
    for f in fs:
        _key(f)
    _write(fs, txt, "juice", cut, 0)
    cmd = ["juicer_tools", "pre", "-n", "-r", str(resolution), "-d", txt, fout, org]
    if shutil.which("juicer_tools"):
        subprocess.run(cmd, check=True)
        os.remove(txt)
        logger.info("Converting %s to juicer's hic file finished." % fout)
    else:
        logger.warning("juicer_tools is not on PATH: %s keeps the text; to make %s run `%s`" % (txt, fout, " ".join(cmd)))
    return txt


def help(argv=None):
    """the flags of jd2washUHelp / jd2juiceHelp (cLoops/utils.py:279-363) under the subcommands washu / juice"""
    ap = argparse.ArgumentParser(prog="python -m cloops_amd.tracks",
                                 description="Convert PETs level data to browser tracks (scripts jd2washU / jd2juice) on MI355X.")
    sub = ap.add_subparsers(dest="cmd", required=True)
    w = sub.add_parser("washu", help="washU long-range track <o>_PETs_washU.txt (bgzip + tabix when on PATH)")
    w.add_argument("-d", dest="dir", required=True, type=str, help="Directory for .jd files, generated by cLoops with option -s 1.")
    w.add_argument("-o", dest="output", required=True, type=str, help="Output prefix.")
    w.add_argument("-ext", dest="ext", type=int, default=75, help="Extension from the middle center of the PET to both ends,default is 75.")
    w.add_argument("-cut", dest="cut", type=int, default=0, help="Distance cutoff for PETs to filter, default is 0.")
    j = sub.add_parser("juice", help="juicer_tools pre text <o>_juice.txt (and <o>_juice.hic when juicer_tools is on PATH)")
    j.add_argument("-d", dest="dir", required=True, type=str, help="Directory for .jd files, generated by cLoops with option -s 1.")
    j.add_argument("-o", dest="output", required=True, type=str, help="Output prefix.")
    j.add_argument("-org", dest="org", required=True, type=str, default="hg38", help="Organism required to generate .hic file,default is hg38.")
    j.add_argument("-res", dest="resolution", type=str, default="1000,5000,10000,20000",
                   help="Resolutions used to generate .hic file,default is 1000,5000,10000,20000")
    j.add_argument("-cut", dest="cut", type=int, default=0, help="Distance cutoff for PETs to filter, default is 0.")
    return ap.parse_args(argv)


def main(argv=None):
    """scripts/jd2washU and scripts/jd2juice"""
    op = help(argv)
    fs = glob.glob(os.path.join(op.dir, "*.jd"))
    if op.cmd == "washu":
        jd2washU(fs, op.output + "_PETs_washU.txt", op.cut, op.ext)
    else:
        jd2hic(fs, op.output + "_juice.hic", op.cut, op.org, op.resolution)
    return 0


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    sys.exit(main())
