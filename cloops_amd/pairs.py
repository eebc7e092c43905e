"""4DN pairs files (`.pairs`, `.pairs.gz`: pairtools, Juicer's and HiC-Pro's exporters, cooler, the 4DN portal) on the GPU: to
BEDPE (`pairs2bedpe`, `python -m cloops_amd.convert pairs`) and straight into the sweep (`parse_pairs_gpu`, `load_pairs`,
`python -m cloops_amd -f x.pairs.gz`), with no BEDPE text in between.  The reference has no script for this format; the rule is
scripts/hicpropairs2bedpe's on other columns, and the reader is defined through it.

Semantics pinned, 4DN pairs v1.0, columns `readID chr1 pos1 chr2 pos2 strand1 strand2`, further ones ignored:
- a line whose first byte is '#' is a header line, wherever it stands: no output, no PET; it counts in the line numbers of error
  messages and not in the lines of a read.  A `#columns:` line in the leading '#' run must start with the seven names above, else
  ValueError("<file>:<line>: columns ...") before anything is read or written;
- a data line is HiC-Pro's rule (cloops_amd.convert, K15, with its Python-2 reading of bytes and its int64 bounds) on the fields
  f0 f1 f2 f5 f3 f4 f6: A = [f1, p1, p1 + ext] when f5 is exactly "+", else [f1, p1 - ext, p1]; B the same from f3, f4, f6; line
  `A0 A1 A2 B0 B1 B2 f0 . f5 f6`; the first line with fewer than 7 fields, a bad position or a value outside int64 stops
  everything with ValueError("<file>:<line>: <reason>"), the output holding exactly the lines in front of it;
- the reader returns what cloops_amd.io.parse_bedpe returns on that text, for every cs / cut / unique / strand_distances.  What
  the device does not decide (a byte >= 0x80, a '\\r' that is not the last byte before the '\\n', a coordinate of 2^62 or more in
  magnitude, and cloops_amd.ingest's four pipeline cases) sends the whole call to `parse_pairs` on the host; the logger / stderr
  says so once and `stats["fallback"]` holds (reason, file, line).
"""
import functools
import gzip
import os
import re
import tempfile

import numpy as np

from . import convert, ingest
from . import io as cio

COLUMNS = (b"readID", b"chr1", b"pos1", b"chr2", b"pos2", b"strand1", b"strand2")
MAGIC = b"## pairs format"
WS = b" \t\n\r\x0b\x0c"                      # Python 2's whitespace of a byte string (K15's reading)
I64 = (-(1 << 63), (1 << 63) - 1)
_INT = re.compile(rb"[+-]?[0-9]+")
BUDGET = convert.BUDGET
THREADS = convert.THREADS


def _open(f):
    return gzip.open(f, "rb") if f.endswith(".gz") else open(f, "rb")


def sniff(f):
    """"pairs" when the first line of `f` (plain or .gz) starts with `## pairs format`, else "bedpe" (also for a file that cannot
    be read: the reader of that format reports it)"""
    try:
        with _open(f) as fh:
            return "pairs" if fh.read(len(MAGIC)) == MAGIC else "bedpe"
    except (OSError, EOFError):
        return "bedpe"


def check_header(f):
    """the leading '#' run of `f`: a `#columns:` line must name the seven columns first"""
    with _open(f) as fh:
        for k, line in enumerate(fh, 1):
            if not line.startswith(b"#"):
                return
            if line.startswith(b"#columns:") and tuple(line[len(b"#columns:"):].split()[:7]) != COLUMNS:
                raise ValueError("%s:%d: columns are not %s" % (f, k, b" ".join(COLUMNS).decode()))


class _Bad(Exception):
    pass


def _int(b):
    s = b.strip(WS)
    if not _INT.fullmatch(s):
        raise _Bad("not an integer")
    return _i64(int(s))


def _i64(v):
    if not I64[0] <= v <= I64[1]:
        raise _Bad("integer outside int64")
    return v


def bedpe_line(line, ext):
    """one data line (bytes, without its '\\n') -> its BEDPE line"""
    f = line.strip(WS).split(b"\t")
    if len(f) < 7:
        raise _Bad("fewer than 7 fields")
    p1, p2 = _int(f[2]), _int(f[4])
    a = (p1, _i64(p1 + ext)) if f[5] == b"+" else (_i64(p1 - ext), p1)
    b = (p2, _i64(p2 + ext)) if f[6] == b"+" else (_i64(p2 - ext), p2)
    return b"\t".join([f[1], b"%d" % a[0], b"%d" % a[1], f[3], b"%d" % b[0], b"%d" % b[1], f[0], b".", f[5], f[6]]) + b"\n"


def _to_bedpe_host(f, fo, ext):
    """the text of pairs2bedpe for `f`, written to the open file `fo` on the host"""
    with _open(f) as fh:
        for k, line in enumerate(fh, 1):
            if line.startswith(b"#"):
                continue
            try:
                fo.write(bedpe_line(line[:-1] if line.endswith(b"\n") else line, ext))
            except _Bad as e:
                raise ValueError("%s:%d: %s" % (f, k, e))


def parse_pairs(fs, cs=(), cut=0, unique=False, strand_distances=None, ext=50):
    """the host restatement, and what a read falls back to: every file converted as `pairs2bedpe` does it, then
    cloops_amd.io.parse_bedpe on the texts -> its triple (n_lines: the data lines)"""
    for f in fs:
        check_header(f)
    with tempfile.TemporaryDirectory() as td:
        outs = []
        for k, f in enumerate(fs):
            outs.append(os.path.join(td, "%d.bedpe" % k))
            with open(outs[-1], "wb") as fo:
                _to_bedpe_host(f, fo, ext)
        return cio.parse_bedpe(outs, cs, cut, unique, strand_distances)


def parse_pairs_gpu(fs, cs=(), cut=0, unique=False, strand_distances=None, ext=50, device=0, budget=BUDGET, stats=None, logger=None):
    """parse_pairs on the device (K18) -> (dict chrom -> int64 [n, 3] rows [id, X, Y] in file order, data lines, n_cis)"""
    for f in fs:
        check_header(f)
    return ingest._parse_gpu(fs, cs, cut, unique, strand_distances, device, budget, stats, logger, "pairs", ext,
                             functools.partial(parse_pairs, ext=ext))


def load_pairs(fs, cs=(), cut=0, unique=False, strand_distances=None, ext=50, device=0, prefix="", budget=BUDGET, stats=None, logger=None):
    """cloops_amd.ingest.load_bedpe for pairs files: every chromosome stays in HBM, registered in pipe.CACHE -> the names"""
    for f in fs:
        check_header(f)
    return ingest._load(fs, cs, cut, unique, strand_distances, device, prefix, budget, stats, logger, "pairs", ext,
                        functools.partial(parse_pairs, ext=ext))


def parseRawPairs(fs, fout, cs, cut, ext=50, logger=None, reader="gpu"):
    """the protocol of cloops_amd.io.parseRawBedpe for pairs files -> (`.jd` files, strand distances)"""
    parse = functools.partial(parse_pairs_gpu if reader == "gpu" else _host_reader, ext=ext)
    return ingest._write_jd(fs, fout, cs, cut, True, logger, parse)


def parseRawPairs2(fs, fout, cs, cut, ext=50, logger=None, reader="gpu"):
    """the protocol of cloops_amd.io.parseRawBedpe2 for pairs files -> `.jd` files"""
    parse = functools.partial(parse_pairs_gpu if reader == "gpu" else _host_reader, ext=ext)
    return ingest._write_jd(fs, fout, cs, cut, False, logger, parse)[0]


def _host_reader(fs, cs, cut, unique, strand_distances, ext, logger=None):
    return parse_pairs(fs, cs, cut, unique, strand_distances, ext)


def pairs2bedpe(f, f_out, ext=50, threads=THREADS, budget=BUDGET, device=0, stats=None):
    """4DN pairs `f` (gzip when it ends in .gz) -> BEDPE `f_out` (gzip when it ends in .gz) on the device (K15, CL_CONV_PAIRS)
    -> (lines of BEDPE, bytes of BEDPE text)"""
    check_header(f)
    written = [0]

    def tap(text):
        written[0] += int(np.count_nonzero(np.frombuffer(text, np.uint8) == 10))
    gz = f_out.endswith(".gz")
    _, nbytes = convert._convert("pairs", f, f_out, ext, f.endswith(".gz"), gz, convert._threads(threads) if gz else 1, budget, device,
                                 stats, tap)
    return written[0], nbytes


def bedpe_name(f, out_dir=None):
    """the output of input `f`: `.pairs` / `.pairs.gz` stripped, `.bedpe.gz` added"""
    b = os.path.join(out_dir, os.path.basename(f)) if out_dir is not None else f
    return re.sub(r'\.pairs(\.gz)?$', '', b) + '.bedpe.gz'
