"""BEDPE input on the GPU: cLoops/io.py:62-129 (parseRawBedpe) and :132-189 (parseRawBedpe2), function for function, with the
array-level loader `parse_bedpe_gpu` (the triple of cloops_amd.io.parse_bedpe) and `load_bedpe`, which leaves every chromosome in
HBM for the sweep; `python -m cloops_amd.ingest -f a.bedpe.gz -o dir` writes the `.jd` directory.

The reference reads one line at a time in Python.  Here the reader thread of cloops_amd.convert reads (or inflates) every file into
page-locked buffers of a byte budget, cut after the last newline and at every file end; kernel K16 indexes and parses every chunk
(`cl_ingest_feed`, two handles on two streams, chunk k on handle k % 2) and hands back the distinct chromosome names of its kept
lines; the host, in chunk order, gives new names their ids (the order of the result's keys), applies the wanted chromosomes and
commits the chunk (`cl_ingest_commit`: the PETs appended to their chromosomes in line order); `cl_ingest_finish` makes one array
per chromosome, removes duplicates when asked and orders the strand distances by line.  The host never touches a PET.

Semantics pinned: exactly cloops_amd.io.parse_bedpe under Python 3's text mode.  What the device does not restate
of Python's int() and text decoding (`1_00`, whitespace or Unicode digits in a numeric field, integers of 2^62 and more, bytes >=
0x80, a lone '\\r') makes a line exotic; a chromosome name longer than 255 bytes, more than 65536 distinct names in a chunk, a line
longer than the chunk budget and two names under one hash count as exotic too.  One exotic line makes the whole call return what
cloops_amd.io.parse_bedpe returns (or raise what it raises) by running it on the host; the logger / stderr says so once and
`stats["fallback"]` holds (reason, file, line).
"""
import argparse
import collections
import ctypes
import gzip
import os
import sys
from datetime import datetime

import numpy as np

from . import convert
from . import io as cio

BUDGET = convert.BUDGET
NAME_MAX = 255               # K16_NAME_LEN
MIN_BUFFER = 4096


class _Chunk(object):
    """what a seam hands back for one chunk: its handle, its lines and its distinct names [(hash, first line, name bytes)]; pairs:
    how many of the lines are header lines"""
    __slots__ = ("h", "lines", "names", "nbytes", "bad", "headers")

    def __init__(self, h, lines, names, nbytes, bad=False, headers=0):
        self.h, self.lines, self.names, self.nbytes, self.bad, self.headers = h, lines, names, nbytes, bad, headers

    def __len__(self):
        return self.nbytes


class Fallback(Exception):
    """the read goes to the host: (reason, file, line)"""


class LineError(str):
    """a seam's reason for a chunk that ends the read with ValueError("<file>:<line>: <reason>") and not with the host's reading:
    a line of a pairs file the converter raises on"""


class _Keep(object):
    """the finished ingest handle and its stream: alive as long as a chromosome made from its arrays"""

    def __init__(self, lib, ing, stream):
        self.lib, self.ing, self.stream = lib, ing, stream

    def close(self):
        if self.ing is not None:
            self.ing.close()
            self.ing = None
            self.lib.cl_stream_destroy(ctypes.c_void_p(self.stream))

    def __del__(self):
        try:
            self.close()
        except Exception:                                               # noqa: BLE001
            pass


class GpuSeam(convert._DeviceSeam):
    """the per-chunk seam on the device: two K16 handles on two streams (chunk k on handle k % 2) and page-locked buffers.  The CPU
    tests put a brute-force seam with the same methods in its place (`make_seam`)."""

    def __init__(self, budget, cut, want_distances, device=0, fmt="bedpe", ext=0):
        from . import api
        convert._DeviceSeam.__init__(self, device, lambda s: api.Ingest(budget, cut, want_distances, device, s, fmt, ext))
        self.device, self.fmt = device, fmt
        self.bufs = []
        self.turn = 0
        self.keep = None
        self.ms_closed = collections.Counter()     # device ms of the handle that finish() closes

    def buffer(self, n):
        """a page-locked input buffer of n bytes; the three of one reader are handed to the next file's reader again"""
        k = self.turn % 3
        self.turn += 1
        if k >= len(self.bufs):
            self.bufs.append((ctypes.c_char * n).from_address(self._pin(n)))
        return self.bufs[k]

    def chunk(self, k, buf, n, last):
        """chunk k of a file: the complete lines of buf[0 .. n) -> (_Chunk, lines in front of the first exotic one, reason or None)"""
        h = k & 1
        if n == 0:
            return _Chunk(h, 0, [], 0), 0, None
        mv = memoryview(buf).cast("B")
        if not last and mv[n - 1] != 10:
            return _Chunk(h, 0, [], n, True), 0, "a line longer than the chunk budget"
        lines, exotic, nn = self.handles[h].feed(ctypes.addressof(buf), n)
        headers = 0
        if self.fmt == "pairs":
            err = self.handles[h].error()
            if err is not None and (exotic < 0 or err[0] - 1 < exotic):
                return _Chunk(h, lines, [], n, True), err[0] - 1, LineError(err[1])
            headers = self.handles[h].headers()
        if exotic >= 0:
            return _Chunk(h, lines, [], n, True), exotic, "a line the device does not read (Python's int() or text decoding decides)"
        if nn < 0:
            return _Chunk(h, lines, [], n, True), 0, "more than 65536 chromosome names in one chunk"
        names = [(hs, first, bytes(mv[off:off + ln])) for hs, first, off, ln in self.handles[h].names(nn)]
        return _Chunk(h, lines, names, n, False, headers), lines, None

    def commit(self, chunk, k, line0, table, n_ids):
        """-> (PETs appended per id, status)"""
        return self.handles[chunk.h].commit(k, line0, table, n_ids)

    def finish(self, n_ids, unique):
        """-> (rows per id, number of distances); the arrays live in `self.keep` from here on"""
        out = self.handles[0].finish(self.handles[1], n_ids, unique)
        self.ms_closed.update(self.handles[1].timing())
        self.handles[1].close()
        self.keep = _Keep(self.lib, self.handles[0], self.streams[0])
        self.lib.cl_stream_destroy(ctypes.c_void_p(self.streams[1]))
        self.handles, self.streams = [], []
        return out

    def rows(self, cid, n):
        return self.keep.ing.rows(cid, n)

    def distances(self, n):
        return self.keep.ing.distances(n)

    def chrom_arrays(self, cid):
        return self.keep.ing.chrom_arrays(cid)

    def timing(self):
        ms = collections.Counter(self.ms_closed)
        for ing in self.handles + ([self.keep.ing] if self.keep is not None and self.keep.ing is not None else []):
            ms.update(ing.timing())
        return ms

    def close(self):
        """frees the handles, streams and buffers (not `keep` once somebody took it: see load_bedpe)"""
        convert._DeviceSeam.close(self)
        self.bufs = []


def make_seam(budget, cut, want_distances, device=0, fmt="bedpe", ext=0):
    return GpuSeam(budget, cut, want_distances, device, fmt, ext)


def rows_matrix(X, Y):
    """int64 [n, 3] rows [id, X, Y] as cloops_amd.io.parse_bedpe builds them (io.py:181-183: id = the row counter)"""
    n = len(X)
    m = np.empty((n, 3), dtype=np.int64)
    m[:, 0] = np.arange(n)
    m[:, 1] = X
    m[:, 2] = Y
    return m


def _budget_for(fs, budget):
    """plain files smaller than the budget need no buffers of the whole budget"""
    if any(f.endswith(".gz") for f in fs):
        return budget
    return min(budget, max([MIN_BUFFER] + [os.path.getsize(f) + 1 for f in fs]))


def _read(fs, cs, cut, unique, want_distances, device, budget, stats, fmt="bedpe", ext=0):
    """the device read -> (seam after finish, chromosome names in key order, rows per id, number of distances, lines: for pairs the
    data lines); raises Fallback, or for pairs the converter's ValueError"""
    budget = int(budget)
    wanted = set(c.encode() if isinstance(c, str) else bytes(c) for c in cs) if cs else set()
    eff = _budget_for(fs, budget) if budget == BUDGET else budget
    seam = make_seam(eff, cut, want_distances, device) if fmt == "bedpe" else make_seam(eff, cut, want_distances, device, fmt, ext)
    ids, by_hash, order = {}, {}, []
    state = {"line": 0, "chunk": 0, "file": None, "headers": 0}

    def write(chunk):                                                   # in chunk order: the dictionary, then the commit
        if chunk.bad:                                                   # the read ends here: _read raises Fallback
            return
        table = []
        for hs, _, name in chunk.names:
            cid = ids.get(name)
            if cid is None:
                if by_hash.setdefault(hs, name) != name:
                    raise Fallback("two chromosome names under one hash", state["file"], state["line"] + 1)
                if len(name) > NAME_MAX:
                    raise Fallback("a chromosome name longer than %d bytes" % NAME_MAX, state["file"], state["line"] + 1)
                cid = -1 if wanted and name not in wanted else len(order)
                if cid >= 0:
                    order.append(name)
                ids[name] = cid
            table.append((hs, cid, name))
        if chunk.lines:
            _, status = seam.commit(chunk, state["chunk"], state["line"], table, len(order))
            if status:
                raise Fallback("two chromosome names under one hash", state["file"], state["line"] + 1)
        state["line"] += chunk.lines
        state["headers"] += getattr(chunk, "headers", 0)
        state["chunk"] += 1

    try:
        for f in fs:
            state["file"] = f
            line0 = state["line"]
            src = gzip.open(f, "rb") if f.endswith(".gz") else open(f, "rb", buffering=0)
            with src:
                lines, _, err, line = convert._run(src, seam, eff, write, stats)
            if isinstance(err, LineError):
                raise ValueError("%s:%d: %s" % (f, line, err))
            if err is not None:
                raise Fallback(err, f, line0 + line)
        rows, n_dist = seam.finish(len(order), unique)
    except BaseException:
        _account(seam, stats)
        seam.close()
        raise
    return seam, [n.decode("ascii") for n in order], rows, n_dist, state["line"] - state["headers"]


def _account(seam, stats):
    for key, v in seam.timing().items():
        stats["device_ms_" + key] += v


class _Stats(collections.Counter):
    """the counters of one call, copied into the caller's `stats` (any mapping) when it ends"""

    def publish(self, user):
        if user is not None:
            for key, v in self.items():
                user[key] = v


def _say(logger, msg):
    if logger is not None:
        logger.info(msg)
    else:
        sys.stderr.write(msg + "\n")


def _fallback(e, stats, logger, what="BEDPE"):
    reason, f, line = e.args
    stats["fallback"] = (reason, f, line)
    _say(logger, "%s reader: %s:%d: %s; reading on the host" % (what, f, line, reason))


def parse_bedpe_gpu(fs, cs=(), cut=0, unique=False, strand_distances=None, device=0, budget=BUDGET, stats=None, logger=None):
    """cloops_amd.io.parse_bedpe on the device -> (dict chrom -> int64 [n, 3] rows [id, X, Y] in file order, n_lines, n_cis)"""
    return _parse_gpu(fs, cs, cut, unique, strand_distances, device, budget, stats, logger)


def _parse_gpu(fs, cs, cut, unique, strand_distances, device, budget, stats, logger, fmt="bedpe", ext=0, host=None):
    """parse_bedpe_gpu for `fmt`; host(fs, cs, cut, unique, strand_distances) is what a Fallback runs (None: cloops_amd.io.parse_bedpe)"""
    user, stats = stats, _Stats()
    stats["fallback"] = None
    try:
        seam, names, rows, n_dist, n_lines = _read(fs, cs, cut, unique, strand_distances is not None, device, budget, stats, fmt, ext)
    except Fallback as e:
        _fallback(e, stats, logger, "BEDPE" if fmt == "bedpe" else fmt)
        stats.publish(user)
        return (host or cio.parse_bedpe)(fs, cs, cut, unique, strand_distances)
    try:
        out = {}
        for cid, name in enumerate(names):
            a, b = seam.rows(cid, int(rows[cid]))
            out[name] = rows_matrix(a, b)
        if strand_distances is not None:
            strand_distances.extend(seam.distances(n_dist).tolist())
    finally:
        _account(seam, stats)
        keep = seam.keep
        seam.close()
        if keep is not None:
            keep.close()
        stats.publish(user)
    return out, n_lines, int(sum(int(r) for r in rows))


def load_bedpe(fs, cs=(), cut=0, unique=False, strand_distances=None, device=0, prefix="", budget=BUDGET, stats=None, logger=None):
    """the read of parse_bedpe_gpu, but every chromosome stays in HBM: wrapped by api.Chromosome.from_device_pointers on one of the
    sweep's shared streams (the ingest's arrays as keepalive) and registered in pipe.CACHE as 'mem://<prefix>/<chr>-<chr>' with
    host copies of X / Y -> the names, in the order of parse_bedpe's keys.  Coordinates outside |v| < 2^29 raise the CL_ERR_DOMAIN
    error of api.Chromosome.  A read that fell back to the host registers the host rows with CACHE.put_arrays."""
    return _load(fs, cs, cut, unique, strand_distances, device, prefix, budget, stats, logger)


def _load(fs, cs, cut, unique, strand_distances, device, prefix, budget, stats, logger, fmt="bedpe", ext=0, host=None):
    """load_bedpe for `fmt`; `host` as in _parse_gpu"""
    from . import api, pipe
    user, stats = stats, _Stats()
    stats["fallback"] = None

    def pseudo(name):
        return "%s/%s-%s" % (prefix, name, name) if prefix else "%s-%s" % (name, name)

    try:
        seam, names, rows, n_dist, n_lines = _read(fs, cs, cut, unique, strand_distances is not None, device, budget, stats, fmt, ext)
    except Fallback as e:
        _fallback(e, stats, logger, "BEDPE" if fmt == "bedpe" else fmt)
        mats, n_lines, n_cis = (host or cio.parse_bedpe)(fs, cs, cut, unique, strand_distances)
        stats["lines"], stats["cis"] = n_lines, n_cis
        stats.publish(user)
        return [pipe.CACHE.put_arrays(pseudo(c), m[:, 1], m[:, 2], device=device, key=(c, c)) for c, m in mats.items()]
    out = []
    keep = seam.keep
    try:
        for cid, name in enumerate(names):
            n = int(rows[cid])
            X, Y = seam.rows(cid, n)
            _, xp, yp = seam.chrom_arrays(cid)

            def make(stream, xp=xp, yp=yp, n=n):
                return api.Chromosome.from_device_pointers(xp, yp, n, device=device, stream=stream, keepalive=keep)
            out.append(pipe.CACHE.put_chrom("mem://" + pseudo(name), pipe._make_chrom(X, Y, device, make=make), X, Y, key=(name, name),
                                            device=device))
        if strand_distances is not None:
            strand_distances.extend(seam.distances(n_dist).tolist())
    except BaseException:
        for f in out:
            pipe.CACHE.drop(f)
        raise
    finally:
        _account(seam, stats)
        seam.close()
    stats["lines"], stats["cis"] = n_lines, int(sum(int(r) for r in rows))
    stats.publish(user)
    return out


def _write_jd(fs, fout, cs, cut, unique, logger, parse=None):
    """parse: the reader (None: parse_bedpe_gpu; cloops_amd.pairs hands in its own)"""
    import joblib
    for f in fs:
        if logger is not None:
            logger.info("Parsing PETs from %s, requiring initial distance cutoff > %s" % (f, cut))
    ds = [] if unique else None
    mats, i, j = (parse or parse_bedpe_gpu)(fs, cs, cut, unique=unique, strand_distances=ds, logger=logger)
    cfs = []
    for c, m in mats.items():
        cf = os.path.join(fout, "%s-%s" % (c, c) + ".jd")
        joblib.dump(m, cf)
        cfs.append(cf)
    if logger is not None:
        logger.info("Totaly %s PETs from %s, in which %s cis PETs" % (i, ",".join(fs), j))
    return cfs, ds


def parseRawBedpe(fs, fout, cs, cut, logger=None):
    """cLoops/io.py:62-129 on the GPU reader: the protocol of cloops_amd.io.parseRawBedpe -> (`.jd` files, strand distances)"""
    return _write_jd(fs, fout, cs, cut, True, logger)


def parseRawBedpe2(fs, fout, cs, cut, logger=None):
    """cLoops/io.py:132-189 on the GPU reader: the protocol of cloops_amd.io.parseRawBedpe2 -> `.jd` files"""
    return _write_jd(fs, fout, cs, cut, False, logger)[0]


def _help(argv):
    ap = argparse.ArgumentParser(prog="python -m cloops_amd.ingest",
                                 description="Read BEDPE or 4DN pairs files on MI355X into a directory of per-chromosome .jd files (what `cloops_amd -s` leaves).")
    ap.add_argument("-f", dest="fnIn", required=True, type=str, help="BEDPE (or, with -fmt pairs, 4DN pairs) file(s), plain or .gz, separated by commas.")
    ap.add_argument("-fmt", dest="fmt", required=False, default="bedpe", choices=["bedpe", "pairs"], help="Input format, default bedpe.")
    ap.add_argument("-ext", dest="ext", required=False, default=50, type=int,
                    help="-fmt pairs: extension from the position of each read, as `convert pairs -ext`; default 50.")
    ap.add_argument("-o", dest="fnOut", required=True, type=str, help="Output directory (created; must not exist).")
    ap.add_argument("-c", dest="chroms", required=False, default="", type=str, help="Chromosomes to keep, separated by commas; default all.")
    ap.add_argument("-cut", dest="cut", required=False, default=0, type=int, help="Initial distance cutoff, default 0.")
    return ap.parse_args(argv)


def main(argv=None):
    """-> exit status"""
    start = datetime.now()
    op = _help(argv)
    fs = op.fnIn.split(",")
    for f in fs:
        if not os.path.isfile(f):
            sys.stderr.write("Error: input file %s not exists!\n" % f)
            return 1
    if os.path.exists(op.fnOut):
        sys.stderr.write("Error: %s exists, unable to create output folder\n" % op.fnOut)
        return 1
    os.makedirs(op.fnOut)
    cs = [c for c in op.chroms.split(",") if c]
    if op.fmt == "pairs":
        from . import pairs
        try:
            cfs = pairs.parseRawPairs2(fs, op.fnOut, cs, op.cut, ext=op.ext)
        except ValueError as e:
            sys.stderr.write("Error: %s\n" % e)
            return 1
    else:
        cfs = parseRawBedpe2(fs, op.fnOut, cs, op.cut)
    sys.stderr.write("%d chromosomes written to %s. Used time: %s Bye!\n" % (len(cfs), op.fnOut, datetime.now() - start))
    return 0


if __name__ == "__main__":
    sys.exit(main())
