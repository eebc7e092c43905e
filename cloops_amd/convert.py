"""Pairs files to BEDPE: scripts/hicpropairs2bedpe (pairs2bedpe) and scripts/juicerLong2bedpe.py (long2bedpe), function for
function, and both scripts as `python -m cloops_amd.convert hicpro|juicer`; `python -m cloops_amd.convert pairs` converts 4DN
pairs files (cloops_amd.pairs, which builds on the pipeline below).

The reference reads one line at a time in Python.  Here a reader thread reads (or inflates) the input straight into page-locked
buffers of a byte budget, cut after the last newline (the tail goes in front of the next chunk); kernel K15 indexes, parses and
renders every chunk (`cl_conv_feed` / `cl_conv_render`, two handles on two streams, chunk k on handle k % 2, so the copies and
kernels of one chunk overlap the copy back and the writing of the one before); the text is written in order, for `.gz` output as
independent gzip members compressed by a pool of host threads.

Semantics pinned:
- hicpro: `line.strip().split('\\t')`, A = [f1, p, p + ext] when f3 is exactly "+", else [f1, p - ext, p], B the same from f4, f5,
  f6; line `A0 A1 A2 B0 B1 B2 f0 . f3 f6`; output gzip (level 9).  juicer: `line.split()`, line `f1 max(0, p1 - ext) p1 + ext f5
  max(0, p2 - ext) p2 + ext . . s1 s2`, s = "+" where f0 / f4 is exactly "0"; output plain text.
- Python 2's reading of bytes: lines end at '\\n' only; whitespace is ASCII \\t \\n \\v \\f \\r and space; an integer is an optional
  sign and ASCII digits with optional whitespace around it ('_' is an error); values that leave int64 with +-ext applied are an error.
- The first line the reference raises on (fewer than 7 fields, a blank line, a bad integer) stops the conversion with
  ValueError("<file>:<line>: <reason>"); the output then holds exactly the lines in front of it (a complete gzip file for .gz).
- Deviations: gz input of hicpro is read (the Python-3 reference cannot); the .gz output is several gzip members; a line longer
  than the chunk budget is an error; int64 bounds.
"""
import argparse
import collections
import ctypes
import glob
import gzip
import os
import queue
import re
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from datetime import datetime

from . import _lib

BUDGET = 64 << 20            # bytes of input per chunk
THREADS = 8                  # -p: gzip member pool
MAX_THREADS = 16
MEMBER = 4 << 20             # bytes of text per gzip member
_NL_WINDOW = 1 << 16


class _DeviceSeam(object):
    """what the seams on the device share (this one and cloops_amd.ingest's): two handles on two library streams, chunk k on handle
    k % 2, and the page-locked blocks they own"""

    def __init__(self, device, make):
        """make(stream) -> the handle (api.Converter, api.Ingest) of that stream"""
        self.lib = _lib.load()
        self.handles, self.streams, self.pins = [], [], []
        for _ in range(2):
            self.streams.append(_lib.stream_create(device))
            self.handles.append(make(self.streams[-1]))

    def _pin(self, n):
        self.pins.append(_lib.host_alloc(n))
        return self.pins[-1]

    def close(self):
        for h in self.handles:
            h.close()
        for s in self.streams:
            self.lib.cl_stream_destroy(ctypes.c_void_p(s))
        for p in self.pins:
            self.lib.cl_host_free(ctypes.c_void_p(p))
        self.handles, self.streams, self.pins = [], [], []


class GpuSeam(_DeviceSeam):
    """the per-chunk seam on the device: two K15 handles on two streams (chunk k on handle k % 2) and page-locked buffers.  The CPU
    tests put a brute-force seam with the same methods in its place (`make_seam`)."""

    def __init__(self, fmt, ext, budget, device=0):
        from . import api
        _DeviceSeam.__init__(self, device, lambda s: api.Converter(fmt, ext, budget, device, s))
        self.outs = [None, None]                  # per handle: (address, capacity) of its page-locked output buffer
        self.ms = collections.Counter()

    def buffer(self, n):
        """a page-locked input buffer of n bytes (a ctypes array: writable, with the buffer protocol)"""
        return (ctypes.c_char * n).from_address(self._pin(n))

    def _out(self, h, n):
        cur = self.outs[h]
        if cur is None or cur[1] < n:
            if cur is not None:
                self.pins.remove(cur[0])
                self.lib.cl_host_free(ctypes.c_void_p(cur[0]))
            cap = max(n, 1 << 20) + (max(n, 1 << 20) >> 3)
            self.outs[h] = cur = (self._pin(cap), cap)
        return cur

    def chunk(self, k, buf, n, last):
        """chunk k: the complete lines of buf[0 .. n) (the last line may lack its newline when `last`) -> (text, lines converted,
        error): text a bytes-like object valid until chunk k + 2 is asked for; error None, or the reason the line after the
        converted ones is bad"""
        h = k & 1
        cv = self.handles[h]
        addr = ctypes.addressof(buf)
        parts, lines, done = [], 0, 0
        while True:
            used, nl, nb, err = cv.feed(addr + done, n - done, last)
            ptr, cap = self._out(h, nb)
            got = cv.render(ptr, cap)
            for key, v in cv.timing().items():
                self.ms[key] += v
            text = memoryview((ctypes.c_char * got).from_address(ptr)).cast("B") if got else b""
            lines += nl
            done += used
            if err is not None or done >= n or used == 0:
                break
            parts.append(bytes(text))                                   # a feed that stopped early on very short lines
        if parts:
            text = b"".join(parts) + bytes(text)
        if err is None and done < n:
            raise RuntimeError("K15 left %d bytes of a chunk unconverted" % (n - done))
        return text, lines, None if err is None else err[1]


def make_seam(fmt, ext, budget, device=0):
    return GpuSeam(fmt, ext, budget, device)


def _last_newline(mv, n):
    """the position after the last '\\n' in mv[0 .. n), 0 if there is none"""
    e = n
    while e > 0:
        s = max(0, e - _NL_WINDOW)
        i = bytes(mv[s:e]).rfind(b"\n")
        if i >= 0:
            return s + i + 1
        e = s
    return 0


class _Reader(threading.Thread):
    """reads (or inflates) the input into three buffers of the seam in turn: chunk = complete lines, the tail carried over"""

    def __init__(self, fh, seam, budget, stats):
        threading.Thread.__init__(self, daemon=True)
        self.fh, self.budget, self.stats = fh, budget, stats
        self.free = queue.Queue()
        for _ in range(3):
            self.free.put(seam.buffer(budget))
        self.chunks = queue.Queue()
        self.stop = threading.Event()

    def _get_free(self):
        while not self.stop.is_set():
            try:
                return self.free.get(timeout=0.1)
            except queue.Empty:
                pass
        return None

    def run(self):
        try:
            carry, k = b"", 0
            while True:
                buf = self._get_free()
                if buf is None:
                    return
                mv = memoryview(buf).cast("B")
                n = len(carry)
                mv[:n] = carry
                t0 = time.perf_counter()
                eof = False
                while n < self.budget:
                    r = self.fh.readinto(mv[n:])
                    if not r:
                        eof = True
                        break
                    n += r
                self.stats["read"] += time.perf_counter() - t0
                cut = n if eof else _last_newline(mv, n)
                if cut == 0 and not self.fh.read(1):                   # a full buffer that ends the input without a newline
                    eof, cut = True, n
                final = eof or cut == 0                                 # no newline in a full buffer: the seam reports it
                if cut == 0:
                    cut = n
                carry = bytes(mv[cut:n])
                self.chunks.put((k, buf, cut, eof, final))
                k += 1
                if final:
                    return
        except BaseException as e:                                      # noqa: BLE001  (handed to the consumer)
            self.chunks.put(e)

    def finish(self):
        self.stop.set()
        self.join()


def _run(fh, seam, budget, write, stats):
    """the pipeline: reader thread -> seam (two chunks in flight) -> write(text) in chunk order -> (lines, bytes, error reason,
    line of the error)"""
    rd = _Reader(fh, seam, budget, stats)
    rd.start()
    pool = ThreadPoolExecutor(2)
    inflight = collections.deque()
    lines = nbytes = 0
    try:
        more = True
        while True:
            while more and len(inflight) < 2:                           # chunk k + 2 waits until chunk k is written
                item = rd.chunks.get()
                if isinstance(item, BaseException):
                    raise item
                k, buf, n, last, final = item
                inflight.append((buf, pool.submit(seam.chunk, k, buf, n, last)))
                more = not final
            if not inflight:
                return lines, nbytes, None, 0
            buf, fut = inflight.popleft()
            t0 = time.perf_counter()
            text, nl, err = fut.result()
            stats["wait_device"] += time.perf_counter() - t0
            rd.free.put(buf)
            t0 = time.perf_counter()
            write(text)
            stats["write"] += time.perf_counter() - t0
            lines += nl
            nbytes += len(text)
            if err is not None:
                return lines, nbytes, err, lines + 1
    finally:
        for _, fut in inflight:
            try:
                fut.result()
            except Exception:                                           # noqa: BLE001
                pass
        pool.shutdown()
        rd.finish()


class _GzWriter(object):
    """gzip members (level 9, gzip.open's default) of at most MEMBER bytes of text each, compressed by a pool of threads and written
    in order; at least one member, so that empty text is a valid gzip file"""

    def __init__(self, fo, threads):
        self.fo = fo
        self.pool = ThreadPoolExecutor(threads)
        self.pending = collections.deque()
        self.limit = 2 * threads
        self.members = 0

    def write(self, text):
        for s in range(0, len(text), MEMBER):
            piece = bytes(text[s:s + MEMBER])                           # the caller's buffer is reused after this call
            self.pending.append(self.pool.submit(gzip.compress, piece, 9, mtime=0))
            while len(self.pending) > self.limit:
                self._flush_one()

    def _flush_one(self):
        self.fo.write(self.pending.popleft().result())
        self.members += 1

    def close(self):
        try:
            while self.pending:
                self._flush_one()
            if self.members == 0:
                self.fo.write(gzip.compress(b"", 9, mtime=0))
        finally:
            self.pool.shutdown()


def _threads(threads):
    threads = int(threads)
    if not 1 <= threads <= MAX_THREADS:
        raise ValueError("threads must be 1 .. %d, got %d" % (MAX_THREADS, threads))
    return threads


def _tapped(write, tap):
    def both(text):
        tap(text)
        write(text)
    return both if tap is not None else write


def _convert(fmt, fin, fout, ext, gz_in, gz_out, threads, budget, device, stats, tap=None):
    """tap(text): sees every chunk's text before it is written (cloops_amd.pairs counts its lines)"""
    stats = stats if stats is not None else collections.Counter()
    seam = make_seam(fmt, ext, budget, device)
    try:
        src = gzip.open(fin, "rb") if gz_in else open(fin, "rb", buffering=0)
        with src, open(fout, "wb") as fo:
            if gz_out:
                gzw = _GzWriter(fo, threads)
                try:
                    lines, nbytes, err, line = _run(src, seam, budget, _tapped(gzw.write, tap), stats)
                finally:
                    t0 = time.perf_counter()
                    gzw.close()
                    stats["write"] += time.perf_counter() - t0
            else:
                lines, nbytes, err, line = _run(src, seam, budget, _tapped(fo.write, tap), stats)
    finally:
        for key, v in getattr(seam, "ms", {}).items():
            stats["device_ms_" + key] += v
        seam.close()
    if err is not None:
        raise ValueError("%s:%d: %s" % (fin, line, err))
    return lines, nbytes


def pairs2bedpe(f_hicpro, f_out, ext=50, threads=THREADS, budget=BUDGET, device=0, stats=None):
    """scripts/hicpropairs2bedpe:9-35: HiC-Pro allValidPairs `f_hicpro` (gzip when it ends in .gz) -> gzipped BEDPE `f_out`
    -> (lines, bytes of BEDPE text)"""
    return _convert("hicpro", f_hicpro, f_out, ext, f_hicpro.endswith(".gz"), True, _threads(threads), budget, device, stats)


def long2bedpe(fin, fout, ext=75, budget=BUDGET, device=0, stats=None):
    """scripts/juicerLong2bedpe.py:10-32: Juicer long format `fin` (read as plain bytes) -> BEDPE text `fout` -> (lines, bytes)"""
    return _convert("juicer", fin, fout, ext, False, False, 1, budget, device, stats)


def hicpro_inputs(inputs, err=None):
    """the files of mainHelp's inputs in the script's order (hicpropairs2bedpe:49-65): missing ones skipped with a warning,
    directories expanded by its four globs, each sorted"""
    err = err or sys.stderr
    out = []
    for inp in inputs:
        if not os.path.exists(inp):
            err.write("Warning: %s not exist, skipping\n" % inp)
            continue
        if os.path.isfile(inp):
            out.append(inp)
        else:
            for pat in ("*_allValidPairs", "*_allValidPairs.gz", os.path.join("*", "*_allValidPairs"),
                        os.path.join("*", "*_allValidPairs.gz")):
                out.extend(sorted(glob.glob(os.path.join(inp, pat))))
    return out


def bedpe_name(f, out_dir=None):
    """hicpropairs2bedpe:66-72: the output of input `f`"""
    b = os.path.join(out_dir, os.path.basename(f)) if out_dir is not None else f
    return re.sub(r'_allValidPairs(.gz)?$', '', b) + '.bedpe.gz'


def _help(argv):
    ap = argparse.ArgumentParser(prog="python -m cloops_amd.convert",
                                 description="Convert pairs files to BEDPE for cLoops (scripts hicpropairs2bedpe / juicerLong2bedpe.py, 4DN pairs) on MI355X.")
    sub = ap.add_subparsers(dest="cmd", required=True)
    h = sub.add_parser("hicpro", help="Convert hicpro allValidPairs file to bedpe format for cLoops")
    h.add_argument(dest="input", nargs="+", type=str,
                   help="HiC-Pro allValidPairs files, folders or folders whose subfolders contain files ended with '_allValidPairs'. "
                        "Files and files inside folder could be gzipped (with additional .gz suffix).")
    h.add_argument("-o", "--out", dest="out", required=False, type=str,
                   help="Output directory. If specified all converted bedpe file will be put inside this folder rather than the same folder of respective input file.")
    h.add_argument("-ext", dest="ext", required=False, type=int, default=50,
                   help="Extension from read center (HiC-Pro output the center of each read), default is 50. ")
    h.add_argument("-p", dest="threads", required=False, type=int, default=THREADS,
                   help="Threads compressing the gzip output, 1 .. %d, default is %d." % (MAX_THREADS, THREADS))
    j = sub.add_parser("juicer", help="Convert Juicer long format file to bedpe format for cLoops")
    j.add_argument("-i", "--input", dest="fin", required=True, type=str, help="Input file name, required.")
    j.add_argument("-o", "--out", dest="fout", required=True, type=str, help="Output file name, required.")
    q = sub.add_parser("pairs", help="Convert 4DN pairs files (.pairs, .pairs.gz) to bedpe format for cLoops")
    q.add_argument(dest="input", nargs="+", type=str, help="4DN pairs files, plain or gzipped (with additional .gz suffix).")
    q.add_argument("-o", "--out", dest="out", required=False, type=str,
                   help="Output directory. If specified all converted bedpe file will be put inside this folder rather than the same folder of respective input file.")
    q.add_argument("-ext", dest="ext", required=False, type=int, default=50, help="Extension from the position of each read, default is 50. ")
    q.add_argument("-p", dest="threads", required=False, type=int, default=THREADS,
                   help="Threads compressing the gzip output, 1 .. %d, default is %d." % (MAX_THREADS, THREADS))
    op = ap.parse_args(argv)
    if op.cmd in ("hicpro", "pairs") and not 1 <= op.threads <= MAX_THREADS:
        ap.error("-p must be 1 .. %d" % MAX_THREADS)
    return op


def main(argv=None):
    """scripts/hicpropairs2bedpe (main, :38-76) and scripts/juicerLong2bedpe.py (main, :35-43) -> exit status"""
    start = datetime.now()
    op = _help(argv)
    try:
        if op.cmd in ("hicpro", "pairs"):
            if op.out is not None:
                if os.path.isfile(op.out):
                    sys.stderr.write("Error: file %s exists, unable to create output folder\n" % op.out)
                    return 1
                if not os.path.isdir(op.out):
                    os.makedirs(op.out)
        if op.cmd == "hicpro":
            for f in hicpro_inputs(op.input):
                pairs2bedpe(f, bedpe_name(f, op.out), ext=op.ext, threads=op.threads)
        elif op.cmd == "pairs":
            from . import pairs
            for f in op.input:
                if not os.path.isfile(f):
                    sys.stderr.write("Error: input file %s not exists!\n" % f)
                    return 1
            for f in op.input:
                pairs.pairs2bedpe(f, pairs.bedpe_name(f, op.out), ext=op.ext, threads=op.threads)
        else:
            if not os.path.isfile(op.fin):
                sys.stderr.write("Error: input file %s not exists!\n" % op.fin)
                return 1
            if os.path.isfile(op.fout):
                sys.stderr.write("Error: output file %s exists! \n" % op.fout)
            long2bedpe(op.fin, op.fout)
    except ValueError as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1
    sys.stderr.write("Process finished. Used time: %s Bye!\n" % (datetime.now() - start))
    return 0


if __name__ == "__main__":
    sys.exit(main())
