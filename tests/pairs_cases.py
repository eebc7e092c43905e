"""The corner corpus, the seeded synthetic, the brute-force oracle and the brute-force seams of the 4DN pairs tests
(tests/test_pairs.py, tests/test_gpu_pairs.py).

The oracle rests on reference-pinned code only: every data line is permuted to HiC-Pro's column order and given to the HiC-Pro
restatement of tests/convert_cases.py (which reproduces scripts/hicpropairs2bedpe's outputs), and the reader's expectation is
cloops_amd.io.parse_bedpe (which reproduces the reference's parsers) on the text that gives.  Nothing of cloops_amd.pairs is used."""
import os

import numpy as np

import convert_cases as CC
import ingest_cases as IC

COLUMNS = "#columns: readID chr1 pos1 chr2 pos2 strand1 strand2"
HEAD = ["## pairs format v1.0", "#sorted: chr1-chr2-pos1-pos2", "#shape: upper triangle", "#chromsize: chr1 248956422", COLUMNS + " pair_type"]
ARGSETS = IC.ARGSETS


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def permute(line):
    """a data line (bytes, no '\\n') in HiC-Pro's column order: f0 f1 f2 f5 f3 f4 f6 ..."""
    f = line.strip(CC.WS).split(b"\t")
    if len(f) < 7:
        return line
    return b"\t".join([f[0], f[1], f[2], f[5], f[3], f[4], f[6]] + f[7:])


def columns_error(data):
    """the 1-based line of a wrong `#columns:` line in the leading '#' run, or None"""
    for k, line in enumerate(CC.split_lines(data), 1):
        if not line.startswith(b"#"):
            return None
        if line.startswith(b"#columns:") and line[9:].split()[:7] != COLUMNS.encode()[9:].split():
            return k
    return None


def convert(data, ext):
    """-> (BEDPE text of the lines in front of the first bad one, physical lines in front of it, (line, reason) or None)"""
    out = []
    lines = CC.split_lines(data)
    for k, line in enumerate(lines, 1):
        if line.startswith(b"#"):
            continue
        try:
            out.append(CC.hicpro_line(permute(line), ext))
        except CC.BadLine as e:
            return b"".join(out), k - 1, (k, str(e))
    return b"".join(out), len(lines), None


def read(dirpath, files, ext, cs, cut, unique):
    """what the reader must give for the files' bytes -> IC.run's tuple, or ("error", file index, line, reason)"""
    from cloops_amd import io as cio
    for k, data in enumerate(files):
        if columns_error(data) is not None:
            return ("error", k, columns_error(data), "columns")
    outs = []
    for k, data in enumerate(files):
        text, _, err = convert(data, ext)
        if err is not None:
            return ("error", k) + err
        outs.append(os.path.join(str(dirpath), "oracle_%d.bedpe" % k))
        with open(outs[-1], "wb") as fh:
            fh.write(text)
    return IC.run(cio.parse_bedpe, outs, cs, cut, unique)


def run(fn, fs, ext, cs, cut, unique, **kw):
    """fn = parse_pairs / parse_pairs_gpu on the written files -> the shape of read()"""
    import re
    try:
        return IC.run(fn, fs, cs, cut, unique, ext=ext, **kw)
    except ValueError as e:
        m = re.match(r"^(.*):(\d+): (.*)$", str(e), flags=re.S)
        assert m, str(e)
        return ("error", fs.index(m.group(1)), int(m.group(2)), "columns" if m.group(3).startswith("columns") else m.group(3))


# ---- the corpus -------------------------------------------------------------------------------------------------------------------
def pair(c1, p1, c2, p2, s1="+", s2="-", rid="r", extra=("UU",)):
    return "\t".join([rid, c1, str(p1), c2, str(p2), s1, s2] + list(extra))


def _t(lines, end="\n", final=True):
    return (end.join(lines) + (end if final and lines else "")).encode("utf-8")


GOOD = [pair("chr1", 100, "chr1", 5000), pair("chr2", 10, "chr2", 700, "-", "-"), pair("chr1", 9000, "chr1", 300, "+", "+")]
LONG_NAME = "c" * 255


def corpus():
    """-> [(name, [bytes of file 1, ...], ext values, exotic)]: cases without a line the converter raises on"""
    return [
        ("header_only", [_t(HEAD)], (50,), False),
        ("empty_file", [b""], (50,), False),
        ("basic", [_t(HEAD + GOOD)], (0, 1, 50, 77), False),
        ("no_header", [_t(GOOD)], (50,), False),
        ("hash_between", [_t(HEAD + GOOD[:1] + ["#a comment\twith\ttabs", "#"] + GOOD[1:] + ["#last"])], (50,), False),
        ("crlf", [_t(HEAD + GOOD, "\r\n")], (50,), False),
        ("no_final_newline", [_t(HEAD + GOOD, final=False)], (50,), False),
        ("no_final_newline_cr", [_t(HEAD + GOOD, final=False) + b"\r"], (50,), False),
        ("extra_columns", [_t([pair("chr1", 100, "chr1", 5000, extra=()), pair("chr1", 100, "chr1", 5000, extra=("UU", "60", "60", "x y")),
                               pair("chr1", 200, "chr1", 6000, "+", "+ ", extra=("UU",))])], (50,), False),
        ("strands", [_t([pair("chr1", 1000, "chr1", 5000, s1, s2) for s1 in ("+", "-", ".", "+ ", "") for s2 in ("+", "-", ".", " +")])], (0, 33), False),
        ("negative", [_t([pair("chr1", 10, "chr1", 20, "-", "-"), pair("chr1", 0, "chr1", 3, "-", "+"), pair("chr1", -5, "chr1", 40, "+", "-"),
                          pair("chr1", "+7", "chr1", " 12 ", "-", "-"), pair("chr1", "007", "chr1", "-0", "-", "-")])], (0, 1, 50, 77), False),
        ("trans", [_t([pair("chr1", 100, "chr2", 5000), pair("chr2", 100, "chr1", 5000), pair("chr1", 100, "chr10", 5000), pair("chr10", 1, "chr10", 900),
                       pair("chr1", 100, "chr1", 5000), pair("chr", 1, "chr", 2), pair("", 1, "", 2)])], (50,), False),
        ("star_minus1", [_t([pair("chr1", 49, "chr1", 5000, "-", "-", rid="*"), pair("chr1", 49, "chr1", 5000, "-", "-"),
                             pair("chr1", 5000, "chr1", 49, "*", "-"), pair("chr1", 5000, "chr1", 49, "*", "+"), pair("chr1", 100, "chr1", 5000, "*", "-", rid="-1"),
                             pair("chr1", 100, "chr1", 5000, rid="-1"), pair("chr1", 100, "chr1", 5000, rid="*"),
                             pair("chr1", -1, "chr1", 5000, "+", "*"), pair("*", 100, "*", 5000, rid="-1"), pair("chr1", 100, "chr1", 5000, extra=("*", "-1"))])],
         (50, 0), False),
        ("equal_midpoints", [_t([pair("chr1", 100, "chr1", 700, "+", "-"), pair("chr1", 100, "chr1", 700, "+", "+"), pair("chr2", 100, "chr2", 700),
                                 pair("chr1", 700, "chr1", 100, "-", "+"), pair("chr1", 101, "chr1", 701, "-", "+"), pair("chr1", 100, "chr1", 700)]),
                             _t(HEAD + [pair("chr1", 100, "chr1", 700), pair("chr3", 5, "chr3", 900, "-", "+")], final=False)], (0, 1, 50), False),
        ("key_order", [_t([pair("chrZ", 1, "chrY", 3), pair("chrZ", 1, "chrZ", 100), pair("chr1", 1, "chr1", 500), pair("chrY", 1, "chrY", 500),
                           pair("chrZ", 1, "chrZ", 500), pair("chr1", 1, "chr1", 50)])], (50,), False),
        ("long_name", [_t([pair(LONG_NAME, 1, LONG_NAME, 600), pair("chr1", 1, "chr1", 600)])], (50,), False),
        ("control_bytes", [_t([pair("chr1", 1, "chr1", 500, rid="a\x0cb"), pair("chr1", 3, "chr1", 500, rid="a\x0bb\x1c\x00"), pair("chr 1", 3, "chr 1", 500)])],
         (50,), False),
        ("big_below_2_62", [_t([pair("chr1", (1 << 62) - 1, "chr1", 5, "-", "-"), pair("chr1", -(1 << 62) + 1, "chr1", 5, "+", "+")])], (0,), False),
        ("utf8_read_name", [_t(GOOD + [pair("chr1", 100, "chr1", 5000, rid="ré")])], (50,), True),
        ("invalid_utf8", [_t(GOOD) + pair("chr1", 100, "chr1", 5000).encode().replace(b"r\t", b"\xff\t", 1) + b"\n"], (50,), True),
        ("lone_cr", [_t(GOOD[:1]) + (GOOD[1] + "\r" + GOOD[2] + "\n").encode()], (50,), True),
        ("cr_in_name", [_t(GOOD + [pair("chr1\r", 100, "chr1\r", 5000)])], (50,), True),
        ("two_pow_62", [_t(GOOD + [pair("chr1", 1 << 62, "chr1", 5, "-", "-")])], (0,), True),
        ("two_pow_62_by_ext", [_t(GOOD + [pair("chr1", (1 << 62) - 1, "chr1", 5, "+", "-")])], (1,), True),
        ("name_256", [_t(GOOD + [pair(LONG_NAME + "c", 1, LONG_NAME + "c", 600)])], (50,), True),
    ]


def error_cases():
    """-> [(name, [files], ext, (file index, line, reason))]: the first line the converter raises on"""
    big = (1 << 63) - 1
    return [
        ("six_fields", [_t(HEAD + GOOD + ["r\tchr1\t100\tchr1\t5000\t+"] + GOOD)], 50, (0, 9, "fewer than 7 fields")),
        ("blank_line", [_t(HEAD + GOOD[:2] + [""] + GOOD)], 50, (0, 8, "fewer than 7 fields")),
        ("blank_last", [_t(GOOD) + b"\n"], 50, (0, 4, "fewer than 7 fields")),
        ("underscore", [_t(GOOD + [pair("chr1", "1_0", "chr1", 5000)])], 50, (0, 4, "not an integer")),
        ("empty_position", [_t(GOOD + [pair("chr1", 100, "chr1", "")] + GOOD)], 50, (0, 4, "not an integer")),
        ("sign_only", [_t([pair("chr1", "+", "chr1", 5)] + GOOD)], 50, (0, 1, "not an integer")),
        ("overflow_by_ext", [_t(GOOD + [pair("chr1", big - 49, "chr1", 5, "+", "-")])], 50, (0, 4, "integer outside int64")),
        ("overflow_parse", [_t(HEAD + [pair("chr1", 5, "chr1", big + 1)])], 0, (0, 6, "integer outside int64")),
        ("error_after_exotic", [_t(GOOD + [pair("chr1", 100, "chr1", 5000, rid="ré"), "x"])], 50, (0, 5, "fewer than 7 fields")),
        ("second_file", [_t(HEAD + GOOD), _t(HEAD + GOOD + ["bad"])], 50, (1, 9, "fewer than 7 fields")),
        ("wrong_columns", [_t(HEAD[:4] + ["#columns: readID chr1 pos1 strand1 chr2 pos2 strand2"] + GOOD)], 50, (0, 5, "columns")),
        ("short_columns", [_t(["## pairs format v1.0", "#columns: readID chr1 pos1 chr2 pos2 strand1", "bad"])], 50, (0, 2, "columns")),
        ("columns_before_bad_line", [_t(GOOD[:1] + ["bad"]), _t(["#columns: chr1 readID"] + GOOD)], 50, (1, 1, "columns")),
    ]


def write_case(dirpath, name, files, gz=()):
    """-> the paths (file k gzipped when k is in `gz`)"""
    import gzip
    out = []
    for k, data in enumerate(files):
        p = os.path.join(str(dirpath), "%s_%d.pairs%s" % (name, k, ".gz" if k in gz else ""))
        with (gzip.open(p, "wb") if k in gz else open(p, "wb")) as fh:
            fh.write(data)
        out.append(p)
    return out


def budgets(files):
    """chunk budgets: None (the default), the longest line, + 1, 2 x + 1: cuts inside the header run and between any two data lines"""
    m = IC.longest_line(files)
    return [None, m, m + 1, 2 * m + 1]


def assert_same(got, want, what):
    if want[0] == "error":
        assert got == want, (what, got, want)
    else:
        IC.assert_same(got, want, what)


# ---- the seeded synthetic -------------------------------------------------------------------------------------------------------
SEED = 4018


def gen_pairs(n, seed=SEED, header=True, dup=True, order="pairs"):
    """n data lines of pairtools-shaped text (readID chr1 pos1 chr2 pos2 strand1 strand2 pair_type), a fifth trans, drawn with
    repeats from a pool of n // 2 + 1 lines when `dup` (duplicates for `unique`), under the usual header -> bytes; order "hicpro":
    the same lines in HiC-Pro's column order (readID chr1 pos1 strand1 chr2 pos2 strand2 pair_type), without a header"""
    rng = np.random.default_rng(seed)
    m = n // 2 + 1 if dup else n
    c1 = rng.integers(0, len(CC.CHROMS), m)
    c2 = np.where(rng.random(m) < 0.8, c1, rng.integers(0, len(CC.CHROMS), m))
    p1 = rng.integers(1, 250_000_000, m)
    p2 = np.maximum(1, p1 + rng.integers(-1_000_000, 5_000_000, m))
    st, st2 = ([b"+", b"-"], rng.integers(0, 2, m)), ([b"+", b"-"], rng.integers(0, 2, m))
    rid = [b"SRR", rng.integers(1000000, 9999999, m), b".", np.arange(m, dtype=np.int64) + 1, b"\t"]
    if order == "hicpro":
        cols = rid + [(CC.CHROMS, c1), b"\t", p1, b"\t", st, b"\t", (CC.CHROMS, c2), b"\t", p2, b"\t", st2, b"\tUU\n"]
    else:
        cols = rid + [(CC.CHROMS, c1), b"\t", p1, b"\t", (CC.CHROMS, c2), b"\t", p2, b"\t", st, b"\t", st2, b"\tUU\n"]
    text = CC._text(cols, m)
    if dup:
        lines = text.split(b"\n")[:-1]
        text = b"".join(lines[i] + b"\n" for i in rng.integers(0, m, n))
    return (_t(HEAD) if header and order == "pairs" else b"") + text


# ---- the brute-force seams: what the kernels are specified to do, one line at a time ------------------------------------------
class ConvSeam(CC.BruteSeam):
    """cloops_amd.convert's per-chunk seam for fmt "pairs": header lines count as converted lines and have no text"""

    def chunk(self, k, buf, n, last):
        assert self.fmt == "pairs"
        data = bytes(buf[:n])
        CC.BruteSeam.chunks.append((k, n, last))
        if not last:
            if b"\n" not in data:
                assert n == self.budget
                return b"", 0, "line longer than the chunk budget"
            assert data.endswith(b"\n"), "a chunk that is not the last must end at a newline"
        text, nl, err = convert(data, self.ext)
        return text, nl, None if err is None else err[1]


def use_conv_brute(monkeypatch):
    from cloops_amd import convert as cv
    CC.BruteSeam.chunks = []
    monkeypatch.setattr(cv, "make_seam", ConvSeam)


def device_exotic(line):
    """the bytes the device does not decide on a data line: a byte >= 0x80, a '\\r' that is not the last byte before the '\\n'"""
    if line.endswith(b"\r"):
        line = line[:-1]
    return any(c >= 0x80 or c == 13 for c in line)


class ReadSeam(IC.BruteSeam):
    """cloops_amd.ingest's seam for fmt "pairs" on the host"""

    def __init__(self, budget, cut, want_distances, device=0, fmt="pairs", ext=0):
        assert fmt == "pairs"
        IC.BruteSeam.__init__(self, budget, cut, want_distances, device)
        self.ext = ext

    def chunk(self, k, buf, n, last):
        from cloops_amd.ingest import LineError
        IC.BruteSeam.chunks.append((k, n, bool(last)))
        h = k & 1
        if n == 0:
            return IC._BruteChunk(h, 0, [], 0), 0, None
        assert n <= self.budget
        data = bytes(memoryview(buf).cast("B")[:n])
        if not last and not data.endswith(b"\n"):
            return IC._BruteChunk(h, 0, [], n, True), 0, "a line longer than the chunk budget"
        lines = CC.split_lines(data)
        recs, headers = [], 0
        for j, l in enumerate(lines):
            if l.startswith(b"#"):
                headers += 1
                recs.append((False, 0, 0, b"", False, False))
                continue
            try:
                bed = CC.hicpro_line(permute(l), self.ext)[:-1]
            except CC.BadLine as e:
                return IC._BruteChunk(h, len(lines), [], n, True), j, LineError(str(e))
            r = IC.brute_line(bed, self.cut)
            if r[5] or device_exotic(l):
                return IC._BruteChunk(h, len(lines), [], n, True), j, "a line the device does not read"
            recs.append(r)
        first = {}
        for j, r in enumerate(recs):
            if r[0]:
                first.setdefault(self.hash(r[3]), (j, r[3]))
        if len(first) > self.names_max:
            return IC._BruteChunk(h, len(lines), [], n, True), 0, "more than 65536 chromosome names in one chunk"
        names = sorted(((hs, j, nm) for hs, (j, nm) in first.items()), key=lambda t: t[1])
        c = IC._BruteChunk(h, len(lines), names, n, False, recs)
        c.headers = headers
        return c, len(lines), None


def use_read_brute(monkeypatch, **attrs):
    from cloops_amd import ingest
    IC.BruteSeam.chunks = []
    for k, v in attrs.items():
        monkeypatch.setattr(ReadSeam, k, staticmethod(v) if callable(v) else v)
    monkeypatch.setattr(ingest, "make_seam", ReadSeam)
