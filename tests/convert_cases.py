"""Test helper for the pairs converters (cloops_amd.convert, K15): a brute-force restatement of the pinned semantics on bytes
(DESIGN.md, K15), the seeded generators of the synthetic pairs files, a seam that routes the host pipeline to the restatement,
and the golden loaders (tests/golden/make_golden_convert.py)."""
import json
import os
import re

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WS = b" \t\n\r\x0b\x0c"                    # Python 2's whitespace of a byte string: what bytes.strip() / bytes.split() use
I64 = (-(1 << 63), (1 << 63) - 1)
_INT = re.compile(rb"[+-]?[0-9]+")


class BadLine(Exception):
    pass


def py2_int(b):
    """Python 2's int() of a byte string, bounded to int64"""
    s = b.strip(WS)
    if not _INT.fullmatch(s):
        raise BadLine("not an integer")
    return _i64(int(s))


def _i64(v):
    if not I64[0] <= v <= I64[1]:
        raise BadLine("integer outside int64")
    return v


def hicpro_line(line, ext):
    """scripts/hicpropairs2bedpe:15-34 on one line (bytes, no '\\n') -> its BEDPE line"""
    f = line.strip(WS).split(b"\t")
    if len(f) < 7:
        raise BadLine("fewer than 7 fields")
    p1, p2 = py2_int(f[2]), py2_int(f[5])
    a = (p1, _i64(p1 + ext)) if f[3] == b"+" else (_i64(p1 - ext), p1)
    b = (p2, _i64(p2 + ext)) if f[6] == b"+" else (_i64(p2 - ext), p2)
    return b"\t".join([f[1], b"%d" % a[0], b"%d" % a[1], f[4], b"%d" % b[0], b"%d" % b[1], f[0], b".", f[3], f[6]]) + b"\n"


def juicer_line(line, ext):
    """scripts/juicerLong2bedpe.py:12-31 on one line (bytes, no '\\n') -> its BEDPE line"""
    f = line.split()
    if len(f) < 7:
        raise BadLine("fewer than 7 fields")
    p1, p2 = py2_int(f[2]), py2_int(f[6])
    lo1, hi1, lo2, hi2 = _i64(p1 - ext), _i64(p1 + ext), _i64(p2 - ext), _i64(p2 + ext)
    s1 = b"+" if f[0] == b"0" else b"-"
    s2 = b"+" if f[4] == b"0" else b"-"
    return b"\t".join([f[1], b"%d" % max(0, lo1), b"%d" % hi1, f[5], b"%d" % max(0, lo2), b"%d" % hi2, b".", b".", s1, s2]) + b"\n"


LINE = {"hicpro": hicpro_line, "juicer": juicer_line}


def split_lines(data):
    """lines end at '\\n' only; the last may lack it; no line after a final '\\n'"""
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def brute(fmt, data, ext):
    """the whole input -> (text, lines converted, None) or (text of the lines before the bad one, their count, reason)"""
    out = []
    for line in split_lines(data):
        try:
            out.append(LINE[fmt](line, ext))
        except BadLine as e:
            return b"".join(out), len(out), str(e)
    return b"".join(out), len(out), None


class BruteSeam(object):
    """the per-chunk seam of cloops_amd.convert on the restatement: plain bytearrays, chunk text as bytes"""
    chunks = []                                     # (k, n, last) of every chunk seen, for the tests

    def __init__(self, fmt, ext, budget, device=0):
        self.fmt, self.ext, self.budget = fmt, ext, budget

    def buffer(self, n):
        return bytearray(n)

    def chunk(self, k, buf, n, last):
        data = bytes(buf[:n])
        BruteSeam.chunks.append((k, n, last))
        if not last:
            if b"\n" not in data:
                assert n == self.budget
                return b"", 0, "line longer than the chunk budget"
            assert data.endswith(b"\n"), "a chunk that is not the last must end at a newline"
        text, nl, err = brute(self.fmt, data, self.ext)
        return text, nl, err

    def close(self):
        pass


def use_brute(monkeypatch):
    from cloops_amd import convert
    BruteSeam.chunks = []
    monkeypatch.setattr(convert, "make_seam", BruteSeam)


# ---- seeded synthetic pairs files -----------------------------------------------------------------------------------------
CHROMS = [b"chr%d" % i for i in range(1, 23)] + [b"chrX", b"chrY", b"chrM"]


def _vocab(words):
    w = max(len(v) for v in words)
    mat = np.zeros((len(words), w), np.uint8)
    for i, v in enumerate(words):
        mat[i, :len(v)] = np.frombuffer(v, np.uint8)
    return mat, np.array([len(v) for v in words], np.int64)


def _ndig(m):
    d = np.ones(len(m), np.int64)
    p = 10
    for _ in range(18):
        d += m >= p
        p *= 10
    return d


def _text(cols, n):
    """n lines made of the columns: bytes constants, int64 arrays (decimal) or (vocabulary, index array) -> bytes"""
    widths = []
    for c in cols:
        if isinstance(c, bytes):
            widths.append(np.full(n, len(c), np.int64))
        elif isinstance(c, tuple):
            widths.append(_vocab(c[0])[1][c[1]])
        else:
            widths.append(_ndig(np.abs(c)) + (c < 0))
    lw = np.sum(widths, axis=0)
    pos = np.concatenate([[0], np.cumsum(lw)[:-1]])
    out = np.zeros(int(lw.sum()), np.uint8)
    for c, w in zip(cols, widths):
        if isinstance(c, bytes):
            for j, ch in enumerate(c):
                out[pos + j] = ch
        elif isinstance(c, tuple):
            mat, _ = _vocab(c[0])
            for j in range(mat.shape[1]):
                sel = w > j
                out[pos[sel] + j] = mat[c[1][sel], j]
        else:
            neg = c < 0
            out[pos[neg]] = ord("-")
            m = np.abs(c)
            e = pos + w                                  # one past the last digit
            for d in range(int((w - neg).max()) if n else 0):
                sel = (w - neg) > d
                out[e[sel] - 1 - d] = 48 + (m[sel] // (10 ** d)) % 10
        pos = pos + w
    return out.tobytes()


def gen_hicpro(n, seed, block=1 << 20):
    """HiC-Pro allValidPairs-shaped lines: read name, chrom, pos, strand, chrom, pos, strand, fragment length, two fragment names,
    two MAPQs (12 columns, positions up to 2.5e8, cis and trans)"""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(0, n, block):
        b = min(block, n - s)
        c1 = rng.integers(0, len(CHROMS), b)
        c2 = np.where(rng.random(b) < 0.8, c1, rng.integers(0, len(CHROMS), b))
        p1 = rng.integers(1, 250_000_000, b)
        p2 = p1 + rng.integers(-1_000_000, 5_000_000, b)
        st = ([b"+", b"-"], rng.integers(0, 2, b))
        st2 = ([b"+", b"-"], rng.integers(0, 2, b))
        out.append(_text([b"SRR", rng.integers(1000000, 9999999, b), b".", np.arange(s, s + b, dtype=np.int64) + 1, b"\t",
                          (CHROMS, c1), b"\t", p1, b"\t", st, b"\t", (CHROMS, c2), b"\t", p2, b"\t", st2, b"\t",
                          rng.integers(100, 900, b), b"\tHIC_", (CHROMS, c1), b"_", rng.integers(1, 999999, b), b"\tHIC_",
                          (CHROMS, c2), b"_", rng.integers(1, 999999, b), b"\t", rng.integers(0, 43, b), b"\t",
                          rng.integers(0, 43, b), b"\n"], b))
    return b"".join(out)


def gen_juicer(n, seed, block=1 << 20):
    """Juicer long-format-shaped lines (space separated): str1 chr1 pos1 frag1 str2 chr2 pos2 frag2 mapq1 mapq2 (strands 0 / 16)"""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(0, n, block):
        b = min(block, n - s)
        c1 = rng.integers(0, len(CHROMS), b)
        c2 = np.where(rng.random(b) < 0.8, c1, rng.integers(0, len(CHROMS), b))
        p1 = rng.integers(1, 250_000_000, b)
        p2 = np.maximum(1, p1 + rng.integers(-1_000_000, 5_000_000, b))
        st = ([b"0", b"16"], rng.integers(0, 2, b))
        st2 = ([b"0", b"16"], rng.integers(0, 2, b))
        out.append(_text([st, b" ", (CHROMS, c1), b" ", p1, b" ", p1 // 4000, b" ", st2, b" ", (CHROMS, c2), b" ", p2, b" ",
                          p2 // 4000, b" ", rng.integers(0, 61, b), b" ", rng.integers(0, 61, b), b"\n"], b))
    return b"".join(out)


GEN = {"hicpro": gen_hicpro, "juicer": gen_juicer}


# ---- goldens --------------------------------------------------------------------------------------------------------------
def golden_meta():
    with open(os.path.join(GOLD, "convert_meta.json")) as fh:
        return json.load(fh)


def golden_case(name):
    """-> (input bytes, expected output bytes: the decompressed text for hicpro)"""
    z = np.load(os.path.join(GOLD, "convert_cases.npz"))
    return z[name + "__in"].tobytes(), z[name + "__out"].tobytes()
