"""The corner corpus, the seeded synthetic and the brute-force seam of the BEDPE reader tests (tests/test_ingest.py,
tests/test_gpu_ingest.py, tests/golden/make_golden_ingest.py).

`BruteSeam` restates, on bytes and one line at a time, what kernel K16 is specified to do: the reading rules, the
device's integer classes (a) / (b) / (c) and the exotic rule; put in place of cloops_amd.ingest.make_seam it lets the host pipeline
(chunks, dictionary, order, fallback) run without a GPU."""
import gzip
import hashlib
import itertools
import json
import os

import numpy as np

from test_io import LINES

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ingest_reference.json")

ARGSETS = list(itertools.product(((), ("chr1",)), (0, 200), (False, True)))         # (cs, cut, unique), distances always on


def argkey(cs, cut, unique):
    return "cs=%s;cut=%d;unique=%d" % (",".join(cs), cut, int(unique))


def pet(c, s1, e1, s2, e2, sa="+", sb="-", rid="r", c2=None, extra=()):
    return "\t".join([c, str(s1), str(e1), c if c2 is None else c2, str(s2), str(e2), rid, "1", sa, sb] + list(extra))


def _t(lines, end="\n", final=True):
    return (end.join(lines) + (end if final and lines else "")).encode("utf-8")


GOOD = [pet("chr1", 100, 201, 5000, 5100), pet("chr2", 10, 20, 700, 800, "-", "-"), pet("chr1", 9000, 9100, 300, 401, "+", "+")]
LONG_NAME = "c" * 255


def _nonint(v):
    return [pet("chr1", v, 20, 300, 400), pet("chr1", 10, v, 300, 400), pet("chr1", 10, 20, v, 400), pet("chr1", 10, 20, 300, v)]


def corpus():
    """-> [(name, [bytes of file 1, ...], exotic)]"""
    many = [pet("n%d" % (k % 3000), 10 + k, 20 + k, 700, 800 + k) for k in range(4000)]
    dup = [pet("chr1", 100, 200, 700, 800, "+", "-"), pet("chr1", 100, 200, 700, 800, "+", "+"), pet("chr2", 100, 200, 700, 800),
           pet("chr1", 101, 199, 701, 799, "-", "+"), pet("chr1", 1, 2, 500, 600), pet("chr1", 700, 800, 100, 200, "-", "+")]
    cases = [
        ("test_io_lines", [_t(LINES)], False),
        ("crlf", [_t(LINES, "\r\n")], False),
        ("no_final_newline", [_t(LINES, final=False)], False),
        ("blank_lines", [_t(["", GOOD[0], "", "", GOOD[1], ""])], False),
        ("only_newlines", [b"\n\n\n"], False),
        ("empty_file", [b""], False),
        ("empty_then_good", [b"", _t(GOOD)], False),
        ("fields_9_10_14", [_t(["\t".join(GOOD[0].split("\t")[:9]), GOOD[1], pet("chr1", 5, 6, 900, 1000, extra=("a", "b", "c", "d"))])], False),
        ("star_minus1_late", [_t([pet("chr1", 5, 6, 900, 1000, extra=("*", "-1")), pet("chr1", 7, 8, 900, 1000, extra=("*",)),
                                  pet("chr1", 9, 10, 900, 1000, extra=("-1", "x")), pet("chr1", 11, 12, 900, 1000, rid="*", extra=("q", "-1")),
                                  pet("chr1", -1, 12, 900, 1000, rid="*"), pet("chr1", "*", 12, 900, -1)])], False),
        ("signs_and_zeros", [_t([pet("chr1", "+100", 201, 5000, 5100), pet("chr1", -300, -299, -50, 61), pet("chr1", -300, 1, -7, 2),
                                 pet("chr1", "00012", "0013", "007", "-0"), pet("chr1", "-7", "0", "-1", "-4")])], False),
        ("nonint_b", [_t(sum((_nonint(v) for v in ("x", "1e5", "1.5", "0x10", "+", "", "-", "12a", "1,000")), []) + GOOD)], False),
        ("equal_sums", [_t([pet("chr1", 100, 200, 150, 150, "+", "-"), pet("chr1", 100, 201, 150, 150), pet("chr1", 7, 7, 7, 7, "-", "+")])], False),
        ("swapped_strands", [_t([pet("chr1", 9000, 9100, 300, 401, "+", "-"), pet("chr1", 9000, 9100, 300, 401, "-", "-"),
                                 pet("chr1", 9000, 9100, 300, 401, "+", "+x"), pet("chr1", 9000, 9100, 300, 401, "", "")])], False),
        ("dups_in_chunk", [_t(dup)], False),
        ("dups_across_files", [_t(dup), _t(list(reversed(dup))), _t(dup, final=False)], False),
        ("names", [_t([pet("chr10", 1, 2, 500, 600), pet("chr1", 1, 2, 500, 600), pet(LONG_NAME, 1, 2, 500, 600), pet("chr1", 3, 4, 500, 600),
                       pet("chr1", 3, 4, 500, 600, c2="chr10"), pet("chr", 3, 4, 500, 600), pet("", 3, 4, 500, 600), pet("chr-1", 3, 4, 500, 600)])], False),
        ("key_order", [_t([pet("chrZ", 1, 2, 3, 4, c2="chrY"), pet("chrZ", 1, 2, 100, 101), pet("chrY", "x", 2, 500, 600), pet("chr1", 1, 2, 500, 600),
                           pet("chrY", 1, 2, 500, 600), pet("chrZ", 1, 2, 500, 600), pet("chr1", 1, 2, 50, 60)])], False),
        ("many_names", [_t(many)], False),
        ("formfeed_in_read_name", [_t([pet("chr1", 1, 2, 500, 600, rid="a\x0cb"), pet("chr1", 3, 4, 500, 600, rid="a\x0bb\x1c\x00")])], False),
        ("underscore", [_t(GOOD + [pet("chr1", "1_00", 201, 5000, 5100)])], True),
        ("spaces", [_t(GOOD + [pet("chr1", " 100 ", 201, 5000, 5100)])], True),
        ("vertical_tab", [_t(GOOD + [pet("chr1", "100\x0b", 201, 5000, 5100)])], True),
        ("file_separator", [_t(GOOD + [pet("chr1", "100\x1c", 201, 5000, 5100)])], True),
        ("twenty_digits", [_t(GOOD + [pet("chr1", "99999999999999999999", 201, 5000, 5100)])], True),
        ("lone_cr", [_t(GOOD[:1]) + (GOOD[1] + "\r" + GOOD[2] + "\n").encode()], True),
        ("utf8_read_name", [_t(GOOD + [pet("chr1", 100, 201, 5000, 5100, rid="ré")])], True),
        ("invalid_utf8", [_t(GOOD) + pet("chr1", 100, 201, 5000, 5100).encode().replace(b"\tr\t", b"\t\xff\t") + b"\n"], True),
        ("arabic_indic_digits", [_t(GOOD + [pet("chr1", "١٢", 201, 5000, 5100)])], True),
    ]
    return cases


def write_case(dirpath, name, files):
    out = []
    for k, data in enumerate(files):
        p = os.path.join(str(dirpath), "%s_%d.bedpe" % (name, k))
        with open(p, "wb") as fh:
            fh.write(data)
        out.append(p)
    return out


def longest_line(files):
    return max([len(l) + 1 for data in files for l in data.split(b"\n")] + [1])


SYNTH_SEED = 20161
SYNTH_CHROMS = ["chr%d" % k for k in range(1, 23)] + ["chrX"]


def synth_bedpe(n, seed=SYNTH_SEED, pool=200000):
    """n lines drawn (with repeats: duplicates for `unique`) from a seeded pool of BEDPE lines over 23 chromosomes; about one in
    thirty is trans, one in fifty holds '*' and '-1' -> bytes"""
    rng = np.random.default_rng(seed)
    m = min(pool, n)
    ca = rng.integers(0, 23, m)
    trans = rng.integers(0, 30, m) == 0
    cb = np.where(trans, (ca + 1) % 23, ca)
    s1 = rng.integers(0, 1 << 26, m)
    s2 = s1 + rng.integers(-5000, 200000, m)
    l1, l2 = rng.integers(20, 150, m), rng.integers(20, 150, m)
    sa, sb = rng.integers(0, 2, m), rng.integers(0, 2, m)
    star = rng.integers(0, 50, m) == 0
    lines = []
    for k in range(m):
        if star[k]:
            lines.append("%s\t%d\t%d\t*\t-1\t-1\tp%d\t1\t%s\t*\n" % (SYNTH_CHROMS[ca[k]], s1[k], s1[k] + l1[k], k, "+-"[sa[k]]))
        else:
            lines.append("%s\t%d\t%d\t%s\t%d\t%d\tp%d\t1\t%s\t%s\n" % (SYNTH_CHROMS[ca[k]], s1[k], s1[k] + l1[k], SYNTH_CHROMS[cb[k]], max(0, s2[k]),
                                                                      max(0, s2[k]) + l2[k], k, "+-"[sa[k]], "+-"[sb[k]]))
    lines = [l.encode() for l in lines]
    idx = rng.integers(0, m, n)
    return b"".join([lines[i] for i in idx])


def write_synth(dirpath, n, seed=SYNTH_SEED):
    """two files holding n lines together: the first half plain, the second gzipped -> their paths"""
    data = synth_bedpe(n, seed)
    cut = data.index(b"\n", len(data) // 2) + 1
    a, b = os.path.join(str(dirpath), "synth_a.bedpe"), os.path.join(str(dirpath), "synth_b.bedpe.gz")
    with open(a, "wb") as fh:
        fh.write(data[:cut])
    with gzip.GzipFile(b, "wb", compresslevel=1, mtime=0) as fh:
        fh.write(data[cut:])
    return [a, b]


# ---- running a reader ---------------------------------------------------------------------------------------------------------------
def run(fn, fs, cs, cut, unique, **kw):
    """fn = cloops_amd.io.parse_bedpe or cloops_amd.ingest.parse_bedpe_gpu -> ("ok", mats, n_lines, n_cis, distances) or
    ("raises", exception type)"""
    ds = []
    try:
        mats, n_lines, n_cis = fn(fs, cs, cut, unique, ds, **kw)
    except (OverflowError, UnicodeDecodeError) as e:
        return ("raises", type(e))
    return ("ok", mats, n_lines, n_cis, ds)


def assert_same(got, want, what):
    """key order, every array (int64, [n, 3]), n_lines, n_cis, the distance list"""
    assert got[0] == want[0], what
    if want[0] == "raises":
        assert got[1] is want[1], what
        return
    assert list(got[1].keys()) == list(want[1].keys()), what
    for c, m in want[1].items():
        g = got[1][c]
        assert g.dtype == np.int64 and g.ndim == 2 and g.shape[1] == 3, what
        assert np.array_equal(g, m), (what, c)
    assert got[2] == want[2] and got[3] == want[3], (what, got[2:4], want[2:4])
    assert list(got[4]) == list(want[4]), what


def budgets(files):
    """the chunk budgets every case runs with: None (the default), the longest line, + 1, + 7, 2 x + 1, 4096"""
    m = longest_line(files)
    return [None, m, m + 1, m + 7, 2 * m + 1, 4096]


# ---- digests -----------------------------------------------------------------------------------------------------------------------
def _sha(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    return hashlib.sha1(repr(a.shape).encode() + a.tobytes()).hexdigest()


def digest_result(mats, ds):
    """what the golden stores of a result: key order, a digest per chromosome's rows, a digest of the distances (None: not asked);
    more than 64 chromosomes: one digest of the keys and one of all rows, in key order"""
    keys, rows = list(mats.keys()), {c: _sha(m) for c, m in mats.items()}
    if len(keys) > 64:
        rows = {"*": hashlib.sha1("".join(rows[c] for c in keys).encode()).hexdigest()}
        keys = ["*", hashlib.sha1("\n".join(keys).encode()).hexdigest()]
    return {"keys": keys, "rows": rows, "ds": None if ds is None else _sha(ds)}


def golden():
    with open(GOLD) as fh:
        return json.load(fh)


def check_against_golden(g, name, cs, cut, unique, mats, ds):
    """asserts the result against the reference's own (where it returned one): rows always; distances for `unique` (parseRawBedpe
    returns them, parseRawBedpe2 has none)"""
    want = g["cases"].get(name, {}).get(argkey(cs, cut, unique))
    if want is None or "raises" in want:
        return False
    got = digest_result(mats, ds)
    assert got["keys"] == want["keys"], (name, cs, cut, unique)
    assert got["rows"] == want["rows"], (name, cs, cut, unique)
    if unique:
        assert got["ds"] == want["ds"], (name, cs, cut, unique)
    return True


# ---- the brute-force seam --------------------------------------------------------------------------------------------------------
def brute_int(b):
    """the device's integer classes -> ("int", v) | ("skip",) | ("exotic",)"""
    body = b[1:] if b[:1] in (b"+", b"-") else b
    if body and all(48 <= c <= 57 for c in body):
        v = int(body)
        if v >= 1 << 62:
            return ("exotic",)
        return ("int", -v if b[:1] == b"-" else v)
    if all(0x21 <= c <= 0x7e and c != 0x5f for c in b):
        return ("skip",)
    return ("exotic",)


def brute_line(line, cut):
    """one line (without its '\\n') -> (kept, cA, cB, name, strands differ, exotic)"""
    if line.endswith(b"\r"):
        line = line[:-1]
    exotic = any(c >= 0x80 or c == 13 for c in line)
    f = line.split(b"\t")
    skip = (b"*" in f and b"-1" in f) or len(f) < 10
    vals = []
    if len(f) >= 10:
        for k in (1, 2, 4, 5):
            r = brute_int(f[k])
            exotic = exotic or r[0] == "exotic"
            skip = skip or r[0] != "int"
            vals.append(r[1] if r[0] == "int" else 0)
    if skip or f[0] != f[3]:
        return False, 0, 0, b"", False, exotic
    if len(f[0]) > 255:
        exotic = True
    sa, sb = vals[0] + vals[1], vals[2] + vals[3]
    if sa > sb:
        sa, sb = sb, sa
    cA, cB = sa // 2, sb // 2
    if cut > 0 and cB - cA < cut:
        return False, 0, 0, b"", False, exotic
    return True, cA, cB, f[0], f[8] != f[9], exotic


def default_hash(name):
    return int.from_bytes(hashlib.sha1(name).digest()[:8], "little") or 1


class _BruteChunk(object):
    def __init__(self, h, lines, names, nbytes, bad=False, recs=()):
        self.h, self.lines, self.names, self.nbytes, self.bad, self.recs = h, lines, names, nbytes, bad, recs

    def __len__(self):
        return self.nbytes


class BruteSeam(object):
    """the methods of cloops_amd.ingest.GpuSeam on the host; `chunks` records (k, n, last) of every chunk of every instance"""
    chunks = []
    hash = staticmethod(default_hash)
    names_max = 65536

    def __init__(self, budget, cut, want_distances, device=0):
        self.budget, self.cut, self.want = budget, cut, want_distances
        self.store = {}                            # id -> [(chunk, line, cA, cB, strands differ)]
        self.final = None

    def buffer(self, n):
        import ctypes
        return (ctypes.c_char * n)()

    def chunk(self, k, buf, n, last):
        BruteSeam.chunks.append((k, n, bool(last)))
        h = k & 1
        if n == 0:
            return _BruteChunk(h, 0, [], 0), 0, None
        assert n <= self.budget
        data = bytes(memoryview(buf).cast("B")[:n])
        if not last and not data.endswith(b"\n"):
            return _BruteChunk(h, 0, [], n, True), 0, "a line longer than the chunk budget"
        lines = data.split(b"\n")
        if data.endswith(b"\n"):
            lines.pop()
        recs = [brute_line(l, self.cut) for l in lines]
        for j, r in enumerate(recs):
            if r[5]:
                return _BruteChunk(h, len(lines), [], n, True), j, "a line the device does not read"
        first = {}
        for j, r in enumerate(recs):
            if r[0]:
                first.setdefault(self.hash(r[3]), (j, r[3]))
        if len(first) > self.names_max:
            return _BruteChunk(h, len(lines), [], n, True), 0, "more than 65536 chromosome names in one chunk"
        names = sorted(((hs, j, nm) for hs, (j, nm) in first.items()), key=lambda t: t[1])
        return _BruteChunk(h, len(lines), names, n, False, recs), len(lines), None

    def commit(self, chunk, k, line0, table, n_ids):
        tab = {hs: (cid, nm) for hs, cid, nm in table}
        counts = [0] * n_ids
        add = []
        for j, r in enumerate(chunk.recs):
            if not r[0]:
                continue
            cid, nm = tab[self.hash(r[3])]
            if nm != r[3]:
                return counts, 1
            if cid >= 0:
                add.append((cid, (k, line0 + j, r[1], r[2], r[4])))
        for cid, row in add:
            self.store.setdefault(cid, []).append(row)
            counts[cid] += 1
        return counts, 0

    def finish(self, n_ids, unique):
        self.final, ds = [], []
        for cid in range(n_ids):
            rows = sorted(self.store.get(cid, []))
            if unique:
                seen, kept = set(), []
                for r in rows:
                    if (r[2], r[3]) not in seen:
                        seen.add((r[2], r[3]))
                        kept.append(r)
                rows = kept
            self.final.append(rows)
            ds += [(r[1], r[3] - r[2]) for r in rows if r[4]]
        self.ds = [d for _, d in sorted(ds)] if self.want else []
        return [len(r) for r in self.final], len(self.ds)

    def rows(self, cid, n):
        assert n == len(self.final[cid])
        return (np.array([r[2] for r in self.final[cid]], dtype=np.int64), np.array([r[3] for r in self.final[cid]], dtype=np.int64))

    def distances(self, n):
        assert n == len(self.ds)
        return np.array(self.ds, dtype=np.int64)

    def timing(self):
        return {}

    keep = None

    def close(self):
        pass


def use_brute(monkeypatch, **attrs):
    from cloops_amd import ingest
    BruteSeam.chunks = []
    for k, v in attrs.items():
        monkeypatch.setattr(BruteSeam, k, staticmethod(v) if callable(v) else v)
    monkeypatch.setattr(ingest, "make_seam", BruteSeam)
