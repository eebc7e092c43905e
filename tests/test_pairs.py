"""CPU: 4DN pairs files (cloops_amd.pairs): the host restatement `parse_pairs` and, with the device seams replaced by the
brute-force seams of tests/pairs_cases.py, the whole chunk pipeline of the converter and of the reader against the oracle (the
HiC-Pro restatement on permuted columns, then cloops_amd.io.parse_bedpe); the fallback decision, error text and line numbers,
`sniff`, the three command lines and the new ABI entries."""
import gzip
import os
import re

import numpy as np
import pytest

import convert_cases as CC
import ingest_cases as IC
import pairs_cases as P
from cloops_amd import _lib, convert, ingest, pairs, pipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = P.corpus()
ERRORS = P.error_cases()


def _read_out(path):
    with open(path, "rb") as fh:
        raw = fh.read()
    return gzip.decompress(raw) if str(path).endswith(".gz") else raw


def test_oracle_is_the_hicpro_rule_on_permuted_columns():
    """the pinned line, spelled out once by hand"""
    assert P.convert(b"r1\tchr1\t100\tchr2\t5000\t+\t-\tUU\n", 50) == (b"chr1\t100\t150\tchr2\t4950\t5000\tr1\t.\t+\t-\n", 1, None)
    assert P.convert(b"#x\nr1\tchr1\t10\tchr1\t20\t-\t+ \tUU\n", 50) == (b"chr1\t-40\t10\tchr1\t-30\t20\tr1\t.\t-\t+ \n", 2, None)
    assert P.convert(b"r\tc\t1\tc\t2\t+\n", 50) == (b"", 0, (1, "fewer than 7 fields"))


@pytest.mark.parametrize("name,files,exts,exotic", CORPUS, ids=[c[0] for c in CORPUS])
def test_host_restatement_and_pipeline_equal_the_oracle(tmp_path, monkeypatch, name, files, exts, exotic):
    """every case x ext x argument set: parse_pairs, and parse_pairs_gpu on the brute seam at every chunk budget, give the oracle's
    triple and distances; the host is asked exactly for the exotic cases"""
    P.use_read_brute(monkeypatch)
    fs = P.write_case(tmp_path, name, files, gz=(1,))
    for ext in exts:
        for cs, cut, unique in P.ARGSETS:
            want = P.read(tmp_path, files, ext, cs, cut, unique)
            P.assert_same(P.run(pairs.parse_pairs, fs, ext, cs, cut, unique), want, (name, ext, cs, cut, unique, "host"))
            for b in P.budgets(files):
                stats = {}
                kw = {"stats": stats} if b is None else {"stats": stats, "budget": b}
                got = P.run(pairs.parse_pairs_gpu, fs, ext, cs, cut, unique, **kw)
                P.assert_same(got, want, (name, ext, cs, cut, unique, b))
                small = b is not None and b < IC.longest_line(files) + (0 if all(f.endswith(b"\n") or not f for f in files) else 1)
                if exotic:
                    assert stats["fallback"] is not None and stats["fallback"][1] in fs, (name, b)
                elif not small:
                    assert stats["fallback"] is None, (name, b, stats["fallback"])


@pytest.mark.parametrize("name,files,ext,err", ERRORS, ids=[c[0] for c in ERRORS])
def test_error_lines(tmp_path, monkeypatch, name, files, ext, err):
    """the reader (host and pipeline) raises the converter's ValueError; the converter writes exactly the lines in front of it, and
    nothing at all under a wrong `#columns:` line"""
    P.use_read_brute(monkeypatch)
    P.use_conv_brute(monkeypatch)
    fs = P.write_case(tmp_path, name, files)
    want = ("error",) + err
    assert P.read(tmp_path, files, ext, (), 0, False) == want
    assert P.run(pairs.parse_pairs, fs, ext, (), 0, True) == want
    for b in P.budgets(files):
        kw = {} if b is None else {"budget": b}
        assert P.run(pairs.parse_pairs_gpu, fs, ext, ("chr1",), 0, False, **kw) == want, b
    k, line, reason = err
    out = str(tmp_path / "o.bedpe.gz")
    for b in P.budgets(files[k:k + 1]):
        kw = {} if b is None else {"budget": b}
        if os.path.exists(out):
            os.remove(out)
        with pytest.raises(ValueError) as ei:
            pairs.pairs2bedpe(fs[k], out, ext=ext, **kw)
        assert str(ei.value).startswith("%s:%d: %s" % (fs[k], line, reason)), str(ei.value)
        if reason == "columns":
            assert not os.path.exists(out)
        else:
            assert _read_out(out) == P.convert(files[k], ext)[0]


def test_converter_pipeline(tmp_path, monkeypatch):
    """pairs2bedpe on the brute seam: text, counts, plain and gzipped input and output, budgets that cut inside the header run"""
    P.use_conv_brute(monkeypatch)
    for name, files, exts, _ in CORPUS:
        fs = P.write_case(tmp_path, name, files, gz=(0,))
        for ext in exts:
            want = P.convert(files[0], ext)[0]
            for b in P.budgets(files[:1]):
                kw = {} if b is None else {"budget": b}
                for out in ("o.bedpe.gz", "o.bedpe"):
                    assert pairs.pairs2bedpe(fs[0], str(tmp_path / out), ext=ext, **kw) == (want.count(b"\n"), len(want)), (name, ext, b)
                    assert _read_out(str(tmp_path / out)) == want, (name, ext, b)
    data = P.gen_pairs(3000)
    f = P.write_case(tmp_path, "synth", [data])[0]
    want = P.convert(data, 50)[0]
    assert want.count(b"\n") == 3000
    CC.BruteSeam.chunks = []
    assert pairs.pairs2bedpe(f, str(tmp_path / "s.bedpe.gz"), budget=20000) == (3000, len(want))
    assert _read_out(str(tmp_path / "s.bedpe.gz")) == want and len(CC.BruteSeam.chunks) > 5


def test_chunk_cuts_at_every_offset(tmp_path, monkeypatch):
    """a header, data, a '#' line between, CRLF, a second file without final newline: every budget from the longest line on gives
    the oracle's result, n_lines counts the data lines only, and the chunks cover every byte once"""
    P.use_read_brute(monkeypatch)
    a = P._t(P.HEAD + P.GOOD[:2] + ["#mid"] + P.GOOD[2:], "\r\n")
    b = P._t(P.HEAD[:2] + P.GOOD + [P.pair("chr3", 5, "chr3", 900, "-", "+")], final=False)
    fs = P.write_case(tmp_path, "cuts", [a, b])
    lo = IC.longest_line([a, b])
    for unique in (False, True):
        want = P.read(tmp_path, [a, b], 50, (), 0, unique)
        assert want[2] == 7 and list(want[1].keys()) == ["chr1", "chr2", "chr3"]
        for budget in range(lo, len(a) + len(b) + 2):
            IC.BruteSeam.chunks = []
            stats = {}
            P.assert_same(P.run(pairs.parse_pairs_gpu, fs, 50, (), 0, unique, budget=budget, stats=stats), want, budget)
            assert stats["fallback"] is None
            assert sum(n for _, n, _ in IC.BruteSeam.chunks) == len(a) + len(b)
            assert all(n <= budget for _, n, _ in IC.BruteSeam.chunks)


def test_fallback_cases_of_the_pipeline(tmp_path, monkeypatch, capsys):
    """a hash collision, too many names, a line over the budget: the host reads, says so once, and the result is the oracle's"""
    files = [P._t(P.HEAD + P.GOOD)]
    fs = P.write_case(tmp_path, "fb", files)
    want = P.read(tmp_path, files, 50, (), 0, True)
    P.use_read_brute(monkeypatch, hash=lambda name: 7)
    stats = {}
    P.assert_same(P.run(pairs.parse_pairs_gpu, fs, 50, (), 0, True, stats=stats), want, "hash")
    assert stats["fallback"][0] == "two chromosome names under one hash"
    P.use_read_brute(monkeypatch, hash=IC.default_hash, names_max=1)
    stats = {}
    P.assert_same(P.run(pairs.parse_pairs_gpu, fs, 50, (), 0, True, stats=stats), want, "names")
    assert stats["fallback"][0].startswith("more than 65536")
    P.use_read_brute(monkeypatch, names_max=65536)
    stats = {}
    P.assert_same(P.run(pairs.parse_pairs_gpu, fs, 50, (), 0, True, stats=stats, budget=IC.longest_line(files) - 1), want, "long")
    assert stats["fallback"][0] == "a line longer than the chunk budget"
    capsys.readouterr()
    said = []

    class Log(object):
        def info(self, m):
            said.append(m)
    ex = P.write_case(tmp_path, "ex", dict((c[0], c[1]) for c in CORPUS)["utf8_read_name"])
    stats = {}
    pairs.parse_pairs_gpu(ex, stats=stats, logger=Log())
    assert stats["fallback"][1:] == (ex[0], 4) and len(said) == 1 and "%s:4:" % ex[0] in said[0] and "reading on the host" in said[0]
    assert capsys.readouterr().err == ""


def test_sniff_and_names(tmp_path):
    a = P.write_case(tmp_path, "a", [P._t(P.HEAD + P.GOOD)], gz=(0,))[0]
    b = P.write_case(tmp_path, "b", [P._t(P.GOOD)])[0]
    c = P.write_case(tmp_path, "c", [P._t(["#columns: x"] + P.GOOD)])[0]
    e = P.write_case(tmp_path, "e", [b""])[0]
    assert a.endswith(".pairs.gz") and [pairs.sniff(f) for f in (a, b, c, e, str(tmp_path / "missing"))] == ["pairs", "bedpe", "bedpe", "bedpe", "bedpe"]
    assert pairs.bedpe_name("/x/y/s.pairs.gz", "/o") == "/o/s.bedpe.gz"
    assert pairs.bedpe_name("/x/y/s.pairs") == "/x/y/s.bedpe.gz"
    assert pairs.bedpe_name("/x/y/s.txt") == "/x/y/s.txt.bedpe.gz"


def test_convert_command_line(tmp_path, monkeypatch, capsys):
    P.use_conv_brute(monkeypatch)
    data = P._t(P.HEAD + P.GOOD)
    a, b = P.write_case(tmp_path, "cl", [data, data], gz=(1,))
    o = tmp_path / "out"
    assert convert.main(["pairs", a, b, "-o", str(o), "-ext", "7", "-p", "2"]) == 0
    assert sorted(os.listdir(str(o))) == ["cl_0.bedpe.gz", "cl_1.bedpe.gz"]
    for n in os.listdir(str(o)):
        assert _read_out(str(o / n)) == P.convert(data, 7)[0]
    assert convert.main(["pairs", a]) == 0
    assert _read_out(str(tmp_path / "cl_0.bedpe.gz")) == P.convert(data, 50)[0]
    assert convert.main(["pairs", str(tmp_path / "missing.pairs")]) == 1
    bad = P.write_case(tmp_path, "bad", [P._t(P.GOOD + ["x"])])[0]
    assert convert.main(["pairs", bad]) == 1
    assert "bad_0.pairs:4: fewer than 7 fields" in capsys.readouterr().err
    assert _read_out(str(tmp_path / "bad_0.bedpe.gz")) == P.convert(P._t(P.GOOD), 50)[0]
    with pytest.raises(SystemExit):
        convert.main(["pairs", a, "-p", "17"])
    capsys.readouterr()


def test_ingest_command_line(tmp_path, monkeypatch, capsys):
    P.use_read_brute(monkeypatch)
    files = [P._t(P.HEAD + P.GOOD), P._t(P.GOOD[:1])]
    a, b = P.write_case(tmp_path, "cl", files)
    out = str(tmp_path / "jd")
    assert ingest.main(["-f", a + "," + b, "-o", out, "-fmt", "pairs", "-ext", "10", "-c", "chr1", "-cut", "200"]) == 0
    assert sorted(os.listdir(out)) == ["chr1-chr1.jd"]
    key, mat = pipe.parseJd(os.path.join(out, "chr1-chr1.jd"))
    want = P.read(tmp_path, files, 10, ("chr1",), 200, False)
    assert key == ("chr1", "chr1") and np.array_equal(mat, want[1]["chr1"])
    bad = P.write_case(tmp_path, "bad", [P._t(P.GOOD + ["x"])])[0]
    assert ingest.main(["-f", bad, "-o", out + "2", "-fmt", "pairs"]) == 1
    assert "bad_0.pairs:4: fewer than 7 fields" in capsys.readouterr().err


def test_main_command_line_options(tmp_path, monkeypatch):
    """`python -m cloops_amd`: -fmt and -ext reach pipe(); auto picks pairs exactly under the magic first line; `-reader host`
    writes the .jd files of parse_pairs"""
    seen = []
    monkeypatch.setattr(pipe, "pipe", lambda *a, **kw: seen.append(kw))
    assert pipe.main(["-f", "x", "-o", "y", "-m", "1"]) == 0 and (seen[-1]["fmt"], seen[-1]["ext"]) == ("auto", 50)
    assert pipe.main(["-f", "x", "-o", "y", "-m", "1", "-fmt", "pairs", "-ext", "0"]) == 0 and (seen[-1]["fmt"], seen[-1]["ext"]) == ("pairs", 0)
    with pytest.raises(SystemExit):
        pipe.main(["-f", "x", "-o", "y", "-m", "1", "-fmt", "sam"])
    monkeypatch.undo()
    with pytest.raises(ValueError, match="fmt must be"):
        pipe.pipe(["x"], str(tmp_path / "p"), [500], [5], fmt="sam")
    files = [P._t(P.HEAD + P.GOOD)]
    f = P.write_case(tmp_path, "m", files)[0]
    called = []

    def sweep(cfs, *a, **kw):
        called.append([pipe.parseJd(c) for c in cfs])
        raise KeyboardInterrupt                                          # the read is what this test is about
    monkeypatch.setattr(pipe, "runSweepFast", sweep)
    with pytest.raises(KeyboardInterrupt):
        pipe.pipe([f], str(tmp_path / "h"), [500], [5], reader="host", ext=10)
    want = P.read(tmp_path, files, 10, (), 0, False)
    assert [k for k, _ in called[0]] == [("chr1", "chr1"), ("chr2", "chr2")]
    for (k, m), c in zip(called[0], ("chr1", "chr2")):
        assert np.array_equal(m, want[1][c])


def test_abi_entries():
    """CL_CONV_PAIRS, cl_ingest_set_format, cl_ingest_error and cl_ingest_headers: in the header (with what each replaces), the
    binding table, the constants and the built library"""
    with open(os.path.join(ROOT, "include", "cloops_hip.h")) as fh:
        src = fh.read()
    for name, proto in (("cl_ingest_set_format", r"int cl_ingest_set_format\(cl_ingest\* c, int32_t format, int64_t ext\);"),
                        ("cl_ingest_error", r"int cl_ingest_error\(cl_ingest\* c, int64_t\* line, int32_t\* kind\);"),
                        ("cl_ingest_headers", r"int cl_ingest_headers\(cl_ingest\* c, int64_t\* n\);")):
        assert re.search(proto, src), name
        assert re.search(r"\* %s -- (?:(?!\n \*\n).)*?replaces" % name, src, flags=re.S), name     # within its own paragraph
        assert name in _lib.PROTOTYPES
    for name, value in (("CL_CONV_PAIRS", 2), ("CL_INGEST_BEDPE", 0), ("CL_INGEST_PAIRS", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), src) and getattr(_lib, name) == value
    from cloops_amd import api
    assert api.Converter.OWN_FORMATS == {"pairs": _lib.CL_CONV_PAIRS}
    assert api.Ingest.FORMATS == {"bedpe": _lib.CL_INGEST_BEDPE, "pairs": _lib.CL_INGEST_PAIRS}
    lib = _lib.load()
    for name in ("cl_ingest_set_format", "cl_ingest_error", "cl_ingest_headers"):
        assert getattr(lib, name) is not None
    if lib.cl_device_count() == 0:                                      # no CPU path: the handles fail loudly
        with pytest.raises(_lib.CloopsHipError):
            api.Converter("pairs", 50)
    with pytest.raises(ValueError):
        api.Converter("sam", 50)
