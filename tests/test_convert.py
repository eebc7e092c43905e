"""CPU: the pairs converters (cloops_amd.convert, scripts/hicpropairs2bedpe and scripts/juicerLong2bedpe.py).  The brute-force
restatement of tests/convert_cases.py reproduces the reference's outputs (tests/golden/make_golden_convert.py) and the deviation
table; with the per-chunk seam routed to it, the host pipeline (chunks, carry, order, gzip members, the written prefix on error)
and both command lines are checked on small budgets."""
import gzip
import os

import pytest

import convert_cases as C
from cloops_amd import convert


def _write(path, data):
    with open(path, "wb") as fh:
        fh.write(data)
    return str(path)


def _read_out(path):
    with open(path, "rb") as fh:
        raw = fh.read()
    return gzip.decompress(raw) if str(path).endswith(".gz") else raw


def test_brute_reproduces_goldens():
    meta = C.golden_meta()
    assert len(meta["cases"]) >= 30
    for g in meta["cases"]:
        data, want = C.golden_case(g["name"])
        text, nl, err = C.brute(g["format"], data, g["ext"])
        assert text == want, g["name"]
        assert nl == g["lines"]
        assert (err is None) == (g["error"] is None), g["name"]


DEVIATIONS = [
    # a lone '\r' is no line break (Python 3's text reading would make two lines of it)
    ("hicpro", b"a\tc\t1\t+\tc\t2\t+\rb\n", 5, b"c\t1\t6\tc\t-3\t2\ta\t.\t+\t+\rb\n", None),
    ("juicer", b"0 c 10 0 0 c 20\r16 x\n", 5, b"c\t5\t15\tc\t15\t25\t.\t.\t+\t+\n", None),
    # '_' in an integer is an error (Python 3's int accepts it)
    ("hicpro", b"a\tc\t1_000\t+\tc\t2\t+\n", 5, b"", "not an integer"),
    ("juicer", b"0 c 10 0 0 c 2_0\n", 5, b"", "not an integer"),
    # 0x1c .. 0x1f are no whitespace (Python 3's str.split / strip take them)
    ("hicpro", b"a\tc\t1\t+\tc\t2\t+\x1c\n", 5, b"c\t1\t6\tc\t-3\t2\ta\t.\t+\t+\x1c\n", None),
    ("juicer", b"0\x1c c 10 0 0 c 20\n", 5, b"c\t5\t15\tc\t15\t25\t.\t.\t-\t+\n", None),
    ("juicer", b"0 c 10 0 0\x1cc 20\n", 5, b"", "fewer than 7 fields"),
    ("juicer", b"0 c\x1f 10 0 0 c 20\n", 5, b"c\x1f\t5\t15\tc\t15\t25\t.\t.\t+\t+\n", None),
    # int64 bounds (Python ints are unbounded)
    ("hicpro", b"a\tc\t9223372036854775807\t+\tc\t2\t+\n", 1, b"", "integer outside int64"),
    ("hicpro", b"a\tc\t9223372036854775807\t-\tc\t2\t+\n", 1, b"c\t9223372036854775806\t9223372036854775807\tc\t2\t3\ta\t.\t-\t+\n", None),
    ("hicpro", b"a\tc\t9223372036854775808\t-\tc\t2\t+\n", 0, b"", "integer outside int64"),
    ("juicer", b"0 c -9223372036854775808 0 0 c 5\n", 1, b"", "integer outside int64"),
    ("juicer", b"0 c -9223372036854775808 0 0 c 5\n", 0, b"c\t0\t-9223372036854775808\tc\t5\t5\t.\t.\t+\t+\n", None),
]


@pytest.mark.parametrize("fmt,data,ext,want,err", DEVIATIONS)
def test_deviation_table(fmt, data, ext, want, err):
    text, nl, e = C.brute(fmt, data, ext)
    assert text == want and e == err


def test_gz_input_is_read_as_plain(tmp_path, monkeypatch):
    """deviation: a gzipped allValidPairs converts as its plain text does (the Python-3 reference raises TypeError on it)"""
    C.use_brute(monkeypatch)
    data, want = C.golden_case("h_basic")
    plain = _write(tmp_path / "a_allValidPairs", data)
    gz = str(tmp_path / "b_allValidPairs.gz")
    with gzip.open(gz, "wb") as fh:
        fh.write(data)
    for f in (plain, gz):
        out = str(tmp_path / "o.bedpe.gz")
        assert convert.pairs2bedpe(f, out, ext=50) == (want.count(b"\n"), len(want))
        assert _read_out(out) == want


def _cases():
    meta = C.golden_meta()
    for g in meta["cases"]:
        data, want = C.golden_case(g["name"])
        yield g, data, want


@pytest.mark.parametrize("budget", [None, 1, 2])                      # None: the default; 1, 2: the longest line (+ 1)
def test_pipeline_on_goldens(tmp_path, monkeypatch, budget):
    C.use_brute(monkeypatch)
    for g, data, want in _cases():
        b = convert.BUDGET if budget is None else max(len(l) + 1 for l in C.split_lines(data) or [b""]) + budget - 1
        f = _write(tmp_path / "in.txt", data)
        out = str(tmp_path / ("o.bedpe.gz" if g["format"] == "hicpro" else "o.bedpe"))
        fn = convert.pairs2bedpe if g["format"] == "hicpro" else convert.long2bedpe
        kw = {"ext": g["ext"], "budget": b}
        if g["error"] is None:
            assert fn(f, out, **kw) == (g["lines"], len(want)), g["name"]
        else:
            with pytest.raises(ValueError) as ei:
                fn(f, out, **kw)
            assert str(ei.value).startswith("%s:%d: " % (f, g["lines"] + 1)), (g["name"], str(ei.value))
        assert _read_out(out) == want, (g["name"], b)


def test_chunks_carry_and_boundaries(tmp_path, monkeypatch):
    """every chunk but the last ends at a newline; the tail goes in front of the next; CRLF split across chunks; a line exactly
    filling a chunk; no final newline; an empty file; a file of only '\\n'"""
    C.use_brute(monkeypatch)
    line = b"r\tc\t10\t+\tc\t20\t-\r\n"
    data = line * 7 + b"r\tc\t10\t+\tc\t20\t-"
    f = _write(tmp_path / "in", data)
    want = C.brute("hicpro", data, 50)[0]
    for budget in range(len(line), 4 * len(line) + 3):
        C.BruteSeam.chunks = []
        out = str(tmp_path / "o.gz")
        assert convert.pairs2bedpe(f, out, budget=budget) == (8, len(want))
        assert _read_out(out) == want
        assert sum(n for _, n, _ in C.BruteSeam.chunks) == len(data)
        assert [k for k, _, _ in C.BruteSeam.chunks] == list(range(len(C.BruteSeam.chunks)))
        assert [last for _, _, last in C.BruteSeam.chunks][-1] is True
    # a line one byte longer than the budget
    with pytest.raises(ValueError, match=r":1: line longer than the chunk budget"):
        convert.pairs2bedpe(f, str(tmp_path / "o.gz"), budget=len(line) - 1)
    jl = b"0 c 10 0 16 c 20\n"
    f2 = _write(tmp_path / "in2", jl * 3 + b"x" * 200 + b"\n" + jl)
    with pytest.raises(ValueError, match=r":4: line longer than the chunk budget"):
        convert.long2bedpe(f2, str(tmp_path / "o2"), budget=100)
    assert _read_out(str(tmp_path / "o2")) == C.brute("juicer", jl * 3, 75)[0]
    # empty file, a file of only '\n'
    e = _write(tmp_path / "empty", b"")
    assert convert.pairs2bedpe(e, str(tmp_path / "e.gz")) == (0, 0)
    assert _read_out(str(tmp_path / "e.gz")) == b""
    assert convert.long2bedpe(e, str(tmp_path / "e.txt")) == (0, 0)
    nl = _write(tmp_path / "nl", b"\n")
    with pytest.raises(ValueError, match=r":1: fewer than 7 fields"):
        convert.pairs2bedpe(nl, str(tmp_path / "nl.gz"))
    assert _read_out(str(tmp_path / "nl.gz")) == b""


def test_gzip_members_order_and_prefix(tmp_path, monkeypatch):
    """many chunks through the member pool: the members are in chunk order and each is a complete gzip member; on an error the
    file is a complete gzip file of exactly the lines in front of it"""
    C.use_brute(monkeypatch)
    monkeypatch.setattr(convert, "MEMBER", 4096)
    data = C.gen_hicpro(20000, 3)
    f = _write(tmp_path / "x_allValidPairs", data)
    want = C.brute("hicpro", data, 50)[0]
    out = str(tmp_path / "x.bedpe.gz")
    for threads in (1, 3, 16):
        assert convert.pairs2bedpe(f, out, threads=threads, budget=50000) == (20000, len(want))
        raw = open(out, "rb").read()
        assert gzip.decompress(raw) == want
        assert raw.count(b"\x1f\x8b\x08") >= len(want) // 4096
    with pytest.raises(ValueError):
        convert.pairs2bedpe(f, out, threads=17)
    with pytest.raises(ValueError):
        convert.pairs2bedpe(f, out, threads=0)
    lines = data.split(b"\n")
    lines[12345] = b"bad"
    f = _write(tmp_path / "y_allValidPairs", b"\n".join(lines))
    with pytest.raises(ValueError, match=r"y_allValidPairs:12346: fewer than 7 fields"):
        convert.pairs2bedpe(f, out, budget=30000, threads=4)
    assert gzip.decompress(open(out, "rb").read()) == C.brute("hicpro", b"\n".join(lines[:12345]) + b"\n", 50)[0]


def test_command_lines(tmp_path, monkeypatch, capsys):
    C.use_brute(monkeypatch)
    data, want = C.golden_case("h_basic")
    d = tmp_path / "hp"
    (d / "s1").mkdir(parents=True)
    (d / "s2").mkdir()
    for p in ("b_allValidPairs", "a_allValidPairs", "s2/d_allValidPairs", "s1/c_allValidPairs", "e.txt"):
        _write(d / p, data)
    with gzip.open(str(d / "z_allValidPairs.gz"), "wb") as fh:
        fh.write(data)
    assert convert.hicpro_inputs([str(d)]) == [str(d / p) for p in ("a_allValidPairs", "b_allValidPairs", "z_allValidPairs.gz",
                                                                     "s1/c_allValidPairs", "s2/d_allValidPairs")]
    assert convert.bedpe_name("/x/y/s_allValidPairs.gz", "/o") == "/o/s.bedpe.gz"
    assert convert.bedpe_name("/x/y/s_allValidPairs") == "/x/y/s.bedpe.gz"
    assert convert.bedpe_name("/x/y/s.pairs") == "/x/y/s.pairs.bedpe.gz"
    o = tmp_path / "out" / "deep"
    assert convert.main(["hicpro", str(d), str(d / "e.txt"), str(tmp_path / "missing"), "-o", str(o), "-p", "2"]) == 0
    assert "Warning: %s not exist, skipping" % (tmp_path / "missing") in capsys.readouterr().err
    assert sorted(os.listdir(str(o))) == ["a.bedpe.gz", "b.bedpe.gz", "c.bedpe.gz", "d.bedpe.gz", "e.txt.bedpe.gz", "z.bedpe.gz"]
    for n in os.listdir(str(o)):
        assert _read_out(str(o / n)) == want
    # without -o the outputs go next to the inputs; -o naming an existing file
    assert convert.main(["hicpro", str(d / "a_allValidPairs")]) == 0
    assert _read_out(str(d / "a.bedpe.gz")) == want
    assert convert.main(["hicpro", str(d / "a_allValidPairs"), "-o", str(d / "e.txt")]) == 1
    assert "Error: file %s exists, unable to create output folder" % (d / "e.txt") in capsys.readouterr().err
    with pytest.raises(SystemExit):
        convert.main(["hicpro", str(d), "-p", "17"])
    # -ext
    dn, wn = C.golden_case("h_extneg")
    fn = _write(tmp_path / "n_allValidPairs", dn)
    assert convert.main(["hicpro", fn, "-ext", "-7"]) == 0
    assert _read_out(str(tmp_path / "n.bedpe.gz")) == wn
    # juicer: -i and -o required; a missing input; an existing output is reported and overwritten; an error exits 1
    jd, jw = C.golden_case("j_basic")
    fi = _write(tmp_path / "m.txt", jd)
    fo = str(tmp_path / "m.bedpe")
    assert convert.main(["juicer", "-i", fi, "-o", fo]) == 0
    assert _read_out(fo) == jw
    _write(fo, b"old")
    assert convert.main(["juicer", "-i", fi, "-o", fo]) == 0
    assert "Error: output file %s exists!" % fo in capsys.readouterr().err
    assert _read_out(fo) == jw
    assert convert.main(["juicer", "-i", str(tmp_path / "nope"), "-o", fo]) == 1
    assert "Error: input file %s not exists!" % (tmp_path / "nope") in capsys.readouterr().err
    with pytest.raises(SystemExit):
        convert.main(["juicer", "-o", fo])
    ed, ew = C.golden_case("j_errint")
    fe = _write(tmp_path / "err.txt", ed)
    assert convert.main(["juicer", "-i", fe, "-o", fo]) == 1
    assert "err.txt:7: not an integer" in capsys.readouterr().err
    assert _read_out(fo) == ew
