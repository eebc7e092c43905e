"""CPU: the BEDPE reader's host pipeline (cloops_amd.ingest) on the brute-force seam of tests/ingest_cases.py, and the two
yardsticks tied together: cloops_amd.io.parse_bedpe reproduces what the reference's own parsers returned on the corner corpus and
the seeded synthetic (tests/golden/make_golden_ingest.py)."""
import collections
import gzip
import hashlib
import os

import numpy as np
import pytest

import ingest_cases as C
from cloops_amd import ingest, pipe
from cloops_amd import io as cio

CORPUS = C.corpus()


def test_corpus_did_not_drift():
    g = C.golden()
    for name, files, _ in CORPUS:
        assert g["inputs"][name] == hashlib.sha1(b"\x00".join(files)).hexdigest(), name
    assert g["inputs"]["synth200k"] == hashlib.sha1(C.synth_bedpe(200000)).hexdigest()


def test_host_parser_reproduces_the_reference(tmp_path):
    """cio.parse_bedpe against the reference's parseRawBedpe2 / parseRawBedpe: every case and argument set the reference returned
    on and cio does not raise on (cio builds int64 arrays: a 20-digit coordinate is its OverflowError)"""
    g = C.golden()
    todo = [(name, C.write_case(tmp_path, name, files)) for name, files, _ in CORPUS] + [("synth200k", C.write_synth(tmp_path, 200000))]
    checked = 0
    for name, fs in todo:
        for cs, cut, unique in C.ARGSETS:
            r = C.run(cio.parse_bedpe, fs, cs, cut, unique)
            if r[0] == "ok":
                checked += C.check_against_golden(g, name, cs, cut, unique, r[1], r[4])
            elif r[1] is UnicodeDecodeError:
                assert g["cases"][name][C.argkey(cs, cut, unique)] == {"raises": "UnicodeDecodeError"}
    assert checked >= 200


@pytest.mark.parametrize("name,files,exotic", CORPUS, ids=[c[0] for c in CORPUS])
def test_pipeline_equals_host_parser(tmp_path, monkeypatch, name, files, exotic):
    """every case x argument set x chunk budget: the triple and the distances of cio.parse_bedpe; the host is asked exactly for the
    exotic cases"""
    C.use_brute(monkeypatch)
    fs = C.write_case(tmp_path, name, files)
    g = C.golden()
    for cs, cut, unique in C.ARGSETS:
        want = C.run(cio.parse_bedpe, fs, cs, cut, unique)
        for b in C.budgets(files):
            stats = {}
            kw = {"stats": stats} if b is None else {"stats": stats, "budget": b}
            got = C.run(ingest.parse_bedpe_gpu, fs, cs, cut, unique, **kw)
            C.assert_same(got, want, (name, cs, cut, unique, b))
            if got[0] == "ok":
                C.check_against_golden(g, name, cs, cut, unique, got[1], got[4])
            small = b is not None and b < C.longest_line(files) + (0 if all(f.endswith(b"\n") or not f for f in files) else 1)
            if exotic:
                assert stats["fallback"] is not None and stats["fallback"][1] in fs, (name, b)
            elif not small:
                assert stats["fallback"] is None, (name, b, stats["fallback"])


def test_chunk_cuts_at_every_offset(tmp_path, monkeypatch):
    """a small input of three files (CRLF, no final newline, duplicates across files): every budget from the longest line to the whole
    input gives the same result; the chunks cover every byte once and are cut at every file end"""
    C.use_brute(monkeypatch)
    a = C._t(C.LINES, "\r\n")
    b = C._t(C.GOOD + [C.pet("chr3", 5, 6, 900, 1000, "-", "+")], final=False)
    c = C._t(list(reversed(C.LINES)) + C.GOOD)
    fs = C.write_case(tmp_path, "cuts", [a, b, c])
    lo = C.longest_line([a, b, c])
    for unique in (False, True):
        want = C.run(cio.parse_bedpe, fs, (), 0, unique)
        assert list(want[1].keys()) == ["chr1", "chr2", "chr3"]
        for budget in range(lo, len(a) + len(b) + len(c) + 2):
            C.BruteSeam.chunks = []
            stats = {}
            got = C.run(ingest.parse_bedpe_gpu, fs, (), 0, unique, budget=budget, stats=stats)
            C.assert_same(got, want, budget)
            assert stats["fallback"] is None
            assert sum(n for _, n, _ in C.BruteSeam.chunks) == len(a) + len(b) + len(c)
            assert sum(1 for _, _, last in C.BruteSeam.chunks if last) == 3
            assert all(n <= budget for _, n, _ in C.BruteSeam.chunks)


def test_dictionary_order_and_wanted_chromosomes(tmp_path, monkeypatch):
    """ids go to names in the order of their first KEPT line, over chunks and files; an unwanted name gets none"""
    C.use_brute(monkeypatch)
    one = C._t([C.pet("chrB", 1, 2, 3, 4, c2="chrA"), C.pet("chrB", 1, 2, 10, 11), C.pet("chrC", 1, 2, 900, 1000), C.pet("chrA", 1, 2, 900, 1000)])
    two = C._t([C.pet("chrB", 1, 2, 900, 1000), C.pet("chrD", 1, 2, 900, 1000), C.pet("chrC", 5, 6, 900, 1000)])
    fs = C.write_case(tmp_path, "order", [one, two])
    for budget in (C.longest_line([one, two]), 4096):
        mats, n_lines, n_cis = ingest.parse_bedpe_gpu(fs, cut=100, budget=budget)
        assert list(mats.keys()) == ["chrC", "chrA", "chrB", "chrD"] and (n_lines, n_cis) == (7, 5)
        mats, _, n_cis = ingest.parse_bedpe_gpu(fs, cs=["chrD", "chrB"], budget=budget)
        assert list(mats.keys()) == ["chrB", "chrD"] and n_cis == 3
        assert mats["chrB"].tolist() == [[0, 1, 10], [1, 1, 950]]


def test_two_names_under_one_hash_never_merge(tmp_path, monkeypatch):
    """a hash is not proof: with every name under one hash the read goes to the host, within a chunk (the commit's byte compare) and
    across chunks (the dictionary)"""
    C.use_brute(monkeypatch, hash=lambda name: 7)
    files = [C._t(C.GOOD)]
    fs = C.write_case(tmp_path, "hash", files)
    want = C.run(cio.parse_bedpe, fs, (), 0, True)
    for budget in (C.longest_line(files), 4096):
        stats = {}
        C.assert_same(C.run(ingest.parse_bedpe_gpu, fs, (), 0, True, budget=budget, stats=stats), want, budget)
        assert stats["fallback"][0] == "two chromosome names under one hash"
    stats = {}
    one = C.write_case(tmp_path, "hash1", [C._t(C.GOOD[:1] * 3)])
    C.assert_same(C.run(ingest.parse_bedpe_gpu, one, (), 0, False, stats=stats), C.run(cio.parse_bedpe, one, (), 0, False), "one name")
    assert stats["fallback"] is None


def test_fallback_is_said_once_and_raises_what_the_host_raises(tmp_path, monkeypatch, capsys):
    C.use_brute(monkeypatch)
    by_name = {c[0]: c for c in CORPUS}
    fs = C.write_case(tmp_path, "u", by_name["invalid_utf8"][1])
    with pytest.raises(UnicodeDecodeError):
        ingest.parse_bedpe_gpu(fs)
    assert capsys.readouterr().err.count("reading on the host") == 1
    fs = C.write_case(tmp_path, "o", by_name["twenty_digits"][1])
    with pytest.raises(OverflowError):
        ingest.parse_bedpe_gpu(fs)
    fs = C.write_case(tmp_path, "s", by_name["underscore"][1])
    stats, said = {}, []

    class Log(object):
        def info(self, m):
            said.append(m)
    mats, n_lines, n_cis = ingest.parse_bedpe_gpu(fs, stats=stats, logger=Log())
    assert (n_lines, n_cis) == (4, 4) and mats["chr1"][-1].tolist() == [2, 150, 5050]
    assert stats["fallback"][1:] == (fs[0], 4) and len(said) == 1 and "%s:4:" % fs[0] in said[0]
    # too many names in a chunk, a line longer than the budget
    monkeypatch.setattr(C.BruteSeam, "names_max", 1)
    fs = C.write_case(tmp_path, "n", [C._t(C.GOOD)])
    stats = {}
    assert list(ingest.parse_bedpe_gpu(fs, stats=stats)[0].keys()) == ["chr1", "chr2"]
    assert stats["fallback"][0].startswith("more than 65536")
    stats = {}
    ingest.parse_bedpe_gpu(fs, budget=C.longest_line([C._t(C.GOOD)]) - 1, stats=stats)
    assert stats["fallback"][0] == "a line longer than the chunk budget"
    capsys.readouterr()


def test_jd_protocol(tmp_path, monkeypatch):
    """parseRawBedpe2 / parseRawBedpe write the files of cloops_amd.io's, byte for byte, plain and gzipped input"""
    C.use_brute(monkeypatch)
    data = C._t(C.LINES + C.GOOD + C.LINES)
    plain = C.write_case(tmp_path, "jd", [data])[0]
    gz = str(tmp_path / "jd.bedpe.gz")
    with gzip.open(gz, "wb") as fh:
        fh.write(data)
    for k, fs in enumerate(([plain], [gz, plain])):
        dirs = [str(tmp_path / ("%s%d" % (w, k))) for w in ("h2", "g2", "h1", "g1")]
        for d in dirs:
            os.mkdir(d)
        h2, g2 = cio.parseRawBedpe2(fs, dirs[0], [], 0), ingest.parseRawBedpe2(fs, dirs[1], [], 0)
        (h1, hd), (g1, gd) = cio.parseRawBedpe(fs, dirs[2], ["chr1"], 100), ingest.parseRawBedpe(fs, dirs[3], ["chr1"], 100)
        assert hd == gd and len(hd) > 0
        for h, g in ((h2, g2), (h1, g1)):
            assert [os.path.basename(f) for f in h] == [os.path.basename(f) for f in g] and len(h) > 0
            for a, b in zip(h, g):
                with open(a, "rb") as fa, open(b, "rb") as fb:
                    assert fa.read() == fb.read()


def test_command_line(tmp_path, monkeypatch, capsys):
    C.use_brute(monkeypatch)
    a, b = C.write_case(tmp_path, "cl", [C._t(C.LINES), C._t(C.GOOD)])
    op = ingest._help(["-f", a + "," + b, "-o", "x", "-c", "chr1,chr2", "-cut", "5"])
    assert (op.fnIn, op.fnOut, op.chroms, op.cut) == (a + "," + b, "x", "chr1,chr2", 5)
    out = str(tmp_path / "out")
    assert ingest.main(["-f", a + "," + b, "-o", out, "-c", "chr1", "-cut", "200"]) == 0
    assert sorted(os.listdir(out)) == ["chr1-chr1.jd"]
    key, mat = pipe.parseJd(os.path.join(out, "chr1-chr1.jd"))
    want, _, _ = cio.parse_bedpe([a, b], ["chr1"], 200)
    assert key == ("chr1", "chr1") and np.array_equal(mat, want["chr1"])
    assert ingest.main(["-f", a, "-o", out]) == 1                        # the directory exists
    assert ingest.main(["-f", a + ".missing", "-o", out + "2"]) == 1
    capsys.readouterr()
    with pytest.raises(ValueError, match="reader must be"):
        pipe.pipe([a], str(tmp_path / "p"), [500], [5], reader="disk")
    assert not os.path.exists(str(tmp_path / "p"))


def test_brute_integer_classes():
    """the device's classes: (a) value, (b) skipped, (c) exotic -- and Python's int() agrees on (a) and (b)"""
    for s, want in ((b"0", 0), (b"+100", 100), (b"-300", -300), (b"00012", 12), (b"-0", 0), (b"4611686018427387903", (1 << 62) - 1)):
        assert C.brute_int(s) == ("int", want) and int(s.decode()) == want
    for s in (b"x", b"1e5", b"1.5", b"0x10", b"+", b"-", b"", b"+-1", b"1-", b"12a"):
        assert C.brute_int(s) == ("skip",)
        with pytest.raises(ValueError):
            int(s.decode())
    for s in (b"1_00", b" 100 ", b"100\x0b", b"100\x1c", b"4611686018427387904", b"-4611686018427387904", b"99999999999999999999", b"1\xd9\xa1",
              b"1\x00", b"\x7f"):
        assert C.brute_int(s) == ("exotic",)
