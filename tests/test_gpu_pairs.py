"""GPU: 4DN pairs files through kernels K15 (CL_CONV_PAIRS) and K18 (cl_ingest_set_format(CL_INGEST_PAIRS)): the converter's bytes
and the reader's full result (rows, key order, n_lines, n_cis, distances) against the oracle of tests/pairs_cases.py -- the corner
corpus, the error cases, seeded synthetic files around the 256-line tile under budgets of one, two and many chunks, a line wider
than the staged tile, every argument set, and a whole `pipe()` run on a pairs file against the same run on its converted BEDPE."""
import gzip
import os

import numpy as np
import pytest

import convert_cases as CC
import golden_util as G
import ingest_cases as IC
import pairs_cases as P

pytestmark = pytest.mark.gpu

CORPUS = P.corpus()
ERRORS = P.error_cases()
SIZES = (1, 255, 256, 257, 513, 20000)


def _read_out(path):
    with open(path, "rb") as fh:
        raw = fh.read()
    return gzip.decompress(raw) if str(path).endswith(".gz") else raw


def _convert_equals(pairs, f, data, ext, out, budget):
    want = P.convert(data, ext)[0]
    kw = {} if budget is None else {"budget": budget}
    assert pairs.pairs2bedpe(f, out, ext=ext, **kw) == (want.count(b"\n"), len(want)), (f, ext, budget)
    assert _read_out(out) == want, (f, ext, budget)


@pytest.mark.parametrize("name,files,exts,exotic", CORPUS, ids=[c[0] for c in CORPUS])
def test_corpus(tmp_path, name, files, exts, exotic):
    """converter bytes and reader result equal the oracle; the device decides every case that is not exotic"""
    from cloops_amd import pairs
    fs = P.write_case(tmp_path, name, files)
    m = IC.longest_line(files)
    for ext in exts:
        for b in (max(4096, m + 1), m + 1):
            _convert_equals(pairs, fs[0], files[0], ext, str(tmp_path / "o.bedpe"), b)
        for cs, cut, unique in (((), 0, False), (("chr1",), 200, True)):
            want = P.read(tmp_path, files, ext, cs, cut, unique)
            for b in (None, m + 1, 2 * m + 1):
                stats = {}
                kw = {"stats": stats} if b is None else {"stats": stats, "budget": b}
                got = P.run(pairs.parse_pairs_gpu, fs, ext, cs, cut, unique, **kw)
                P.assert_same(got, want, (name, ext, cs, cut, unique, b))
                assert (stats["fallback"] is not None) == exotic, (name, ext, b, stats["fallback"])


@pytest.mark.parametrize("name,files,ext,err", ERRORS, ids=[c[0] for c in ERRORS])
def test_error_cases(tmp_path, name, files, ext, err):
    """the converter raises at the right line after exactly the lines in front of it; the reader raises the same ValueError"""
    from cloops_amd import pairs
    fs = P.write_case(tmp_path, name, files)
    k, line, reason = err
    for b in (None, IC.longest_line(files) + 1):
        kw = {} if b is None else {"budget": b}
        assert P.run(pairs.parse_pairs_gpu, fs, ext, (), 0, True, **kw) == ("error",) + err, b
        out = str(tmp_path / "o.bedpe")
        if os.path.exists(out):
            os.remove(out)
        with pytest.raises(ValueError) as ei:
            pairs.pairs2bedpe(fs[k], out, ext=ext, **kw)
        assert str(ei.value).startswith("%s:%d: %s" % (fs[k], line, reason)), str(ei.value)
        if reason == "columns":
            assert not os.path.exists(out)
        else:
            assert _read_out(out) == P.convert(files[k], ext)[0]


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """n -> (path, bytes, oracle of ((), 0, True) at ext 50): made once"""
    d = tmp_path_factory.mktemp("synth")
    out = {}
    for n in SIZES:
        data = P.gen_pairs(n)
        f = P.write_case(d, "s%d" % n, [data])[0]
        out[n] = (f, data, P.read(d, [data], 50, (), 0, True))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_synthetic_sizes_and_chunks(synth, tmp_path, n):
    """1, 255, 256, 257, 513 and 20 000 data lines under budgets of one, two and many chunks"""
    from cloops_amd import pairs
    f, data, want = synth[n]
    assert want[0] == "ok" and want[2] == n
    m = IC.longest_line([data])
    for b in (None, max(m, len(data) // 2 + m), max(m, len(data) // 9)):
        stats = {}
        kw = {"stats": stats} if b is None else {"stats": stats, "budget": b}
        P.assert_same(P.run(pairs.parse_pairs_gpu, [f], 50, (), 0, True, **kw), want, (n, b))
        assert stats["fallback"] is None, (n, b, stats["fallback"])
        _convert_equals(pairs, f, data, 50, str(tmp_path / "o.bedpe"), b)
    _convert_equals(pairs, f, data, 50, str(tmp_path / "o.bedpe.gz"), None)


def test_every_argument_set(synth, tmp_path):
    """cs x cut x unique with and without the distances on the 20 000-line file, plain and gzipped"""
    from cloops_amd import pairs
    f, data, _ = synth[20000]
    gz = P.write_case(tmp_path, "z", [data], gz=(0,))[0]
    for cs, cut, unique in P.ARGSETS:
        want = P.read(tmp_path, [data], 50, cs, cut, unique)
        stats = {}
        P.assert_same(P.run(pairs.parse_pairs_gpu, [f if unique else gz], 50, cs, cut, unique, stats=stats), want, (cs, cut, unique))
        assert stats["fallback"] is None
        mats, n_lines, n_cis = pairs.parse_pairs_gpu([f], cs, cut, unique, None, ext=50)         # no distances asked
        assert (n_lines, n_cis) == want[2:4] and all(np.array_equal(mats[c], want[1][c]) for c in want[1])


def test_line_wider_than_the_staged_tile(tmp_path):
    """one line of more than 40 KiB: its tile is read from global memory"""
    from cloops_amd import pairs
    lines = P.HEAD + P.GOOD + [P.pair("chr1", 777, "chr1", 99000, "-", "+", extra=("UU", "x" * 45000))] + P.GOOD * 100
    data = P._t(lines)
    f = P.write_case(tmp_path, "wide", [data])[0]
    want = P.read(tmp_path, [data], 50, (), 0, False)
    stats = {}
    P.assert_same(P.run(pairs.parse_pairs_gpu, [f], 50, (), 0, False, stats=stats), want, "wide")
    assert stats["fallback"] is None and want[2] == 304
    _convert_equals(pairs, f, data, 50, str(tmp_path / "o.bedpe"), None)


def test_load_pairs_leaves_the_chromosomes_in_hbm(synth):
    from cloops_amd import pairs, pipe
    f, data, _ = synth[20000]
    want = P.read(os.path.dirname(f), [data], 50, (), 0, False)
    stats = {}
    names = pairs.load_pairs([f], prefix="pp", stats=stats)
    try:
        assert names == ["mem://pp/%s-%s" % (c, c) for c in want[1]] and stats["fallback"] is None
        assert (stats["lines"], stats["cis"]) == want[2:4]
        for nm, c in zip(names, want[1]):
            r = pipe.CACHE.get(nm)
            assert np.array_equal(r.X, want[1][c][:, 1]) and np.array_equal(r.Y, want[1][c][:, 2])
            assert len(r.chrom.neighbor_counts(1000)) == len(r.X)
    finally:
        for nm in names:
            pipe.CACHE.drop(nm)


def test_pipe_on_pairs_equals_pipe_on_its_bedpe(tmp_path):
    """the chr21 mid-points written as a pairs file: `pipe()` on it (format found by its first line) writes the `.loop` that `pipe()`
    writes on the BEDPE pairs2bedpe makes of it"""
    from cloops_amd import pairs, pipe
    X, Y = G.chr21_xy()
    k = np.arange(len(X))
    body = CC._text([b"r", k, b"\tchr21\t", X, b"\tchr21\t", Y, b"\t+\t-\tUU\n"], len(X))
    f = P.write_case(tmp_path, "chr21", [P._t(P.HEAD) + body], gz=(0,))[0]
    bed = pairs.bedpe_name(f)
    assert pairs.pairs2bedpe(f, bed, ext=0)[0] == len(X)
    eps, minPts = pipe.MODES[1][:2]
    pipe.pipe([f], str(tmp_path / "from_pairs"), eps, minPts, ext=0)
    pipe.pipe([bed], str(tmp_path / "from_bedpe"), eps, minPts)
    with open(str(tmp_path / "from_pairs.loop"), "rb") as fa, open(str(tmp_path / "from_bedpe.loop"), "rb") as fb:
        a, b = fa.read(), fb.read()
    assert a == b and a.count(b"\n") > 10
