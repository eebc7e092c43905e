"""CPU: the host side of the coverage tracks (cloops_amd.coverage): the command line's arguments, the ends / norm mapping, which
chromosomes are taken and in which order, the fixed-point formatter against `decimal`, the text twin of the device render, the json
layout, and the error without the library.  No GPU, no built library."""
import decimal
import os

import numpy as np
import pytest

from cloops_amd import coverage


def test_argument_parsing():
    op = coverage.help(["-d", "jd", "-o", "out"])
    assert (op.d, op.output, op.ext, op.res, op.cut, op.ends, op.norm, op.chroms) == ("jd", "out", 75, 0, 0, "both", "none", "")
    op = coverage.help(["-d", "jd", "-o", "out", "-ext", "40", "-res", "1000", "-cut", "4601", "-ends", "left", "-norm", "cpm", "-c", "chr1,chr2"])
    assert (op.ext, op.res, op.cut, op.ends, op.norm, op.chroms) == (40, 1000, 4601, "left", "cpm", "chr1,chr2")
    for bad in (["-o", "out"], ["-d", "jd"], ["-d", "jd", "-o", "out", "-ends", "up"], ["-d", "jd", "-o", "out", "-norm", "rpkm"],
                ["-d", "jd", "-o", "out", "-ext", "x"]):
        with pytest.raises(SystemExit):
            coverage.help(bad)


def test_main_command_flags():
    """-bdg / -bdgext of the main command reach pipe() (-ext keeps its own meaning there)"""
    from cloops_amd import pipe
    seen = {}

    def fake(fs, fout, eps, minPts, *a, **kw):
        seen.update(kw)

    orig, pipe.pipe = pipe.pipe, fake
    try:
        assert pipe.main(["-f", "a.bedpe", "-o", "o", "-m", "1", "-bdg", "-bdgext", "60", "-ext", "30"]) == 0
        assert (seen["bdg"], seen["bdg_ext"], seen["ext"]) == (True, 60, 30)
        assert pipe.main(["-f", "a.bedpe", "-o", "o", "-m", "1"]) == 0
        assert (seen["bdg"], seen["bdg_ext"]) == (False, 75)
    finally:
        pipe.pipe = orig


def test_ends_and_norm_mapping():
    assert [coverage.ends_code(e) for e in ("left", "right", "both", 1, 2, 3)] == [1, 2, 3, 1, 2, 3]
    for bad in ("x", 0, 4, None, True):
        with pytest.raises(ValueError):
            coverage.ends_code(bad)
    assert coverage.scale_of("none", 12345) is None
    assert coverage.scale_of("cpm", 12345) == (10 ** 9, 12345)
    assert coverage.scale_of("cpm", 0) is None                          # nothing to scale
    assert coverage.CPM_NUM <= 1 << 30                                   # what cl_cov_text takes
    with pytest.raises(ValueError):
        coverage.scale_of("rpkm", 5)


def test_chromosome_order_and_selection(tmp_path):
    d = str(tmp_path)
    for name in ("chr2-chr2.jd", "chr10-chr10.jd", "chrX-chrX.jd", "chr1-chr2.jd", "chr1.jd", "chr3-chr3.txt", "a-b-c.jd"):
        open(os.path.join(d, name), "w").close()
    got = coverage.chrom_files(d)
    assert [c for c, _ in got] == ["chr10", "chr2", "chrX"]              # plain string order, cis files only
    assert [os.path.basename(f) for _, f in got] == ["chr10-chr10.jd", "chr2-chr2.jd", "chrX-chrX.jd"]
    assert [c for c, _ in coverage.chrom_files(d, {"chrX", "chr2", "chr7"})] == ["chr2", "chrX"]
    assert coverage.chrom_files(d, ["chr7"]) == []
    files = [os.path.join(d, n) for n in ("chrX-chrX.jd", "chr1-chr2.jd", "chr10-chr10.jd")]
    assert [c for c, _ in coverage.chrom_files(files)] == ["chr10", "chrX"]
    with pytest.raises(ValueError):
        coverage.chrom_files(os.path.join(d, "nothing_here"))


def test_fixed_point_against_decimal():
    rng = np.random.default_rng(20)
    cases = [(1, 1, 2), (3, 1, 2), (1, 1000, 3), (0, 5, 7), (1, 10 ** 9, 199348), (326, 10 ** 9, 199348), (2 ** 32 - 1, 2 ** 30, 1), (1, 1, 2001), (1, 1, 2000),
             (9, 1, 1000), (10, 1, 1), (999, 1, 1)]
    cases += [(int(d), int(n), int(m)) for d, n, m in zip(rng.integers(0, 1 << 32, 3000), rng.integers(1, (1 << 30) + 1, 3000), rng.integers(1, 1 << 40, 3000))]
    cases += [(int(d), 10 ** 9, int(m)) for d, m in zip(rng.integers(0, 100000, 1500), rng.integers(1, 10 ** 9, 1500))]
    cases += [(int(d), int(n), 2 * int(h)) for d, n, h in zip(rng.integers(0, 1000, 500), rng.integers(1, 50, 500), rng.integers(1, 20, 500))]     # many exact halves
    halves = 0
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        for d, n, m in cases:
            exact = decimal.Decimal(d) * n / m                            # thousandths
            want = exact.quantize(decimal.Decimal(1), rounding=decimal.ROUND_HALF_UP)
            halves += (d * n) % m * 2 == m
            got = coverage.fixed_point(d, n, m)
            whole, frac = got.split(".")
            assert len(frac) == 3 and int(whole) * 1000 + int(frac) == int(want), (d, n, m, got)
            assert whole == str(int(whole))                               # no sign, no padding
    assert halves > 20
    assert coverage.fixed_point(1, 1, 2) == "0.001" and coverage.fixed_point(0, 5, 7) == "0.000" and coverage.fixed_point(10, 1000, 3) == "3.333"
    assert coverage.fixed_point(5, 1000, 1) == "5.000" and coverage.fixed_point(1234567, 1000, 1000) == "1234.567"


def test_format_runs():
    s, e, d = np.array([0, 150, 2000]), np.array([150, 160, 2150]), np.array([1, 12, 100000], np.uint32)
    assert coverage.format_runs("chr1", s, e, d) == b"chr1\t0\t150\t1\nchr1\t150\t160\t12\nchr1\t2000\t2150\t100000\n"
    assert coverage.format_runs("c", s, e, d, (10 ** 9, 4000000)) == b"c\t0\t150\t0.250\nc\t150\t160\t3.000\nc\t2000\t2150\t25000.000\n"
    assert coverage.format_runs("c", [], [], []) == b""


def test_json_layout():
    stats = {"chr2": {"n_runs": 3, "max_depth": 7, "n_ends": 10, "area": 1500}, "chr10": {"n_runs": 5, "max_depth": 4, "n_ends": 20, "area": 3000}}
    js = coverage.summary_of(stats, 75, 0, 0, "both", "cpm")
    assert js == {"ext": 75, "res": 0, "cut": 0, "ends": 3, "norm": "cpm", "chroms": stats,
                  "total": {"n_runs": 8, "max_depth": 7, "n_ends": 30, "area": 4500}}
    assert coverage.summary_of({}, 40, 1000, 5, "left", "none")["total"] == {"n_runs": 0, "max_depth": 0, "n_ends": 0, "area": 0}
    assert tuple(coverage.STAT_KEYS) == ("n_runs", "max_depth", "n_ends", "area")


def test_without_the_library(tmp_path, monkeypatch):
    """no CPU fallback: without libcloops_hip.so jd2bedgraph raises the package's ImportError, as the other modules do"""
    import joblib
    from cloops_amd import _lib, pipe
    d = os.path.join(str(tmp_path), "jd")
    os.makedirs(d)
    joblib.dump(np.array([[0, 100, 900], [1, 200, 5000]], np.int64), os.path.join(d, "chr1-chr1.jd"))
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SO_PATH", "/nonexistent/libcloops_hip.so")
    pipe.CACHE.clear()
    for norm in coverage.NORMS:
        with pytest.raises(ImportError):
            coverage.jd2bedgraph(d, os.path.join(str(tmp_path), "out_" + norm), norm=norm)
    for bad in (dict(ends="up"), dict(norm="rpkm"), dict(ext=0), dict(res=-1)):      # refused before anything is loaded
        with pytest.raises(ValueError):
            coverage.jd2bedgraph(d, os.path.join(str(tmp_path), "bad"), **bad)
    pipe.CACHE.clear()
