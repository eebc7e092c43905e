"""CPU: the host side of cloops_amd.matrix -- regions and their bins, the three texts byte for byte on a hand-written example through
the oracle's stand-in chromosome, the suffixes, the command lines, the cpm scale, and that a refused argument writes nothing."""
import json
import os
import threading

import numpy as np
import pytest

import matrix_cases as MC
from cloops_amd import matrix


class Record(object):
    def __init__(self, X, Y):
        self.chrom, self.lock = MC.OracleChrom(X, Y), threading.Lock()


@pytest.fixture
def standin(monkeypatch):
    """matrix._records served by stand-in chromosomes: chr1 = the twelve rows, chr2 = 300 scattered ones"""
    recs = {"chr1": Record(*MC.twelve()), "chr2": Record(*MC.scattered(1, 300, 5000, 900, both=True))}
    monkeypatch.setattr(matrix, "_records", lambda jd, chroms=(): [(n, recs[n]) for n in sorted(recs) if len(chroms) == 0 or n in chroms])
    return recs


def _read(prefix, suffixes):
    out = {}
    for s in suffixes:
        with open(prefix + s) as fh:
            out[s] = fh.read()
    return out


# ---- the oracle on the hand-written rows ---------------------------------------------------------------------------
W5 = np.array([[1, 1, 0, 0, 2], [0, 1, 0, 2, 0], [0, 0, 1, 0, 1], [0, 0, 0, 1, 1], [0, 1, 0, 0, 0]])
W5M = np.array([[1, 1, 0, 0, 2], [1, 1, 0, 2, 1], [0, 0, 1, 0, 1], [0, 2, 0, 1, 1], [2, 1, 1, 1, 0]])


def test_oracle_on_the_twelve_rows():
    X, Y = MC.twelve()
    out, n_in, nk = MC.window_oracle(X, Y, 0, 100, 0, 0, 5, 5)
    assert np.array_equal(out, W5) and (n_in, nk) == (12, 12) and out.dtype == np.uint32
    out, n_in, nk = MC.window_oracle(X, Y, 0, 100, 0, 0, 5, 5, True)
    assert np.array_equal(out, W5M) and (n_in, nk) == (20, 12) and np.array_equal(out, out.T)
    bx, by, cnt, nk = MC.cells_oracle(X, Y, 0, 100, True)
    assert list(zip(bx.tolist(), by.tolist(), cnt.tolist())) == [(0, 0, 1), (0, 1, 1), (0, 4, 2), (1, 1, 1), (1, 3, 2), (1, 4, 1), (2, 2, 1),
                                                                  (2, 4, 1), (3, 3, 1), (3, 4, 1)]
    out, nx, ny, nk = MC.v4c_oracle(X, Y, 0, 100, 100, 200, 0, 5)
    assert out.tolist() == [1, 2, 0, 2, 1] and (nx, ny, nk) == (3, 3, 12)
    assert np.array_equal(out, W5M[1] + (np.arange(5) == 1) * W5[1, 1])                  # the identity with the two windows
    assert MC.window_oracle(X, Y, 300, 100, 0, 0, 5, 5)[1:] == (2, 2)                    # a cut keeps Y - X >= cut: rows 9 and 12
    assert np.array_equal(MC.bins([-1, 0, -100, -101, 99, 100], 100), [-1, 0, -1, -2, 0, 1])


# ---- regions -----------------------------------------------------------------------------------------------------
def test_region_parsing():
    assert matrix.parse_region("chr21:20000000-21000000") == ("chr21", 20000000, 21000000)
    assert matrix.parse_region("chrX:0-1") == ("chrX", 0, 1) and matrix.parse_region("HLA-A*01:5-9") == ("HLA-A*01", 5, 9)
    for bad in ("", "chr1", "chr1:", "chr1:5", "chr1:5-", "chr1:a-b", "chr1:5-9-12", "chr1 :5-9", ":5-9", "chr1:9-5", "chr1:5-5", "chr1:-5-9",
                "chr1:1,000-2,000", None, 7, ("chr1", 5, 9)):
        with pytest.raises(ValueError):
            matrix.parse_region(bad)


def test_bins_overlapping_a_region():
    assert matrix.region_bins(20000000, 21000000, 5000) == (4000, 200)      # ends on a bin boundary: bin 4200 is not touched
    assert matrix.region_bins(20000000, 21000001, 5000) == (4000, 201)
    assert matrix.region_bins(20004999, 20005000, 5000) == (4000, 1)        # one bp, the last of its bin
    assert matrix.region_bins(20005000, 20005001, 5000) == (4001, 1)
    assert matrix.region_bins(0, 1, 1) == (0, 1) and matrix.region_bins(7, 12, 1) == (7, 5)
    assert matrix.bin_label("chr1", 3, 100) == "chr1:300-400"
    for res in (0, -5, 1 << 29, "x", None):
        with pytest.raises(ValueError):
            matrix.check_res(res)
    assert matrix.check_res((1 << 29) - 1) == (1 << 29) - 1 and matrix.check_res("5000") == 5000


def test_smallest_res_that_fits():
    r = ("chr1", 0, 8192 * 10)
    assert matrix.window_fits(r, ("chr1", 0, 2048 * 10), 10) and not matrix.window_fits(r, ("chr1", 0, 2049 * 10), 10)     # 2^24 cells, one more
    assert not matrix.window_fits(("chr1", 0, 8193 * 10), ("chr1", 0, 10), 10)                                            # 8193 bins a side
    for r1, r2 in ((r, r), (("chr1", 5, 5 + 100000000), ("chr1", 0, 1000)), (("chr1", 3, 4), ("chr1", 3, 4)),
                   (("chr1", 123456, 98765432), ("chr1", 123456, 98765432))):
        res = matrix.smallest_res(r1, r2)
        assert matrix.window_fits(r1, r2, res) and (res == 1 or not matrix.window_fits(r1, r2, res - 1))
    assert matrix.smallest_res(r, r) == 20                                                                            # 4096 x 4096


# ---- the three texts ------------------------------------------------------------------------------------------------
LABELS = ["chr1:0-100", "chr1:100-200", "chr1:200-300", "chr1:300-400", "chr1:400-500"]
MATRIX_TXT = ("\t" + "\t".join(LABELS) + "\n"
              "chr1:0-100\t1\t1\t0\t0\t2\n"
              "chr1:100-200\t1\t1\t0\t2\t1\n"
              "chr1:200-300\t0\t0\t1\t0\t1\n"
              "chr1:300-400\t0\t2\t0\t1\t1\n"
              "chr1:400-500\t2\t1\t1\t1\t0\n")
CELLS_TXT = ("chr1\t0\t100\tchr1\t0\t100\t1\n"
             "chr1\t0\t100\tchr1\t100\t200\t1\n"
             "chr1\t0\t100\tchr1\t400\t500\t2\n"
             "chr1\t100\t200\tchr1\t100\t200\t1\n"
             "chr1\t100\t200\tchr1\t300\t400\t2\n"
             "chr1\t100\t200\tchr1\t400\t500\t1\n"
             "chr1\t200\t300\tchr1\t200\t300\t1\n"
             "chr1\t200\t300\tchr1\t400\t500\t1\n"
             "chr1\t300\t400\tchr1\t300\t400\t1\n"
             "chr1\t300\t400\tchr1\t400\t500\t1\n")
V4C_TXT = ('track type=bedGraph name="v4c chr1:100-200"\n'
           "chr1\t0\t100\t1\n"
           "chr1\t100\t200\t2\n"
           "chr1\t300\t400\t2\n"
           "chr1\t400\t500\t1\n")


def test_window_text(standin, tmp_path):
    out = os.path.join(str(tmp_path), "w")
    js = matrix.jd2window("jd", out, "chr1:0-500", res=100)
    got = _read(out, matrix.SUFFIXES[:2])
    assert got["_matrix.txt"] == MATRIX_TXT
    want = {"region": "chr1:0-500", "region2": "chr1:0-500", "res": 100, "nx": 5, "ny": 5, "cut": 0, "mirror": True, "n_in": 20, "n_kept": 12,
            "max": 2}
    assert js == want and got["_matrix.json"] == json.dumps(want, indent=1, sort_keys=True) + "\n"
    # two regions: not mirrored unless asked for; rows 1 .. 2 against columns 3 .. 4
    js = matrix.jd2window("jd", out, "chr1:100-300", region2="chr1:300-500", res=100)
    assert _read(out, ["_matrix.txt"])["_matrix.txt"] == ("\tchr1:300-400\tchr1:400-500\nchr1:100-200\t2\t0\nchr1:200-300\t0\t1\n")
    assert (js["mirror"], js["n_in"], js["nx"], js["ny"]) == (False, 3, 2, 2)
    js = matrix.jd2window("jd", out, "chr1:100-300", region2="chr1:300-500", res=100, mirror=True)
    assert _read(out, ["_matrix.txt"])["_matrix.txt"] == ("\tchr1:300-400\tchr1:400-500\nchr1:100-200\t2\t1\nchr1:200-300\t0\t1\n")
    assert js["mirror"] is True and js["n_in"] == 4
    assert matrix.jd2window("jd", out, "chr1:0-500", res=100, cut=300)["n_kept"] == 2


def test_cells_text(standin, tmp_path):
    out = os.path.join(str(tmp_path), "c")
    js = matrix.jd2cells("jd", out, res=100, chroms={"chr1"})
    got = _read(out, matrix.SUFFIXES[2:4])
    assert got["_cells.txt"] == CELLS_TXT
    want = {"res": 100, "cut": 0, "fold": True, "chroms": {"chr1": {"n_cells": 10, "n_kept": 12, "max_count": 2}},
            "total": {"n_cells": 10, "n_kept": 12, "max_count": 2}}
    assert js == want and got["_cells.json"] == json.dumps(want, indent=1, sort_keys=True) + "\n"
    assert standin["chr1"].chrom.cells is None                              # freed behind the export
    js = matrix.jd2cells("jd", out, res=100, chroms={"chr1"}, fold=False)
    lines = _read(out, ["_cells.txt"])["_cells.txt"].splitlines()
    assert lines[-1] == "chr1\t400\t500\tchr1\t100\t200\t1" and len(lines) == 10 and js["fold"] is False
    # both chromosomes in name order; chunked fetches give the same text
    js = matrix.jd2cells("jd", out, res=250)
    text = _read(out, ["_cells.txt"])["_cells.txt"]
    assert list(js["chroms"]) == ["chr1", "chr2"] and js["total"]["n_kept"] == 312
    names = [line.split("\t")[0] for line in text.splitlines()]
    assert names == sorted(names) and set(names) == {"chr1", "chr2"}
    assert sum(int(line.split("\t")[6]) for line in text.splitlines()) == 312
    ch = standin["chr2"].chrom
    whole = matrix.chrom_cells(ch, "chr2", 250, 0, True)
    assert matrix.chrom_cells(ch, "chr2", 250, 0, True, chunk=7) == whole and whole[1]["n_cells"] > 7


def test_v4c_text(standin, tmp_path):
    out = os.path.join(str(tmp_path), "v")
    js = matrix.jd2v4c("jd", out, "chr1:100-200", res=100)
    got = _read(out, matrix.SUFFIXES[4:])
    assert got["_v4c.bedGraph"] == V4C_TXT
    want = {"viewpoint": "chr1:100-200", "res": 100, "cut": 0, "norm": "none", "n_x": 3, "n_y": 3, "n_kept": 12, "bin0": 0, "n_bins": 5, "max": 2}
    assert js == want and got["_v4c.json"] == json.dumps(want, indent=1, sort_keys=True) + "\n"
    js = matrix.jd2v4c("jd", out, "chr1:100-200", region="chr1:250-400", res=100, norm="cpm")
    assert _read(out, ["_v4c.bedGraph"])["_v4c.bedGraph"] == 'track type=bedGraph name="v4c chr1:100-200"\nchr1\t300\t400\t333333.333\n'
    assert (js["bin0"], js["n_bins"], js["n_x"], js["n_y"], js["max"]) == (2, 2, 3, 3, 2)


def test_cpm_scale():
    from cloops_amd.coverage import fixed_point
    assert matrix.cpm_scale("none", 6) is None and matrix.cpm_scale("cpm", 0) is None and matrix.cpm_scale("cpm", 6) == (10 ** 9, 6)
    assert fixed_point(1, *matrix.cpm_scale("cpm", 6)) == "166666.667" and fixed_point(2, *matrix.cpm_scale("cpm", 6)) == "333333.333"
    assert fixed_point(3, *matrix.cpm_scale("cpm", 3000000)) == "1.000"
    with pytest.raises(ValueError):
        matrix.cpm_scale("rpkm", 6)
    assert matrix.format_v4c("c", 10, -2, [0, 5, 0], ("c", 0, 9)) == 'track type=bedGraph name="v4c c:0-9"\nc\t-10\t0\t5\n'


def test_suffixes_against_the_files_written(standin, tmp_path):
    out = os.path.join(str(tmp_path), "s")
    matrix.jd2window("jd", out, "chr1:0-500", res=100)
    matrix.jd2cells("jd", out, res=100)
    matrix.jd2v4c("jd", out, "chr1:100-200", res=100)
    assert sorted(os.listdir(str(tmp_path))) == sorted("s" + s for s in matrix.SUFFIXES)
    assert matrix.SUFFIXES == ("_matrix.txt", "_matrix.json", "_cells.txt", "_cells.json", "_v4c.bedGraph", "_v4c.json")


def test_kept_span():
    ch = MC.OracleChrom(*MC.twelve())
    assert matrix.kept_span(ch, 100, 0) == (0, 5) and matrix.kept_span(ch, 100, 0, chunk=3) == (0, 5) and ch.cells is None
    assert matrix.kept_span(ch, 100, 10000) == (0, 0)
    assert matrix.kept_span(MC.OracleChrom([-150, 320], [-120, 100]), 100, 0) == (-2, 6)


# ---- refused arguments write nothing ----------------------------------------------------------------------------------
def test_nothing_is_written_when_an_argument_is_refused(standin, tmp_path):
    out = os.path.join(str(tmp_path), "r")
    W, C, V = matrix.jd2window, matrix.jd2cells, matrix.jd2v4c
    bad = [lambda: W("jd", out, "chr1:0-500-9"), lambda: W("jd", out, "chr1:500-0"), lambda: W("jd", out, "chr1:-5-100"),
           lambda: W("jd", out, "chr9:0-500"),                                           # an unknown chromosome
           lambda: W("jd", out, "chr1:0-500", region2="chr2:0-500"),                     # a trans window
           lambda: W("jd", out, "chr1:0-500", res=0), lambda: W("jd", out, "chr1:0-500", res=1 << 29),
           lambda: W("jd", out, "chr1:0-100000", res=10),                                # 10 000 bins a side
           lambda: C("jd", out, res=0), lambda: C("jd", out, res="x"),
           lambda: V("jd", out, "chr1:200-100"), lambda: V("jd", out, "chr9:100-200"), lambda: V("jd", out, "chr1:100-200", norm="rpkm"),
           lambda: V("jd", out, "chr1:100-200", region="chr2:0-500"), lambda: V("jd", out, "chr1:100-200", region="chr1:0-20000000", res=1),
           lambda: V("jd", out, "chr1:100-200", res=-1)]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    assert os.listdir(str(tmp_path)) == []
    assert all(r.chrom.calls == [] for r in standin.values())                # ... and before any work on a chromosome
    with pytest.raises(ValueError) as ei:
        W("jd", out, "chr1:0-100000", res=10)
    assert "smallest -res that fits is 25" in str(ei.value)                  # 100 000 bp in 4096 x 4096 bins


def test_a_trans_file_is_left_out(tmp_path):
    from cloops_amd.coverage import chrom_files
    d = str(tmp_path)
    for name in ("chr1-chr1.jd", "chr1-chr2.jd", "chr2-chr2.jd"):
        open(os.path.join(d, name), "w").close()
    assert [c for c, _ in chrom_files(d)] == ["chr1", "chr2"] and [c for c, _ in chrom_files(d, {"chr2"})] == ["chr2"]
    with pytest.raises(ValueError):
        matrix.jd2cells("/nonexistent/jd", os.path.join(d, "out"))


# ---- command lines -------------------------------------------------------------------------------------------------
def test_help_defaults_and_overrides():
    op = matrix.help(["window", "-d", "jd", "-o", "out", "-r", "chr21:20000000-21000000"])
    assert (op.cmd, op.res, op.cut, op.region2, op.mirror, op.plot) == ("window", 5000, 0, None, False, False)
    op = matrix.help(["window", "-d", "jd", "-o", "out", "-r", "chr21:1-2", "-r2", "chr21:5-9", "-res", "100", "-cut", "7", "-mirror", "-plot"])
    assert (op.region, op.region2, op.res, op.cut, op.mirror, op.plot) == ("chr21:1-2", "chr21:5-9", 100, 7, True, True)
    op = matrix.help(["cells", "-d", "jd", "-o", "out"])
    assert (op.cmd, op.res, op.cut, op.chroms, op.nofold) == ("cells", 10000, 0, "", False)
    op = matrix.help(["cells", "-d", "jd", "-o", "out", "-res", "2500", "-cut", "3", "-c", "chr1,chr2", "-nofold"])
    assert (op.res, op.cut, op.chroms, op.nofold) == (2500, 3, "chr1,chr2", True)
    op = matrix.help(["v4c", "-d", "jd", "-o", "out", "-v", "chr21:34000000-34010000"])
    assert (op.cmd, op.res, op.cut, op.region, op.norm) == ("v4c", 1000, 0, None, "none")
    op = matrix.help(["v4c", "-d", "jd", "-o", "out", "-v", "chr21:5-9", "-r", "chr21:0-100", "-res", "10", "-cut", "2", "-norm", "cpm"])
    assert (op.view, op.region, op.res, op.cut, op.norm) == ("chr21:5-9", "chr21:0-100", 10, 2, "cpm")
    for bad in ([], ["window", "-d", "jd", "-o", "out"], ["v4c", "-d", "jd", "-o", "out"], ["v4c", "-d", "jd", "-o", "out", "-v", "a:1-2", "-norm", "x"],
                ["heatmap", "-d", "jd", "-o", "out"]):
        with pytest.raises(SystemExit):
            matrix.help(bad)


def test_main_runs_the_subcommands(standin, tmp_path):
    out = os.path.join(str(tmp_path), "m")
    assert matrix.main(["window", "-d", "jd", "-o", out, "-r", "chr1:0-500", "-res", "100"]) == 0
    assert matrix.main(["cells", "-d", "jd", "-o", out, "-res", "100", "-c", "chr1"]) == 0
    assert matrix.main(["v4c", "-d", "jd", "-o", out, "-v", "chr1:100-200", "-res", "100"]) == 0
    got = _read(out, matrix.SUFFIXES)
    assert (got["_matrix.txt"], got["_cells.txt"], got["_v4c.bedGraph"]) == (MATRIX_TXT, CELLS_TXT, V4C_TXT)


def test_pipe_takes_the_flag():
    import inspect
    from cloops_amd import pipe
    sig = inspect.signature(pipe.pipe).parameters
    assert sig["mat"].default == 0 and sig["mat_res"].default == 10000
    assert list(sig)[-2:] == ["mat", "mat_res"]                              # appended: the earlier parameters keep their places


def test_constants_agree():
    from cloops_amd import _lib
    assert (matrix.WMAX, matrix.CELLS_MAX) == (_lib.CL_MAT_WMAX, _lib.CL_MAT_CELLS_MAX) == (8192, 1 << 24)
