"""GPU: kernel K11 (cl_quant_counts) against the numpy brute force of test_quant.py, against K8 on the same handle, and the two
command lines (python -m cloops_amd.quant / cloops_amd.deloops) on .jd directories written by cloops_amd.io against the
goldens of the real scripts."""
import gzip
import os

import numpy as np
import pytest

import golden_util as G
import sig_cases as S
from test_quant import GOLD, QUANT_GOLD, brute_counts, _read

pytestmark = pytest.mark.gpu


def _wins(recs):
    from cloops_amd import cModel
    return cModel._windows(recs)[3]


def _records(name):
    """the significant loops of a golden .loop file as records [c, s, e, c, s, e]"""
    from cloops_amd import quant
    ivac, ivbc = quant._anchor_columns(os.path.join(GOLD, name), None, None)
    out = []
    for i, line in enumerate(open(os.path.join(GOLD, name))):
        f = line.rstrip("\n").split("\t")
        if i == 0 or float(f[-1]) < 1:
            continue
        out.append(quant.parseIv(f[ivac]) + quant.parseIv(f[ivbc]))
    return out


def _subsample():
    z = np.load(os.path.join(GOLD, "chr21_quant_subsample.npz"))
    return np.flatnonzero(np.unpackbits(z["mask"])[:int(z["n"])])


def _check(ch, X, Y, wins, cut):
    got, n = ch.quant_counts(wins, cut)
    want, n2 = brute_counts(X, Y, wins, cut)
    assert n == n2
    assert np.array_equal(got, want)
    return got


def test_chr21_vs_brute_and_k8():
    from cloops_amd import api
    X, Y = G.chr21_xy()
    rows = _subsample()
    wins = _wins(_records("chr21_v2.loop") + _records("chr21_v1.loop"))
    for XX, YY in ((X, Y), (X[rows], Y[rows])):
        ch = api.Chromosome(XX, YY)
        for cut in (0, 4601):
            got = _check(ch, XX, YY, wins, cut)
            k8, n8 = ch.sig_counts(wins, cut)                       # same handle, same sorted tables
            assert np.array_equal(got[:, 2], k8[:, 22])
            assert np.array_equal(got[:, 0], k8[:, 0]) and np.array_equal(got[:, 1], k8[:, 11])
            again, _ = ch.quant_counts(wins, cut)
            assert np.array_equal(again, got)                        # deterministic
        ch.close()


def test_synthetic_edges():
    from cloops_amd import api
    rng = np.random.default_rng(11)
    # duplicate coordinates and PETs exactly on window bounds
    X = np.repeat(np.array([0, 5, 100, 100, 250, 400, 1000, 1000, 1500], np.int64), 3)
    Y = X + np.repeat(np.array([50, 95, 200, 300, 150, 600, 1000, 1000, 20], np.int64), 3)
    recs = [["c", 0, 100, "c", 300, 400],          # shifted windows clamped at 0 by max([0, ...])
            ["c", 100, 250, "c", 400, 1000],       # bounds on PET coordinates
            ["c", 5, 5, "c", 100, 100],            # one-point windows
            ["c", 3000, 3100, "c", 5000, 5200],    # empty windows
            ["c", 1000, 1500, "c", 2000, 2000]]
    wins = _wins(recs)
    assert (wins[0, 1:11] == 0).any()
    ch = api.Chromosome(X, Y)
    for cut in (0, 100, 500):
        _check(ch, X, Y, wins, cut)
    w2 = wins.copy()
    w2[:, 22 + 3] = w2[:, 3] - 7                                   # an inverted window holds nothing
    _check(ch, X, Y, w2, 0)
    got, n = ch.quant_counts(np.zeros((0, 44), np.int32))          # n_records == 0
    assert got.shape == (0, 123) and n == len(X)
    ch.close()
    # a record whose A span holds many thousands of PETs
    X = np.sort(rng.integers(0, 200000, 60000)).astype(np.int64)
    Y = X + rng.integers(0, 400000, 60000)
    wins = _wins([["c", 90000, 110000, "c", 150000, 190000], ["c", 0, 200000, "c", 0, 600000], ["c", 1000, 1500, "c", 9000, 9900]])
    ch = api.Chromosome(X, Y)
    got = _check(ch, X, Y, wins, 0)
    assert got[1, 2] > 20000
    _check(ch, X, Y, wins, 150000)
    ch.close()


@pytest.mark.parametrize("n", [0, 1])
def test_tiny_chromosomes(n):
    from cloops_amd import api
    X = np.array([10], np.int64)[:n]
    Y = np.array([30], np.int64)[:n]
    wins = _wins([["c", 0, 20, "c", 25, 40], ["c", 50, 60, "c", 70, 90]])
    ch = api.Chromosome(X, Y)
    for cut in (0, 15, 25):
        _check(ch, X, Y, wins, cut)
    ch.close()


def test_between_sweep_steps():
    """K11 between two sweep steps leaves the steps' results unchanged; with a run in flight it is refused"""
    from cloops_amd import api, _lib
    X, Y = G.chr21_xy()
    wins = _wins(_records("chr21_v2.loop"))

    def sweep(with_quant):
        ch = api.Chromosome(X, Y)
        ch.set_device_labels(False)
        ch.cand_reset()
        out = []
        for step, (eps, cut) in enumerate(((1000, 0), (2000, 4601))):
            ch.step_async("v2", eps, 5, cut, step)
            if with_quant and step == 1:
                with pytest.raises(_lib.CloopsHipError):
                    ch.quant_counts(wins)
            ch.wait()
            ni, ns, st = ch.step_result()
            out.append((ni, ns, st["n_all"], st["sumx"], st["loghist"].tolist()))
            if with_quant:
                _check(ch, X, Y, wins, cut)
        out.append(ch.cand_finish(4601, 100000).tolist())
        ch.close()
        return out
    assert sweep(True) == sweep(False)


SIG_CASE_CUTS = [(name, k) for name in S.QUANT_NAMES for k in range(3)]


@pytest.mark.parametrize("name_k", SIG_CASE_CUTS, ids=lambda p: "%s-%s" % (p[0], ("cut0", "part", "none")[p[1]]))
def test_cases_of_sig_counts(name_k):
    """K8's edge cases through K11: the Y-side halves of ra and rb meet reversed rows, negative coordinates, the ends of int32 and
    slices around the workgroup's stride; at the cut that keeps no row the table is all zero"""
    from cloops_amd import api
    c = S.case(name_k[0])
    cut = S.cuts_of(c)[name_k[1]]
    ch = api.Chromosome(c.X, c.Y)
    got = _check(ch, c.X, c.Y, c.windows, cut)
    if name_k[1] == 2:
        assert not got.any() and ch.quant_counts(c.windows, cut)[1] == 0
    else:
        k8, n8 = ch.sig_counts(c.windows, cut)                              # same handle, same sorted tables
        assert np.array_equal(got[:, 0], k8[:, 0]) and np.array_equal(got[:, 1], k8[:, 11]) and np.array_equal(got[:, 2], k8[:, 22])
    ch.close()


def _io_dirs(root):
    """.jd directories written by cloops_amd.io (parseRawBedpe2) from the example BEDPE and from its subsample's lines"""
    from cloops_amd import io as cio
    bed = G.write_example_bedpe(root)
    with gzip.open(bed, "rt") as fh:
        lines = fh.readlines()
    sub = os.path.join(str(root), "sub.bedpe")
    with open(sub, "w") as fh:
        fh.writelines([lines[i] for i in _subsample()])
    out = []
    for name, f in (("chr21_A", bed), ("chr21_B", sub)):
        d = os.path.join(str(root), name)
        os.makedirs(d)
        cio.parseRawBedpe2([f], d, [], 0)
        out.append(d)
    return out


def test_command_lines_match_goldens(tmp_path):
    import subprocess
    import sys
    from cloops_amd import pipe
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    da, db = _io_dirs(tmp_path)
    dirs = {"A": da, "B": db}
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for fname, ds, dis, prefix in QUANT_GOLD:
        out = os.path.join(str(tmp_path), prefix)
        subprocess.check_call([sys.executable, "-m", "cloops_amd.quant", "-f", os.path.join(GOLD, "chr21_v2.loop"), "-d", dirs[ds],
                               "-o", out, "-dis", str(dis)], env=env, cwd=str(tmp_path), timeout=300)
        assert _read(out + "_quantLoops.txt") == _read(os.path.join(GOLD, fname)), fname
    for rep in range(2):                                           # deterministic across runs
        subprocess.check_call([sys.executable, "-m", "cloops_amd.deloops", "-fa", os.path.join(GOLD, "chr21_v2.loop"),
                               "-fb", os.path.join(GOLD, "chr21_v1.loop"), "-da", da, "-db", db], env=env, cwd=str(tmp_path), timeout=300)
        for name in ("chr21_A.deloop", "chr21_B.deloop"):
            assert _read(os.path.join(str(tmp_path), name)) == _read(os.path.join(GOLD, name)), name
    # in process: both datasets resident in the cache at once, the .jd files read once
    from cloops_amd import deloops, quant
    pipe.CACHE.clear()
    ra = quant.preDs(os.path.join(GOLD, "chr21_v2.loop"), da)
    rb = quant.preDs(os.path.join(GOLD, "chr21_v1.loop"), db)
    deloops.callDeLoops(ra, rb, os.path.join(str(tmp_path), "in_A"), os.path.join(str(tmp_path), "in_B"))
    r1 = pipe.CACHE.get(ra["chr21"]["f"])
    deloops.callDeLoops(ra, rb, os.path.join(str(tmp_path), "in_A"), os.path.join(str(tmp_path), "in_B"))
    assert pipe.CACHE.get(ra["chr21"]["f"]) is r1
    assert _read(os.path.join(str(tmp_path), "in_A.deloop")) == _read(os.path.join(GOLD, "chr21_A.deloop"))
    pipe.CACHE.clear()
