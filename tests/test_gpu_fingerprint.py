"""GPU: kernel K12 (cl_contact_hist) against the numpy brute force of test_fingerprint.py, its argument errors, determinism, its
effect on a sweep (none), and the command line (python -m cloops_amd.fingerprint) on .jd directories written by cloops_amd.io
against the goldens of the script's own functions."""
import ctypes
import gzip
import os

import joblib
import numpy as np
import pytest

import golden_util as G
from test_fingerprint import DIRS, GOLD, _read, brute_hist, datasets, golden_arrays, golden_cases, golden_meta

pytestmark = pytest.mark.gpu


def _check(ch, X, Y, bs, cut=0):
    v, m, kept, minc = ch.contact_hist(bs, cut)
    wv, wm, wkept, wminc = brute_hist(X, Y, bs, cut)
    assert kept == wkept and minc == wminc, (bs, cut)
    assert np.array_equal(v, wv) and np.array_equal(m, wm), (bs, cut)
    assert v.dtype == np.int64 and m.dtype == np.int64
    return v, m


def test_chr21_vs_brute():
    from cloops_amd import api
    X, Y = G.chr21_xy()
    ch = api.Chromosome(X, Y)
    meta = golden_meta()
    for bs in meta["bin_sizes"]:
        v, m = _check(ch, X, Y, bs)
        if bs == 1000000:
            assert v.max() > 2048                                     # a count beyond the LDS histogram: the overflow list
    for cut in (1, 4601, 100000):
        _check(ch, X, Y, 2000, cut)
    ch.close()


def test_golden_datasets_vs_brute():
    from cloops_amd import api
    ga = golden_arrays()
    data = datasets()
    for name, bs, cut, tag in golden_cases():
        parts = []
        for x, y in data[name].values():
            ch = api.Chromosome(x, y)
            parts.append(np.repeat(*_check(ch, x, y, bs, cut)))
            ch.close()
        assert np.array_equal(np.sort(np.concatenate(parts)), ga["counts_%s_%s" % (name, tag)]), (name, tag)


def test_edges():
    from cloops_amd import api
    rng = np.random.default_rng(12)
    big = 2 ** 29 - 1                                                  # the largest coordinate a handle takes (cl_chrom_create)
    cases = [
        (np.array([5], np.int64), np.array([9], np.int64), (1, 2, 2000)),                                 # one PET
        (np.full(100000, 777, np.int64), np.full(100000, 9000, np.int64), (1, 2000)),                     # one cell of 100 000
        (np.arange(0, 60000, 3, dtype=np.int64), np.arange(0, 60000, 3, dtype=np.int64) + 11, (1, 2)),    # every count 1
        (rng.integers(0, 10 ** 6, 50000), None, (1, 2, 3, 1000, 2 ** 31 - 1)),                           # bs 1 .. beyond the extent
        (big - rng.integers(0, 10 ** 7, 40000), None, (1, 7, 2000)),                                       # near 2^29 - 1
    ]
    for X, Y, sizes in cases:
        if Y is None:
            Y = np.minimum(X + rng.integers(0, 10 ** 6, len(X)), big)
        ch = api.Chromosome(X, Y)
        for bs in sizes:
            _check(ch, X, Y, bs)
        ch.close()
    # the widest span a handle takes (|X|, |Y| < 2^29, cl_chrom_create): 31 key bits per axis at bs 1
    X = np.array([-big, -big, 0, 5, big - 3, big], np.int64)
    Y = np.array([big, big, 10, 5, big, big], np.int64)
    ch = api.Chromosome(X, Y)
    for bs in (1, 3, 2 ** 28, 2 ** 31 - 1):
        _check(ch, X, Y, bs)
    ch.close()
    # mixed: a few heavy cells above the LDS range among many small ones
    X = np.concatenate([np.repeat([10, 50000, 90000], [5000, 2049, 2048]), rng.integers(0, 10 ** 6, 30000)]).astype(np.int64)
    Y = X + np.concatenate([np.zeros(9097, np.int64), rng.integers(0, 10 ** 5, 30000)])
    ch = api.Chromosome(X, Y)
    for bs in (1, 100, 5000):
        _check(ch, X, Y, bs)
    ch.close()


def test_cut_edges():
    from cloops_amd import api
    X = np.array([100, 200, 300, 400], np.int64)
    Y = np.array([150, 260, 1300, 410], np.int64)
    ch = api.Chromosome(X, Y)
    v, m = _check(ch, X, Y, 10, 1000)                               # one row left
    assert v.tolist() == [1] and m.tolist() == [1]
    v, m, kept, minc = ch.contact_hist(10, 1001)                    # none left
    assert kept == 0 and minc is None and len(v) == 0 and len(m) == 0
    ch.close()
    ch = api.Chromosome(X[:0], Y[:0])                                # no PET at all
    assert ch.contact_hist(10)[2] == 0
    ch.close()


def test_module_on_resident_chromosomes():
    """jds2FingerPrint on 'mem://' chromosomes of pipe.CACHE (genome-wide C, two chromosomes) equals the golden group vector;
    a cut that leaves no row raises ValueError like np.min"""
    from cloops_amd import fingerprint, pipe
    ga = golden_arrays()
    pipe.CACHE.clear()
    try:
        fs = [pipe.CACHE.put_arrays("%s-%s" % (c, c), x, y) for c, (x, y) in datasets()["synth_C"].items()]
        assert np.array_equal(fingerprint.jds2FingerPrint(fs, 0, 2000), ga["groups_synth_C_bs2000"])
        assert np.array_equal(fingerprint.jds2FingerPrint(fs, 4601, 2000), ga["groups_synth_C_bs2000_cut4601"])
        with pytest.raises(ValueError):
            fingerprint.jd2contactMatrixUpper(fs[0], 10 ** 9, 2000)
        with pytest.raises(ValueError):
            fingerprint.jds2FingerPrint(fs, 0, 0)
    finally:
        pipe.CACHE.clear()


def test_argument_errors():
    from cloops_amd import api, _lib
    lib = _lib.load()
    X, Y = G.chr21_xy()
    ch = api.Chromosome(X, Y)
    vals = np.zeros(64, np.int64)
    mult = np.zeros(64, np.int64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    nd, nc, nk, mc = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(0)
    r = lambda *a: lib.cl_contact_hist(*a)
    assert r(None, 0, 2000, 64, vp(vals), vp(mult), ctypes.byref(nd), None, None, None) == _lib.CL_ERR_ARG
    for bs in (0, -5):
        assert r(ch._h, 0, bs, 64, vp(vals), vp(mult), ctypes.byref(nd), None, None, None) == _lib.CL_ERR_ARG
    assert r(ch._h, 0, 2000, -1, vp(vals), vp(mult), ctypes.byref(nd), None, None, None) == _lib.CL_ERR_ARG
    assert r(ch._h, 0, 2000, 64, None, vp(mult), ctypes.byref(nd), None, None, None) == _lib.CL_ERR_ARG
    assert r(ch._h, 0, 2000, 64, vp(vals), vp(mult), None, None, None, None) == _lib.CL_ERR_ARG
    # capacity below the number of distinct counts: an error code, the needed size reported, nothing written
    want = brute_hist(X, Y, 2000)
    small = np.full(3, -7, np.int64)
    assert r(ch._h, 0, 2000, 3, vp(small), vp(small), ctypes.byref(nd), None, None, None) == _lib.CL_ERR_ARG
    assert nd.value == len(want[0]) and small.tolist() == [-7, -7, -7]
    with pytest.raises(ValueError):
        ch.contact_hist(0)
    # the handle still works, with every optional output given
    big = np.zeros(len(want[0]), np.int64)
    big2 = np.zeros(len(want[0]), np.int64)
    assert r(ch._h, 0, 2000, len(big), vp(big), vp(big2), ctypes.byref(nd), ctypes.byref(nc), ctypes.byref(nk), ctypes.byref(mc)) == 0
    assert np.array_equal(big, want[0]) and np.array_equal(big2, want[1])
    assert nc.value == want[1].sum() and nk.value == len(X) and mc.value == want[3]
    ch.close()


def test_repeatable_and_two_streams():
    from cloops_amd import api, _lib
    lib = _lib.load()
    X, Y = G.chr21_xy()
    s1, s2 = lib.cl_stream_create(0), lib.cl_stream_create(0)
    try:
        a = api.Chromosome(X, Y, stream=s1)
        b = api.Chromosome(X[::-1].copy(), Y[::-1].copy(), stream=s2)           # row order does not matter
        for bs, cut in ((1, 0), (2000, 0), (1000000, 0), (2000, 4601)):
            ra = [a.contact_hist(bs, cut) for _ in range(3)]
            rb = b.contact_hist(bs, cut)
            for r in ra[1:] + [rb]:
                assert np.array_equal(r[0], ra[0][0]) and np.array_equal(r[1], ra[0][1]) and r[2:] == ra[0][2:]
        a.close()
        b.close()
    finally:
        lib.cl_stream_destroy(s1)
        lib.cl_stream_destroy(s2)


def test_between_sweep_steps():
    """K12 between two sweep steps on the same handle leaves the steps' results unchanged"""
    from cloops_amd import api
    X, Y = G.chr21_xy()

    def sweep(with_fp):
        ch = api.Chromosome(X, Y)
        ch.set_device_labels(False)
        ch.cand_reset()
        out = []
        for step, (eps, cut) in enumerate(((1000, 0), (2000, 4601), (2000, 13532))):
            ch.step_async("v2", eps, 5, cut, step)
            ch.wait()
            ni, ns, st = ch.step_result()
            out.append((ni, ns, st["n_all"], st["sumx"], st["loghist"].tolist()))
            if with_fp:
                _check(ch, X, Y, 2000, cut)
                _check(ch, X, Y, 1000000)
        out.append(ch.cand_finish(4601, 100000).tolist())
        ch.close()
        return out
    assert sweep(True) == sweep(False)


def _io_dirs(root):
    """.jd directories: A and B written by cloops_amd.io (parseRawBedpe2) from the example BEDPE and its subsample's lines, C (no
    BEDPE) written as the same [id, X, Y] int64 pickles"""
    from cloops_amd import io as cio
    from test_gpu_quant import _subsample
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
    d = os.path.join(str(root), "synth_C")
    os.makedirs(d)
    for chrom, (x, y) in datasets()["synth_C"].items():
        joblib.dump(np.stack([np.arange(len(x)), x, y], 1).astype(np.int64), os.path.join(d, "%s-%s.jd" % (chrom, chrom)))
    return out + [d]


def test_command_line_matches_goldens(tmp_path):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dirs = ",".join(_io_dirs(tmp_path))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = lambda *a: subprocess.check_call([sys.executable, "-m", "cloops_amd.fingerprint", "-d", dirs] + list(a), env=env,
                                           cwd=str(tmp_path), timeout=300)
    run("-o", "x", "-labels", "A,B,C", "-bs", "2000")
    assert _read(os.path.join(str(tmp_path), "x_fingerprint.txt")) == _read(os.path.join(GOLD, "fp_labels_fingerprint.txt"))
    run("-o", "y", "-bs", "10000", "-plot", "1", "-cut", "4601", "-p", "4")
    assert _read(os.path.join(str(tmp_path), "y_fingerprint.txt")) == _read(os.path.join(GOLD, "fp_bs10000_fingerprint.txt"))
    assert os.path.getsize(os.path.join(str(tmp_path), "y_fingerprint.pdf")) > 0
    assert list(DIRS) == golden_meta()["dirs"]
