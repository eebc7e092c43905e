"""GPU: kernel K13 (cl_anchor_mask) against the numpy brute force of test_cleanpets.py on the goldens and on edge cases, its argument
errors, determinism, its effect on a sweep (none), and the command line (python -m cloops_amd.cleanpets) on .jd directories written
by cloops_amd.io against the row sets of the script's own functions."""
import ctypes
import os

import joblib
import numpy as np
import pytest

import golden_util as G
from test_cleanpets import GOLD, brute_mask, components, datasets, golden_meta, golden_rows, write_jd_dirs

pytestmark = pytest.mark.gpu

LIM = (1 << 29) - 1                                                     # the largest |coordinate| a handle takes (cl_chrom_create)


def np_mask(X, Y, starts, ends):
    """sort-and-sweep merge + closed searchsorted membership (for sets too large for brute_mask) -> (bool [n], merged count)"""
    s = np.asarray(starts, np.int64)
    e = np.asarray(ends, np.int64)
    if len(s) == 0:
        return np.zeros(len(X), bool), 0
    o = np.lexsort((e, s))
    s, e = s[o], e[o]
    reach = np.maximum.accumulate(e)
    first = np.flatnonzero(np.r_[True, s[1:] > reach[:-1]])
    ms, me = s[first], reach[np.r_[first[1:], len(s)] - 1]

    def inside(v):
        k = np.searchsorted(ms, np.asarray(v, np.int64), side="right") - 1
        return (k >= 0) & (np.asarray(v, np.int64) <= me[np.maximum(k, 0)])
    return inside(X) | inside(Y), len(ms)


def _check(ch, X, Y, starts, ends, brute=True):
    mask, nm, nk = ch.anchor_mask(starts, ends)
    want, wm = np_mask(X, Y, starts, ends)
    if brute:
        assert np.array_equal(want, brute_mask(X, Y, starts, ends))
        assert wm == components(list(starts), list(ends))
    rows = ch.rows_of_mask(mask)
    assert mask.dtype == np.uint64 and len(mask) == (len(X) + 63) // 64
    assert np.array_equal(rows, np.flatnonzero(want)) and nk == len(rows) and nm == wm
    bits = np.unpackbits(mask.view(np.uint8), bitorder="little")
    assert not bits[len(X):].any()                                      # bits past n are 0
    return rows, nm


def _pool(loopf, sig=True):
    """the anchor pool of the chr21 loops of `loopf` (preDs needs a .jd to keep the chromosome: a one-row one)"""
    import tempfile
    from cloops_amd import cleanpets
    X, Y = G.chr21_xy()
    with tempfile.TemporaryDirectory() as td:
        dirs = write_jd_dirs(td, {"c": {"chr21": (X[:1], Y[:1])}})
        return cleanpets.preDs(os.path.join(GOLD, loopf), dirs["c"], sig)["chr21"]["rs"]


def test_goldens_vs_brute():
    from cloops_amd import api, cleanpets
    meta = golden_meta()
    data = datasets()
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        dirs = write_jd_dirs(td)
        for name, loopf, dname, sig, chroms in meta["cases"]:
            recs = cleanpets.preDs(os.path.join(GOLD, loopf), dirs[dname], sig, set(chroms) if chroms else [])
            for chrom, v in recs.items():
                x, y = data[dname][chrom]
                s, e = cleanpets._anchor_pool(v["rs"])
                ch = api.Chromosome(x, y)
                rows, nm = _check(ch, x, y, s, e)
                ch.close()
                g = meta["results"][name]["chroms"][chrom]
                assert np.array_equal(rows, golden_rows(name, chrom, len(x))), (name, chrom)
                assert len(rows) == g["kept"] and nm == g["anchors"], (name, chrom)


def test_edges():
    from cloops_amd import api, _lib
    rng = np.random.default_rng(31)
    # no anchors; one PET
    x, y = np.array([5], np.int64), np.array([9], np.int64)
    ch = api.Chromosome(x, y)
    mask, nm, nk = ch.anchor_mask([], [])
    assert mask.tolist() == [0] and nm == 0 and nk == 0
    for s, e in (([9], [9]), ([4], [4]), ([6], [8]), ([0, 10], [5, 20]), ([10], [20]), ([-5], [4])):
        _check(ch, x, y, s, e)
    ch.close()
    # row counts around a mask word and the 2048-row tile: every word is written, tail bits 0 (mask pre-filled with ones)
    lib = _lib.load()
    for n in (63, 64, 65, 127, 2047, 2048, 2049, 4095, 4097, 3 * 2048 + 1):
        x = rng.integers(0, 100000, n)
        y = x + rng.integers(0, 50000, n)
        s = rng.integers(0, 150000, 30)
        e = s + rng.integers(0, 3000, 30)
        ch = api.Chromosome(x, y)
        _check(ch, x, y, s, e)
        nw = (n + 63) // 64
        m = np.full(nw, np.uint64(0xFFFFFFFFFFFFFFFF))
        s64, e64 = np.ascontiguousarray(s, np.int64), np.ascontiguousarray(e, np.int64)
        nm, nk = ctypes.c_int64(-1), ctypes.c_int64(-1)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        assert lib.cl_anchor_mask(ch._h, len(s), vp(s64), vp(e64), vp(m), ctypes.byref(nm), ctypes.byref(nk)) == 0
        bits = np.unpackbits(m.view(np.uint8), bitorder="little")
        assert np.array_equal(np.flatnonzero(bits), np.flatnonzero(brute_mask(x, y, s, e))) and nk.value == bits.sum()
        ch.close()
    # coordinates at the handle's limit; anchors at it, beyond it, and spanning everything
    x = np.array([-LIM, -LIM, 0, LIM - 1, -LIM + 1], np.int64)
    y = np.array([-LIM, LIM, LIM, LIM, LIM - 1], np.int64)
    ch = api.Chromosome(x, y)
    big = 1 << 40
    for s, e in (([LIM], [LIM]), ([-LIM], [-LIM]), ([LIM + 1], [big]), ([-big], [-LIM - 1]), ([-big], [big]),
                 ([LIM + 1, -big], [big, -LIM - 1]), ([1 << 31, (1 << 31) + 10], [(1 << 31) + 5, (1 << 31) + 20]),
                 ([-(1 << 31) - 20, -(1 << 31)], [-(1 << 31) - 10, -(1 << 31) + 3]), ([-big, LIM], [-LIM, big]),
                 ([LIM - 1, LIM], [LIM - 1, LIM])):
        _check(ch, x, y, s, e)
    assert ch.anchor_mask([1 << 31, (1 << 31) + 10], [(1 << 31) + 5, (1 << 31) + 20])[1:] == (2, 0)   # merged before the clamp
    ch.close()
    with pytest.raises(_lib.CloopsHipError) as ei:                     # the handle's stated limit
        api.Chromosome(np.array([0], np.int64), np.array([1 << 29], np.int64))
    assert ei.value.code == _lib.CL_ERR_DOMAIN
    # zero rows: the merge count alone
    ch = api.Chromosome(np.zeros(0, np.int64), np.zeros(0, np.int64))
    mask, nm, nk = ch.anchor_mask([1, 5, 20], [5, 9, 30])
    assert len(mask) == 0 and nm == 2 and nk == 0
    ch.close()


def test_many_anchors_directory_form():
    """10^6 random anchors on a 2 M-row chromosome (beyond the LDS form), and a clustered set whose buckets hold many anchors"""
    from cloops_amd import api
    rng = np.random.default_rng(8)
    n, L = 2000000, 248000000
    x = rng.integers(0, L, n)
    y = np.minimum(x + rng.integers(0, 3000000, n), L)
    ch = api.Chromosome(x, y)
    s = rng.integers(0, L, 1000000)
    e = s + rng.integers(0, 400, 1000000)
    _check(ch, x, y, s, e, brute=False)
    cs = np.r_[rng.integers(0, 200000, 6000), rng.integers(0, L, 3000)]
    ce = cs + rng.integers(0, 30, len(cs))
    _check(ch, x, y, cs, ce, brute=False)
    sub = rng.choice(n, 20000, replace=False)
    xs, ys = x[sub], y[sub]
    ch2 = api.Chromosome(xs, ys)
    _check(ch2, xs, ys, cs, ce)                                         # np_mask against the brute force on a sample
    ch2.close()
    ch.close()


def test_search_form_boundary():
    """merged sets of exactly 255 / 256 / 257 anchors (the LDS form's limit) and just above or at powers of two (the fixed-length
    search's steps), rows at both ends of every anchor and between them"""
    from cloops_amd import api
    rng = np.random.default_rng(17)
    for na in (1, 2, 3, 5, 17, 33, 64, 65, 129, 200, 255, 256, 257, 300, 513):
        starts = np.sort(rng.choice(100000, na, replace=False)) * 10
        ends = starts + rng.integers(0, 8, na)                            # disjoint: the next start is at least 10 further
        edge = np.r_[starts - 1, starts, ends, ends + 1]
        x = np.r_[edge, rng.integers(-5, 1000020, 3000)]
        y = np.r_[rng.permutation(edge), rng.integers(-5, 1000020, 3000)]
        ch = api.Chromosome(x, y)
        _, nm = _check(ch, x, y, starts, ends, brute=False)
        assert nm == na
        ch.close()


def test_argument_errors():
    from cloops_amd import api, _lib
    lib = _lib.load()
    X, Y = G.chr21_xy()
    ch = api.Chromosome(X, Y)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    s, e = np.array([100, 200], np.int64), np.array([150, 250], np.int64)
    m = np.zeros((len(X) + 63) // 64, np.uint64)
    nm, nk = ctypes.c_int64(0), ctypes.c_int64(0)
    r = lambda *a: lib.cl_anchor_mask(*a)
    E = _lib.CL_ERR_ARG
    assert r(None, 2, vp(s), vp(e), vp(m), ctypes.byref(nm), ctypes.byref(nk)) == E
    assert r(ch._h, 2, vp(s), vp(e), None, ctypes.byref(nm), ctypes.byref(nk)) == E
    assert r(ch._h, 2, vp(s), vp(e), vp(m), None, ctypes.byref(nk)) == E
    assert r(ch._h, 2, vp(s), vp(e), vp(m), ctypes.byref(nm), None) == E
    assert r(ch._h, -1, vp(s), vp(e), vp(m), ctypes.byref(nm), ctypes.byref(nk)) == E
    assert r(ch._h, 2, None, vp(e), vp(m), ctypes.byref(nm), ctypes.byref(nk)) == E
    assert r(ch._h, 2, vp(s), None, vp(m), ctypes.byref(nm), ctypes.byref(nk)) == E
    bad = np.array([100, 300], np.int64)
    assert r(ch._h, 2, vp(bad), vp(e), vp(m), ctypes.byref(nm), ctypes.byref(nk)) == E          # start > end
    assert r(ch._h, 0, None, None, vp(m), ctypes.byref(nm), ctypes.byref(nk)) == 0 and nm.value == 0 and nk.value == 0
    with pytest.raises(ValueError):
        ch.anchor_mask([1, 2], [3])
    # runs in flight
    ch.cluster_async("v2", 2000, 5)
    assert r(ch._h, 2, vp(s), vp(e), vp(m), ctypes.byref(nm), ctypes.byref(nk)) == E
    ch.wait()
    # the handle still works
    _check(ch, X, Y, s, e)
    ch.close()


def test_repeatable_and_two_streams():
    from cloops_amd import api, _lib, cleanpets
    lib = _lib.load()
    X, Y = G.chr21_xy()
    s, e = cleanpets._anchor_pool(_pool("chr21_v2.loop", sig=False))
    s1, s2 = lib.cl_stream_create(0), lib.cl_stream_create(0)
    try:
        a = api.Chromosome(X, Y, stream=s1)
        b = api.Chromosome(X, Y, stream=s2)
        ra = [a.anchor_mask(s, e) for _ in range(3)] + [b.anchor_mask(s[::-1].copy(), e[::-1].copy())]
        for r in ra[1:]:
            assert np.array_equal(r[0], ra[0][0]) and r[1:] == ra[0][1:]
        assert ra[0][1:] == (292, 30225)
        a.close()
        b.close()
    finally:
        lib.cl_stream_destroy(s1)
        lib.cl_stream_destroy(s2)


def test_between_sweep_steps():
    """K13 between two sweep steps on the same handle leaves the steps' results unchanged"""
    from cloops_amd import api
    X, Y = G.chr21_xy()
    rng = np.random.default_rng(3)
    s = rng.integers(X.min(), Y.max(), 8000)                            # beyond the LDS form: the directory is built too
    e = s + rng.integers(0, 2000, 8000)

    def sweep(with_k13):
        ch = api.Chromosome(X, Y)
        ch.set_device_labels(False)
        ch.cand_reset()
        out = []
        for step, (eps, cut) in enumerate(((1000, 0), (2000, 4601), (2000, 13532))):
            ch.step_async("v2", eps, 5, cut, step)
            ch.wait()
            ni, ns, st = ch.step_result()
            out.append((ni, ns, st["n_all"], st["sumx"], st["loghist"].tolist()))
            if with_k13:
                _check(ch, X, Y, s, e, brute=False)
                _check(ch, X, Y, s[:50], e[:50])
        out.append(ch.cand_finish(4601, 100000).tolist())
        ch.close()
        return out
    assert sweep(True) == sweep(False)


def test_module_on_mem_names(tmp_path):
    from cloops_amd import cleanpets, pipe
    X, Y = G.chr21_xy()
    pipe.CACHE.clear()
    f = pipe.CACHE.put_arrays("chr21-chr21", X, Y)
    out = str(tmp_path)
    assert cleanpets.getAnchorPETs(f, _pool("chr21_v2.loop"), out) == (202, 229, len(X), 27072)
    nmat = joblib.load(os.path.join(out, "chr21-chr21.jd"))
    rows = golden_rows("chr21_v2_sig", "chr21", len(X))
    assert np.array_equal(nmat, np.stack([rows, X[rows], Y[rows]], 1))
    pipe.CACHE.clear()


def _io_dirs(root):
    """.jd directories: chr21 written by cloops_amd.io (parseRawBedpe2) from the example BEDPE, synth as [id, X, Y] int64 pickles"""
    from cloops_amd import io as cio
    bed = G.write_example_bedpe(root)
    d = os.path.join(str(root), "chr21")
    os.makedirs(d)
    cio.parseRawBedpe2([bed], d, [], 0)
    return {"chr21": d, "synth": write_jd_dirs(os.path.join(str(root), "s"), {"synth": datasets()["synth"]})["synth"]}


def test_command_line_matches_goldens(tmp_path):
    import subprocess
    import sys
    from cloops_amd import pipe, fingerprint
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dirs = _io_dirs(tmp_path)
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    meta = golden_meta()
    data = datasets()
    for case, loopf, dname, sig, chroms in meta["cases"]:
        out = os.path.join(str(tmp_path), "out_" + case)
        cmd = [sys.executable, "-m", "cloops_amd.cleanpets", "-d", dirs[dname], "-f", os.path.join(GOLD, loopf), "-o", out, "-p", "2"]
        cmd += ([] if sig else ["-s"]) + (["-c", ",".join(chroms)] if chroms else [])
        p = subprocess.run(cmd, env=env, cwd=str(tmp_path), timeout=300, capture_output=True, text=True)
        res = meta["results"][case]
        if "exception" in res:
            assert p.returncode != 0 and "ZeroDivisionError" in p.stderr and os.path.isdir(out)
            continue
        assert p.returncode == 0, p.stderr
        s = res["summary"]
        assert ("loops:%d, anchors:%d,raw PETs: %d, PETs in anchors:%d, ratio:%s" % (s["loops"], s["anchors"], s["raw"], s["kept"], s["ratio"])
                in p.stderr), p.stderr
        assert sorted(os.listdir(out)) == sorted("%s-%s.jd" % (c, c) for c in res["chroms"])
        for chrom in res["chroms"]:
            x, y = data[dname][chrom]
            rows = golden_rows(case, chrom, len(x))
            jd = os.path.join(out, "%s-%s.jd" % (chrom, chrom))
            nmat = joblib.load(jd)
            assert nmat.dtype == np.int64 and np.array_equal(nmat, np.stack([rows, x[rows], y[rows]], 1)), (case, chrom)
            key, mat = pipe.parseJd(jd)                                  # read back unchanged by the other modules
            assert key == (chrom, chrom) and np.array_equal(mat, nmat)
            if len(rows) > 1:
                r = pipe.CACHE.get(jd)
                assert np.array_equal(r.X, x[rows]) and np.array_equal(r.Y, y[rows])
                assert fingerprint.jd2contactMatrixUpper(jd, 0, 2000)[1].sum() > 0
    pipe.CACHE.clear()
