"""GPU: kernel K14 (cl_track_build / cl_track_chunks / cl_track_render) against the brute-force renderer of test_tracks.py on the
goldens and on edge cases, chunking, determinism, argument errors, its effect on a sweep (none), and the command lines
(python -m cloops_amd.tracks, python -m cloops_amd -w -j)."""
import ctypes
import hashlib
import os
import subprocess
import sys

import joblib
import numpy as np
import pytest

import golden_util as G
from test_tracks import GOLD, brute_text, datasets, golden_meta, golden_text, write_jd_dirs

pytestmark = pytest.mark.gpu

LIM = (1 << 29) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def render(ch, kind, cut, ext, ids, key=("c", "c"), budget=None):
    """K14 text of a resident chromosome: one render per chunk, every chunk ending at a newline -> bytes"""
    nr, nb = ch.track_build(kind, cut, ext, ids, key[0], key[1])
    rec, byt = ch.track_chunks(budget or ch.TRACK_BUDGET)
    parts = [ch.track_render(k) for k in range(len(rec) - 1)]
    assert all(p.endswith(b"\n") and len(p) > 0 for p in parts)
    if budget:
        assert all(len(p) <= budget for p in parts)
    t = b"".join(parts)
    assert len(t) == nb and t.count(b"\n") == nr and byt[-1] == nb and rec[-1] == nr
    return t


def test_goldens_vs_brute():
    from cloops_amd import api
    data = datasets()
    meta = golden_meta()
    for g in meta["washu"] + meta["juice"]:
        kind = "washu" if g in meta["washu"] else "juice"
        chroms = data[g["data"]]
        out = []
        for c in sorted(chroms, key=str.encode) if kind == "washu" else sorted(chroms):
            i, x, y = chroms[c]
            ch = api.Chromosome(x, y)
            ext = g.get("ext", 0)
            t = render(ch, kind, g["cut"], ext, i, (c, c))
            assert t == brute_text(kind, (c, c), i, x, y, g["cut"], ext), (g["name"], c)
            assert render(ch, kind, g["cut"], ext, i, (c, c), budget=300) == t
            ch.close()
            out.append(t)
        assert b"".join(out) == golden_text(g["name"]), g["name"]
    i, x, y = data["chr21"]["chr21"]
    ch = api.Chromosome(x, y)
    for g in meta["full"]:
        t = render(ch, g["kind"], g["cut"], g["ext"], None if g["kind"] == "juice" else i, ("chr21", "chr21"), budget=1 << 20)
        assert t.count(b"\n") == g["lines"] and hashlib.sha256(t).hexdigest() == g["sha256"], g
    ch.close()


def test_edges():
    from cloops_amd import api
    rng = np.random.default_rng(12)
    # one PET; nothing left after the cut; ids None = the row numbers
    ch = api.Chromosome(np.array([5]), np.array([9]))
    for kind in ("washu", "juice"):
        assert render(ch, kind, 0, 3, None) == brute_text(kind, ("c", "c"), [0], [5], [9], 0, 3)
        assert ch.track_build(kind, 5, 3, None, "c", "c") == (0, 0)
        rec, byt = ch.track_chunks(1000)
        assert rec.tolist() == [0] and byt.tolist() == [0]
    ch.close()
    # tile tails of the filter (2048 rows) and of the render (256 lines), a cut, int64 ids, the coordinate limit
    for n in (1, 63, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 4097):
        x = rng.integers(-LIM, LIM - 200000, n)
        y = x + rng.integers(0, 200000, n)
        x[: n // 7] = -LIM
        y[: n // 11] = LIM
        ids = rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64)
        ch = api.Chromosome(x, y)
        for kind, cut, ext in (("washu", 0, 75), ("washu", 50000, 0), ("washu", 0, -(1 << 40)), ("washu", 0, 1 << 40),
                               ("juice", 0, 0), ("juice", 50000, 0)):
            want = brute_text(kind, ("chrA_long_name", "chrA_long_name"), ids, x, y, cut, ext)
            assert render(ch, kind, cut, ext, ids, ("chrA_long_name", "chrA_long_name")) == want, (n, kind, cut, ext)
            assert render(ch, kind, cut, ext, ids, ("chrA_long_name", "chrA_long_name"), budget=700) == want, (n, kind, cut, ext)
        ch.close()
    # names of CL_TRACK_NAME_MAX bytes: the longest lines the template allows, at the smallest budget
    nm = "n" * 64
    x = np.array([-LIM, 0, LIM]); y = np.array([LIM, LIM, LIM])
    ids = np.array([-(1 << 63), 0, (1 << 63) - 1], np.int64)
    ch = api.Chromosome(x, y)
    ext = -(1 << 62)
    want = brute_text("washu", (nm, nm), ids, x, y, 0, ext)
    assert render(ch, "washu", 0, ext, ids, (nm, nm), budget=2 * 64 + 111) == want
    ch.close()


def test_many_chunks():
    """several million PETs, a 1 MiB budget: the chunks concatenated equal one render; a sample of lines against the brute force"""
    from cloops_amd import api
    rng = np.random.default_rng(3)
    n = 3000000
    x = rng.integers(0, 248000000, n)
    y = np.minimum(x + rng.integers(0, 2000000, n), LIM)
    x[::97] = x[5]                                                      # ties
    ids = np.arange(n, dtype=np.int64) * 3 + (1 << 33)
    ch = api.Chromosome(x, y)
    one = render(ch, "washu", 1000, 75, ids, ("chr1", "chr1"), budget=1 << 31)
    many = render(ch, "washu", 1000, 75, ids, ("chr1", "chr1"), budget=1 << 20)
    assert many == one
    rec, byt = ch.track_chunks(1 << 20)
    assert len(rec) > 100 and np.all(np.diff(byt) <= 1 << 20)
    # sampled lines: the pinned order from numpy
    keep = np.flatnonzero(y - x >= 1000)
    p = np.stack([x[keep], y[keep]], 1).ravel()
    order = np.lexsort((np.arange(len(p)), p))
    lines = one.split(b"\n")[:-1]
    assert len(lines) == len(p)
    for j in np.r_[0, len(p) - 1, rng.integers(0, len(p), 300)]:
        g = order[j]
        r, side = keep[g >> 1], g & 1
        pp, qq = (x[r], y[r]) if side == 0 else (y[r], x[r])
        want = "chr1\t%d\t%d\tchr1:%d-%d,1\t%d\t.\n" % (max(0, pp - 75), pp + 75, max(0, qq - 75), qq + 75, ids[r])
        assert lines[j] + b"\n" == want.encode(), j
    # the double-buffered iterator gives the same bytes
    ch.track_build("washu", 1000, 75, ids, "chr1", "chr1")
    assert b"".join(bytes(m) for m in ch.track_iter(1 << 20)) == one
    ch.close()


def test_repeatable_and_two_streams():
    from cloops_amd import api, _lib
    lib = _lib.load()
    i, x, y = datasets()["chr21"]["chr21"]
    s1, s2 = lib.cl_stream_create(0), lib.cl_stream_create(0)
    try:
        a = api.Chromosome(x, y, stream=s1)
        b = api.Chromosome(x, y, stream=s2)
        ra = [render(a, "washu", 0, 75, i, ("chr21", "chr21"), budget=1 << 18) for _ in range(3)]
        rb = render(b, "washu", 0, 75, i, ("chr21", "chr21"), budget=1 << 16)
        assert ra[0] == ra[1] == ra[2] == rb
        assert render(a, "juice", 0, 0, None, ("chr21", "chr21")) == render(b, "juice", 0, 0, i, ("chr21", "chr21"))
        a.track_free()
        a.close()
        b.close()
    finally:
        lib.cl_stream_destroy(s1)
        lib.cl_stream_destroy(s2)


def test_argument_errors():
    from cloops_amd import api, _lib
    lib = _lib.load()
    i, x, y = datasets()["sub"]["chr21"]
    ch = api.Chromosome(x, y)
    E = _lib.CL_ERR_ARG
    nr, nb, nc = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    r = ctypes.byref
    b = lambda *a: lib.cl_track_build(*a)
    assert b(None, 0, 0, 75, None, b"c", b"c", r(nr), r(nb)) == E
    assert b(ch._h, 0, 0, 75, None, b"c", b"c", None, r(nb)) == E
    assert b(ch._h, 0, 0, 75, None, b"c", b"c", r(nr), None) == E
    assert b(ch._h, 0, 0, 75, None, None, b"c", r(nr), r(nb)) == E
    assert b(ch._h, 2, 0, 75, None, b"c", b"c", r(nr), r(nb)) == E                       # unknown kind
    assert b(ch._h, -1, 0, 75, None, b"c", b"c", r(nr), r(nb)) == E
    assert b(ch._h, 0, -1, 75, None, b"c", b"c", r(nr), r(nb)) == E                      # cut < 0
    assert b(ch._h, 0, 0, 75, None, b"c" * 65, b"c", r(nr), r(nb)) == E                  # name too long
    assert b(ch._h, 0, 0, 75, None, b"c" * 64, b"c" * 64, r(nr), r(nb)) == 0
    assert lib.cl_track_chunks(None, 1 << 20, 0, None, None, r(nc)) == E
    assert lib.cl_track_chunks(ch._h, 1 << 20, 0, None, None, None) == E
    assert lib.cl_track_chunks(ch._h, 2 * 64 + 110, 0, None, None, r(nc)) == E           # budget below the longest line
    assert lib.cl_track_chunks(ch._h, 1 << 20, 0, None, None, r(nc)) == 0 and nc.value == 1
    bnd = np.zeros(2, np.int64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.cl_track_chunks(ch._h, 1 << 20, 1, vp(bnd), vp(bnd), r(nc)) == E           # cap below chunks + 1
    out = np.zeros(1 << 20, np.uint8)
    assert lib.cl_track_render(None, 0, vp(out), len(out), r(nb)) == E
    assert lib.cl_track_render(ch._h, 1, vp(out), len(out), r(nb)) == E                  # chunk index out of range
    assert lib.cl_track_render(ch._h, -1, vp(out), len(out), r(nb)) == E
    assert lib.cl_track_render(ch._h, 0, None, len(out), r(nb)) == E
    assert lib.cl_track_render(ch._h, 0, vp(out), 10, r(nb)) == E                        # capacity below the chunk
    assert lib.cl_track_render(ch._h, 0, vp(out), len(out), r(nb)) == 0 and nb.value > 0
    assert lib.cl_track_free(None) == E
    assert lib.cl_track_free(ch._h) == 0
    assert lib.cl_track_chunks(ch._h, 1 << 20, 0, None, None, r(nc)) == E                # nothing built any more
    assert lib.cl_track_render(ch._h, 0, vp(out), len(out), r(nb)) == E
    with pytest.raises(ValueError):
        ch.track_build("bed", 0, 0, None, "c", "c")
    # runs in flight
    ch.cluster_async("v2", 2000, 5)
    assert b(ch._h, 0, 0, 75, None, b"c", b"c", r(nr), r(nb)) == E
    ch.wait()
    assert render(ch, "washu", 0, 75, i, ("chr21", "chr21")) == brute_text("washu", ("chr21", "chr21"), i, x, y, 0, 75)
    ch.close()


def test_between_sweep_steps():
    """K14 between two sweep steps on the same handle leaves the steps' results unchanged"""
    from cloops_amd import api
    X, Y = G.chr21_xy()

    def sweep(with_k14):
        ch = api.Chromosome(X, Y)
        ch.set_device_labels(False)
        ch.cand_reset()
        out = []
        for step, (eps, cut) in enumerate(((1000, 0), (2000, 4601), (2000, 13532))):
            ch.step_async("v2", eps, 5, cut, step)
            ch.wait()
            ni, ns, st = ch.step_result()
            out.append((ni, ns, st["n_all"], st["sumx"], st["loghist"].tolist()))
            if with_k14:
                render(ch, "washu", cut, 75, None, budget=1 << 16)
                render(ch, "juice", 0, 0, None)
        out.append(ch.cand_finish(4601, 100000).tolist())
        ch.close()
        return out
    assert sweep(True) == sweep(False)


def _env():
    return dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))


def test_command_line_on_io_and_cleanpets_dirs(tmp_path):
    from cloops_amd import io as cio
    bed = G.write_example_bedpe(tmp_path)
    d = str(tmp_path / "chr21")
    os.makedirs(d)
    cio.parseRawBedpe2([bed], d, [], 0)
    meta = golden_meta()
    for g in meta["full"]:
        pre = str(tmp_path / ("full_%s_%d" % (g["kind"], g["cut"])))
        cmd = [sys.executable, "-m", "cloops_amd.tracks", g["kind"], "-d", d, "-o", pre, "-cut", str(g["cut"])]
        cmd += ["-ext", str(g["ext"])] if g["kind"] == "washu" else ["-org", "hg38"]
        p = subprocess.run(cmd, env=dict(_env(), PATH="/usr/bin:/bin"), cwd=str(tmp_path), timeout=300, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        out = pre + ("_PETs_washU.txt" if g["kind"] == "washu" else "_juice.txt")
        t = open(out, "rb").read()
        assert t.count(b"\n") == g["lines"] and hashlib.sha256(t).hexdigest() == g["sha256"], g
    # synth and the subsample as .jd directories
    dirs = write_jd_dirs(tmp_path / "gold", {k: v for k, v in datasets().items() if k != "chr21"})
    for g in meta["washu"] + meta["juice"]:
        kind = "washu" if g in meta["washu"] else "juice"
        pre = str(tmp_path / g["name"])
        cmd = [sys.executable, "-m", "cloops_amd.tracks", kind, "-d", dirs[g["data"]], "-o", pre, "-cut", str(g["cut"])]
        cmd += ["-ext", str(g["ext"])] if kind == "washu" else ["-org", "hg38"]
        p = subprocess.run(cmd, env=dict(_env(), PATH="/usr/bin:/bin"), cwd=str(tmp_path), timeout=300, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        out = pre + ("_PETs_washU.txt" if kind == "washu" else "_juice.txt")
        assert open(out, "rb").read() == golden_text(g["name"]), g["name"]
    # the .jd directory cloops_amd.cleanpets writes
    clean = str(tmp_path / "clean")
    p = subprocess.run([sys.executable, "-m", "cloops_amd.cleanpets", "-d", d, "-f", os.path.join(GOLD, "chr21_v2.loop"), "-o", clean],
                       env=_env(), cwd=str(tmp_path), timeout=300, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    pre = str(tmp_path / "clean_tracks")
    p = subprocess.run([sys.executable, "-m", "cloops_amd.tracks", "washu", "-d", clean, "-o", pre],
                       env=dict(_env(), PATH="/usr/bin:/bin"), cwd=str(tmp_path), timeout=300, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    mat = joblib.load(os.path.join(clean, "chr21-chr21.jd"))
    assert open(pre + "_PETs_washU.txt", "rb").read() == brute_text("washu", ("chr21", "chr21"), mat[:, 0], mat[:, 1], mat[:, 2], 0, 75)


def test_mem_names(tmp_path):
    from cloops_amd import pipe, tracks
    i, x, y = datasets()["sub"]["chr21"]
    pipe.CACHE.clear()
    f = pipe.CACHE.put_arrays("chr21-chr21", x, y)
    out = str(tmp_path / "m.txt")
    tracks.jd2washU([f], out, 0, 75)
    assert open(out, "rb").read() == brute_text("washu", ("chr21", "chr21"), np.arange(len(x)), x, y, 0, 75)
    pipe.CACHE.clear()


def test_pipe_w_j(tmp_path):
    """python -m cloops_amd ... -w -j: the loop tracks of <o>.loop; <o>.loop as without the flags"""
    from cloops_amd import tracks
    bed = G.write_example_bedpe(tmp_path)
    outs = {}
    for tag, extra in (("plain", []), ("wj", ["-w", "-j"])):
        o = str(tmp_path / tag)
        p = subprocess.run([sys.executable, "-m", "cloops_amd", "-f", bed, "-o", o, "-m", "1"] + extra, env=_env(), cwd=str(tmp_path),
                           timeout=600, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        outs[tag] = o
    assert open(outs["plain"] + ".loop").read() == open(outs["wj"] + ".loop").read()
    assert not os.path.exists(outs["plain"] + "_loops_washU.txt") and not os.path.exists(outs["plain"] + "_loops_juicebox.txt")
    tracks.loops2washU(outs["wj"] + ".loop", str(tmp_path / "w.txt"))
    tracks.loops2juice(outs["wj"] + ".loop", str(tmp_path / "j.txt"))
    assert open(outs["wj"] + "_loops_washU.txt").read() == open(str(tmp_path / "w.txt")).read()
    assert open(outs["wj"] + "_loops_juicebox.txt").read() == open(str(tmp_path / "j.txt")).read()
    assert not os.path.isdir(outs["wj"])                                  # the working directory is removed after the tracks
    if open(outs["wj"] + ".loop").read() == open(os.path.join(GOLD, "chr21_v2.loop")).read():
        assert open(outs["wj"] + "_loops_washU.txt", "rb").read() == golden_text("loops2washU__v2__1")
        assert open(outs["wj"] + "_loops_juicebox.txt", "rb").read() == golden_text("loops2juice__v2__1")
