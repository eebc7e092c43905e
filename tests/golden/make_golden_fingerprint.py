#!/usr/bin/env python
"""Golden outputs of scripts/jd2fingerprint.  Build container only:
    python tests/golden/make_golden_fingerprint.py

The script's own functions (jd2contactMatrixUpper, contactMatrixUpper2Bins, jds2FingerPrint, getFingerPrint) are sliced out
of its parsed source, never its `__main__` block, with parseJd sliced by lines out of cLoops/io.py (a py2-only module), and exec'd in memory
with these patches (the script is Python 2; its Python-2 integer arithmetic is what is pinned):
  - `xrange` -> `range`;
  - `/` -> `//` at the two cell lines (`(t[0] - minC) / binSize`, `(t[1] - minC) / binSize`) and at `step = len(ds) / bins`;
  - `logger` = a logging logger (the script's is a module global set up by its main).
plotFingerPrint is a no-op (plot = 0); Parallel runs with one job.

Datasets: A = the chr21 example's PETs (chr21_input.npz); B = its seeded subsample (chr21_quant_subsample.npz, made by
make_golden_quant.py); C = a small seeded two-chromosome set with heavy duplicate cells (fingerprint_setC.npz, made once here
and then read back), so the genome-wide concatenation is covered.  Writes:
  fp_labels_fingerprint.txt   getFingerPrint("chr21_A,chr21_B,synth_C", "A,B,C", bs 2000)
  fp_bs10000_fingerprint.txt  getFingerPrint("chr21_A,chr21_B,synth_C", "", bs 10000)  (default labels: the directory names)
  fingerprint_arrays.npz      per dataset and bs in BIN_SIZES (and bs 2000 under cut 4601): the sorted counts of the cells
                              (jd2contactMatrixUpper of every .jd, concatenated) and the group vector (contactMatrixUpper2Bins)
  fingerprint_meta.json       the exception type of getFingerPrint where the script raises (112 groups for A at bs 1e6,
                              step 0 for C at bs 1e6)
"""
import ast
import contextlib
import io
import json
import logging
import os
import sys
import tempfile

import joblib
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import refload  # noqa: E402
import golden_util as G  # noqa: E402

SETC = os.path.join(HERE, "fingerprint_setC.npz")
BIN_SIZES = (1, 500, 2000, 10000, 1000000)
CUT = 4601
DIRS = ("chr21_A", "chr21_B", "synth_C")


def _functions(relpath, want, patches=()):
    with open(os.path.join(refload.REF_ROOT, relpath)) as fh:
        src = fh.read()
    for a, b in patches:
        assert a in src, (relpath, a)
        src = src.replace(a, b)
    tree = ast.parse(src)
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert len(body) == len(want), relpath
    return ast.Module(body=body, type_ignores=[])


def script_namespace():
    import pandas as pd
    from glob import glob
    from joblib import Parallel, delayed
    ns = {"np": np, "pd": pd, "os": os, "glob": glob, "joblib": joblib, "Parallel": Parallel, "delayed": delayed,
          "logger": logging.getLogger("jd2fingerprint"), "plotFingerPrint": lambda *a: None}
    with open(os.path.join(refload.REF_ROOT, "cLoops", "io.py")) as fh:          # py2-only module: its parseJd by lines
        lines = fh.read().split("\n")
    s = [i for i, l in enumerate(lines) if l.startswith("def parseJd(")][0]
    e = [i for i, l in enumerate(lines) if i > s and l.startswith("def ")][0]
    exec(compile("\n".join(lines[s:e]), "io.py:parseJd", "exec"), ns)
    patches = (("xrange", "range"),
               ("nx = (t[0] - minC) / binSize", "nx = (t[0] - minC) // binSize"),
               ("ny = (t[1] - minC) / binSize", "ny = (t[1] - minC) // binSize"),
               ("step = len(ds) / bins", "step = len(ds) // bins"))
    want = {"jd2contactMatrixUpper", "contactMatrixUpper2Bins", "jds2FingerPrint", "getFingerPrint"}
    exec(compile(_functions("scripts/jd2fingerprint", want, patches), "jd2fingerprint:functions", "exec"), ns)
    return ns


def set_c():
    """dataset C: {chrom: (X, Y)} -- two chromosomes drawn from a few anchor positions (heavy duplicate cells, one cell of
    3000 identical PETs beyond the GPU's LDS histogram range), made once with a fixed seed, then read back"""
    if not os.path.exists(SETC):
        rng = np.random.default_rng(20171012)
        out = {}
        for chrom, base, npos, n in (("chrC1", 1000000, 400, 12000), ("chrC2", 50000000, 250, 8300)):
            pos = base + np.sort(rng.choice(600000, npos, replace=False))
            w = 1.0 / np.arange(1, npos + 1) ** 0.8
            a = rng.choice(npos, n, p=w / w.sum())
            b = rng.choice(npos, n, p=w / w.sum())
            x, y = np.minimum(pos[a], pos[b]), np.maximum(pos[a], pos[b])
            jit = rng.integers(0, 3000, (2, n))
            x, y = x + jit[0] * (rng.random(n) < 0.5), y + jit[1] * (rng.random(n) < 0.5)
            out["X_" + chrom], out["Y_" + chrom] = x.astype(np.int32), np.maximum(x, y).astype(np.int32)
        out["X_chrC1"][:3000] = base_dup = 1234567
        out["Y_chrC1"][:3000] = base_dup + 50000
        np.savez_compressed(SETC, **out)
    z = np.load(SETC)
    return {k[2:]: (z["X_" + k[2:]].astype(np.int64), z["Y_" + k[2:]].astype(np.int64)) for k in z.files if k.startswith("X_")}


def datasets():
    """{dir name: {chrom: (X, Y)}} of A, B, C"""
    X, Y = G.chr21_xy()
    zs = np.load(os.path.join(HERE, "chr21_quant_subsample.npz"))
    rows = np.flatnonzero(np.unpackbits(zs["mask"])[:int(zs["n"])])
    return {"chr21_A": {"chr21": (X, Y)}, "chr21_B": {"chr21": (X[rows], Y[rows])}, "synth_C": set_c()}


def write_jd_dirs(root, data):
    for d, chroms in data.items():
        os.makedirs(os.path.join(root, d))
        for chrom, (x, y) in chroms.items():
            mat = np.stack([np.arange(len(x)), x, y], 1).astype(np.int64)
            joblib.dump(mat, os.path.join(root, d, "%s-%s.jd" % (chrom, chrom)))


def main():
    ns = script_namespace()
    data = datasets()
    arrays, meta = {}, {"bin_sizes": list(BIN_SIZES), "cut": CUT, "dirs": list(DIRS), "raises": {}}
    with tempfile.TemporaryDirectory() as td:
        write_jd_dirs(td, data)
        dirs = ",".join(os.path.join(td, d) for d in DIRS)
        for name in DIRS:
            jds = sorted(ns["glob"](os.path.join(td, name, "*.jd")))
            for bs, cut, tag in [(bs, 0, "bs%d" % bs) for bs in BIN_SIZES] + [(2000, CUT, "bs2000_cut%d" % CUT)]:
                ds = np.concatenate([ns["jd2contactMatrixUpper"](jd, cut, bs) for jd in jds])
                ds.sort()
                arrays["counts_%s_%s" % (name, tag)] = ds.astype(np.int64)
                try:
                    arrays["groups_%s_%s" % (name, tag)] = ns["contactMatrixUpper2Bins"](ds.copy(), 100)
                except Exception as e:                       # step 0
                    meta["raises"]["groups_%s_%s" % (name, tag)] = type(e).__name__
                g = ns["jds2FingerPrint"](jds, cut, bs, 1, 100) if "groups_%s_%s" % (name, tag) in arrays else None
                if g is not None:
                    assert np.array_equal(g, arrays["groups_%s_%s" % (name, tag)])
        with contextlib.redirect_stdout(io.StringIO()):
            ns["getFingerPrint"](dirs, "A,B,C", os.path.join(HERE, "fp_labels"), binSize=2000, cpu=1, plot=0)
            ns["getFingerPrint"](dirs, "", os.path.join(HERE, "fp_bs10000"), binSize=10000, cpu=1, plot=0)
            for name in ("chr21_A", "synth_C"):
                try:
                    ns["getFingerPrint"](os.path.join(td, name), "", os.path.join(td, "x"), binSize=1000000, cpu=1, plot=0)
                    meta["raises"]["getFingerPrint_%s_bs1000000" % name] = None
                except Exception as e:
                    meta["raises"]["getFingerPrint_%s_bs1000000" % name] = type(e).__name__
                assert not os.path.exists(os.path.join(td, "x_fingerprint.txt"))
    np.savez_compressed(os.path.join(HERE, "fingerprint_arrays.npz"), **arrays)
    with open(os.path.join(HERE, "fingerprint_meta.json"), "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for k in sorted(arrays):
        if k.startswith("counts"):
            g = arrays.get(k.replace("counts", "groups"))
            print(k, len(arrays[k]), "cells, max", arrays[k].max(), "groups", None if g is None else len(g))
    print(json.dumps(meta["raises"]))


if __name__ == "__main__":
    main()
