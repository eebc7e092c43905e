#!/usr/bin/env python
"""Golden outputs of scripts/quantifyLoops.py and scripts/deLoops on the chr21 example.  Build container only:
    python tests/golden/make_golden_quant.py

The scripts' own functions are sliced out of their parsed source (never their module-level `main()`) and exec'd in a
namespace wired to the converted reference cModel (tests/refload.py:ref_cmodel_namespace: getGenomeCoverage, getCounts,
getPETsforRegions, getNearbyPairRegions in Python-2 integer arithmetic, getBonPvalues); mechanical py2 -> py3 patch:
xrange -> range.  `preDs` is called with ivac=10, ivbc=11: the anchor columns of the `.loop` files this project writes.

Dataset A = the chr21 example's PETs (chr21_input.npz); dataset B = a seeded subsample of them, its kept rows stored as a
bit mask in chr21_quant_subsample.npz.  Writes:
  chr21_quantLoops.txt          quantifyLoops -f chr21_v2.loop -d A -o chr21
  chr21_dis4601_quantLoops.txt  quantifyLoops -f chr21_v2.loop -d B -o chr21_dis4601 -dis 4601
  chr21_A.deloop, chr21_B.deloop  deLoops -fa chr21_v2.loop -fb chr21_v1.loop -da chr21_A -db chr21_B
"""
import ast
import contextlib
import io
import os
import sys
import tempfile

import joblib
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import refload  # noqa: E402
import golden_util as G  # noqa: E402

SUBSAMPLE = os.path.join(HERE, "chr21_quant_subsample.npz")


class _Log(object):
    def info(self, *a):
        pass
    warning = error = info


def script_namespace(relpath, want):
    import pandas as pd
    from joblib import Parallel, delayed
    from scipy.stats import poisson
    cm = refload.ref_cmodel_namespace()
    ns = {"np": np, "pd": pd, "os": os, "poisson": poisson, "Parallel": Parallel, "delayed": delayed, "logger": _Log(),
          "cFlush": lambda *a: None, "parseIv": cm["parseIv"]}
    for name in ("getGenomeCoverage", "getCounts", "getNearbyPairRegions", "getPETsforRegions", "getBonPvalues"):
        ns[name] = cm[name]
    with open(os.path.join(refload.REF_ROOT, relpath)) as fh:
        src = fh.read().replace("xrange", "range")
    tree = ast.parse(src)
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert len(body) == len(want), relpath
    exec(compile(ast.Module(body=body, type_ignores=[]), relpath + ":functions", "exec"), ns)
    return ns


def subsample_rows(n):
    """the kept rows of dataset B: a seeded 60 % of the example's PETs, stored as a bit mask (made once, then read back)"""
    if not os.path.exists(SUBSAMPLE):
        keep = np.random.default_rng(20200119).random(n) < 0.6
        np.savez_compressed(SUBSAMPLE, n=np.int64(n), mask=np.packbits(keep))
    z = np.load(SUBSAMPLE)
    assert int(z["n"]) == n
    return np.flatnonzero(np.unpackbits(z["mask"])[:n])


def main():
    X, Y = G.chr21_xy()
    rows = subsample_rows(len(X))
    q = script_namespace("scripts/quantifyLoops.py", {"preDs", "getPermutatedBg", "estSigOneChr", "quantifyLoops"})
    d = script_namespace("scripts/deLoops", {"preDs", "getPermutatedBg", "estSigOneLoop", "estSigTvsC", "estSigOneChr", "callDeLoops"})
    with tempfile.TemporaryDirectory() as td:
        da, db = os.path.join(td, "chr21_A"), os.path.join(td, "chr21_B")
        for dd, sel in ((da, np.arange(len(X))), (db, rows)):
            os.makedirs(dd)
            joblib.dump(np.stack([sel, X[sel], Y[sel]], 1).astype(np.int64), os.path.join(dd, "chr21-chr21.jd"))
        v2, v1 = os.path.join(HERE, "chr21_v2.loop"), os.path.join(HERE, "chr21_v1.loop")
        with contextlib.redirect_stdout(io.StringIO()):
            q["quantifyLoops"](q["preDs"](v2, da, [], ivac=10, ivbc=11), os.path.join(HERE, "chr21"), 0, 1)
            q["quantifyLoops"](q["preDs"](v2, db, [], ivac=10, ivbc=11), os.path.join(HERE, "chr21_dis4601"), 4601, 1)
            ra = d["preDs"](v2, da, [], ivac=10, ivbc=11)
            rb = d["preDs"](v1, db, [], ivac=10, ivbc=11)
            assert set(ra.keys()) == set(rb.keys()) == {"chr21"}
            d["callDeLoops"](ra, rb, os.path.join(HERE, "chr21_A"), os.path.join(HERE, "chr21_B"), 0, 1)
    for f in ("chr21_quantLoops.txt", "chr21_dis4601_quantLoops.txt", "chr21_A.deloop", "chr21_B.deloop"):
        print(f, sum(1 for _ in open(os.path.join(HERE, f))) - 1, "rows")


if __name__ == "__main__":
    main()
