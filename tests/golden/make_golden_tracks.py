#!/usr/bin/env python
"""Golden outputs of the browser-track converters of cLoops/io.py (loops2washU, loops2juice, jd2washU, jd2hic).  Build
container only:
    python tests/golden/make_golden_tracks.py

The functions parseJd, loops2washU, parseIv, loops2juice, jd2washU and jd2hic are sliced by lines out of cLoops/io.py (a
py2-only module) and exec'd in memory with these patches:
  - `print <expr>` -> `_ = <expr>` (Python-2 print statements; the text is not part of any output);
  - `callSys([...])` -> `CALLS.append([...])`: the run stops before `bedtools sort` / `bgzip` / `tabix` / `juicer_tools`, and the
    temporary file the loop wrote (named by `random.random()`, in the working directory) is what is kept.
The expected washU file is that temporary text stable-sorted by (chromosome bytes, start, end) -- the order `bedtools sort`
gives, with its open ties pinned to generation order (the order K14 pins).  The expected juice text is the temporary
text itself, the files handed over in sorted name order.

Datasets (`.jd` files of [id, X, Y] int64 rows written here in temporary directories):
  chr21   the chr21 example (chr21_input.npz), ids = row numbers: the sha256 and line count of the texts only
  sub     a seeded 1 500-row subsample of it, ids = the original row numbers
  synth   a hand-built set on three chromosomes (chr10, chr2, chrX: byte order differs from the natural order): equal X across
          rows (ties), X = Y, coordinates at the handle's limit +-(2^29 - 1), ids >= 2^31 and negative ids
Loop files: chr21_v1.loop / chr21_v2.loop rewritten into the reference's column order (tracks_ref_v1.loop / tracks_ref_v2.loop:
loopId ES FDR binomial_p-value distance hypergeometric_p-value iva ivb poisson_p-value ra rab rb significant) and converted with
significant 1 and 0.  Writes tracks_ref_v*.loop, tracks_synth.npz (the synth rows), tracks_texts.npz (every expected text as
uint8, compressed) and tracks_meta.json (cases, line counts, sha256).
"""
import hashlib
import json
import logging
import os
import random
import sys
import tempfile

import joblib
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import refload  # noqa: E402
import golden_util as G  # noqa: E402

LIM = (1 << 29) - 1
WASHU = [("sub", 0, 0), ("sub", 0, 75), ("sub", 0, 10 ** 7), ("sub", 5000, 75), ("synth", 0, 75), ("synth", 0, 0),
         ("synth", 0, -30), ("synth", 0, 10 ** 7), ("synth", 3, 75)]
JUICE = [("sub", 0), ("sub", 5000), ("synth", 0), ("synth", 3)]
FULL = [("washu", "chr21", 0, 75), ("washu", "chr21", 4601, 0), ("juice", "chr21", 0, 0)]
REF_ORDER = ["loopId", "ES", "FDR", "binomial_p-value", "distance", "hypergeometric_p-value", "iva", "ivb", "poisson_p-value",
             "ra", "rab", "rb", "significant"]


def namespace():
    with open(os.path.join(refload.REF_ROOT, "cLoops", "io.py")) as fh:
        lines = fh.read().split("\n")
    out = []
    for name in ("parseJd", "loops2washU", "parseIv", "loops2juice", "jd2washU", "jd2hic"):
        s = [i for i, l in enumerate(lines) if l.startswith("def %s(" % name)][0]
        e = [i for i, l in enumerate(lines) if i > s and l.startswith("def ")] + [len(lines)]
        out += lines[s:e[0]]
    src = "\n".join(out)
    n_print = src.count("print ")
    src = src.replace("print ", "_ = ")
    assert n_print == 6, n_print
    assert src.count("callSys(") == 2
    src = src.replace("callSys(", "CALLS.append(")
    ns = {"np": np, "os": os, "joblib": joblib, "random": random, "CALLS": []}
    exec(compile(src, "cLoops/io.py:converters", "exec"), ns)
    return ns


def synth():
    """{chrom: (ids, X, Y)}"""
    big = 1 << 31
    return {
        "chr2": (np.array([5, 6, 7, 8, 9, -1, big, -big - 5], np.int64),
                 np.array([100, 100, 100, 40, 40, 0, 7, 100], np.int64),
                 np.array([300, 250, 300, 40, 140, 0, 7, 100], np.int64)),
        "chr10": (np.array([0, 1, 2, 3, (1 << 62) + 3], np.int64),
                  np.array([-LIM, -LIM, 0, LIM, -5], np.int64),
                  np.array([LIM, -LIM, LIM, LIM, 70], np.int64)),
        "chrX": (np.array([-(1 << 63), (1 << 63) - 1, 11], np.int64),
                 np.array([10, 20, 10], np.int64),
                 np.array([20, 20, 10], np.int64)),
    }


def datasets():
    X, Y = G.chr21_xy()
    X = np.asarray(X, np.int64)
    Y = np.asarray(Y, np.int64)
    rng = np.random.default_rng(14)
    rows = np.sort(rng.choice(len(X), 1500, replace=False))
    return {"chr21": {"chr21": (np.arange(len(X), dtype=np.int64), X, Y)},
            "sub": {"chr21": (rows.astype(np.int64), X[rows], Y[rows])},
            "synth": synth()}


def write_dir(root, chroms):
    os.makedirs(root)
    fs = []
    for c, (i, x, y) in chroms.items():
        f = os.path.join(root, "%s-%s.jd" % (c, c))
        joblib.dump(np.stack([i, x, y], 1).astype(np.int64), f)
        fs.append(f)
    return sorted(fs)


def washu_sort(text):
    lines = text.split("\n")[:-1]
    keyed = [(l.split("\t")[0].encode(), int(l.split("\t")[1]), int(l.split("\t")[2])) for l in lines]
    order = sorted(range(len(lines)), key=lambda k: keyed[k])         # stable: ties keep generation order
    return "".join(lines[k] + "\n" for k in order)


def run_ref(ns, fn, *args):
    """fn writes its temporary text into the working directory and stops before callSys -> that text"""
    with tempfile.TemporaryDirectory() as td:
        cwd = os.getcwd()
        os.chdir(td)
        try:
            ns["CALLS"].clear()
            fn(*args)
            tmp = ns["CALLS"][0][0].split()[-3] if fn is ns["jd2washU"] else ns["CALLS"][0][0].split("-d ")[1].split()[0]
            with open(tmp) as fh:
                return fh.read()
        finally:
            os.chdir(cwd)


def sha(t):
    return hashlib.sha256(t.encode()).hexdigest()


def main():
    ns = namespace()
    data = datasets()
    texts, meta = {}, {"washu": [], "juice": [], "full": [], "loops": []}
    with tempfile.TemporaryDirectory() as td:
        dirs = {name: write_dir(os.path.join(td, name), chroms) for name, chroms in data.items()}
        for d, cut, ext in WASHU:
            name = "washu__%s__%d__%d" % (d, cut, ext)
            t = washu_sort(run_ref(ns, ns["jd2washU"], dirs[d], "out.txt", cut, ext))
            texts[name] = np.frombuffer(t.encode(), np.uint8)
            meta["washu"].append({"name": name, "data": d, "cut": cut, "ext": ext, "lines": t.count("\n"), "sha256": sha(t)})
        for d, cut in JUICE:
            name = "juice__%s__%d" % (d, cut)
            t = run_ref(ns, ns["jd2hic"], dirs[d], "out.hic", cut, "hg38", "1000,5000")
            texts[name] = np.frombuffer(t.encode(), np.uint8)
            meta["juice"].append({"name": name, "data": d, "cut": cut, "lines": t.count("\n"), "sha256": sha(t)})
        for kind, d, cut, ext in FULL:
            if kind == "washu":
                t = washu_sort(run_ref(ns, ns["jd2washU"], dirs[d], "out.txt", cut, ext))
            else:
                t = run_ref(ns, ns["jd2hic"], dirs[d], "out.hic", cut, "hg38", "1000,5000")
            meta["full"].append({"kind": kind, "data": d, "cut": cut, "ext": ext, "lines": t.count("\n"), "sha256": sha(t),
                                 "bytes": len(t.encode())})
    lg = logging.getLogger("make_golden_tracks")
    for v in ("v1", "v2"):
        src = os.path.join(HERE, "chr21_%s.loop" % v)
        ref = os.path.join(HERE, "tracks_ref_%s.loop" % v)
        rows = [l.split("\n")[0].split("\t") for l in open(src)]
        head = rows[0]
        idx = [head.index(c) for c in REF_ORDER]
        with open(ref, "w") as fh:
            for r in rows:
                fh.write("\t".join(r[k] for k in idx) + "\n")
        for sig in (1, 0):
            with tempfile.TemporaryDirectory() as td:
                w, j = os.path.join(td, "w.txt"), os.path.join(td, "j.txt")
                ns["loops2washU"](ref, w, lg, sig)
                ns["loops2juice"](ref, j, lg, sig)
                for kind, f in (("loops2washU", w), ("loops2juice", j)):
                    name = "%s__%s__%d" % (kind, v, sig)
                    t = open(f).read()
                    texts[name] = np.frombuffer(t.encode(), np.uint8)
                    meta["loops"].append({"name": name, "loop": "chr21_%s.loop" % v, "ref_loop": os.path.basename(ref),
                                          "kind": kind, "significant": sig, "lines": t.count("\n"), "sha256": sha(t)})
    s = synth()
    np.savez_compressed(os.path.join(HERE, "tracks_synth.npz"), **{"%s__%s" % (k, c): v[n] for c, v in s.items()
                                                                  for n, k in enumerate(("ids", "X", "Y"))})
    np.savez_compressed(os.path.join(HERE, "tracks_texts.npz"), **texts)
    meta["sub_rows"] = datasets()["sub"]["chr21"][0].tolist()
    with open(os.path.join(HERE, "tracks_meta.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
    print("wrote", len(texts), "texts")


if __name__ == "__main__":
    main()
