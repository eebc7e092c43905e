#!/usr/bin/env python
"""Golden outputs of scripts/jd2cleanWashuPETs.py.  Build container only:
    python tests/golden/make_golden_cleanpets.py

The script's own functions (preDs, getCorLink, checkAnchorOverlap, mergeAnchor, mergeAllAnchors, getAnchors, getAnchorPETs,
jd2cleanWashuPETs) are sliced out of its parsed source, never its `__main__` block, with parseJd sliced by lines out of
cLoops/io.py (a py2-only module) and parseIv from the converted reference cModel namespace, and exec'd in memory with one patch:
`for chrom in records.keys():` -> `for chrom in list(records.keys()):` (Python 3 raises when preDs deletes a chromosome while
iterating).  `logger` records the messages; Parallel runs with one job.  preDs is called with the anchor columns by header name
(iva / ivb), the columns this project's `.loop` files hold them in.

Datasets: the chr21 example's PETs (chr21_input.npz, ids = row numbers) and a small hand-built set (cleanpets_synth.npz and
cleanpets_synth.loop, made once here and then read back): touching, adjacent-but-separate, nested and duplicate anchors, an iva
overlapping its own ivb, a repeated loopId, non-significant loops, a chromosome without a `.jd`, a `.jd` with zero rows, a `.jd`
without loops, and PETs at s - 1, s, e and e + 1 of every anchor.  Writes data only:
  cleanpets_masks.npz   per case and chromosome the kept rows as an np.packbits mask
  cleanpets_meta.json   per case: the records (loops per chromosome), per-chromosome (loops, merged anchors, raw, kept), the
                        summary numbers of the log line, whether the script's output rows came out ascending, or the exception
"""
import ast
import json
import logging
import os
import sys
import tempfile
from copy import deepcopy

import joblib
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import refload  # noqa: E402
import golden_util as G  # noqa: E402

SYNTH = os.path.join(HERE, "cleanpets_synth.npz")
SYNTH_LOOP = os.path.join(HERE, "cleanpets_synth.loop")

# (loopId, iva, ivb, significant): hand-built so that every merge rule and the edge rows are exercised
SYNTH_LOOPS = [
    ("chrA-chrA-1", ("chrA", 80000, 80500), ("chrA", 85000, 85500), 1),      # replaced by the repeated id below
    ("chrA-chrA-2", ("chrA", 1000, 2000), ("chrA", 2000, 3000), 1),          # iva touches its own ivb: one anchor
    ("chrA-chrA-3", ("chrA", 3001, 3500), ("chrA", 10000, 20000), 1),        # 3001: adjacent to 3000, a separate anchor
    ("chrA-chrA-4", ("chrA", 12000, 13000), ("chrA", 50000, 50100), 1),      # nested in [10000, 20000]
    ("chrA-chrA-5", ("chrA", 50000, 50100), ("chrA", 50000, 50100), 1),      # duplicates
    ("chrA-chrA-6", ("chrA", 70000, 71000), ("chrA", 70500, 72000), 1),      # iva overlaps its own ivb
    ("chrA-chrA-1", ("chrA", 90000, 90500), ("chrA", 95000, 95500), 1),      # repeated loopId: replaces the first
    ("chrA-chrA-7", ("chrA", 100000, 100500), ("chrA", 110000, 110500), 0),  # not significant
    ("chrA-chrA-8", ("chrA", 110500, 110600), ("chrA", 120000, 120000), 0),  # touches the one above; a one-base anchor
    ("chrB-chrB-1", ("chrB", 5000, 6000), ("chrB", 6001, 7000), 1),
    ("chrB-chrB-2", ("chrB", 6500, 6600), ("chrB", 40000, 41000), 1),
    ("chrC-chrC-1", ("chrC", 1000, 2000), ("chrC", 5000, 6000), 1),          # no chrC-chrC.jd
    ("chrE-chrE-1", ("chrE", 300, 400), ("chrE", 900, 1000), 0),             # only non-significant loops
    ("chrZ-chrZ-1", ("chrZ", 100, 200), ("chrZ", 300, 400), 1),              # a .jd with zero rows
]
SYNTH_JD = ("chrA", "chrB", "chrD", "chrE", "chrZ")                        # chrD: a .jd without loops

# (name, loop file, dataset, sig, chroms)
CASES = [
    ("chr21_v2_sig", "chr21_v2.loop", "chr21", True, []),
    ("chr21_v2_all", "chr21_v2.loop", "chr21", False, []),
    ("chr21_v1_sig", "chr21_v1.loop", "chr21", True, []),
    ("synth_sig", "cleanpets_synth.loop", "synth", True, []),
    ("synth_all", "cleanpets_synth.loop", "synth", False, []),
    ("synth_chroms", "cleanpets_synth.loop", "synth", False, ["chrA", "chrC", "chrQ"]),
    ("synth_none", "cleanpets_synth.loop", "synth", True, ["chrC", "chrD"]),    # nothing left: m / 1.0 / n raises
]


def write_synth_loop():
    head = ["loopId", "distance", "ra", "rb", "rab", "ES", "iva", "ivb", "significant"]
    with open(SYNTH_LOOP, "w") as fh:
        fh.write("\t".join(head) + "\n")
        for lid, a, b, sig in SYNTH_LOOPS:
            fh.write("\t".join([lid, "%.1f" % (b[1] - a[1]), "5", "5", "3", "2.0", "%s:%d-%d" % a, "%s:%d-%d" % b, "%.1f" % sig]) + "\n")


def synth():
    """{chrom: (X, Y)} of the hand-built set, made once (fixed seed), then read back"""
    if not os.path.exists(SYNTH):
        rng = np.random.default_rng(20171010)
        out = {}
        for chrom in SYNTH_JD:
            ivs = [iv for _, a, b, _ in SYNTH_LOOPS for iv in (a, b) if iv[0] == chrom]
            xs, ys = [], []
            if chrom != "chrZ":
                for _, s, e in ivs:
                    for v in (s - 1, s, e, e + 1):
                        xs += [v, 5]                       # X at the edge (Y beyond every anchor) ...
                        ys += [500000 + v, v]              # ... and Y at the edge (X before every anchor)
                x = rng.integers(0, 130000, 400)
                y = x + rng.integers(0, 60000, 400)
                xs += x.tolist()
                ys += y.tolist()
            o = rng.permutation(len(xs))
            out["X_" + chrom] = np.asarray(xs, np.int64)[o]
            out["Y_" + chrom] = np.asarray(ys, np.int64)[o]
        np.savez_compressed(SYNTH, **out)
    z = np.load(SYNTH)
    return {k[2:]: (z["X_" + k[2:]].astype(np.int64), z["Y_" + k[2:]].astype(np.int64)) for k in z.files if k.startswith("X_")}


class _Log(object):
    def __init__(self):
        self.msgs = []

    def info(self, m):
        self.msgs.append(("info", m))

    def warning(self, m):
        self.msgs.append(("warning", m))


def script_namespace():
    from joblib import Parallel, delayed
    ns = {"np": np, "os": os, "joblib": joblib, "Parallel": Parallel, "delayed": delayed, "deepcopy": deepcopy, "logger": _Log(),
          "parseIv": refload.ref_cmodel_namespace()["parseIv"]}
    with open(os.path.join(refload.REF_ROOT, "cLoops", "io.py")) as fh:          # py2-only module: its parseJd by lines
        lines = fh.read().split("\n")
    s = [i for i, l in enumerate(lines) if l.startswith("def parseJd(")][0]
    e = [i for i, l in enumerate(lines) if i > s and l.startswith("def ")][0]
    exec(compile("\n".join(lines[s:e]), "io.py:parseJd", "exec"), ns)
    with open(os.path.join(refload.REF_ROOT, "scripts", "jd2cleanWashuPETs.py")) as fh:
        src = fh.read()
    a, b = "for chrom in records.keys():", "for chrom in list(records.keys()):"
    assert a in src
    src = src.replace(a, b)
    want = {"preDs", "getCorLink", "checkAnchorOverlap", "mergeAnchor", "mergeAllAnchors", "getAnchors", "getAnchorPETs",
            "jd2cleanWashuPETs"}
    body = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert len(body) == len(want)
    exec(compile(ast.Module(body=body, type_ignores=[]), "jd2cleanWashuPETs.py:functions", "exec"), ns)
    return ns


def datasets():
    X, Y = G.chr21_xy()
    return {"chr21": {"chr21": (X, Y)}, "synth": synth()}


def main():
    write_synth_loop()
    data = datasets()
    masks, meta = {}, {}
    with tempfile.TemporaryDirectory() as td:
        for name, chroms in data.items():
            os.makedirs(os.path.join(td, name))
            for chrom, (x, y) in chroms.items():
                joblib.dump(np.stack([np.arange(len(x)), x, y], 1).astype(np.int64), os.path.join(td, name, "%s-%s.jd" % (chrom, chrom)))
        for case, loopf, dname, sig, chroms in CASES:
            ns = script_namespace()
            f, d = os.path.join(HERE, loopf), os.path.join(td, dname)
            out = os.path.join(td, "out_" + case)
            os.mkdir(out)
            ch = set(chroms) if chroms else []
            ivac, ivbc = (10, 11) if loopf.startswith("chr21") else (6, 7)
            records = ns["preDs"](f, d, sig, chroms=ch, ivac=ivac, ivbc=ivbc)
            m = {"records": {k: len(v["rs"]) for k, v in sorted(records.items())}, "chroms": {}}
            # jd2cleanWashuPETs with the same records (its own preDs call has no column arguments)
            ns["preDs"], pre_orig = (lambda *a, **k: records), ns["preDs"]
            try:
                ns["jd2cleanWashuPETs"](f, d, sig, out, chroms=ch, cpu=1)
                info = [t for lvl, t in ns["logger"].msgs if lvl == "info"]
                tail = info[-1].split("\t", 1)[1].split(",", 1)[1]
                nums = [t.split(":")[1] for t in tail.replace(", ", ",").split(",")]
                m["summary"] = {"loops": int(nums[0]), "anchors": int(nums[1]), "raw": int(nums[2]), "kept": int(nums[3]),
                                "ratio": float(nums[4])}
            except ZeroDivisionError:
                m["exception"] = "ZeroDivisionError"
            ns["preDs"] = pre_orig
            asc = True
            for chrom in sorted(records):
                nmat = joblib.load(os.path.join(out, "%s-%s.jd" % (chrom, chrom)))
                x, y = data[dname][chrom]
                rows = nmat[:, 0].astype(np.int64)
                assert np.array_equal(nmat[:, 1], x[rows]) and np.array_equal(nmat[:, 2], y[rows]) and nmat.dtype == np.int64
                asc = asc and bool(np.all(np.diff(rows) > 0))
                keep = np.zeros(len(x), bool)
                keep[rows] = True
                masks["%s__%s" % (case, chrom)] = np.packbits(keep)
                anchors = ns["getAnchors"](records[chrom]["rs"])
                m["chroms"][chrom] = {"loops": len(records[chrom]["rs"]), "anchors": len(anchors), "raw": len(x), "kept": int(keep.sum()),
                                      "anchor_list": sorted([int(a), int(b)] for a, b in anchors)}
            m["ascending"] = asc
            m["warnings"] = sum(1 for lvl, _ in ns["logger"].msgs if lvl == "warning")
            meta[case] = m
            print(case, m.get("summary", m.get("exception")), "ascending" if asc else "scrambled")
    np.savez_compressed(os.path.join(HERE, "cleanpets_masks.npz"), **masks)
    with open(os.path.join(HERE, "cleanpets_meta.json"), "w") as fh:
        json.dump({"cases": [list(c[:4]) + [sorted(c[4])] for c in CASES], "results": meta}, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
