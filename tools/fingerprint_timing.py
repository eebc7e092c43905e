"""Timing of K12 (cl_contact_hist) and of the fingerprint command path (cloops_amd.fingerprint) on the benchmark genome: the
200 M-PET synthetic genome of bench.py (cloops_amd.synth), resident in HBM, at bin size 2000.

Reports, as one JSON document (stdout, and the file given by --out):
  per chromosome   PETs, non-empty cells, distinct counts, largest count, wall of the first contact_hist call and the median of
                   three more (the whole call: K12's kernels, the sort, the allocation and release of its scratch, the copies)
  whole command    jds2FingerPrint over all chromosomes + the table write of getFingerPrint, chromosomes resident (.jd loading
                   excluded)
  host reference   the script's `for t in mat` dict-of-dicts loop (scripts/jd2fingerprint:32-50, Python-2 floor division)
                   restated on the host over a SAMPLE of one chromosome's rows, its per-PET time extrapolated linearly to all
                   PETs -- labelled as an extrapolation
Kernel times proper come from running this under `rocprofv3 --kernel-trace --stats` (k12_* rows).

    timeout -k 10 1200 python tools/fingerprint_timing.py [--n-total 2e8] [--bs 2000] [--sample 2000000] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def reference_loop(mat, binSize):
    """scripts/jd2fingerprint:32-50 on the rows [id, X, Y] of `mat`, Python-2 integer division"""
    mat = mat[:, 1:]
    minC = np.min(mat)
    ds = {}
    for t in mat:
        nx = (t[0] - minC) // binSize
        ny = (t[1] - minC) // binSize
        if nx not in ds:
            ds[nx] = {}
        if ny not in ds[nx]:
            ds[nx][ny] = 0
        ds[nx][ny] += 1
    nds = []
    for nx in ds.keys():
        for ny in ds[nx].keys():
            nds.append(ds[nx][ny])
    return np.array(nds)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-total", type=float, default=2e8)
    ap.add_argument("--bs", type=int, default=2000)
    ap.add_argument("--sample", type=int, default=2000000, help="rows of the host reference sample")
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    op = ap.parse_args(argv)
    import bench
    import pandas as pd
    from cloops_amd import fingerprint, pipe
    from cloops_amd.synth import chrom_sizes, synth_chrom
    out = {"n_total": int(op.n_total), "bin_size": op.bs}
    t0 = time.perf_counter()
    fs, host = [], {}
    for ci, (name, length, n) in enumerate(chrom_sizes(int(op.n_total))):
        X, Y = synth_chrom(n, length, 1000 * bench.CFG + ci)
        fs.append(pipe.CACHE.put_arrays("%s-%s" % (name, name), X, Y))
        host[fs[-1]] = (name, X, Y)
    out["synthesis_s"] = round(time.perf_counter() - t0, 2)
    per, tot_first, tot_warm = [], 0.0, 0.0
    for f in fs:
        ch = pipe.CACHE.get(f).chrom
        t0 = time.perf_counter()
        v, m, kept, _ = ch.contact_hist(op.bs)
        first = time.perf_counter() - t0
        warm = []
        for _ in range(3):
            t0 = time.perf_counter()
            ch.contact_hist(op.bs)
            warm.append(time.perf_counter() - t0)
        w = float(np.median(warm))
        tot_first += first
        tot_warm += w
        per.append({"chrom": host[f][0], "pets": int(kept), "cells": int(m.sum()), "distinct_counts": int(len(v)),
                    "max_count": int(v.max()), "first_call_s": round(first, 5), "warm_call_s": round(w, 5)})
    out["per_chrom"] = per
    out["pets_total"] = int(sum(p["pets"] for p in per))
    out["cells_total"] = int(sum(p["cells"] for p in per))
    out["k12_first_calls_s_total"] = round(tot_first, 4)
    out["k12_warm_calls_s_total"] = round(tot_warm, 4)
    t0 = time.perf_counter()
    s = fingerprint.jds2FingerPrint(fs, 0, op.bs)
    out["jds2FingerPrint_s"] = round(time.perf_counter() - t0, 3)
    out["groups"] = int(len(s))
    if len(s) == 100:
        with tempfile.TemporaryDirectory() as td:
            t0 = time.perf_counter()
            data = pd.DataFrame({"random": np.linspace(0, 1, 100), "synth": s})
            data.index = np.linspace(0, 1, 100)
            data.to_csv(os.path.join(td, "x_fingerprint.txt"))
            out["table_write_s"] = round(time.perf_counter() - t0, 4)
    # the reference's loop on a sample of the smallest chromosome's rows, extrapolated
    f = min(fs, key=lambda q: len(host[q][1]))
    name, X, Y = host[f]
    k = min(op.sample, len(X))
    mat = np.stack([np.arange(k), X[:k], Y[:k]], 1).astype(np.int64)
    t0 = time.perf_counter()
    nds = reference_loop(mat, op.bs)
    loop_s = time.perf_counter() - t0
    sub = pipe.CACHE.put_arrays("sample-sample", X[:k], Y[:k])
    v, m, _, _ = pipe.CACHE.get(sub).chrom.contact_hist(op.bs)
    same = bool(np.array_equal(np.sort(nds), np.repeat(v, m)))
    out["host_reference_loop"] = {
        "label": "EXTRAPOLATED from a sample: the script's dict-of-dicts loop restated on the host, one core",
        "sample_chrom": name, "sample_rows": int(k), "sample_s": round(loop_s, 2), "per_pet_us": round(loop_s / k * 1e6, 4),
        "counts_equal_k12": same, "extrapolated_all_pets_s": round(loop_s / k * out["pets_total"], 1)}
    pipe.CACHE.clear()
    js = json.dumps(out, indent=1)
    print(js)
    if op.out:
        with open(op.out, "w") as fh:
            fh.write(js)
    return 0


if __name__ == "__main__":
    sys.exit(main())
