"""Timing of K29 (cl_dot_lambdas, cl_dot_hist) on synthetic cells at two shapes (nb, dmax, p, w): (25 000, 200, 2, 5) and (50 000, 400,
4, 7).

The PETs are made from a seed: 400 per bin of 1 kb, X uniform, Y - X log-uniform from half a bin to 1.2 dmax bins, those beyond the
window dropped; raw mode, every bin valid, K26's smoothed expected values, dmin = p + 2, the 40 default edges.  Reports, as one JSON
document (stdout, and --out, by default profiles/dots_timing.json), in wall clock (the calls are synchronous):
  lambdas_s, hist_s   one cl_dot_lambdas (two clears, k29_fill, k29_lambdas, the host's check of the expected values) and one cl_dot_hist
                      (k29_hist and the copy of the histogram to the host): medians of --reps after two warm-up calls
  lds_bytes           what the walks of k29_lambdas read from LDS: 2 ((2w+1)^2 - (2p+1)^2) reads of 8 bytes per candidate pixel
  kernel              with --kernel-trace DIR: the median durations of k29_fill, k29_lambdas and k29_hist from a rocprofv3 kernel
                      trace of `--trace-only` (a run of its own)

    timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/dots_bench.py --trace-only
    timeout -k 10 300 python tools/dots_bench.py --kernel-trace DIR [--reps 5] [--out FILE]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

CASES = ((25000, 200, 2, 5), (50000, 400, 4, 7))
RES, PER_BIN, CHUNKS = 1000, 400, 40
KERNELS = ("k29_fill", "k29_lambdas", "k29_hist")


def say(msg):
    sys.stderr.write("dots_bench: %s\n" % msg)
    sys.stderr.flush()


def sample(nb, dmax, seed):
    rng = np.random.default_rng(seed)
    n = nb * PER_BIN
    X = rng.integers(0, nb * RES, n)
    Y = X + np.exp(rng.uniform(np.log(RES / 2.0), np.log(dmax * RES * 1.2), n)).astype(np.int64)
    keep = Y < nb * RES
    return X[keep], Y[keep]


def trace_medians(d, calls):
    """the kernel trace of a --trace-only run (`calls` calls per case, the cases in order) -> per case {kernel: median seconds}"""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not f:
        raise SystemExit("no *kernel_trace.csv under %s" % d)
    with open(f[0]) as fh:
        rows = list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = [{} for _ in CASES]
    for name in KERNELS:
        t = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9 for r in rows if name in r["Kernel_Name"]]
        assert len(t) == calls * len(CASES), (name, len(t))
        for k in range(len(CASES)):
            out[k][name + "_s"] = float(np.median(t[k * calls:(k + 1) * calls]))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dots_timing.json"))
    ap.add_argument("--trace-only", action="store_true", help="the calls of a kernel trace: no timing, no file")
    ap.add_argument("--kernel-trace", default=None, help="directory of a rocprofv3 kernel trace of --trace-only: adds the kernels' times")
    op = ap.parse_args(argv)
    import torch
    from cloops_amd import api, dots, expected
    traced = trace_medians(op.kernel_trace, 3) if op.kernel_trace else None
    out = {"device": torch.cuda.get_device_name(0), "reps": op.reps, "res": RES, "pets_per_bin": PER_BIN, "chunks": CHUNKS, "cases": []}
    edges = dots.default_edges(CHUNKS)
    for k, (nb, dmax, p, w) in enumerate(CASES):
        X, Y = sample(nb, dmax, nb)
        ch = api.Chromosome(X, Y)
        n_cells = ch.mat_cells(RES, fold=True)[0]
        b0, bins, _ = ch.bal_marginals(2)
        ch.exp_diagonals(balanced=False)
        pairs, _, vs = ch.exp_diagonals_get()
        ch.exp_set(expected.expected_of(pairs, vs, 2)[0])
        dmin = p + 2
        tl, th = [], []
        for it in range(3 if op.trace_only else op.reps + 2):
            t0 = time.perf_counter()
            n_cand, n_full = ch.dot_lambdas(p, w, dmin, dmax)
            t1 = time.perf_counter()
            hist, n_beyond = ch.dot_hist(edges)
            t2 = time.perf_counter()
            if it >= 2:
                tl.append(t1 - t0)
                th.append(t2 - t1)
        ch.close()
        if op.trace_only:
            continue
        reads = 2 * ((2 * w + 1) ** 2 - (2 * p + 1) ** 2)
        c = {"nb": int(bins), "dmax": dmax, "dmin": dmin, "p": p, "w": w, "pets": int(len(X)), "cells": int(n_cells), "n_cand": int(n_cand),
             "n_full": int(n_full), "n_beyond": int(n_beyond), "lambdas_s": float("%.4g" % np.median(tl)), "hist_s": float("%.4g" % np.median(th)),
             "lds_reads_per_pixel": reads, "lds_bytes": int(n_cand) * reads * 8, "band_bytes": int(bins) * (dmax + 4 * w) * 8,
             "la_bytes": 4 * int(bins) * (dmax - dmin) * 8}
        if traced:
            c["kernel"] = {n: float("%.4g" % v) for n, v in traced[k].items()}
            c["kernel"]["lds_bytes_per_s"] = float("%.4g" % (c["lds_bytes"] / traced[k]["k29_lambdas_s"]))
        say(str(c))
        out["cases"].append(c)
    if op.trace_only:
        return 0
    js = json.dumps(out, indent=1)
    print(js)
    if op.out:
        os.makedirs(os.path.dirname(os.path.abspath(op.out)), exist_ok=True)
        with open(op.out, "w") as fh:
            fh.write(js + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
