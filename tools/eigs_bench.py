"""Timing of K27 (cl_eig_build / cl_eig_iterate) on one chr1-sized chromosome, against K25's iteration over the same cells and numpy's
dense eigh.

The chromosome is chr1 of the 200 M-PET genome of bench.py (cloops_amd.synth, 16.4 M PETs, the same seed); the cells are K24's folded
ones at 100 kb and at 10 kb, balanced by K25 and given expected values by K26 at the defaults of cloops_amd.compartments.  Reports, as
one JSON document (stdout, and --out, by default profiles/eigs_timing.json), in wall clock (every call ends in a stream synchronise):
  build               cl_eig_build: the cell values in both orders and the row pointers (median of --reps)
  iteration_s         one iteration of the subspace iteration: cl_eig_iterate with tol = 0 for --iters iterations, over their number
                      (median of --reps)
  full                cl_eig_iterate at the defaults (3 pairs, tol 1e-8, at most 1000 iterations): iterations, converged, time
  k25_iteration_s     one iteration of cl_bal_iterate over the same cells, the same way (tol = 0, --iters iterations)
  product             with --kernel-trace DIR: the median duration of k27_mul (and of K25's k25_marg) from a rocprofv3 kernel trace of
                      `--trace-only` (a run of its own), the bytes the block product must move -- per cell and order the other bin and
                      the value (12 bytes), the block read and written once (128 bytes per bin), the row pointers -- over that time,
                      and its share of the 8 TB/s peak
  numpy_eigh_s        at 100 kb: np.linalg.eigh of the dense matrix (tests/compartments_cases.py) on one core, and whether the device's
                      eigenvalues agree with it to the residuals

    timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/eigs_bench.py --trace-only
    timeout -k 10 600 python tools/eigs_bench.py --kernel-trace DIR [--reps 5] [--out FILE]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):      # numpy's eigh on one core
    os.environ[_v] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

PEAK = 8e12                            # bytes per second


def say(msg):
    sys.stderr.write("eigs_bench: %s\n" % msg)
    sys.stderr.flush()


def walls(reps, fn):
    """-> (result of the last run, median wall seconds); one warm-up call, then `reps` timed ones"""
    fn()
    ts, r = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return r, float(np.median(ts))


def trace_medians(d):
    """the kernel trace of a --trace-only run -> per case (split at k27_vals) the median seconds of k27_mul and of k25_marg<K25D>"""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not f:
        raise SystemExit("no *kernel_trace.csv under %s" % d)
    with open(f[0]) as fh:
        rows = list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cases, marg = [], []
    for r in rows:
        name, t = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
        if "k25_marg" in name and "K25D" in name:
            marg.append(t)
        elif "k27_vals" in name:
            cases.append({"mul": [], "marg": marg})
            marg = []
        elif "k27_mul" in name and cases:
            cases[-1]["mul"].append(t)
    return [{"k27_mul_s": float(np.median(c["mul"])), "k25_marg_s": float(np.median(c["marg"])) if c["marg"] else None} for c in cases if c["mul"]]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-total", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eigs_timing.json"))
    ap.add_argument("--trace-only", action="store_true", help="the calls of a kernel trace: no timing, no numpy, no file")
    ap.add_argument("--kernel-trace", default=None, help="directory of a rocprofv3 kernel trace of --trace-only: adds the product")
    op = ap.parse_args(argv)
    import torch
    import bench
    import compartments_cases as CC
    from cloops_amd import api, balance, compartments, expected
    from cloops_amd.synth import chrom_sizes, synth_chrom
    name, length, n = chrom_sizes(int(op.n_total))[0]
    X, Y = synth_chrom(n, length, 1000 * bench.CFG)
    out = {"chrom": name, "pets": int(n), "device": torch.cuda.get_device_name(0), "reps": op.reps, "iters": op.iters, "peak_bytes_per_s": PEAK,
           "cases": {}}
    traced = trace_medians(op.kernel_trace) if op.kernel_trace else None
    ok = True
    ch = api.Chromosome(X, Y)
    for k, (label, res) in enumerate((("100kb", 100000), ("10kb", 10000))):
        c = out["cases"][label] = {"res": res}
        n_cells = ch.mat_cells(res, fold=True)[0]
        b0, nb, _ = ch.bal_marginals(2)
        s, z = ch.bal_marginals_get()
        mask = balance.valid_bins(s, z)
        if op.trace_only:
            ch.bal_iterate(mask, max_iters=8, tol=0.0)
        else:
            _, t = walls(op.reps, lambda: ch.bal_iterate(mask, max_iters=op.iters, tol=0.0))
            c["k25_iteration_s"] = float("%.4g" % (t / op.iters))
        it = ch.bal_iterate(mask)
        w = ch.bal_weights()
        valid = ~np.isnan(w)
        ch.exp_diagonals()
        p, _, vs = ch.exp_diagonals_get()
        e, _ = expected.expected_of(p, vs, 2)
        ch.exp_set(e)
        oe = np.concatenate([ch.exp_cells_get(f, min(1 << 22, n_cells - f)) for f in range(0, n_cells, 1 << 22)])
        clip, dmax = compartments.clip_of(oe, 99.9), compartments.pick_dmax(p, e, 2)
        if op.trace_only:
            ch.eig_build(clip, dmax)
            ch.eig_iterate(3, max_iters=16, tol=0.0)
            continue
        (n_valid, n_in), t = walls(op.reps, lambda: ch.eig_build(clip, dmax))
        c.update(n_cells=int(n_cells), nb=int(nb), n_valid=int(n_valid), n_in=int(n_in), dmax=int(dmax), clip=float(clip), bal_iters=it[0],
                 build_s=float("%.4g" % t))
        _, t = walls(op.reps, lambda: ch.eig_iterate(3, max_iters=op.iters, tol=0.0))
        c["iteration_s"] = float("%.4g" % (t / op.iters))
        (its, cv, lam, resid), t = walls(max(2, op.reps // 2), lambda: ch.eig_iterate(3))
        c["full"] = {"iters": its, "converged": cv, "wall_s": float("%.4g" % t), "eigvals": lam.tolist(), "resid": resid.tolist()}
        c["product_bytes"] = int(2 * n_cells * 12 + nb * 128 + 2 * (nb + 1) * 4)
        if traced:
            c["product"] = dict(traced[k])
            c["product"]["bytes_per_s"] = float("%.4g" % (c["product_bytes"] / traced[k]["k27_mul_s"]))
            c["product"]["share_of_peak"] = round(c["product_bytes"] / traced[k]["k27_mul_s"] / PEAK, 4)
        if nb <= 4000:
            cells = ch.mat_cells_get()
            M = CC.dense_M(cells, b0, nb, 2, valid, w, e, clip, dmax)
            t0 = time.perf_counter()
            ev = np.linalg.eigh(M[np.ix_(valid, valid)])[0]
            c["numpy_eigh_s"] = round(time.perf_counter() - t0, 4)
            ev = ev[np.argsort(-np.abs(ev))][:3]
            same = bool(cv and np.all(np.abs(ev - lam) <= resid + 1e-9 * abs(ev[0])))
            c["equal_numpy"] = same
            c["speedup_over_eigh"] = round(c["numpy_eigh_s"] / c["full"]["wall_s"], 1)
            ok &= same
        say("%s %s" % (label, c))
    ch.mat_free()
    ch.close()
    if op.trace_only:
        return 0
    js = json.dumps(out, indent=1)
    print(js)
    if op.out:
        os.makedirs(os.path.dirname(os.path.abspath(op.out)), exist_ok=True)
        with open(op.out, "w") as fh:
            fh.write(js + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
