"""Timing of K28 (cl_scc_moments) on two chr1-sized chromosomes, against the numpy restatement on one core.

The chromosomes are chr1 of the 200 M-PET genome of bench.py (cloops_amd.synth, 16.4 M PETs) and chr1 of a second seed of the same
generator; the cells are K24's folded ones at 100 kb (h = 3) and at 10 kb (h = 20), both with dmax = 5 Mb.  Reports, as one JSON
document (stdout, and --out, by default profiles/scc_timing.json), in wall clock (the call is synchronous):
  wall_s              cl_scc_moments: both band fills, the fused kernel and the read-back (median of --reps after a warm-up call)
  kernel              with --kernel-trace DIR: the median duration of k28_moments (and of k28_fill) from a rocprofv3 kernel trace of
                      `--trace-only` (a run of its own), the band bytes the kernel must move -- both band arrays read once, nb (D + 4h) 4
                      bytes each -- over that time, and its share of the 8 TB/s peak
  numpy_s             at 100 kb: the restatement of tests/similarity_cases.py (dense matrices, prefix-sum boxes, Python-int moments) on
                      one core, and whether the device's six arrays equal it

    timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/scc_bench.py --trace-only
    timeout -k 10 600 python tools/scc_bench.py --kernel-trace DIR [--reps 5] [--out FILE]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):      # the restatement on one core
    os.environ[_v] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

PEAK = 8e12                            # bytes per second
CASES = (("100kb_h3", 100000, 3), ("10kb_h20", 10000, 20))
DMAX = 5000000


def say(msg):
    sys.stderr.write("scc_bench: %s\n" % msg)
    sys.stderr.flush()


def trace_medians(d):
    """the kernel trace of a --trace-only run -> per case (a case is two k28_fill and the k28_moments that follow, three times) the
    median seconds of k28_moments and of k28_fill"""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not f:
        raise SystemExit("no *kernel_trace.csv under %s" % d)
    with open(f[0]) as fh:
        rows = list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    mom = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9 for r in rows if "k28_moments" in r["Kernel_Name"]]
    fill = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9 for r in rows if "k28_fill" in r["Kernel_Name"]]
    per = len(mom) // len(CASES)
    return [{"k28_moments_s": float(np.median(mom[k * per:(k + 1) * per])), "k28_fill_s": float(np.median(fill[2 * k * per:2 * (k + 1) * per]))}
            for k in range(len(CASES))]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-total", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scc_timing.json"))
    ap.add_argument("--trace-only", action="store_true", help="the calls of a kernel trace: no timing, no numpy, no file")
    ap.add_argument("--kernel-trace", default=None, help="directory of a rocprofv3 kernel trace of --trace-only: adds the kernel's time")
    op = ap.parse_args(argv)
    import torch
    import bench
    import similarity_cases as SC
    from cloops_amd import api, similarity
    from cloops_amd.synth import chrom_sizes, synth_chrom
    name, length, n = chrom_sizes(int(op.n_total))[0]
    Xa, Ya = synth_chrom(n, length, 1000 * bench.CFG)
    Xb, Yb = synth_chrom(n, length, 1000 * bench.CFG + 1)
    out = {"chrom": name, "pets": int(n), "device": torch.cuda.get_device_name(0), "reps": op.reps, "dmax": DMAX, "peak_bytes_per_s": PEAK, "cases": {}}
    traced = trace_medians(op.kernel_trace) if op.kernel_trace else None
    ok = True
    cha, chb = api.Chromosome(Xa, Ya), api.Chromosome(Xb, Yb)
    for k, (label, res, h) in enumerate(CASES):
        c = out["cases"][label] = {"res": res, "h": h}
        na, ka, ma = cha.mat_cells(res, fold=True)
        nb_, kb, mb = chb.mat_cells(res, fold=True)
        sa, sb = similarity.cells_span(cha), similarity.cells_span(chb)
        b0 = min(sa[0], sb[0])
        nb = max(sa[1], sb[1]) - b0 + 1
        D = min(nb, DMAX // res + 1)
        call = lambda: cha.scc_moments(chb, b0, nb, h=h, n_diags=D)
        if op.trace_only:
            for _ in range(3):
                call()
            continue
        call()
        ts, got = [], None
        for _ in range(op.reps):
            t0 = time.perf_counter()
            got = call()
            ts.append(time.perf_counter() - t0)
        rec = similarity.combine(got)
        c.update(bins=int(nb), diags=int(D), cells_a=int(na), cells_b=int(nb_), smax=int(max(similarity.smax_of(h, ma, ka), similarity.smax_of(h, mb, kb))),
                 wall_s=float("%.4g" % np.median(ts)), scc=rec["scc"], pcc=rec["pcc"], pixels=rec["pixels"], band_bytes=int(2 * nb * (D + 4 * h) * 4))
        if traced:
            c["kernel"] = dict(traced[k])
            c["kernel"]["bytes_per_s"] = float("%.4g" % (c["band_bytes"] / traced[k]["k28_moments_s"]))
            c["kernel"]["share_of_peak"] = round(c["band_bytes"] / traced[k]["k28_moments_s"] / PEAK, 4)
        if nb <= 4000:
            ca, cb = cha.mat_cells_get(), chb.mat_cells_get()
            t0 = time.perf_counter()
            want = SC.as_arrays(SC.moments_oracle(ca, cb, b0, nb, h, D))
            c["numpy_s"] = round(time.perf_counter() - t0, 4)
            same = all(np.array_equal(g, w) for g, w in zip(got, want))
            c["equal_numpy"] = same
            c["speedup_over_numpy"] = round(c["numpy_s"] / c["wall_s"], 1)
            ok &= same
        say("%s %s" % (label, c))
    cha.close()
    chb.close()
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
