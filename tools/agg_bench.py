"""Timing of K19 (cl_agg_loops): the aggregate pile-up around 100 000 loop centres on one chr1-sized chromosome.

The chromosome is chr1 of the 200 M-PET genome of bench.py (cloops_amd.synth, 16.4 M PETs, the same seed); the centres are the
(X, Y) of --loops PETs drawn from it with a seed; res 1000, w 10, corner 3.  Reports, as one JSON document (stdout, and --out):
  first call          wall clock of the first agg_loops call on the handle: the table's sort included
  steady call         median of --reps further calls, as wall clock (the call ends in a stream synchronise) and between two events
                      recorded on the handle's stream around the call (centre upload, loop sort, kernel, copies back)
  bytes               the X and Y of the candidates of every loop's X range (8 B per candidate, counted on the host with
                      np.searchsorted) + 8 B per loop centre + the outputs; over the steady event time as a share of the HBM peak
  host                what a user would otherwise run: numpy on a pre-sorted X (the sort is timed apart), np.searchsorted +
                      np.bincount per loop on a --host-sample sample, SCALED linearly to --loops; its per-loop totals are compared
                      with the GPU's
The developer library (CLOOPS_DEVEL_LIB=1, python -m cloops_amd.build --devel) with CLOOPS_K19_WAVE=1 times the wave-per-loop form.

    timeout -k 10 600 python tools/agg_bench.py [--loops 100000] [--reps 20] [--host-sample 2000] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

HBM_SPEC = 8.0e12


def host_agg(xs, ys, cx, cy, res, w):
    """numpy on the X-sorted rows (xs ascending, ys its payload) -> (S, per-loop totals)"""
    W = 2 * w + 1
    S = np.zeros(W * W, np.int64)
    tot = np.zeros(len(cx), np.int64)
    for k in range(len(cx)):
        ox, oy = cx[k] - w * res - res // 2, cy[k] - w * res - res // 2
        b, e = np.searchsorted(xs, ox, "left"), np.searchsorted(xs, ox + W * res, "left")
        dy = ys[b:e] - oy
        m = (dy >= 0) & (dy < W * res)
        cells = (xs[b:e][m] - ox) // res * W + dy[m] // res
        M = np.bincount(cells, minlength=W * W)
        S += M
        tot[k] = M.sum()
    return S.reshape(W, W), tot


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-total", type=float, default=2e8)
    ap.add_argument("--loops", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-sample", type=int, default=2000)
    ap.add_argument("--res", type=int, default=1000)
    ap.add_argument("--w", type=int, default=10)
    ap.add_argument("--out", default=None)
    op = ap.parse_args(argv)
    import torch
    import bench
    from cloops_amd import api
    from cloops_amd.synth import chrom_sizes, synth_chrom
    res, w, corner = op.res, op.w, 3
    W = 2 * w + 1
    name, length, n = chrom_sizes(int(op.n_total))[0]
    X, Y = synth_chrom(n, length, 1000 * bench.CFG)
    rng = np.random.default_rng(19)
    pick = rng.choice(n, op.loops, replace=False)
    cx, cy = X[pick].astype(np.int64), Y[pick].astype(np.int64)
    out = {"chrom": name, "pets": int(n), "loops": op.loops, "res": res, "w": w, "corner": corner, "device": torch.cuda.get_device_name(0),
           "devel_k19_wave": os.environ.get("CLOOPS_K19_WAVE")}
    stream = torch.cuda.Stream()
    ch = api.Chromosome(X, Y, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    S, stats, _, kept = ch.agg_loops(cx, cy, res, w, corner)
    out["first_call_s"] = round(time.perf_counter() - t0, 6)
    walls, evs = [], []
    for _ in range(op.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        S2, stats2, _, _ = ch.agg_loops(cx, cy, res, w, corner)
        walls.append(time.perf_counter() - t0)
        e1.record(stream)
        e1.synchronize()
        evs.append(e0.elapsed_time(e1) * 1e-3)
        assert np.array_equal(S2, S) and np.array_equal(stats2, stats)
    out["steady_call_wall_s"] = round(float(np.median(walls)), 6)
    out["steady_call_events_s"] = round(float(np.median(evs)), 6)
    out["steady_call_events_min_max_s"] = [round(min(evs), 6), round(max(evs), 6)]
    walls = []
    for _ in range(5):                                                   # without the per-loop statistics: S alone
        t0 = time.perf_counter()
        ch.agg_loops(cx, cy, res, w, corner, want_stats=False)
        walls.append(time.perf_counter() - t0)
    out["steady_call_sum_only_wall_s"] = round(float(np.median(walls)), 6)
    ch.close()
    # the bytes the kernel has to touch, and the host's way on the same arrays
    t0 = time.perf_counter()
    o = np.argsort(X, kind="stable")
    xs, ys = X[o].astype(np.int64), Y[o].astype(np.int64)
    out["host_sort_s"] = round(time.perf_counter() - t0, 3)
    ox = cx - w * res - res // 2
    cand = np.searchsorted(xs, ox + W * res, "left") - np.searchsorted(xs, ox, "left")
    nbytes = int(cand.sum()) * 8 + op.loops * 8 + op.loops * 6 * 4 + W * W * 8
    out["candidates_total"] = int(cand.sum())
    out["candidates_per_loop_median_max"] = [int(np.median(cand)), int(cand.max())]
    out["pets_in_windows"] = int(S.sum())
    out["bytes"] = nbytes
    out["bytes_over_steady_events_of_hbm_spec"] = round(nbytes / out["steady_call_events_s"] / HBM_SPEC, 4)
    k = min(op.host_sample, op.loops)
    t0 = time.perf_counter()
    hS, htot = host_agg(xs, ys, cx[:k], cy[:k], res, w)
    th = time.perf_counter() - t0
    out["host_numpy"] = {"label": "SCALED from a sample: np.searchsorted + np.bincount per loop on a pre-sorted X, one core",
                         "sample_loops": k, "sample_s": round(th, 4), "scaled_to_loops_s": round(th * op.loops / k, 3),
                         "totals_equal_gpu": bool(np.array_equal(htot, stats[:k, 0]))}
    out["gpu_first_call_faster_than_host"] = bool(out["first_call_s"] < out["host_numpy"]["scaled_to_loops_s"])
    js = json.dumps(out, indent=1)
    print(js)
    if op.out:
        os.makedirs(os.path.dirname(os.path.abspath(op.out)), exist_ok=True)
        with open(op.out, "w") as fh:
            fh.write(js)
    return 0 if out["host_numpy"]["totals_equal_gpu"] and out["gpu_first_call_faster_than_host"] else 1


if __name__ == "__main__":
    sys.exit(main())
