"""Timing of K23 (cl_kdis_build): the k-distances of one chr1-sized chromosome, and how far the walk goes.

The chromosome is chr1 of the 200 M-PET genome of bench.py (cloops_amd.synth, 16.4 M PETs, the same seed), ks = (4, 9, 19).  Reports, as
one JSON document (stdout, and --out, by default profiles/kdis_timing.json), each step as the median of --reps runs in wall clock (every
call ends in a stream synchronise) and between two events recorded on the handle's stream around the call:
  build               kdis_build((4, 9, 19), 0) on the sorted rows (K19's table is held): k23_walk<32> and k23_hist
  build_sorting       the same with the cut alternating between 1 and 0, so that every call sorts the rows again
  build_k4 / k19 / k64   one k each: the list capacities 8, 32 and 64
  get, hist           kdis_get of one k (three arrays of 16.4 M int32 to the host), kdis_hist
  scan                derived on the host from d_19 and the sorted X: per row the rows whose X lies within d_19 of its own X -- what the
                      stopping rule leaves of the table once the threshold has settled (the walk reads somewhat more on its way there)
                      -- as mean, median, 99 % and maximum per row, and the mean over the waves of 64 consecutive rows of their largest
                      (a wave runs until its last lane is done)
  ckdtree             scipy's cKDTree(p = 1).query(k = 20) over a --sample row subsample on the host, on one core and on --workers
                      cores: the only exact alternative a user has; its d_19 are compared with a GPU build over the same subsample
  estimate            what cloops_amd.esteps makes of the histograms (the synthetic genome has no loops: the figures show the output)

    timeout -k 10 900 python tools/kdis_bench.py [--reps 5] [--sample 1000000] [--workers 16] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

KS = (4, 9, 19)


def say(msg):
    sys.stderr.write("kdis_bench: %s\n" % msg)
    sys.stderr.flush()


def timed(stream, reps, fn):
    """-> (result of the last run, median wall s, median events s, [min, max] events s); fn(i) is run i"""
    import torch
    walls, evs, r = [], [], None
    for i in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        r = fn(i)
        walls.append(time.perf_counter() - t0)
        e1.record(stream)
        e1.synchronize()
        evs.append(e0.elapsed_time(e1) * 1e-3)
    return r, {"wall_s": round(float(np.median(walls)), 6), "events_s": round(float(np.median(evs)), 6),
               "events_min_max_s": [round(min(evs), 6), round(max(evs), 6)]}


def scan_figures(xs, d):
    """rows with |dx| < d around every row of the sorted xs (itself left out) -> the figures of `scan`"""
    xs, d = xs.astype(np.int64), d.astype(np.int64)
    n = np.searchsorted(xs, xs + d, "left") - np.searchsorted(xs, xs - d, "right") - 1
    n = np.maximum(n, 0)
    waves = n[:len(n) // 64 * 64].reshape(-1, 64).max(1)
    return {"mean": round(float(n.mean()), 1), "median": int(np.median(n)), "p99": int(np.percentile(n, 99)), "max": int(n.max()),
            "mean_of_wave_max": round(float(waves.mean()), 1), "rows": int(len(n)), "total": int(n.sum())}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-total", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=1000000)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kdis_timing.json"))
    op = ap.parse_args(argv)
    import torch
    import bench
    from cloops_amd import api, esteps
    from cloops_amd.synth import chrom_sizes, synth_chrom
    name, length, n = chrom_sizes(int(op.n_total))[0]
    X, Y = synth_chrom(n, length, 1000 * bench.CFG)
    out = {"chrom": name, "pets": int(n), "device": torch.cuda.get_device_name(0), "reps": op.reps, "ks": list(KS), "steps": {}}
    stream = torch.cuda.Stream()
    ch = api.Chromosome(X, Y, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = ch.kdis_build(KS)
    out["first_build_s"] = round(time.perf_counter() - t0, 6)               # allocations and the sort included
    out["n_kept"] = first
    say("first build %.3f s" % out["first_build_s"])
    steps = out["steps"]
    reps2 = 2 * ((op.reps + 1) // 2)                                         # (an even number: the last run is cut 0)
    r, steps["build"] = timed(stream, op.reps, lambda i: ch.kdis_build(KS))
    assert r == first
    say("build %s" % steps["build"])
    r, steps["build_sorting"] = timed(stream, reps2, lambda i: ch.kdis_build(KS, 1 - (i & 1)))
    assert r == first
    for k in (4, 19, 64):
        r, steps["build_k%d" % k] = timed(stream, max(2, op.reps // 2), lambda i: ch.kdis_build([k]))
        say("build_k%d %s" % (k, steps["build_k%d" % k]))
    ch.kdis_build(KS)
    (xs, ys, d19), steps["get"] = timed(stream, 3, lambda i: ch.kdis_get(2))
    hist, steps["hist"] = timed(stream, 3, lambda i: ch.kdis_hist(2))
    steps["build"]["rows_per_s"] = round(first / steps["build"]["events_s"], 0)
    out["scan"] = scan_figures(xs, d19)
    out["scan"]["rows_read_per_s"] = round(out["scan"]["total"] / steps["build"]["events_s"], 0)
    out["d19_quantiles"] = {str(q): int(np.percentile(d19, q)) for q in (1, 50, 99, 100)}
    say("scan %s" % out["scan"])
    per = {name: {"n_kept": first, "hist": {}, "n_zero": {}, "n_none": {}}}
    for w, k in enumerate(KS):
        h, nz, nn = ch.kdis_hist(w)
        per[name]["hist"][k], per[name]["n_zero"][k], per[name]["n_none"][k] = h.astype(np.int64), nz, nn
    out["estimate"] = esteps.outputs_of(per, list(KS), 0)[1]["estimates"]
    ch.close()
    ok = True
    if op.sample > 0:
        from scipy.spatial import cKDTree
        sel = np.sort(np.random.default_rng(23).choice(len(X), min(op.sample, len(X)), replace=False))
        sx, sy = X[sel].astype(np.int64), Y[sel].astype(np.int64)
        o = np.argsort(sx, kind="stable")
        pts = np.stack([sx[o], sy[o]], 1).astype(np.float64)
        host = {"label": "scipy cKDTree(p=1).query(k=20)", "rows": int(len(sel))}
        t0 = time.perf_counter()
        tree = cKDTree(pts)
        host["tree_s"] = round(time.perf_counter() - t0, 3)
        for workers in sorted({1, max(1, op.workers)}):
            t0 = time.perf_counter()
            dd, _ = tree.query(pts, k=KS[-1] + 1, p=1, workers=workers)
            host["query_%d_workers_s" % workers] = round(time.perf_counter() - t0, 3)
            say("ckdtree %s" % host)
        sub = api.Chromosome(sx, sy, stream=stream.cuda_stream)
        sub.kdis_build(KS)                                                   # (warm: allocations and the sort)
        _, host["gpu_build_same_rows"] = timed(stream, 3, lambda i: sub.kdis_build(KS))
        gx, gy, gd = sub.kdis_get(2)
        sub.close()
        same = np.array_equal(gx, sx[o]) and np.array_equal(gy, sy[o]) and np.array_equal(gd, dd[:, KS[-1]].astype(np.int64))
        host["results_equal_gpu"] = bool(same)
        host["rows_per_s_1_worker"] = round(len(sel) / (host["query_1_workers_s"]), 0)
        out["ckdtree"] = host
        ok = bool(same)
    js = json.dumps(out, indent=1)
    print(js)
    if op.out:
        os.makedirs(os.path.dirname(os.path.abspath(op.out)), exist_ok=True)
        with open(op.out, "w") as fh:
            fh.write(js + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
