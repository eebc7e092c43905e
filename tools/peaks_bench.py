"""Timing of K21 (cl_peak_sort / cl_peak_call / cl_peak_count / cl_peak_summits): the peaks of both ends of one chr1-sized chromosome.

The chromosome is chr1 of the 200 M-PET genome of bench.py (cloops_amd.synth, 16.4 M PETs, the same seed).  Reports, as one JSON
document (stdout, and --out, by default profiles/peaks_timing.json), each step as the median of --reps runs in wall clock (every call
ends in a stream synchronise) and between two events recorded on the handle's stream around the call:
  sort                peaks_sort(0, 3): the key pass and the radix sort
  call_150_5          one peaks_call(150, 5) on the sorted ends
  sweep               the four calls of the default sweep, eps (100, 200) x minPts (5, 10), each with its peaks_get, after one sort
  count               one peaks_count over the merged peaks of that sweep and their two flank windows
  summits             one peaks_summits over the merged peaks, w = 100
  k20_rebuild         K20's steady coverage_build(0, 3, 75, 0) on the same handle in the same run: the same sort and the same kind of
                      search pass over the same array -- the yardstick
  host                the numpy closed form on one core for the same steps (np.sort, searchsorted, cumsum), median of --host-reps;
                      its peaks, counts and summits are compared with the GPU's

    timeout -k 10 900 python tools/peaks_bench.py [--reps 10] [--host-reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

EPS, MINPTS, FLANK = (100, 200), (5, 10), (5, 10)


def host_peaks(S, eps, minPts):
    """the closed form of include/cloops_hip.h (cl_peak_sort) -> (start, end, n_points, n_cores)"""
    lb = lambda x: np.searchsorted(S, x, "left")
    ub = lambda x: np.searchsorted(S, x, "right")
    core = (ub(S + eps) - lb(S - eps)) >= minPts
    cp = S[core]
    if len(cp) == 0:
        z = np.zeros(0, np.int64)
        return z, z, z, z
    head = np.ones(len(cp), bool)
    head[1:] = (cp[1:] - cp[:-1]) > eps
    first = np.flatnonzero(head)
    last = np.append(first[1:] - 1, len(cp) - 1)
    a, b = cp[first], cp[last]
    left = a - eps
    left[1:] = np.maximum(left[1:], b[:-1] + eps + 1)
    i0, i1 = lb(left), ub(b + eps)
    return S[i0], S[i1 - 1] + 1, i1 - i0, last - first + 1


def host_summits(S, s, e, w):
    """ascending disjoint intervals: the largest of n_w (m + 1) + (m - index) per index range"""
    m = len(S)
    nw = np.searchsorted(S, S + w, "right") - np.searchsorted(S, S - w, "left")
    key = np.append(nw.astype(np.int64) * (m + 1) + (m - np.arange(m, dtype=np.int64)), 0)
    i0, i1 = np.searchsorted(S, s, "left"), np.searchsorted(S, e, "left")
    top = np.maximum.reduceat(key, np.stack([i0, i1], 1).ravel())[0::2]
    has = i1 > i0
    return np.where(has, S[np.minimum(m - top % (m + 1), m - 1)], -1), np.where(has, top // (m + 1), 0)


def timed(stream, reps, fn):
    """-> (result of the last run, median wall s, median events s, [min, max] events s)"""
    import torch
    walls, evs, r = [], [], None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        r = fn()
        walls.append(time.perf_counter() - t0)
        e1.record(stream)
        e1.synchronize()
        evs.append(e0.elapsed_time(e1) * 1e-3)
    return r, {"wall_s": round(float(np.median(walls)), 6), "events_s": round(float(np.median(evs)), 6),
               "events_min_max_s": [round(min(evs), 6), round(max(evs), 6)]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-total", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peaks_timing.json"))
    op = ap.parse_args(argv)
    import torch
    import bench
    from cloops_amd import api
    from cloops_amd.peaks import flank_windows, merge_intervals
    from cloops_amd.synth import chrom_sizes, synth_chrom
    name, length, n = chrom_sizes(int(op.n_total))[0]
    X, Y = synth_chrom(n, length, 1000 * bench.CFG)
    out = {"chrom": name, "pets": int(n), "device": torch.cuda.get_device_name(0), "reps": op.reps, "steps": {}}
    stream = torch.cuda.Stream()
    ch = api.Chromosome(X, Y, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = ch.peaks_sort(0, 3)
    out["first_sort_s"] = round(time.perf_counter() - t0, 6)              # allocations included
    out["n_ends"] = first[0]
    ch.peaks_call(150, 5)                                                  # (warm: the scratch of a call)
    steps = out["steps"]
    r, steps["sort"] = timed(stream, op.reps, lambda: ch.peaks_sort(0, 3))
    assert r == first
    one, steps["call_150_5"] = timed(stream, op.reps, lambda: ch.peaks_call(150, 5))
    out["call_150_5"] = dict(zip(("n_peaks", "n_cores", "n_clustered"), one))

    def sweep():
        got = []
        for e in EPS:
            for m in MINPTS:
                ch.peaks_call(e, m)
                got.append(ch.peaks_get())
        return got

    cands, steps["sweep"] = timed(stream, op.reps, sweep)
    ms, me = merge_intervals(np.concatenate([c[0] for c in cands]), np.concatenate([c[1] for c in cands]))
    wins = flank_windows(ms, me, FLANK)
    cs, ce = np.concatenate([ms] + [w[0] for w in wins]), np.concatenate([me] + [w[1] for w in wins])
    out["candidates"], out["merged"] = int(sum(len(c[0]) for c in cands)), int(len(ms))
    counts, steps["count"] = timed(stream, op.reps, lambda: ch.peaks_count(cs, ce))
    summits, steps["summits"] = timed(stream, op.reps, lambda: ch.peaks_summits(ms, me, min(EPS)))
    cov = ch.coverage_build(0, 3, 75, 0)                                   # (warm: K20's allocations)
    r, steps["k20_rebuild"] = timed(stream, op.reps, lambda: ch.coverage_build(0, 3, 75, 0))
    assert r == cov
    for k in ("call_150_5", "sweep", "count", "summits"):
        steps[k]["events_over_k20_rebuild"] = round(steps[k]["events_s"] / steps["k20_rebuild"]["events_s"], 3)
    ch.close()
    ok = True
    if op.host_reps > 0:                                                   # --host-reps 0: the device alone (a run under a profiler)
        host = {"label": "closed form in numpy, one core", "reps": op.host_reps}

        def med(f):
            ts, r = _repeat(f, op.host_reps)
            return round(float(np.median(ts)), 3), r

        host["sort_s"], S = med(lambda: np.sort(np.concatenate([X, Y]).astype(np.int64)))
        host["call_150_5_s"], h1 = med(lambda: host_peaks(S, 150, 5))
        host["sweep_s"], hs = med(lambda: [host_peaks(S, e, m) for e in EPS for m in MINPTS])
        host["count_s"], hc = med(lambda: np.maximum(0, np.searchsorted(S, ce, "left") - np.searchsorted(S, cs, "left")))
        host["summits_s"], hm = med(lambda: host_summits(S, ms, me, min(EPS)))
        same = (len(h1[0]) == one[0] and all(np.array_equal(a, b) for h, g in zip(hs, cands) for a, b in zip(h, g))
                and np.array_equal(hc, counts) and np.array_equal(hm[0], summits[0]) and np.array_equal(hm[1], summits[1]))
        host["results_equal_gpu"] = bool(same)
        out["host_numpy"] = host
        ok = bool(same)
    js = json.dumps(out, indent=1)
    print(js)
    if op.out:
        os.makedirs(os.path.dirname(os.path.abspath(op.out)), exist_ok=True)
        with open(op.out, "w") as fh:
            fh.write(js + "\n")
    return 0 if ok else 1


def _repeat(f, reps):
    ts, r = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    return ts, r


if __name__ == "__main__":
    sys.exit(main())
