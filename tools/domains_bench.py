"""Timing of K22 (cl_dom_tracks / cl_dom_get / cl_dom_count): the insulation tracks and domain counts of one chr1-sized chromosome.

The chromosome is chr1 of the 200 M-PET genome of bench.py (cloops_amd.synth, 16.4 M PETs, the same seed).  Reports, as one JSON
document (stdout, and --out, by default profiles/domains_timing.json), each step as the median of --reps runs in wall clock (every call
ends in a stream synchronise) and between two events recorded on the handle's stream around the call:
  tracks_sorting      domains_tracks(cut, 10000, 10) with the cut alternating between 1 and 0, so that every call sorts the rows again:
                      what the first call of a chromosome costs once its scratch exists
  tracks_second_w     domains_tracks(0, 10000, w) with w alternating between 20 and 10 on the sorted rows: no sort, k22_tracks and the scan
  get                 domains_get of the three tracks
  count               domains_count over the called domains (the host rules at the defaults; 1 Mb pieces if they call fewer than two)
  k20_rebuild         K20's steady coverage_build(0, 3, 0, 10000) on the same handle in the same run: one sort and one pass over the
                      same rows -- the yardstick
  host                the numpy range form on one core (floor division, np.add.at, cumsum), median of --host-reps; its tracks and
                      counts are compared with the GPU's

    timeout -k 10 900 python tools/domains_bench.py [--reps 10] [--host-reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

RES, W = 10000, 10


def host_tracks(X, Y, res, w):
    """the range form of include/cloops_hip.h (cl_dom_tracks) -> (cross, up, down, n_bins, bmin)"""
    bx, by = X // res, Y // res
    bmin, bmax = int(min(bx.min(), by.min())), int(max(bx.max(), by.max()))
    nb = bmax - bmin + 2
    fwd = bx <= by
    bx, by = bx[fwd], by[fwd]
    out = []
    for lo, hi in ((np.maximum(bx + 1, by - w + 1), np.minimum(bx + w, by)), (by + 1, bx + w), (by - w + 1, bx)):
        lo, hi = np.maximum(lo, bmin), np.minimum(hi, bmax + 1)
        ok = lo <= hi
        d = np.bincount(lo[ok] - bmin, minlength=nb + 1) - np.bincount(hi[ok] + 1 - bmin, minlength=nb + 1)
        out.append(np.cumsum(d)[:nb])
    return out[0], out[1], out[2], nb, bmin


def host_counts(X, Y, s, e):
    """ascending disjoint intervals -> (intra, nx, ny)"""
    k = np.searchsorted(s, X, "right") - 1
    kk = np.maximum(k, 0)
    inx = (k >= 0) & (X < e[kk])
    j = np.searchsorted(s, Y, "right") - 1
    jj = np.maximum(j, 0)
    iny = (j >= 0) & (Y < e[jj])
    n = len(s)
    return (np.bincount(kk[inx & iny & (kk == jj)], minlength=n), np.bincount(kk[inx], minlength=n), np.bincount(jj[iny], minlength=n))


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-total", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "domains_timing.json"))
    op = ap.parse_args(argv)
    import torch
    import bench
    from cloops_amd import api, domains
    from cloops_amd.synth import chrom_sizes, synth_chrom
    name, length, n = chrom_sizes(int(op.n_total))[0]
    X, Y = synth_chrom(n, length, 1000 * bench.CFG)
    out = {"chrom": name, "pets": int(n), "device": torch.cuda.get_device_name(0), "reps": op.reps, "res": RES, "w": W, "steps": {}}
    stream = torch.cuda.Stream()
    ch = api.Chromosome(X, Y, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = ch.domains_tracks(0, RES, W)
    out["first_tracks_s"] = round(time.perf_counter() - t0, 6)             # allocations and the sort included
    out["n_bins"], out["bin0"], out["n_kept"] = first
    steps = out["steps"]
    reps2 = 2 * ((op.reps + 1) // 2)                                        # (an even number: the last run is cut 0, w 10)
    r, steps["tracks_sorting"] = timed(stream, reps2, lambda i: ch.domains_tracks(1 - (i & 1), RES, W))
    assert r == first
    r, steps["tracks_second_w"] = timed(stream, reps2, lambda i: ch.domains_tracks(0, RES, W if (i & 1) else 2 * W))
    assert r == first
    trk, steps["get"] = timed(stream, op.reps, lambda i: ch.domains_get())
    s, valid = domains.score_of(*trk, 20)
    bidx, _ = domains.boundaries_of(s, valid, W, 0.05)
    a, b = domains.domains_of(bidx, valid, 500)
    out["boundaries"], out["domains"] = int(len(bidx)), int(len(a))
    if len(a) < 2:
        a = np.arange(0, first[0] - 1, 100, dtype=np.int64)
        b = np.minimum(a + 100, first[0] - 1)
    ds, de = (a + first[1]) * RES, (b + first[1]) * RES
    out["count_intervals"] = int(len(ds))
    cnt, steps["count"] = timed(stream, op.reps, lambda i: ch.domains_count(ds, de))
    cov = ch.coverage_build(0, 3, 0, RES)                                   # (warm: K20's allocations)
    r, steps["k20_rebuild"] = timed(stream, op.reps, lambda i: ch.coverage_build(0, 3, 0, RES))
    assert r == cov
    for k in ("tracks_sorting", "tracks_second_w", "count"):
        steps[k]["events_over_k20_rebuild"] = round(steps[k]["events_s"] / steps["k20_rebuild"]["events_s"], 3)
    ch.close()
    ok = True
    if op.host_reps > 0:                                                    # --host-reps 0: the device alone (a run under a profiler)
        host = {"label": "range form in numpy, one core", "reps": op.host_reps}
        X64, Y64 = X.astype(np.int64), Y.astype(np.int64)

        def med(f):
            ts, r = [], None
            for _ in range(op.host_reps):
                t0 = time.perf_counter()
                r = f()
                ts.append(time.perf_counter() - t0)
            return round(float(np.median(ts)), 3), r

        host["tracks_s"], ht = med(lambda: host_tracks(X64, Y64, RES, W))
        host["count_s"], hc = med(lambda: host_counts(X64, Y64, ds, de))
        same = (ht[3], ht[4]) == first[:2] and all(np.array_equal(u, v) for u, v in zip(ht[:3], trk)) \
            and all(np.array_equal(u, v) for u, v in zip(hc, cnt))
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


if __name__ == "__main__":
    sys.exit(main())
