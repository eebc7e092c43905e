"""Timing of K20 (cl_cov_build / cl_cov_text / cl_cov_render): the coverage of one chr1-sized chromosome by both ends of its PETs.

The chromosome is chr1 of the 200 M-PET genome of bench.py (cloops_amd.synth, 16.4 M PETs, the same seed).  Two settings: windows of
ext 75 and bins of res 1000.  Reports, as one JSON document (stdout, and --out), per setting:
  first build         wall clock of the first coverage_build on the handle: allocations and the sort included
  steady rebuild      median of --reps further builds, as wall clock (a build ends in a stream synchronise) and between two events
                      recorded on the handle's stream around the call; every build sorts again
  floor bytes         what a build must move at the least: X and Y once (8 B per row) and the runs out (12 B per run); over the steady
                      event time as a share of the HBM peak
  text                coverage_text + every chunk of coverage_iter (rendered on the device, copied to page-locked memory, not
                      written anywhere): bytes of text over the median wall clock of --reps passes
  host                the events oracle in numpy on one core (np.unique over the 2 n_ends break points, np.add.at, cumsum, merge),
                      median of --host-reps runs; its runs are compared with the GPU's

    timeout -k 10 900 python tools/coverage_bench.py [--reps 10] [--host-reps 3] [--out FILE]
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


def host_runs(X, Y, ext, res):
    """the events oracle: unique positions, summed +-1, cumsum, drop zero depth, merge abutting equal depths -> (start, end, depth)"""
    p = np.concatenate([X, Y]).astype(np.int64)
    if res == 0:
        s, e = np.maximum(0, p - ext), p + ext
    else:
        b = (p // res) * res
        s, e = np.maximum(0, b), b + res
    ok = e > s
    s, e = s[ok], e[ok]
    u, inv = np.unique(np.concatenate([s, e]), return_inverse=True)
    d = np.zeros(len(u), np.int64)
    np.add.at(d, inv[:len(s)], 1)
    np.add.at(d, inv[len(s):], -1)
    depth = np.cumsum(d)[:-1]
    st, en = u[:-1], u[1:]
    k = depth > 0
    st, en, depth = st[k], en[k], depth[k]
    first = np.ones(len(st), bool)
    first[1:] = (st[1:] != en[:-1]) | (depth[1:] != depth[:-1])
    idx = np.flatnonzero(first)
    last = np.append(idx[1:] - 1, len(st) - 1)
    return st[idx], en[last], depth[idx]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-total", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    op = ap.parse_args(argv)
    import torch
    import bench
    from cloops_amd import api
    from cloops_amd.synth import chrom_sizes, synth_chrom
    name, length, n = chrom_sizes(int(op.n_total))[0]
    X, Y = synth_chrom(n, length, 1000 * bench.CFG)
    out = {"chrom": name, "pets": int(n), "device": torch.cuda.get_device_name(0), "reps": op.reps, "settings": {}}
    ok = True
    for label, ext, res in (("ext75", 75, 0), ("res1000", 0, 1000)):
        stream = torch.cuda.Stream()
        ch = api.Chromosome(X, Y, stream=stream.cuda_stream)          # a fresh handle per setting: the first build pays its allocations
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tot = ch.coverage_build(0, 3, ext, res)
        r = {"first_build_s": round(time.perf_counter() - t0, 6), "n_runs": tot[0], "max_depth": tot[1], "n_ends": tot[2], "area": tot[3]}
        walls, evs = [], []
        for _ in range(op.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            again = ch.coverage_build(0, 3, ext, res)
            walls.append(time.perf_counter() - t0)
            e1.record(stream)
            e1.synchronize()
            evs.append(e0.elapsed_time(e1) * 1e-3)
            assert again == tot
        r["steady_rebuild_wall_s"] = round(float(np.median(walls)), 6)
        r["steady_rebuild_events_s"] = round(float(np.median(evs)), 6)
        r["steady_rebuild_events_min_max_s"] = [round(min(evs), 6), round(max(evs), 6)]
        r["floor_bytes"] = int(n) * 8 + tot[0] * 12
        r["floor_bytes_over_steady_events_of_hbm_spec"] = round(r["floor_bytes"] / r["steady_rebuild_events_s"] / HBM_SPEC, 5)
        walls, nbytes = [], 0
        for _ in range(op.reps):
            t0 = time.perf_counter()
            nbytes = ch.coverage_text(name)
            got = sum(len(mv) for mv in ch.coverage_iter())
            walls.append(time.perf_counter() - t0)
            assert got == nbytes
        r["text_bytes"] = int(nbytes)
        r["text_wall_s"] = round(float(np.median(walls)), 6)
        r["text_bytes_per_s"] = round(nbytes / float(np.median(walls)), 1)
        gs, ge, gd = ch.coverage_runs()
        ch.close()
        hw = []
        for _ in range(op.host_reps):
            t0 = time.perf_counter()
            hs, he, hd = host_runs(X, Y, ext, res)
            hw.append(time.perf_counter() - t0)
        if hw:                                                         # --host-reps 0: the device alone (a run under a profiler)
            same = bool(np.array_equal(hs, gs) and np.array_equal(he, ge) and np.array_equal(hd, gd))
            r["host_numpy"] = {"label": "events oracle in numpy, one core", "reps": op.host_reps, "median_s": round(float(np.median(hw)), 3),
                               "runs_equal_gpu": same}
            r["gpu_first_build_faster_than_host"] = bool(r["first_build_s"] < r["host_numpy"]["median_s"])
            ok = ok and same
        out["settings"][label] = r
    js = json.dumps(out, indent=1)
    print(js)
    if op.out:
        os.makedirs(os.path.dirname(os.path.abspath(op.out)), exist_ok=True)
        with open(op.out, "w") as fh:
            fh.write(js)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
