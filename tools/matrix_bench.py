"""Timing of K24 (cl_mat_window / cl_mat_cells / cl_mat_v4c) on one chr1-sized chromosome, against numpy on the same rows.

The chromosome is chr1 of the 200 M-PET genome of bench.py (cloops_amd.synth, 16.4 M PETs, the same seed).  Reports, as one JSON document
(stdout, and --out, by default profiles/matrix_timing.json), each case as the median of --reps runs after a warm-up call, in wall clock
(every call ends in a stream synchronise and includes the copy of its result to the host) and between two events recorded on the
handle's stream around the call, with the bytes of K19's table the kernels read (8 per row and phase), the GB/s that makes over the
event time, and the time numpy takes for the same integers on one core (np.add.at for the dense forms; np.unique over packed 64-bit
keys for the cells, the faster twin of the oracle's np.unique(axis=0)); every GPU result is compared with numpy's:
  window              a 1000 x 1000 diagonal mirrored window at 5 kb in the middle of the chromosome (the strip path: LDS counters over a
                      tile's X bins x 1000)
  window_global       the same window with every add a global atomic          } --devel only: the developer build reads
  window_agg          the same window with wave aggregation in front of the   } CLOOPS_K24_GLOBAL / CLOOPS_K24_AGG at every call; the
                      LDS atomics                                             } shipped library has one form and no switch
  window_small        a 90 x 90 window at 5 kb (the whole window in LDS)
  cells_10kb / _1kb   the folded cells of the chromosome, and the copy of all of them to the host (get)
  v4c                 a 10 kb viewpoint over the whole chromosome at 1 kb (248 957 bins: above the LDS budget)

    timeout -k 10 900 python tools/matrix_bench.py [--reps 5] [--devel] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def say(msg):
    sys.stderr.write("matrix_bench: %s\n" % msg)
    sys.stderr.flush()


def timed(stream, reps, fn):
    """-> (result of the last run, figures); one warm-up call, then `reps` timed ones"""
    import torch
    fn()
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


def with_bytes(fig, rows):
    fig["table_rows"] = int(rows)
    fig["table_bytes"] = int(rows) * 8
    fig["GBps"] = round(fig["table_bytes"] / fig["events_s"] / 1e9, 2)
    return fig


def host_time(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, round(time.perf_counter() - t0, 4)


def packed_cells(X, Y, res, fold):
    bx, by = X.astype(np.int64) // res, Y.astype(np.int64) // res
    if fold:
        bx, by = np.minimum(bx, by), np.maximum(bx, by)
    u, c = np.unique(bx * (1 << 32) + by, return_counts=True)
    return (u >> 32).astype(np.int32), (u & 0xffffffff).astype(np.int32), c.astype(np.uint32)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-total", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--devel", action="store_true", help="load the developer build and time the window's other forms too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_timing.json"))
    op = ap.parse_args(argv)
    if op.devel:
        os.environ["CLOOPS_DEVEL_LIB"] = "1"
    import torch
    import bench
    import matrix_cases as MC
    from cloops_amd import api
    from cloops_amd.synth import chrom_sizes, synth_chrom
    name, length, n = chrom_sizes(int(op.n_total))[0]
    X, Y = synth_chrom(n, length, 1000 * bench.CFG)
    X64, Y64 = X.astype(np.int64), Y.astype(np.int64)
    out = {"chrom": name, "pets": int(n), "device": torch.cuda.get_device_name(0), "reps": op.reps, "devel": bool(op.devel), "cases": {}}
    cases, ok = out["cases"], True
    stream = torch.cuda.Stream()
    ch = api.Chromosome(X, Y, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ch.mat_window(5000, 0, 0, 8, 8)
    out["first_call_s"] = round(time.perf_counter() - t0, 6)                # the sort of K19's table included
    xs = np.sort(X64)

    def rows_with_bx(b0, nb, res):
        return int(np.searchsorted(xs, (b0 + nb) * res) - np.searchsorted(xs, b0 * res))

    # ---- windows
    res, nw = 5000, 1000
    b0 = int(length // 2 // res) - nw // 2
    rows = 2 * rows_with_bx(b0, nw, res)                                     # both phases read the window's X range
    want, t_np = host_time(lambda: MC.window_oracle(X64, Y64, 0, res, b0, b0, nw, nw, True))
    forms = [("window", {})]
    if op.devel:
        forms += [("window_global", {"CLOOPS_K24_GLOBAL": "1"}), ("window_agg", {"CLOOPS_K24_AGG": "1"})]
    for label, env in forms:
        os.environ.update(env)
        got, fig = timed(stream, op.reps, lambda: ch.mat_window(res, b0, b0, nw, nw, mirror=True))
        for k in env:
            del os.environ[k]
        cases[label] = with_bytes(fig, rows)
        cases[label].update(numpy_s=t_np, n_in=got[1], equal_numpy=bool(np.array_equal(got[0], want[0]) and got[1:] == want[1:]))
        ok &= cases[label]["equal_numpy"]
        say("%s %s" % (label, cases[label]))
    ns = 90
    want, t_np = host_time(lambda: MC.window_oracle(X64, Y64, 0, res, b0, b0, ns, ns, True))
    got, fig = timed(stream, op.reps, lambda: ch.mat_window(res, b0, b0, ns, ns, mirror=True))
    cases["window_small"] = with_bytes(fig, 2 * rows_with_bx(b0, ns, res))
    cases["window_small"].update(numpy_s=t_np, n_in=got[1], equal_numpy=bool(np.array_equal(got[0], want[0]) and got[1:] == want[1:]))
    ok &= cases["window_small"]["equal_numpy"]
    say("window_small %s" % cases["window_small"])
    # ---- cells
    for label, cres in (("cells_10kb", 10000), ("cells_1kb", 1000)):
        want, t_np = host_time(lambda: packed_cells(X64, Y64, cres, True))
        got, fig = timed(stream, max(2, op.reps // 2), lambda: ch.mat_cells(cres, fold=True))
        cells, gfig = timed(stream, 2, lambda: ch.mat_cells_get())
        cases[label] = with_bytes(fig, n)
        same = got[0] == len(want[0]) and all(np.array_equal(a, b) for a, b in zip(cells, want))
        cases[label].update(numpy_s=t_np, n_cells=got[0], max_count=got[2], get=gfig, equal_numpy=bool(same))
        ok &= bool(same)
        say("%s %s" % (label, cases[label]))
    ch.mat_free()
    # ---- virtual 4C
    vres = 1000
    v0 = int(length // 2)
    nb = int(length // vres) + 1
    want, t_np = host_time(lambda: MC.v4c_oracle(X64, Y64, 0, vres, v0, v0 + 10000, 0, nb))
    got, fig = timed(stream, op.reps, lambda: ch.mat_v4c(vres, v0, v0 + 10000, 0, nb))
    cases["v4c"] = with_bytes(fig, n + want[1])
    cases["v4c"].update(numpy_s=t_np, n_x=got[1], n_y=got[2], n_bins=nb, equal_numpy=bool(np.array_equal(got[0], want[0]) and got[1:] == want[1:]))
    ok &= cases["v4c"]["equal_numpy"]
    say("v4c %s" % cases["v4c"])
    ch.close()
    js = json.dumps(out, indent=1)
    print(js)
    if op.out:
        os.makedirs(os.path.dirname(os.path.abspath(op.out)), exist_ok=True)
        with open(op.out, "w") as fh:
            fh.write(js + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
