"""Timing of K25 (cl_bal_marginals / cl_bal_iterate) on one chr1-sized chromosome, against the numpy oracle on the same cells.

The chromosome is chr1 of the 200 M-PET genome of bench.py (cloops_amd.synth, 16.4 M PETs, the same seed); the cells are K24's folded
ones at 10 kb and at 1 kb.  Reports, as one JSON document (stdout, and --out, by default profiles/balance_timing.json), each figure as
the median of --reps runs after a warm-up call, in wall clock (every call ends in a stream synchronise) and between two events recorded
on the handle's stream around the call:
  marginals           cl_bal_marginals: the transposed order (keys, radix sort of pairs, gather) and the integer pass
  iterate_1 / _17 / _33   cl_bal_iterate with tol = 0 and that many iterations: one, two and three blocks of enqueued iterations.  Their
                      slope is one full iteration (two marginal passes in one launch, the carry fold, the three kernels of the update);
                      what is left of iterate_1 is the call's fixed cost (the mask's copy, the init, the record's read, the weights)
  balance             the whole balance at the defaults of cloops_amd.balance: marginals to the host, the mask, cl_bal_iterate to
                      tol 1e-5 (at most 200 iterations), the weights to the host
  bytes_per_iteration 12 bytes x 2 orders x cells (bin, other bin, count), and the GB/s that makes over one iteration
against the oracle of tests/balance_cases.py on one core over the same cells (np.bincount: one iteration, and the whole balance), with
the iteration counts of both and the largest relative difference of the weights.

    timeout -k 10 900 python tools/balance_bench.py [--reps 5] [--out FILE]
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
    sys.stderr.write("balance_bench: %s\n" % msg)
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


def host_time(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, round(time.perf_counter() - t0, 4)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-total", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "balance_timing.json"))
    op = ap.parse_args(argv)
    import torch
    import bench
    import balance_cases as BC
    from cloops_amd import api, balance
    from cloops_amd.synth import chrom_sizes, synth_chrom
    name, length, n = chrom_sizes(int(op.n_total))[0]
    X, Y = synth_chrom(n, length, 1000 * bench.CFG)
    out = {"chrom": name, "pets": int(n), "device": torch.cuda.get_device_name(0), "reps": op.reps, "cases": {}}
    ok = True
    stream = torch.cuda.Stream()
    ch = api.Chromosome(X, Y, stream=stream.cuda_stream)
    for label, res in (("10kb", 10000), ("1kb", 1000)):
        c = out["cases"][label] = {"res": res}
        n_cells = ch.mat_cells(res, fold=True)[0]
        bx, by, cnt = ch.mat_cells_get()
        (b0, nb, n_used), c["marginals"] = timed(stream, op.reps, lambda: ch.bal_marginals(2))
        c.update(n_cells=int(n_cells), nb=int(nb), n_used=int(n_used), bytes_per_iteration=int(n_cells) * 24)
        want, c["numpy_marginals_s"] = host_time(lambda: BC.marginals_oracle(bx, by, cnt, 2))
        s, z = ch.bal_marginals_get()
        same = (b0, nb, n_used) == want[:3] and np.array_equal(s, want[3]) and np.array_equal(z, want[4])
        valid = balance.valid_bins(s, z)
        c["n_valid"] = int(valid.sum())
        for k in (1, 17, 33):
            r, c["iterate_%d" % k] = timed(stream, op.reps, lambda: ch.bal_iterate(valid, max_iters=k, tol=0.0))
            same &= r[0] == k
        per = (c["iterate_33"]["events_s"] - c["iterate_1"]["events_s"]) / 32
        c["one_iteration_s"] = round(per, 7)
        c["call_fixed_s"] = round(c["iterate_1"]["events_s"] - per, 7)
        c["GBps"] = round(c["bytes_per_iteration"] / per / 1e9, 1)

        def whole():
            s, z = ch.bal_marginals_get()
            r = ch.bal_iterate(balance.valid_bins(s, z))
            return r, ch.bal_weights()
        (r, w), c["balance"] = timed(stream, max(2, op.reps // 2), whole)
        _, c["numpy_one_iteration_s"] = host_time(lambda: BC.ice_oracle(bx, by, cnt, 2, valid, 1, 0.0))
        o, c["numpy_balance_s"] = host_time(lambda: BC.ice_oracle(bx, by, cnt, 2, valid, 200, 1e-5))
        c.update(iters=r[0], converged=bool(r[1]), var=r[2], numpy_iters=o["iters"], numpy_var=o["var"],
                 weights_rel_diff=BC.rel_diff(w, o["weight"]), one_step_bound=BC.one_step_bound(bx, by, 2))
        c["speedup_one_iteration"] = round(c["numpy_one_iteration_s"] / per, 1)
        c["speedup_balance"] = round(c["numpy_balance_s"] / c["balance"]["wall_s"], 1)
        c["equal_numpy"] = bool(same and r[0] == o["iters"] and bool(r[1]) == o["converged"])
        ok &= c["equal_numpy"]
        say("%s %s" % (label, c))
    ch.mat_free()
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
