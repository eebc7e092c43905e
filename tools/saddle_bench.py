"""Timing of K30 (cl_sad_sums) on one chr1-sized chromosome, against K26's cl_exp_diagonals in the same process on the same state.

The chromosome is chr1 of the 200 M-PET genome of bench.py (cloops_amd.synth, 16.4 M PETs, the same seed); the cells are K24's folded
ones at 100 kb and at 10 kb, balanced by K25 and given expected values by K26 at the defaults of cloops_amd.saddle; the track is K27's
first vector, the classes those of Q = 50 (`saddle.edges_of` / `saddle.classes_of`).  Reports, as one JSON document (stdout, and --out,
by default profiles/saddle_timing.json), in wall clock (every call ends in a stream synchronise), medians of --reps after a warm-up:
  sad_sums_s          cl_sad_sums: the host's look at K26's state, the pair counts, the sums over the cells, the tables back
  exp_diagonals_s     cl_exp_diagonals: the yardstick -- it builds a sort over the same cells and sums them by key
  bytes_per_cell      what the sums must read of a cell: bx, by, cnt (12 bytes; the weights, classes and expected values are gathered
                      from nb-sized arrays that stay in cache)
  no_slower           sad_sums_s <= exp_diagonals_s: the target
  --trace-only        the calls alone, for one `rocprofv3 --kernel-trace --stats` run of its own that names the kernel that takes the time
and the lines of cloops_amd/saddle.py set against cloops_amd/compartments.py (the command's own host code beside its sibling's).

    timeout -k 10 600 python tools/saddle_bench.py [--reps 5] [--out FILE]
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/saddle_bench.py --trace-only
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def say(msg):
    sys.stderr.write("saddle_bench: %s\n" % msg)
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


def code_lines(path):
    """the lines of a module that are neither blank nor part of its leading docstring"""
    with open(path) as fh:
        text = fh.read()
    body = text.split('"""', 2)[2] if text.startswith('"""') else text
    return sum(1 for line in body.splitlines() if line.strip())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-total", type=float, default=2e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--q", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "saddle_timing.json"))
    ap.add_argument("--trace-only", action="store_true", help="the calls of a kernel trace: no timing, no file")
    op = ap.parse_args(argv)
    import torch
    import bench
    from cloops_amd import api, balance, compartments, expected, saddle
    from cloops_amd.synth import chrom_sizes, synth_chrom
    name, length, n = chrom_sizes(int(op.n_total))[0]
    X, Y = synth_chrom(n, length, 1000 * bench.CFG)
    src = os.path.join(ROOT, "cloops_amd")
    out = {"chrom": name, "pets": int(n), "device": torch.cuda.get_device_name(0), "reps": op.reps, "q": op.q, "cases": {},
           "host_lines": {"saddle.py": code_lines(os.path.join(src, "saddle.py")), "compartments.py": code_lines(os.path.join(src, "compartments.py"))}}
    ch = api.Chromosome(X, Y)
    for label, res in (("100kb", 100000), ("10kb", 10000)):
        c = out["cases"][label] = {"res": res}
        n_cells = ch.mat_cells(res, fold=True)[0]
        b0, nb, _ = ch.bal_marginals(2)
        s, z = ch.bal_marginals_get()
        ch.bal_iterate(balance.valid_bins(s, z))
        valid = ~np.isnan(ch.bal_weights())
        if op.trace_only:
            ch.exp_diagonals()
        else:
            _, c["exp_diagonals_s"] = walls(op.reps, lambda: ch.exp_diagonals())
        p, _, vs = ch.exp_diagonals_get()
        e, _ = expected.expected_of(p, vs, 2)
        ch.exp_set(e)
        hi = min(compartments.pick_dmax(p, e, 2), nb)
        oe = np.concatenate([ch.exp_cells_get(f, min(1 << 22, n_cells - f)) for f in range(0, n_cells, 1 << 22)])
        ch.eig_build(compartments.clip_of(oe, 99.9), hi)
        ch.eig_iterate(1)
        track = ch.eig_vectors(0)
        ch.eig_free()
        cls = saddle.classes_of(track, valid, saddle.edges_of(track, op.q))
        if op.trace_only:
            ch.sad_sums(cls, op.q + 2, 2, hi)
            continue
        (n_binned, n_pairs, n_in), t = walls(op.reps, lambda: ch.sad_sums(cls, op.q + 2, 2, hi))
        tables = ch.sad_get()
        c.update(n_cells=int(n_cells), nb=int(nb), lo=2, hi=int(hi), n_binned=int(n_binned), n_pairs=int(n_pairs), n_in=int(n_in),
                 sad_sums_s=float("%.4g" % t), exp_diagonals_s=float("%.4g" % c["exp_diagonals_s"]), bytes_per_cell=12,
                 cell_bytes_per_s=float("%.4g" % (12.0 * n_cells / t)), no_slower=bool(t <= c["exp_diagonals_s"]),
                 strength=saddle.strength_of(tables[0], tables[1], 0.2)["strength"])
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
    return 0


if __name__ == "__main__":
    sys.exit(main())
