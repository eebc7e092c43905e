"""What the distance-cutoff pictures (`plot`, K17) add to a sweep: one runSweepFast with and without them over the synthetic
genome of tools/sweep_bench.py, and collect / evaluate timed on their own on chr1 for the last step.

    python tools/plot_timing.py [n_total] [mode] [out_prefix]
"""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cloops_amd import pipe
from cloops_amd.synth import synth_genome

MODES = {1: ([500, 1000, 2000], [5]), 2: ([1000, 2000, 5000], [5]), 3: ([5000, 7500, 10000], [50, 40, 30, 20]),
         4: ([2500, 5000, 7500, 10000], [30, 20])}          # cLoops/pipe.py:329-344
n_total = int(float(sys.argv[1])) if len(sys.argv) > 1 else 40000000
mode = int(sys.argv[2]) if len(sys.argv) > 2 else 4
prefix = sys.argv[3] if len(sys.argv) > 3 else os.path.join(tempfile.mkdtemp(), "plot")
eps, minPts = MODES[mode]
fs = [pipe.CACHE.put_arrays("%s-%s" % (name, name), X, Y) for name, X, Y in synth_genome(n_total, cfg=mode)]
print("%d chromosomes, mode %d" % (len(fs), mode), flush=True)
for rep, plot in enumerate((None, prefix, None, prefix)):
    t0 = time.perf_counter()
    dataI, cut, cuts, steps = pipe.runSweepFast(fs, eps, minPts, cut=0, plot=plot)
    dt = time.perf_counter() - t0
    print("rep %d plot=%s: sweep %.3f s, sum wall_s %.3f s, sum plot_s %.3f s (%d of %d steps drawn); cuts %s" % (
        rep, plot is not None, dt, sum(s["wall_s"] for s in steps), sum(s.get("plot_s", 0.0) for s in steps),
        sum("kde" in s for s in steps), len(steps), [s.get("cut_out") for s in steps]), flush=True)
    if plot is not None:
        print("   plot_s per step: %s" % " ".join("%.4f" % s.get("plot_s", 0.0) for s in steps), flush=True)
# chr1 on its own: the handle still holds the last step's run
st = steps[-1]
r = pipe.CACHE.get(fs[0])
for rep in range(3):
    t0 = time.perf_counter()
    col = r.chrom.dist_collect(st["cut_in"])
    t1 = time.perf_counter()
    tk = []
    for g in (0, 1):
        grid, h = st["kde"]["grid"][g], st["kde"]["h"][g]
        t2 = time.perf_counter()
        r.chrom.dist_kde(g, grid[0], grid[1] - grid[0], 1.0 / h, len(grid))
        tk.append(time.perf_counter() - t2)
    print("chr1 (%d PETs) rep %d: collect %.2f ms (n_pos %s), evaluate inter %.2f ms + self %.2f ms at G = %d" % (
        len(r), rep, (t1 - t0) * 1e3, col["n_pos"], tk[0] * 1e3, tk[1] * 1e3, len(grid)), flush=True)
