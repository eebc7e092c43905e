#!/usr/bin/env python
"""developer tool (CPU only): what a floor at half the incoming cut would leave out of an eps' base layout on the bench genome.

For chr1 and chr21 of the synthetic 200 M genome (bench.py's seeds) and every step of the recorded mode-3 chain it prints the share
of the rows with Y - X below cut_in / 2, and whether a later cut_in of the same eps falls below the floor that the eps' first
run under a cut would set (that run would rebuild the layout with every row).

    python tools/layout_floor_shares.py [chromosome index ...]      (default: 0 20)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cloops_amd.synth import synth_chrom, chrom_sizes      # noqa: E402

N_TOTAL, CFG = 200000000, 3
EPS, MINPTS = [5000, 7500, 10000], [50, 40, 30, 20]
CHAIN = [4536, 6098, 6306, 5711, 3871, 5004, 5256, 5517, 4896, 5977, 6250, 6428]      # cut_out of the 12 steps (docs/history_r1-r4.md)


def main(argv):
    which = [int(a) for a in argv] or [0, 20]
    cut_in = [0] + CHAIN[:-1]
    sizes = chrom_sizes(N_TOTAL)
    for ci in which:
        name, length, n = sizes[ci]
        X, Y = synth_chrom(n, length, 1000 * CFG + ci)
        d = np.sort(Y.astype(np.int64) - X)
        print("%s: %d rows" % (name, n))
        step = 0
        for ep in EPS:
            floor = None
            for m in MINPTS:
                c = cut_in[step]
                if floor is None:                        # the eps' layout is built by its first run
                    floor = c // 2
                    built = ("builds the layout, floor %d" % floor) if c > 0 else "builds the layout, no cut: every row"
                elif c < floor:
                    built, floor = "REBUILD with every row (cut below the floor %d)" % floor, 0
                else:
                    built = "same layout (floor %d)" % floor
                below_half = int(np.searchsorted(d, c // 2, "left"))
                below_cut = int(np.searchsorted(d, c, "left"))
                print("  step %2d eps %5d minPts %2d cut_in %4d: %.4f of the rows below cut_in / 2, %.4f below cut_in (%.3f of those below half); %s"
                      % (step, ep, m, c, below_half / float(n), below_cut / float(n), below_half / float(max(1, below_cut)), built))
                step += 1


if __name__ == "__main__":
    main(sys.argv[1:])
