"""Timing of K11 (cl_quant_counts) and of the two command paths built on it (cloops_amd.quant / cloops_amd.deloops) on the
benchmark genome: the candidate loops of the 200 M-PET mode-3 sweep (bench.py's workload, cloops_amd.synth) quantified
against that genome (dataset A) and against a seeded subsample of it (dataset B, resident through Chromosome.subsample).

Reports, as one JSON document (stdout, and the file given by --out):
  per chromosome   loops, PETs, wall of the first quant_counts call (builds K8's sorted tables) and of a warm one (the
                   launch + the windows / counts copies), and K11's bytes moved (model below)
  whole commands   wall of quantifyLoops on A and on B and of callDeLoops A vs B, .jd loading excluded (chromosomes resident)
  host reference   a host restatement of the reference's counting (a coordinate -> PET-ids dict per axis, np.searchsorted +
                   set unions / intersections per window, 1 + 100 pair counts per loop as quantifyLoops does) on a SAMPLE of
                   loops of one chromosome, extrapolated linearly to all loops -- labelled as an extrapolation
Kernel times proper come from running this under `rocprofv3 --kernel-trace --stats` (k11_quant rows).

Bytes model per record: the 44 window words, the X-table slice of the A span (8 B per entry), the two Y-table slices of
A_0 and B_0 (8 B per entry), 7 binary searches of ceil(log2 m) + 1 probes at one 64-B line each, the 123 output words.

    timeout -k 10 900 python tools/quant_timing.py [--n-total 2e8] [--frac 0.6] [--sample 200] [--out FILE]
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

HBM_MEASURED = 6.29e12          # B/s, float4 copy on MI355X
HBM_SPEC = 8.0e12


def k11_bytes(X, Y, wins, m):
    lo, hi = wins[:, :22].astype(np.int64), wins[:, 22:].astype(np.int64)
    xs, ys = np.sort(X), np.sort(Y)
    span = np.searchsorted(xs, hi[:, :11].max(1), "right") - np.searchsorted(xs, lo[:, :11].min(1), "left")
    ya = np.searchsorted(ys, hi[:, 0], "right") - np.searchsorted(ys, lo[:, 0], "left")
    yb = np.searchsorted(ys, hi[:, 11], "right") - np.searchsorted(ys, lo[:, 11], "left")
    probes = 7 * (math.ceil(math.log2(max(m, 2))) + 1) * 64
    return int((8 * (np.maximum(span, 0) + np.maximum(ya, 0) + np.maximum(yb, 0))).sum() + len(wins) * (176 + probes + 492))


class HostModel(object):
    """host restatement of the reference's coverage model: per axis the sorted distinct coordinates and coordinate -> ids"""

    def __init__(self, X, Y):
        self.axes = []
        for v in (X, Y):
            d = {}
            for i, c in enumerate(v.tolist()):
                d.setdefault(c, []).append(i)
            self.axes.append((np.sort(np.fromiter(d.keys(), np.int64, len(d))), d))

    def ids(self, iv, axis):
        keys, d = self.axes[axis]
        a, b = np.searchsorted(keys, iv[0], side="left"), np.searchsorted(keys, iv[1], side="right")
        ps = []
        for i in range(a, b):
            ps.extend(d[keys[i]])
        return set(ps)

    def pets_for_regions(self, iva, ivb):
        ras, rat, rbs, rbt = self.ids(iva, 0), self.ids(iva, 1), self.ids(ivb, 0), self.ids(ivb, 1)
        return len(ras | rat), len(rbs | rbt), len(ras & rbt)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-total", type=float, default=2e8)
    ap.add_argument("--frac", type=float, default=0.6, help="dataset B keeps this fraction of every chromosome's PETs")
    ap.add_argument("--sample", type=int, default=200, help="loops of the host reference sample")
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    op = ap.parse_args(argv)
    import bench
    from cloops_amd import api, cModel, deloops, pipe, quant
    from cloops_amd.synth import chrom_sizes, synth_chrom
    out = {"n_total": int(op.n_total), "frac_B": op.frac}
    t0 = time.perf_counter()
    fs, host = [], {}
    for ci, (name, length, n) in enumerate(chrom_sizes(int(op.n_total))):
        X, Y = synth_chrom(n, length, 1000 * bench.CFG + ci)
        fs.append(pipe.CACHE.put_arrays("%s-%s" % (name, name), X, Y))
        host[fs[-1]] = (X, Y)
    out["synthesis_s"] = round(time.perf_counter() - t0, 2)
    t0 = time.perf_counter()
    dataI, cut, cuts, steps = pipe.runSweepFast(fs, bench.MODE3[0], bench.MODE3[1], cut=0, variant=bench.VARIANT)
    out["sweep_s"] = round(time.perf_counter() - t0, 3)
    out["final_cut"] = int(cut)
    # the candidate loops per chromosome, and dataset B
    ra, rb = {}, {}
    rng = np.random.default_rng(7)
    chroms = []
    for f in fs:
        r = pipe.CACHE.get(f)
        key = r.key[0]
        boxes = np.asarray(dataI[r.key]["boxes"] if r.key in dataI else np.zeros((0, 4)), np.int64).reshape(-1, 4)
        if len(boxes) == 0:
            continue
        rs = {"%s-%s-%d" % (key, key, i): [key, int(b[0]), int(b[1]), key, int(b[2]), int(b[3])] for i, b in enumerate(boxes)}
        X, Y = host[f]
        rows = np.flatnonzero(rng.random(len(X)) < op.frac).astype(np.int32)
        fb = pipe.CACHE.put_chrom("mem://B/%s-%s" % (key, key), r.chrom.subsample(rows), X[rows], Y[rows], key=r.key)
        ra[key] = {"rs": rs, "f": f}
        rb[key] = {"rs": rs, "f": fb}
        chroms.append((key, f, fb, rs))
    # K11 per chromosome
    per, tot_bytes, tot_warm = [], 0, 0.0
    for key, f, fb, rs in chroms:
        wins = quant._loop_windows(rs)
        ch = pipe.CACHE.get(f).chrom
        t0 = time.perf_counter()
        _, N = ch.quant_counts(wins, 0)
        cold = time.perf_counter() - t0
        warm = []
        for _ in range(5):
            t0 = time.perf_counter()
            ch.quant_counts(wins, 0)
            warm.append(time.perf_counter() - t0)
        X, Y = host[f]
        nb = k11_bytes(X, Y, wins, N)
        w = float(np.median(warm))
        tot_bytes += nb
        tot_warm += w
        per.append({"chrom": key, "loops": len(rs), "pets": int(N), "first_call_s": round(cold, 5), "warm_call_s": round(w, 6),
                    "k11_bytes": nb, "bytes_per_warm_call_s_TBps": round(nb / w / 1e12, 4)})
    out["per_chrom"] = per
    out["loops_total"] = int(sum(p["loops"] for p in per))
    out["k11_bytes_total"] = int(tot_bytes)
    out["k11_warm_calls_s_total"] = round(tot_warm, 5)
    out["k11_bytes_over_warm_calls_vs_hbm"] = {"TBps": round(tot_bytes / tot_warm / 1e12, 4),
                                               "of_measured_6.29": round(tot_bytes / tot_warm / HBM_MEASURED, 5),
                                               "of_spec_8.0": round(tot_bytes / tot_warm / HBM_SPEC, 5)}
    # whole commands on resident chromosomes
    with tempfile.TemporaryDirectory() as td:
        for tag, recs in (("quantifyLoops_A_s", ra), ("quantifyLoops_B_s", rb)):
            t0 = time.perf_counter()
            quant.quantifyLoops(recs, os.path.join(td, "q"))
            out[tag] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        deloops.callDeLoops(ra, rb, os.path.join(td, "A"), os.path.join(td, "B"))
        out["callDeLoops_s"] = round(time.perf_counter() - t0, 3)
    # the reference-shaped host path on a sample, extrapolated
    key, f, fb, rs = min(chroms, key=lambda c: len(host[c[1]][0]))
    X, Y = host[f]
    t0 = time.perf_counter()
    model = HostModel(X, Y)
    build_s = time.perf_counter() - t0
    items = list(rs.values())[:op.sample]
    wins = cModel._windows(items)[3]
    counts, _ = pipe.CACHE.get(f).chrom.quant_counts(wins, 0)
    t0 = time.perf_counter()
    mism = 0
    for q, r in enumerate(items):
        ra0, rb0, rab0 = model.pets_for_regions([r[1], r[2]], [r[4], r[5]])
        mism += (ra0, rb0, rab0) != (counts[q, 0], counts[q, 1], counts[q, 2])
        for k in range(1, 11):
            for l in range(1, 11):
                mism += model.pets_for_regions([wins[q, k], wins[q, 22 + k]], [wins[q, 11 + l], wins[q, 33 + l]])[2] != counts[q, 2 + 11 * k + l]
    per_loop = (time.perf_counter() - t0) / max(1, len(items))
    out["host_reference_shaped"] = {
        "label": "EXTRAPOLATED from a sample: host restatement of the reference's set counting, one core",
        "sample_chrom": key, "sample_chrom_pets": int(len(X)), "sample_loops": len(items), "model_build_s": round(build_s, 2),
        "per_loop_s": round(per_loop, 5), "count_mismatches_vs_k11": int(mism),
        "extrapolated_all_loops_s": round(per_loop * out["loops_total"], 1)}
    pipe.CACHE.clear()
    js = json.dumps(out, indent=1)
    print(js)
    if op.out:
        with open(op.out, "w") as fh:
            fh.write(js)
    return 0


if __name__ == "__main__":
    sys.exit(main())
