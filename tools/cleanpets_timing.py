"""Timing of K13 (cl_anchor_mask) and of the command path built on it (cloops_amd.cleanpets) on the benchmark genome: the 200 M-PET
genome of bench.py (cloops_amd.synth), resident, with two anchor sets per chromosome:
  sig   the anchors of a seeded sample of --sig-loops candidate loops per chromosome (a significant-loop-sized set)
  all   the anchors of every candidate loop of the mode-3 sweep (3.65 M loops genome-wide), obtained as quant_timing.py does

Reports, as one JSON document (stdout, and the file given by --out):
  per chromosome and set   rows, anchors, merged anchors, kept rows, wall of the first anchor_mask call and the median of 5 warm
                           ones (host merge, anchor upload, kernels, mask copy), and the kernel's bytes per launch
                           (8 B per row read + n / 8 written + 8 B per merged anchor staged) over the warm call vs HBM peak
  chr1 sizes               chr1 with disjoint anchor sets of SIZES merged anchors (the crossover of the two search forms)
  whole command            jd2cleanWashuPETs on the resident chromosomes (kept rows written as .jd files), and the write + read of
                           chr1's .jd alone (what a command on .jd directories adds per chromosome)
  host reference           the script's pairwise merge and its dict / set loop restated on the host over a sample, extrapolated
                           (merge: quadratically in the anchors; the loop: linearly in rows + kept rows) -- labelled as such
Kernel times proper come from running this under `rocprofv3 --kernel-trace --stats` (k13_mask / k13_dir rows).  The developer
library (CLOOPS_DEVEL_LIB=1, python -m cloops_amd.build --devel) with CLOOPS_K13_LDS=0 times the directory form on every set.

    timeout -k 10 900 python tools/cleanpets_timing.py [--n-total 2e8] [--sig-loops 1000] [--sample 3000] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

HBM_SPEC = 8.0e12
SIZES = (16, 64, 128, 200, 256, 257, 512, 1024)


def host_merge(anchors):
    """the script's mergeAllAnchors (pairwise, greedy) repeated until nothing merges, restated"""
    while True:
        nrs, skips = [], set()
        for i in range(len(anchors)):
            if i in skips:
                continue
            a, b = anchors[i]
            for j in range(i + 1, len(anchors)):
                if j in skips:
                    continue
                c, d = anchors[j]
                if c <= a <= d or c <= b <= d or a <= c <= b or a <= d <= b:
                    skips.add(j)
                    a, b = min(a, c), max(b, d)
            nrs.append([a, b])
        if len(nrs) == len(anchors):
            return nrs
        anchors = nrs


def host_rows(X, Y, anchors):
    """the script's coordinate -> rows dicts, closed searchsorted per anchor and set updates, restated -> sorted rows"""
    links = []
    for v in (X, Y):
        ts = {}
        for i, c in enumerate(v.tolist()):
            ts.setdefault(c, []).append(i)
        links.append((np.sort(v), ts))
    ps = set()
    for s, e in anchors:
        for keys, ts in links:
            for i in range(np.searchsorted(keys, s, side="left"), np.searchsorted(keys, e, side="right")):
                ps.update(ts[keys[i]])
    return np.array(sorted(ps), np.int64)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-total", type=float, default=2e8)
    ap.add_argument("--sig-loops", type=int, default=1000, help="loops per chromosome of the significant-sized set")
    ap.add_argument("--sample", type=int, default=3000, help="anchors of the host merge sample")
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    op = ap.parse_args(argv)
    import bench
    from cloops_amd import cleanpets, pipe
    from cloops_amd.synth import chrom_sizes, synth_chrom
    out = {"n_total": int(op.n_total), "sig_loops_per_chrom": op.sig_loops, "devel_k13_lds": os.environ.get("CLOOPS_K13_LDS")}
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
    rng = np.random.default_rng(13)
    sets = {"sig": {}, "all": {}}
    for f in fs:
        r = pipe.CACHE.get(f)
        key = r.key[0]
        boxes = np.asarray(dataI[r.key]["boxes"] if r.key in dataI else np.zeros((0, 4)), np.int64).reshape(-1, 4)
        if len(boxes) == 0:
            continue
        rs = {"%s-%s-%d" % (key, key, i): [key, int(b[0]), int(b[1]), key, int(b[2]), int(b[3])] for i, b in enumerate(boxes)}
        pick = sorted(rng.choice(len(boxes), min(op.sig_loops, len(boxes)), replace=False).tolist())
        ids = list(rs.keys())
        sets["all"][f] = rs
        sets["sig"][f] = {ids[i]: rs[ids[i]] for i in pick}
    out["loops_total"] = {k: int(sum(len(v) for v in s.values())) for k, s in sets.items()}
    for tag, s in sets.items():
        per, tot_warm, tot_bytes = [], 0.0, 0
        for f, rs in s.items():
            ch = pipe.CACHE.get(f).chrom
            starts, ends = cleanpets._anchor_pool(rs)
            t0 = time.perf_counter()
            _, nm, nk = ch.anchor_mask(starts, ends)
            cold = time.perf_counter() - t0
            warm = []
            for _ in range(5):
                t0 = time.perf_counter()
                ch.anchor_mask(starts, ends)
                warm.append(time.perf_counter() - t0)
            w = float(np.median(warm))
            nb = 8 * ch.n + (ch.n + 63) // 64 * 8 + 8 * nm
            tot_warm += w
            tot_bytes += nb
            per.append({"chrom": f[len("mem://"):], "rows": ch.n, "anchors": len(starts), "merged": nm, "kept": nk,
                        "first_call_s": round(cold, 5), "warm_call_s": round(w, 6), "k13_bytes": nb,
                        "bytes_over_warm_call_of_hbm_spec": round(nb / w / HBM_SPEC, 4)})
        out["set_" + tag] = {"per_chrom": per, "warm_calls_s_total": round(tot_warm, 5), "k13_bytes_total": int(tot_bytes),
                             "bytes_over_warm_calls_of_hbm_spec": round(tot_bytes / tot_warm / HBM_SPEC, 4)}
    # chr1 with 10^6 seeded random anchors of up to 2 kb: a merged set far beyond the LDS form (the directory form's regime)
    f1 = fs[0]
    ch = pipe.CACHE.get(f1).chrom
    X, Y = host[f1]
    starts = rng.integers(int(X.min()), int(Y.max()), 1000000)
    ends = starts + rng.integers(0, 2000, 1000000)
    ch.anchor_mask(starts, ends)
    warm = []
    for _ in range(5):
        t0 = time.perf_counter()
        _, nm, nk = ch.anchor_mask(starts, ends)
        warm.append(time.perf_counter() - t0)
    out["chr1_random_1e6"] = {"rows": ch.n, "anchors": len(starts), "merged": nm, "kept": nk, "warm_call_s": round(float(np.median(warm)), 6),
                              "k13_bytes": 8 * ch.n + (ch.n + 63) // 64 * 8 + 8 * nm}
    # chr1 with disjoint 2 kb anchors, merged sets of exactly SIZES[k] anchors: where the two search forms cross (the launches come in
    # this order, 1 + 5 per size, after the sets above; the developer library with CLOOPS_K13_LDS=0 gives the directory form's times)
    span = (int(X.min()), int(Y.max()))
    out["chr1_sizes"] = []
    for k in SIZES:
        starts = np.sort(rng.choice((span[1] - span[0]) // 4000, k, replace=False)) * 4000 + span[0]
        ends = starts + 1999
        ch.anchor_mask(starts, ends)
        warm = []
        for _ in range(5):
            t0 = time.perf_counter()
            _, nm, nk = ch.anchor_mask(starts, ends)
            warm.append(time.perf_counter() - t0)
        out["chr1_sizes"].append({"merged": nm, "kept": nk, "warm_call_s": round(float(np.median(warm)), 6)})
    # whole command on the resident chromosomes, and the .jd I/O of one chromosome
    import joblib
    with tempfile.TemporaryDirectory() as td:
        for tag, s in sets.items():
            recs = {f: {"rs": rs, "f": f} for f, rs in s.items()}
            o = os.path.join(td, tag)
            os.mkdir(o)
            t0 = time.perf_counter()
            ds = [cleanpets.getAnchorPETs(recs[k]["f"], recs[k]["rs"], o) for k in recs]
            out["command_resident_%s_s" % tag] = round(time.perf_counter() - t0, 3)
            out["kept_%s" % tag] = int(sum(d[3] for d in ds))
            out["ratio_%s" % tag] = sum(d[3] for d in ds) / 1.0 / sum(d[2] for d in ds)
        X, Y = host[fs[0]]
        mat = np.stack([np.arange(len(X)), X, Y], 1).astype(np.int64)
        jd = os.path.join(td, "chr1-chr1.jd")
        t0 = time.perf_counter()
        joblib.dump(mat, jd)
        out["chr1_jd_write_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        pipe.parseJd(jd)
        out["chr1_jd_read_s"] = round(time.perf_counter() - t0, 3)
        out["chr1_rows"] = int(len(X))
    # the script's way on the host, over samples, extrapolated
    f = min(sets["sig"], key=lambda g: len(host[g][0]))
    rs = sets["sig"][f]
    starts, ends = cleanpets._anchor_pool(rs)
    pool = [[int(a), int(b)] for a, b in zip(starts, ends)]
    sample = pool[:op.sample]
    t0 = time.perf_counter()
    host_merge(sample)
    tm = time.perf_counter() - t0
    X, Y = host[f]
    t0 = time.perf_counter()
    rows = host_rows(X, Y, host_merge(pool))
    tl = time.perf_counter() - t0
    mask, nm, nk = pipe.CACHE.get(f).chrom.anchor_mask(starts, ends)
    same = bool(np.array_equal(rows, pipe.CACHE.get(f).chrom.rows_of_mask(mask)))
    extra_merge = {tag: round(sum(tm * (2 * len(rs2) / len(sample)) ** 2 for rs2 in s.values()), 1) for tag, s in sets.items()}
    rows_total = sum(len(host[g][0]) for g in fs)
    out["host_reference_shaped"] = {
        "label": "EXTRAPOLATED from samples: host restatement of the script's merge and set loop, one core",
        "merge_sample_anchors": len(sample), "merge_sample_s": round(tm, 3),
        "merge_extrapolated_quadratic_s": extra_merge,
        "loop_sample_chrom": f[len("mem://"):], "loop_sample_rows": int(len(X)), "loop_sample_anchors": len(pool),
        "loop_sample_s": round(tl, 2), "loop_rows_equal_k13": same,
        "loop_extrapolated_linear_in_rows_s": round(tl * rows_total / len(X), 1)}
    pipe.CACHE.clear()
    js = json.dumps(out, indent=1)
    print(js)
    if op.out:
        with open(op.out, "w") as fh:
            fh.write(js)
    return 0


if __name__ == "__main__":
    sys.exit(main())
