"""Timing of the 4DN pairs path (cloops_amd.pairs: load_pairs, K18; pairs2bedpe, K15 with CL_CONV_PAIRS) on one seeded synthetic
file (tests/pairs_cases.py gen_pairs) written to a temporary directory, plain and .gz, against the route that existed before the
format was read: the same data in HiC-Pro's column order (what an `awk` reshaping gives; not timed), `convert hicpro`
(cloops_amd.convert.pairs2bedpe, .bedpe.gz out) and then `load_bedpe` on its output.  Both routes run in alternation, `--reps`
times each, in the same call on the same machine.

Reports, as one JSON document (stdout, and the file given by --out):
  per input kind    wall seconds of every repetition of load_pairs, of pairs2bedpe (.bedpe.gz out) and of the two steps of the old
                    route; the host and device stage seconds of the last load_pairs; the lines and cis PETs read
  equal             whether both routes left the same chromosomes (names in order, X and Y of each) and the same BEDPE text

    timeout -k 10 1100 python tools/pairs_timing.py [--lines 2e7] [--reps 2] [--budget-mb 64] [--out FILE]
"""
import argparse
import collections
import gzip
import hashlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

BLOCK = 1 << 20


def resident_digest(pipe, names):
    h = hashlib.sha1()
    for nm in names:
        r = pipe.CACHE.get(nm)
        h.update(repr(r.key).encode() + np.ascontiguousarray(r.X, dtype=np.int64).tobytes() + np.ascontiguousarray(r.Y, dtype=np.int64).tobytes())
    return h.hexdigest()


def text_digest(path):
    h = hashlib.sha1()
    with gzip.open(path, "rb") as fh:
        for blob in iter(lambda: fh.read(16 << 20), b""):
            h.update(blob)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=float, default=2e7)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--budget-mb", type=int, default=64)
    ap.add_argument("--ext", type=int, default=50)
    ap.add_argument("--tmp", default=tempfile.gettempdir())
    ap.add_argument("--out", default=None)
    op = ap.parse_args()
    import pairs_cases as P
    from ingest_timing import gz_members
    from cloops_amd import convert, ingest, pairs, pipe
    n, budget = int(op.lines), op.budget_mb << 20
    res = {"lines": n, "budget_bytes": budget, "ext": op.ext, "reps": op.reps, "runs": {},
           "note": "wall: host clock around each call; old route = convert hicpro on the column-permuted file, then load_bedpe on its .bedpe.gz"}
    tmp = tempfile.mkdtemp(dir=op.tmp)
    try:
        t0 = time.perf_counter()
        new_plain, old_plain = os.path.join(tmp, "synth.pairs"), os.path.join(tmp, "synth_allValidPairs")
        with open(new_plain, "wb") as fa, open(old_plain, "wb") as fb:
            fa.write(P._t(P.HEAD))
            for s in range(0, n, BLOCK):
                b = min(BLOCK, n - s)
                fa.write(P.gen_pairs(b, P.SEED + s, header=False, dup=False))
                fb.write(P.gen_pairs(b, P.SEED + s, header=False, dup=False, order="hicpro"))
        for f in (new_plain, old_plain):
            with open(f, "rb") as fh:
                gz_members(fh.read(), f + ".gz")
        res["gen_s"], res["text_bytes"] = time.perf_counter() - t0, os.path.getsize(new_plain)
        warm = os.path.join(tmp, "warm.pairs")
        with open(warm, "wb") as fh:
            fh.write(P.gen_pairs(300000))
        pairs.parse_pairs_gpu([warm], unique=True, strand_distances=[], ext=op.ext, budget=budget)      # library load, code objects
        pairs.pairs2bedpe(warm, os.path.join(tmp, "warm.bedpe.gz"), ext=op.ext, budget=budget)
        for kind, sfx in (("plain", ""), ("gz", ".gz")):
            fnew, fold = new_plain + sfx, old_plain + sfx
            run = collections.defaultdict(list)
            run["file_bytes"] = os.path.getsize(fnew)
            digests = {}
            for rep in range(op.reps):
                stats = collections.Counter()
                t0 = time.perf_counter()
                names = pairs.load_pairs([fnew], ext=op.ext, budget=budget, prefix="timing", stats=stats)
                run["load_pairs_wall_s"].append(time.perf_counter() - t0)
                digests["new"] = resident_digest(pipe, names)
                for m in names:
                    pipe.CACHE.drop(m)
                run["lines"], run["cis"], run["fallback"] = stats["lines"], stats["cis"], stats["fallback"]
                run["load_pairs_host_s"] = {k: v for k, v in stats.items() if k in ("read", "wait_device", "write")}
                run["load_pairs_device_s"] = {k[len("device_ms_"):]: v / 1e3 for k, v in stats.items() if k.startswith("device_ms_")}
                old_bed = os.path.join(tmp, "old.bedpe.gz")
                t0 = time.perf_counter()
                convert.pairs2bedpe(fold, old_bed, ext=op.ext, budget=budget)
                run["old_convert_hicpro_wall_s"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                names = ingest.load_bedpe([old_bed], budget=budget, prefix="timing")
                run["old_load_bedpe_wall_s"].append(time.perf_counter() - t0)
                digests["old"] = resident_digest(pipe, names)
                for m in names:
                    pipe.CACHE.drop(m)
                new_bed = os.path.join(tmp, "new.bedpe.gz")
                t0 = time.perf_counter()
                run["bedpe_lines"], run["bedpe_bytes"] = pairs.pairs2bedpe(fnew, new_bed, ext=op.ext, budget=budget)
                run["pairs2bedpe_wall_s"].append(time.perf_counter() - t0)
                if rep == 0:
                    run["equal_text"] = text_digest(new_bed) == text_digest(old_bed)
            run["equal_chromosomes"] = digests["new"] == digests["old"]
            run["old_route_wall_s"] = [a + b for a, b in zip(run["old_convert_hicpro_wall_s"], run["old_load_bedpe_wall_s"])]
            res["runs"][kind] = dict(run)
            print(json.dumps({kind: dict(run)}), file=sys.stderr)
        res["equal"] = all(r["equal_chromosomes"] and r["equal_text"] for r in res["runs"].values())
    finally:
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
        os.rmdir(tmp)
    out = json.dumps(res, indent=1)
    print(out)
    if op.out:
        with open(op.out, "w") as fh:
            fh.write(out)


if __name__ == "__main__":
    main()
