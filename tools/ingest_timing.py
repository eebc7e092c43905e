"""Timing of K16 (cloops_amd.ingest: parse_bedpe_gpu / load_bedpe) on a seeded synthetic BEDPE (tests/ingest_cases.py synth_bedpe)
written to a temporary directory, plain and .gz, `unique` off and on, with cloops_amd.io.parse_bedpe (the host reader, the same
function as before K16) alternating on the same files in the same call as the baseline.

Reports, as one JSON document (stdout, and the file given by --out):
  per run           lines, cis PETs, text / file bytes; wall seconds and lines/s of parse_bedpe_gpu, of load_bedpe (every chromosome
                    resident and synchronised) and of cio.parse_bedpe; host seconds of the pipeline's stages (the reader thread's read /
                    inflate, the wait for the device, the ordered dictionary + commit); device seconds from the handles' events (copy
                    to the device, line index, parse kernel, names table, commit, finish) summed over the chunks; whether both readers
                    returned the same result (digests of every chromosome's rows and of the distances)
  relations         device stages against the reader thread's read time (plain), wall against inflate time (.gz)
  command line      wall seconds of `python -m cloops_amd -f <example> -o out -m 1` with -reader gpu and -reader host
Kernel times proper come from running `--lines 5e6 --only-gpu` under `rocprofv3 --kernel-trace --stats` (k15_* / k16_* rows and rocPRIM's).

    timeout -k 10 1100 python tools/ingest_timing.py [--lines 2e7] [--budget-mb 64] [--only-gpu] [--out FILE]
"""
import argparse
import collections
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def gz_members(data, path, threads=16, level=1, member=16 << 20):
    with open(path, "wb") as fo, ThreadPoolExecutor(threads) as pool:
        for blob in pool.map(lambda s: gzip.compress(data[s:s + member], level, mtime=0), range(0, len(data), member)):
            fo.write(blob)


def digest(mats, ds):
    h = hashlib.sha1()
    for c, m in mats.items():
        h.update(c.encode() + repr(m.shape).encode() + np.ascontiguousarray(m, dtype=np.int64).tobytes())
    h.update(np.asarray(ds, dtype=np.int64).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=float, default=2e7)
    ap.add_argument("--budget-mb", type=int, default=64)
    ap.add_argument("--only-gpu", action="store_true", help="no host baseline, no command line (for a run under rocprofv3)")
    ap.add_argument("--tmp", default=tempfile.gettempdir())
    ap.add_argument("--out", default=None)
    op = ap.parse_args()
    import golden_util as G
    import ingest_cases as C
    from cloops_amd import ingest, pipe
    from cloops_amd import io as cio
    n = int(op.lines)
    budget = op.budget_mb << 20
    res = {"lines": n, "budget_bytes": budget, "runs": {},
           "note": "wall: host clock around each call; device_s: HIP events of the two handles, summed over chunks (the two streams overlap)"}
    tmp = tempfile.mkdtemp(dir=op.tmp)
    try:
        t0 = time.perf_counter()
        data = C.synth_bedpe(n)
        plain = os.path.join(tmp, "synth.bedpe")
        with open(plain, "wb") as fh:
            fh.write(data)
        gz_members(data, plain + ".gz")
        res["gen_s"], res["text_bytes"] = time.perf_counter() - t0, len(data)
        del data
        warm = os.path.join(tmp, "warm.bedpe")
        with open(warm, "wb") as fh:
            fh.write(C.synth_bedpe(300000))
        ingest.parse_bedpe_gpu([warm], unique=True, strand_distances=[], budget=budget)    # library load, code objects, the first buffers
        for kind, f in (("plain", plain), ("gz", plain + ".gz")):
            for unique in (False, True):
                name = "%s_unique%d" % (kind, int(unique))
                run = {"file_bytes": os.path.getsize(f)}
                stats, ds = collections.Counter(), []
                t0 = time.perf_counter()
                mats, nl, nc = ingest.parse_bedpe_gpu([f], unique=unique, strand_distances=ds, budget=budget, stats=stats)
                wall = time.perf_counter() - t0
                run.update({"lines": nl, "cis": nc, "distances": len(ds), "fallback": stats["fallback"], "parse_bedpe_gpu_wall_s": wall,
                            "parse_bedpe_gpu_lines_per_s": nl / wall,
                            "host_s": {k: v for k, v in stats.items() if k in ("read", "wait_device", "write")},
                            "device_s": {k[len("device_ms_"):]: v / 1e3 for k, v in stats.items() if k.startswith("device_ms_")}})
                gpu_digest = digest(mats, ds)
                del mats
                stats = collections.Counter()
                t0 = time.perf_counter()
                names = ingest.load_bedpe([f], unique=unique, strand_distances=[], budget=budget, prefix="timing", stats=stats)
                wall = time.perf_counter() - t0
                run.update({"load_bedpe_wall_s": wall, "load_bedpe_lines_per_s": nl / wall, "chromosomes": len(names),
                            "load_bedpe_host_s": {k: v for k, v in stats.items() if k in ("read", "wait_device", "write")}})
                for m in names:
                    pipe.CACHE.drop(m)
                if not op.only_gpu:
                    ds = []
                    t0 = time.perf_counter()
                    mats, hl, hc = cio.parse_bedpe([f], unique=unique, strand_distances=ds)
                    wall = time.perf_counter() - t0
                    run.update({"host_parse_bedpe_wall_s": wall, "host_parse_bedpe_lines_per_s": hl / wall,
                                "equal": (hl, hc) == (nl, nc) and digest(mats, ds) == gpu_digest})
                    del mats
                dev = run["device_s"]
                stages = sum(dev.get(k, 0) for k in ("index", "parse", "names", "commit", "finish"))
                run["device_stages_s"] = stages
                run["reads_plus_copies_s"] = run["host_s"].get("read", 0) + dev.get("h2d", 0)
                kern = dev.get("index", 0) + dev.get("parse", 0)
                run["index_parse_text_GBps"] = res["text_bytes"] / kern / 1e9 if kern > 0 else None
                res["runs"][name] = run
                print(json.dumps({name: run}), file=sys.stderr)
        if not op.only_gpu:
            bed = G.write_example_bedpe(tmp)
            env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
            cli = {}
            for rep in range(2):
                for reader in ("gpu", "host"):
                    out = "cli_%s_%d" % (reader, rep)
                    t0 = time.perf_counter()
                    p = subprocess.run([sys.executable, "-m", "cloops_amd", "-f", bed, "-o", out, "-m", "1", "-reader", reader], env=env, cwd=tmp,
                                       timeout=300, capture_output=True, text=True)
                    assert p.returncode == 0, p.stderr
                    cli.setdefault(reader, []).append(time.perf_counter() - t0)
                    os.remove(os.path.join(tmp, out + ".loop"))
            res["command_line_example_mode1_wall_s"] = cli
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
