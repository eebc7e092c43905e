"""Timing of K15 (cloops_amd.convert: pairs2bedpe / long2bedpe) on seeded synthetic pairs files (tests/convert_cases.py GEN) written
to a temporary directory: juicer plain -> plain, hicpro plain -> gz and gz -> gz at -p THREADS.

Reports, as one JSON document (stdout, and the file given by --out):
  per run           lines, input / output bytes, wall seconds, lines/s; host seconds of the pipeline's stages (the reader thread's
                    read / inflate, the wait for the device, the ordered write or compression hand-off); device seconds from the
                    handles' events (copy to the device, the feed kernels, the render kernel, copy back) summed over the chunks
  kernel rate       input bytes over the K15 kernels' event time (feed + render), per run
  host reference    the reference's per-line loops (scripts/hicpropairs2bedpe:15-34, scripts/juicerLong2bedpe.py:12-31) restated in
                    Python 3 over a --sample-line sample into memory, extrapolated linearly -- labelled as such
Kernel times proper come from running this under `rocprofv3 --kernel-trace --stats` (k15_* rows and rocPRIM's scans).

    timeout -k 10 900 python tools/convert_timing.py [--lines 2e7] [--budget-mb 64] [--threads 8] [--sample 1e6] [--out FILE]
"""
import argparse
import collections
import gzip
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_hicpro(lines, ext=50):
    """scripts/hicpropairs2bedpe:15-34, Python 3, into a StringIO"""
    f = io.StringIO()
    for line in lines:
        line = line.strip().split('\t')
        if line[3] == "+":
            petA = [line[1], int(line[2]), int(line[2]) + ext]
        else:
            petA = [line[1], int(line[2]) - ext, int(line[2])]
        if line[6] == "+":
            petB = [line[4], int(line[5]), int(line[5]) + ext]
        else:
            petB = [line[4], int(line[5]) - ext, int(line[5])]
        newline = [petA[0], petA[1], petA[2], petB[0], petB[1], petB[2], line[0], '.', line[3], line[6]]
        f.write("\t".join(map(str, newline)) + "\n")
    return f.tell()


def host_juicer(lines, ext=75):
    """scripts/juicerLong2bedpe.py:12-31, Python 3, into a StringIO"""
    f = io.StringIO()
    for line in lines:
        line = line.split("\n")[0].split()
        nline = [line[1], max(0, int(line[2]) - ext), int(line[2]) + ext, line[5], max(0, int(line[6]) - ext), int(line[6]) + ext,
                 ".", ".", "+", "+"]
        if line[0] != "0":
            nline[-2] = "-"
        if line[4] != "0":
            nline[-1] = "-"
        f.write("\t".join(list(map(str, nline))) + "\n")
    return f.tell()


def gz_members(data, path, threads, level=1, member=16 << 20):
    with open(path, "wb") as fo, ThreadPoolExecutor(threads) as pool:
        for blob in pool.map(lambda s: gzip.compress(data[s:s + member], level, mtime=0), range(0, len(data), member)):
            fo.write(blob)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=float, default=2e7)
    ap.add_argument("--budget-mb", type=int, default=64)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--sample", type=float, default=1e6)
    ap.add_argument("--skip-reference", action="store_true")
    ap.add_argument("--tmp", default=tempfile.gettempdir())
    ap.add_argument("--out", default=None)
    op = ap.parse_args()
    import convert_cases as C
    from cloops_amd import convert
    n = int(op.lines)
    budget = op.budget_mb << 20
    res = {"lines_per_file": n, "budget_bytes": budget, "threads": op.threads, "runs": {},
           "note": "wall: host clock around each conversion; device_s: HIP events of the two handles, summed over chunks"}
    tmp = tempfile.mkdtemp(dir=op.tmp)
    try:
        files = {}
        for fmt, seed in (("juicer", 101), ("hicpro", 102)):
            t0 = time.perf_counter()
            data = C.GEN[fmt](n, seed)
            path = os.path.join(tmp, fmt + "_allValidPairs")
            with open(path, "wb") as fh:
                fh.write(data)
            res["gen_%s_s" % fmt] = time.perf_counter() - t0
            files[fmt] = (path, len(data))
            if fmt == "hicpro":
                gz_members(data, path + ".gz", 16)
                files["hicpro_gz"] = (path + ".gz", len(data))
            del data
        # warm-up: library load, the first handles and page-locked buffers
        warm = os.path.join(tmp, "warm")
        with open(warm, "wb") as fh:
            fh.write(C.GEN["juicer"](1000, 1))
        convert.long2bedpe(warm, warm + ".out", budget=budget)
        runs = [("juicer_plain_to_plain", "juicer", files["juicer"][0], os.path.join(tmp, "j.bedpe")),
                ("hicpro_plain_to_gz", "hicpro", files["hicpro"][0], os.path.join(tmp, "h.bedpe.gz")),
                ("hicpro_gz_to_gz", "hicpro_gz", files["hicpro_gz"][0], os.path.join(tmp, "hg.bedpe.gz"))]
        for name, key, fin, fout in runs:
            stats = collections.Counter()
            t0 = time.perf_counter()
            if key == "juicer":
                nl, nb = convert.long2bedpe(fin, fout, budget=budget, stats=stats)
            else:
                nl, nb = convert.pairs2bedpe(fin, fout, threads=op.threads, budget=budget, stats=stats)
            wall = time.perf_counter() - t0
            inb = files[key][1]
            dev = {k[len("device_ms_"):]: v / 1e3 for k, v in stats.items() if k.startswith("device_ms_")}
            kern = dev.get("feed", 0) + dev.get("render", 0)
            res["runs"][name] = {"lines": nl, "input_text_bytes": inb, "input_file_bytes": os.path.getsize(fin), "output_text_bytes": nb,
                                 "output_file_bytes": os.path.getsize(fout), "wall_s": wall, "lines_per_s": nl / wall,
                                 "host_s": {k: v for k, v in stats.items() if not k.startswith("device_ms_")}, "device_s": dev,
                                 "kernel_input_GBps": inb / kern / 1e9 if kern > 0 else None, "chunks": -(-inb // budget)}
            print(json.dumps({name: res["runs"][name]}), file=sys.stderr)
            os.remove(fout)
        if not op.skip_reference:
            s = int(op.sample)
            for fmt, fn in (("hicpro", host_hicpro), ("juicer", host_juicer)):
                with open(files[fmt][0]) as fh:
                    lines = [fh.readline() for _ in range(s)]
                t0 = time.perf_counter()
                fn(lines)
                th = time.perf_counter() - t0
                res["host_reference_%s" % fmt] = {"sample_lines": s, "sample_s": th, "lines_per_s": s / th,
                                                  "extrapolated_s_for_lines_per_file": th * n / s,
                                                  "note": "Python 3 restatement of the script's per-line loop into StringIO, one core; "
                                                          "file reading and gzip not included"}
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
