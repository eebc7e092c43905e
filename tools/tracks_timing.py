"""Timing of K14 (cl_track_build / cl_track_chunks / cl_track_render) on the benchmark genome: the 200 M-PET genome of bench.py
(cloops_amd.synth, seed family 3), one resident chromosome at a time, washU text (ext 75, cut 0) and juice text.

Reports, as one JSON document (stdout, and the file given by --out):
  per chromosome and kind   rows, records, text bytes, chunks; wall of track_build (synchronous: kernels + the two small
                            read-backs) and of every track_render (synchronous: kernel + device-to-host copy into a page-locked
                            buffer), summed over the chunks
  copy rate                 device-to-host of one chunk-sized buffer into page-locked memory (hipMemcpy through torch), alone
  file-write rate           --write-mb of rendered text written to a file under --tmp and flushed (os.fsync), alone
  host reference            the reference's per-PET loop of jd2washU (cLoops/io.py:301-318) restated in Python 3 over --sample
                            rows into an in-memory buffer, extrapolated linearly to the genome -- labelled as such; its
                            `bedtools sort` / `bgzip` / `tabix` steps are not measured
Kernel times proper come from running this under `rocprofv3 --kernel-trace --stats` (k14_* rows and rocPRIM's sort / scans).

    timeout -k 10 900 python tools/tracks_timing.py [--n-total 2e8] [--chroms N] [--budget-mb 64] [--write-mb 1024] [--out FILE]
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def host_loop(ids, X, Y, ext, key="chr1"):
    """cLoops/io.py:301-318, Python 3, into a StringIO"""
    f = io.StringIO()
    for i, x, y in zip(ids.tolist(), X.tolist(), Y.tolist()):
        a = (key, max([0, x - ext]), x + ext)
        b = (key, max([0, y - ext]), y + ext)
        linea = [a[0], a[1], a[2], "%s:%s-%s,1" % (b[0], b[1], b[2]), i, "."]
        lineb = [b[0], b[1], b[2], "%s:%s-%s,1" % (a[0], a[1], a[2]), i, "."]
        f.write("\t".join(map(str, linea)) + "\n")
        f.write("\t".join(map(str, lineb)) + "\n")
    return f.tell()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-total", type=float, default=2e8)
    ap.add_argument("--chroms", type=int, default=0, help="only the first N chromosomes (0: all)")
    ap.add_argument("--budget-mb", type=int, default=64)
    ap.add_argument("--write-mb", type=int, default=1024)
    ap.add_argument("--sample", type=int, default=200000)
    ap.add_argument("--tmp", default=tempfile.gettempdir())
    ap.add_argument("--out", default=None)
    op = ap.parse_args()
    from cloops_amd import api, synth
    import ctypes
    budget = op.budget_mb << 20
    res = {"n_total": int(op.n_total), "budget_bytes": budget, "chroms": [], "wall_note": "synchronous calls, host wall clock"}
    lib = None
    pin = None
    tot = {"washu": [0, 0, 0.0, 0.0], "juice": [0, 0, 0.0, 0.0]}       # records, bytes, build s, render s
    sample = None
    for ci, (name, X, Y) in enumerate(synth.synth_genome(int(op.n_total), 3)):
        if op.chroms and ci >= op.chroms:
            break
        ch = api.Chromosome(X, Y)
        lib = ch._lib
        if pin is None:
            pin = lib.cl_host_alloc(budget)
        row = {"chrom": name, "rows": int(len(X))}
        for kind, ext in (("washu", 75), ("juice", 0)):
            for rep in range(2):                                       # the first build allocates the scratch
                t0 = time.perf_counter()
                nr, nb = ch.track_build(kind, 0, ext, None, name, name)
                tb = time.perf_counter() - t0
            rec, byt = ch.track_chunks(budget)
            t0 = time.perf_counter()
            for k in range(len(rec) - 1):
                ch.track_render(k, (pin, budget))
            tr = time.perf_counter() - t0
            row[kind] = {"records": nr, "bytes": nb, "chunks": len(rec) - 1, "build_s": tb, "render_s": tr,
                         "render_GBps": nb / tr / 1e9 if tr > 0 else None}
            tot[kind][0] += nr
            tot[kind][1] += nb
            tot[kind][2] += tb
            tot[kind][3] += tr
        if ci == 0:
            sample = (X[: op.sample].astype(np.int64), Y[: op.sample].astype(np.int64))
            # file-write rate: rendered washU text of this chromosome, up to --write-mb
            ch.track_build("washu", 0, 75, None, name, name)
            path = os.path.join(op.tmp, "tracks_timing_%d.txt" % os.getpid())
            written, tw = 0, 0.0
            try:
                with open(path, "wb") as fo:
                    for mv in ch.track_iter(budget):
                        t0 = time.perf_counter()
                        fo.write(mv)
                        tw += time.perf_counter() - t0
                        written += len(mv)
                        if written >= op.write_mb << 20:
                            break
                    t0 = time.perf_counter()
                    fo.flush()
                    os.fsync(fo.fileno())
                    tw += time.perf_counter() - t0
            finally:
                if os.path.exists(path):
                    os.remove(path)
            res["file_write"] = {"bytes": written, "s": tw, "GBps": written / tw / 1e9 if tw > 0 else None}
            # overlap: the double-buffered iterator writing the whole text to /dev/null
            t0 = time.perf_counter()
            n_iter = 0
            with open(os.devnull, "wb") as fo:
                for mv in ch.track_iter(budget):
                    fo.write(mv)
                    n_iter += len(mv)
            res["iter_devnull"] = {"bytes": n_iter, "s": time.perf_counter() - t0}
        ch.track_free()
        ch.close()
        res["chroms"].append(row)
        print(json.dumps(row), file=sys.stderr)
    for kind, (nr, nb, tb, tr) in tot.items():
        res[kind] = {"records": nr, "bytes": nb, "build_s": tb, "render_s": tr}
    # device-to-host copy rate alone
    try:
        import torch
        d = torch.empty(budget, dtype=torch.uint8, device="cuda")
        h = torch.empty(budget, dtype=torch.uint8, pin_memory=True)
        h.copy_(d)
        torch.cuda.synchronize()
        ts = []
        for _ in range(10):
            t0 = time.perf_counter()
            h.copy_(d)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res["d2h"] = {"bytes": budget, "median_s": float(np.median(ts)), "GBps": budget / float(np.median(ts)) / 1e9}
    except Exception as e:                                              # noqa: BLE001
        res["d2h"] = {"error": repr(e)}
    if pin is not None:
        lib.cl_host_free(ctypes.c_void_p(pin))
    # the reference's loop restated on the host over a sample, extrapolated
    X, Y = sample
    t0 = time.perf_counter()
    host_loop(np.arange(len(X)), X, Y, 75)
    th = time.perf_counter() - t0
    res["host_reference_extrapolated"] = {"sample_rows": int(len(X)), "sample_s": th,
                                          "genome_s_extrapolated": th * int(op.n_total) / len(X),
                                          "note": "Python 3 restatement of cLoops/io.py:301-318 into StringIO, one core; sort/bgzip/tabix not measured"}
    out = json.dumps(res, indent=1)
    print(out)
    if op.out:
        with open(op.out, "w") as fh:
            fh.write(out)


if __name__ == "__main__":
    main()
