#!/usr/bin/env python
"""Golden vectors of the BEDPE reader tests: what the reference's OWN parseRawBedpe2 / parseRawBedpe (cLoops/io.py:62-189, sliced
and patched for Python 3 by refload.ref_io_namespace) return on the corner corpus and on one seeded synthetic of
tests/ingest_cases.py, per case and argument set, stored as digests (data only).  Run where the reference checkout is:

    python tests/golden/make_golden_ingest.py

Writes tests/golden/ingest_reference.json: cases[name][argument set] = {"keys": chromosomes in the order of their files, "rows":
{chromosome: sha1 of its int64 [n, 3] rows}, "ds": sha1 of the strand distances (parseRawBedpe only)} or {"raises": exception
name} where the reference does not return (a file name longer than the file system takes, too many open files, bytes that do not
decode); inputs[name] = sha1 of the case's bytes, to catch a drifted corpus.
"""
import contextlib
import hashlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import refload  # noqa: E402
import ingest_cases as C  # noqa: E402

SYNTH_LINES = 200000


class _Log(object):
    def info(self, *a):
        pass


def _chrom(path):
    s = os.path.basename(path)[:-len(".txt")]
    return s[:(len(s) - 1) // 2]


def _load(path):
    with open(path) as fh:
        rows = [[int(v) for v in l.split("\t")] for l in fh.read().split("\n") if l]
    return np.asarray(rows, dtype=np.int64).reshape(len(rows), 3)


def reference_result(ns, fs, cs, cut, unique):
    with tempfile.TemporaryDirectory() as td:
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                if unique:
                    cfs, ds = ns["parseRawBedpe"](fs, td, list(cs), cut, _Log())
                else:
                    cfs, ds = ns["parseRawBedpe2"](fs, td, list(cs), cut, _Log()), None
            import gc
            gc.collect()                                               # the reference leaves closing its files to the collector
            mats = {}
            for f in cfs:
                mats[_chrom(f)] = _load(f)
            return C.digest_result(mats, ds)
        except Exception as e:                                          # noqa: BLE001
            return {"raises": type(e).__name__}


def main():
    assert refload.available(), "reference checkout missing"
    ns = refload.ref_io_namespace()
    out = {"cases": {}, "inputs": {}}
    with tempfile.TemporaryDirectory() as td:
        todo = [(name, C.write_case(td, name, files), files) for name, files, _ in C.corpus()]
        fs = C.write_synth(td, SYNTH_LINES)
        todo.append(("synth200k", fs, [C.synth_bedpe(SYNTH_LINES)]))
        for name, paths, files in todo:
            out["inputs"][name] = hashlib.sha1(b"\x00".join(files)).hexdigest()
            out["cases"][name] = {C.argkey(cs, cut, unique): reference_result(ns, paths, cs, cut, unique) for cs, cut, unique in C.ARGSETS}
    with open(C.GOLD, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
    n = sum(1 for c in out["cases"].values() for r in c.values() if "raises" not in r)
    print("%d cases, %d results, %d of them returned by the reference" % (len(out["cases"]), sum(len(c) for c in out["cases"].values()), n))


if __name__ == "__main__":
    main()
