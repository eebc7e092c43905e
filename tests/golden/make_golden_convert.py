#!/usr/bin/env python
"""Golden outputs of the pairs converters scripts/hicpropairs2bedpe (pairs2bedpe) and scripts/juicerLong2bedpe.py (long2bedpe).
Build container only:
    python tests/golden/make_golden_convert.py

Both functions are sliced by lines out of the scripts and exec'd in memory under Python 3, unchanged.  They run on plain-text
inputs only: the Python-3 reference cannot read a gzipped pairs file (gzip.open yields bytes and `.split('\\t')` raises
TypeError).  The inputs are ASCII without lone '\\r', so the Python-3 text reading of the reference and the pinned Python-2 reading
of bytes agree on them (the cases where they differ are the deviation table of tests/test_convert.py).  The hicpro output is
decompressed.  For an error case the exception's type and message and the lines written before it are recorded.

Writes convert_cases.npz (every case's input and expected output as uint8, compressed) and convert_meta.json (case, format, ext,
lines, sha256, error).  The seeded synthetics (tests/convert_cases.py GEN, about 5e6 lines each) keep only their generator
parameters and the sha256 / line count of the expected output.
"""
import gzip
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import refload  # noqa: E402
import convert_cases as C  # noqa: E402

SYNTH = [("synth_hicpro", "hicpro", 50, 5_000_000, 15), ("synth_juicer", "juicer", 75, 5_000_000, 16)]


def namespace():
    ns = {"gzip": gzip, "os": os}
    for rel, name in (("scripts/hicpropairs2bedpe", "pairs2bedpe"), ("scripts/juicerLong2bedpe.py", "long2bedpe")):
        with open(os.path.join(refload.REF_ROOT, rel)) as fh:
            lines = fh.read().split("\n")
        s = [i for i, l in enumerate(lines) if l.startswith("def %s(" % name)][0]
        e = [i for i, l in enumerate(lines) if i > s and l.startswith("def ")][0]
        exec(compile("\n".join(lines[s:e]), rel, "exec"), ns)
    return ns


def _h(*rows):
    return b"".join(b"\t".join(r) + b"\n" for r in rows)


def hicpro_cases():
    P, M = b"+", b"-"
    long_name = b"R" * 230
    cases = {
        "h_basic": (_h([b"r1", b"chr1", b"1000", P, b"chr1", b"5000", M, b"300", b"HIC_chr1_1", b"HIC_chr1_9", b"42", b"42"],
                       [b"r2", b"chr2", b"77", M, b"chr3", b"9999999", P],
                       [b"r3", b"chrX", b"0", P, b"chrX", b"0", M, b"x"]), 50),
        "h_negative": (_h([b"r1", b"chr1", b"10", M, b"chr1", b"49", M], [b"r2", b"chr1", b"0", M, b"chr1", b"-5", P]), 50),
        "h_ext0": (_h([b"r1", b"chr1", b"10", M, b"chr1", b"49", P]), 0),
        "h_extneg": (_h([b"r1", b"chr1", b"10", M, b"chr1", b"49", P], [b"r2", b"c", b"3", P, b"c", b"2", M]), -7),
        "h_ext1e7": (_h([b"r1", b"chr1", b"10", M, b"chr1", b"49", P]), 10 ** 7),
        "h_strands": (_h([b"r1", b"c", b"10", b"+ ", b"c", b"20", b"+ ", b"extra"], [b"r2", b"c", b"10", b"++", b"c", b"20", b"", b"e"],
                         [b"r3", b"c", b"10", b"", b"c", b"20", b"*", b"e"], [b"r4", b"c", b"10", b" +", b"c", b"20", b"-+"]), 50),
        "h_seven_trailing": (b"r1\tc\t10\t+\tc\t20\t+   \nr2\tc\t10\t-\tc\t20\t-\t \t\n", 50),
        "h_leading": (b"   r1\tc\t10\t+\tc\t20\t+\n\t r2\tc\t11\t-\tc\t21\t-\n", 50),
        "h_crlf": (b"r1\tc\t10\t+\tc\t20\t+\r\nr2\tc\t11\t-\tc\t21\t-\textra\r\n", 50),
        "h_nonl": (b"r1\tc\t10\t+\tc\t20\t+\nr2\tc\t11\t-\tc\t21\t-", 50),
        "h_emptychrom": (_h([b"r1", b"", b"10", P, b"c", b"20", P], [b"r2", b"c", b"10", P, b"", b"20", M]), 50),
        "h_ints": (_h([b"r1", b"c", b"+12", P, b"c", b"0007", M], [b"r2", b"c", b" 12 ", P, b"c", b"-0", M],
                      [b"r3", b"c", b"  -40", M, b"c", b"000", P]), 50),
        "h_longname": (_h([long_name, b"chrUn_" + b"x" * 210, b"10", P, b"c", b"20", M]), 50),
        "h_10k": (_h([b"r1", b"c", b"10", P, b"c", b"20", M, b"y" * 10000], [b"r2", b"c", b"11", P, b"c", b"21", M]), 50),
        "h_big": (_h([b"r1", b"c", b"%d" % (1 << 40), P, b"c", b"%d" % ((1 << 40) + 12345), M],
                     [b"r2", b"c", b"-%d" % (1 << 40), M, b"c", b"%d" % ((1 << 40) - 1), P]), 75),
        "h_err6": (_h([b"r1", b"c", b"10", P, b"c", b"20", M], [b"r2", b"c", b"10", P, b"c", b"20"], [b"r3", b"c", b"1", P, b"c", b"2", P]), 50),
        "h_errint": (_h(*([[b"r", b"c", b"%d" % i, P, b"c", b"20", M] for i in range(5)] + [[b"r", b"c", b"12a", P, b"c", b"20", M]] +
                          [[b"r", b"c", b"1", P, b"c", b"2", M]])), 50),
        "h_errblank": (_h([b"r1", b"c", b"10", P, b"c", b"20", M]) + b"\n" + _h([b"r2", b"c", b"10", P, b"c", b"20", M]), 50),
        "h_errtrail": (_h([b"r1", b"c", b"10", P, b"c", b"20", M], [b"r2", b"c", b"10", P, b"c", b"20", M]) + b"\n", 50),
    }
    return cases


def juicer_cases():
    def j(*rows):
        return b"".join(b" ".join(r) + b"\n" for r in rows)
    row = [b"0", b"chr1", b"1000", b"5", b"16", b"chr1", b"5000", b"9", b"60", b"100M", b"ACGT", b"60", b"100M", b"TTGA", b"rA", b"rB"]
    cases = {
        "j_basic": (j(row, [b"16", b"chr2", b"77", b"1", b"0", b"chr3", b"9999999", b"2"], [b"0", b"chrX", b"0", b"0", b"0", b"chrX", b"1", b"0"]), 75),
        "j_negative": (j([b"0", b"c", b"10", b"0", b"0", b"c", b"-500", b"0"]), 75),
        "j_ext0": (j([b"0", b"c", b"10", b"0", b"16", b"c", b"49", b"0"]), 0),
        "j_extneg": (j([b"0", b"c", b"10", b"0", b"16", b"c", b"49", b"0"]), -7),
        "j_ext1e7": (j([b"0", b"c", b"10", b"0", b"16", b"c", b"49", b"0"]), 10 ** 7),
        "j_strands": (j([b"00", b"c", b"10", b"0", b"-0", b"c", b"20", b"0"], [b"+0", b"c", b"10", b"0", b"0", b"c", b"20", b"0"],
                        [b"1", b"c", b"10", b"0", b"x", b"c", b"20", b"0"]), 75),
        "j_seven_trailing": (b"0 c 10 0 16 c 20   \n16\tc\t11\t0\t0\tc\t21 \t \n", 75),
        "j_leading": (b"   0 c 10 0 16 c 20 x\n \t 16  c   11 0   0 c 21\n", 75),
        "j_crlf": (b"0 c 10 0 16 c 20 x\r\n16 c 11 0 0 c 21\r\n", 75),
        "j_nonl": (b"0 c 10 0 16 c 20 x\n16 c 11 0 0 c 21", 75),
        "j_ints": (j([b"0", b"c", b"+12", b"0", b"16", b"c", b"0007", b"0"], [b"0", b"c", b"-0", b"0", b"16", b"c", b"000", b"0"]), 75),
        "j_longname": (j([b"0", b"chrUn_" + b"x" * 210, b"10", b"0", b"16", b"chrUn_" + b"y" * 220, b"20", b"0"]), 75),
        "j_10k": (j([b"0", b"c", b"10", b"0", b"16", b"c", b"20", b"0", b"z" * 10000], [b"0", b"c", b"11", b"0", b"16", b"c", b"21", b"0"]), 75),
        "j_big": (j([b"0", b"c", b"%d" % (1 << 40), b"0", b"16", b"c", b"%d" % ((1 << 40) + 9), b"0"],
                    [b"0", b"c", b"-%d" % (1 << 40), b"0", b"16", b"c", b"%d" % ((1 << 40) - 1), b"0"]), 75),
        "j_err6": (j(row, [b"0", b"c", b"10", b"0", b"16", b"c"], row), 75),
        "j_errint": (j(*([row] * 6 + [[b"0", b"c", b"1e3", b"0", b"16", b"c", b"20", b"0"]] + [row])), 75),
        "j_errblank": (j(row, row) + b"\n" + j(row), 75),
        "j_errtrail": (j(row, row) + b"\n", 75),
    }
    return cases


def run_reference(ns, fmt, data, ext, tmp):
    fin = os.path.join(tmp, "in.txt")
    with open(fin, "wb") as fh:
        fh.write(data)
    fout = os.path.join(tmp, "out" + (".bedpe.gz" if fmt == "hicpro" else ".bedpe"))
    error = None
    try:
        if fmt == "hicpro":
            ns["pairs2bedpe"](fin, fout, ext=ext)
        else:
            ns["long2bedpe"](fin, fout, ext=ext)
    except (IndexError, ValueError) as e:
        error = "%s: %s" % (type(e).__name__, e)
    if fmt == "hicpro":
        with gzip.open(fout, "rb") as fh:
            out = fh.read()
    else:
        with open(fout, "rb") as fh:
            out = fh.read()
    os.remove(fout)
    return out, error


def main():
    ns = namespace()
    arrays, meta = {}, {"cases": [], "synth": []}
    with tempfile.TemporaryDirectory() as tmp:
        for fmt, cases in (("hicpro", hicpro_cases()), ("juicer", juicer_cases())):
            for name, (data, ext) in cases.items():
                out, error = run_reference(ns, fmt, data, ext, tmp)
                arrays[name + "__in"] = np.frombuffer(data, np.uint8)
                arrays[name + "__out"] = np.frombuffer(out, np.uint8)
                meta["cases"].append({"name": name, "format": fmt, "ext": ext, "lines": out.count(b"\n"),
                                      "sha256": hashlib.sha256(out).hexdigest(), "error": error})
                print(name, len(data), len(out), error)
        for name, fmt, ext, n, seed in SYNTH:
            data = C.GEN[fmt](n, seed)
            out, error = run_reference(ns, fmt, data, ext, tmp)
            assert error is None
            meta["synth"].append({"name": name, "format": fmt, "ext": ext, "n": n, "seed": seed, "lines": out.count(b"\n"),
                                  "in_sha256": hashlib.sha256(data).hexdigest(), "sha256": hashlib.sha256(out).hexdigest()})
            print(name, len(data), len(out))
    np.savez_compressed(os.path.join(HERE, "convert_cases.npz"), **arrays)
    with open(os.path.join(HERE, "convert_meta.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


if __name__ == "__main__":
    main()
