"""CPU: PETs at loop anchors (cloops_amd.cleanpets, scripts/jd2cleanWashuPETs.py).  The K13 row mask is replaced by a numpy brute
force over the PETs and the raw anchors (`brute_mask`, also the yardstick of the GPU tests in test_gpu_cleanpets.py); fed through
the host functions it must reproduce the row sets, counts and log numbers that the script's own functions wrote
(tests/golden/make_golden_cleanpets.py)."""
import json
import os

import joblib
import numpy as np
import pytest

import golden_util as G

GOLD = G.GOLD


def golden_meta():
    with open(os.path.join(GOLD, "cleanpets_meta.json")) as fh:
        return json.load(fh)


def golden_rows(case, chrom, n):
    z = np.load(os.path.join(GOLD, "cleanpets_masks.npz"))
    return np.flatnonzero(np.unpackbits(z["%s__%s" % (case, chrom)])[:n])


def datasets():
    """{dataset: {chrom: (X, Y)}}: the chr21 example and the hand-built set of the golden script"""
    X, Y = G.chr21_xy()
    z = np.load(os.path.join(GOLD, "cleanpets_synth.npz"))
    s = {k[2:]: (z[k].astype(np.int64), z["Y_" + k[2:]].astype(np.int64)) for k in z.files if k.startswith("X_")}
    return {"chr21": {"chr21": (X, Y)}, "synth": s}


def write_jd_dirs(root, data=None):
    """the datasets as .jd directories of [id, X, Y] int64 rows -> {dataset: dir}"""
    out = {}
    for name, chroms in (data or datasets()).items():
        d = os.path.join(str(root), name)
        os.makedirs(d)
        for chrom, (x, y) in chroms.items():
            joblib.dump(np.stack([np.arange(len(x)), x, y], 1).astype(np.int64), os.path.join(d, "%s-%s.jd" % (chrom, chrom)))
        out[name] = d
    return out


def brute_mask(X, Y, starts, ends):
    """numpy restatement of cl_anchor_mask's rows: X or Y in some closed raw interval (membership of the union does not need the
    merge) -> bool [n]"""
    X = np.asarray(X, np.int64)
    Y = np.asarray(Y, np.int64)
    s = np.asarray(starts, np.int64)
    e = np.asarray(ends, np.int64)
    keep = np.zeros(len(X), bool)
    for k in range(0, len(s), 256):
        ss, ee = s[None, k:k + 256], e[None, k:k + 256]
        keep |= ((X[:, None] >= ss) & (X[:, None] <= ee)).any(1) | ((Y[:, None] >= ss) & (Y[:, None] <= ee)).any(1)
    return keep


def components(starts, ends):
    """merged-anchor count the slow way: connected components of the 'overlap or share an endpoint' graph, O(A^2)"""
    n = len(starts)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for i in range(n):
        for j in range(i + 1, n):
            if starts[i] <= ends[j] and starts[j] <= ends[i]:
                parent[find(i)] = find(j)
    return len({find(i) for i in range(n)})


def brute_backend(monkeypatch):
    """route cleanpets._anchor_rows (K13 on the resident chromosome) to brute_mask on the .jd file"""
    from cloops_amd import cleanpets, pipe

    def anchor_rows(f, starts, ends):
        key, mat = pipe.parseJd(f, 0)
        mat = np.asarray(mat).reshape(-1, 3)
        rows = np.flatnonzero(brute_mask(mat[:, 1], mat[:, 2], starts, ends))
        return key, mat[rows], len(mat), components(list(starts), list(ends))
    monkeypatch.setattr(cleanpets, "_anchor_rows", anchor_rows)


def _check_case(case, out, dirs_data):
    """the .jd files of `out` against the golden row sets of `case`"""
    meta = golden_meta()["results"][case]
    data = datasets()[dirs_data]
    assert sorted(f for f in os.listdir(out)) == sorted("%s-%s.jd" % (c, c) for c in meta["chroms"])
    for chrom, m in meta["chroms"].items():
        x, y = data[chrom]
        nmat = joblib.load(os.path.join(out, "%s-%s.jd" % (chrom, chrom)))
        rows = golden_rows(case, chrom, len(x))
        assert nmat.dtype == np.int64 and nmat.shape == (len(rows), 3), (case, chrom)
        assert np.array_equal(nmat, np.stack([rows, x[rows], y[rows]], 1)), (case, chrom)       # ascending row order
        assert len(rows) == m["kept"]


def _run_case(tmp_path, case, monkeypatch):
    from cloops_amd import cleanpets
    brute_backend(monkeypatch)
    name, loopf, dname, sig, chroms = [c for c in golden_meta()["cases"] if c[0] == case][0]
    dirs = write_jd_dirs(tmp_path)
    out = os.path.join(str(tmp_path), "out_" + case)
    os.mkdir(out)
    res = cleanpets.jd2cleanWashuPETs(os.path.join(GOLD, loopf), dirs[dname], sig, out, chroms=set(chroms) if chroms else [])
    return res, out, dname


@pytest.mark.parametrize("case", ["chr21_v2_sig", "chr21_v2_all", "chr21_v1_sig", "synth_sig", "synth_all", "synth_chroms"])
def test_goldens_through_host_code(tmp_path, monkeypatch, case):
    res, out, dname = _run_case(tmp_path, case, monkeypatch)
    s = golden_meta()["results"][case]["summary"]
    assert res == (s["loops"], s["anchors"], s["raw"], s["kept"], s["ratio"])
    _check_case(case, out, dname)


def test_no_chromosome_left_raises(tmp_path, monkeypatch):
    assert golden_meta()["results"]["synth_none"]["exception"] == "ZeroDivisionError"
    with pytest.raises(ZeroDivisionError):
        _run_case(tmp_path, "synth_none", monkeypatch)


def test_records():
    """preDs: significance, repeated loopIds, chromosomes without a .jd or without loops, -c; columns by header name"""
    from cloops_amd import cleanpets
    meta = golden_meta()
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        dirs = write_jd_dirs(td)
        for name, loopf, dname, sig, chroms in meta["cases"]:
            r = cleanpets.preDs(os.path.join(GOLD, loopf), dirs[dname], sig, set(chroms) if chroms else [])
            assert {k: len(v["rs"]) for k, v in r.items()} == meta["results"][name]["records"], name
            for k, v in r.items():
                assert v["f"] == os.path.join(dirs[dname], "%s-%s.jd" % (k, k))
        r = cleanpets.preDs(os.path.join(GOLD, "cleanpets_synth.loop"), dirs["synth"])
        assert r["chrA"]["rs"]["chrA-chrA-1"] == ["chrA", 90000, 90500, "chrA", 95000, 95500]      # the later line wins


def test_get_anchors_matches_golden():
    from cloops_amd import cleanpets
    meta = golden_meta()
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        dirs = write_jd_dirs(td)
        for name, loopf, dname, sig, chroms in meta["cases"]:
            r = cleanpets.preDs(os.path.join(GOLD, loopf), dirs[dname], sig, set(chroms) if chroms else [])
            for chrom, v in r.items():
                assert cleanpets.getAnchors(v["rs"]) == meta["results"][name]["chroms"][chrom]["anchor_list"], (name, chrom)


def test_merge_count_against_components():
    from cloops_amd import cleanpets
    rng = np.random.default_rng(5)
    for t in range(200):
        a = int(rng.integers(1, 40))
        span = int(rng.choice([30, 200, 5000]))
        s = rng.integers(0, span, a)
        e = s + rng.integers(0, int(rng.choice([1, 5, 40])), a)
        loops = {"l%d" % k: ["c", int(s[2 * k]), int(e[2 * k]), "c", int(s[2 * k + 1]), int(e[2 * k + 1])] for k in range(a // 2)}
        if not loops:
            continue
        ps, pe = cleanpets._anchor_pool(loops)
        got = cleanpets.getAnchors(loops)
        assert len(got) == components(list(ps), list(pe)), t
        # disjoint, not touching, ascending, and covering exactly the union
        assert all(got[k + 1][0] > got[k][1] for k in range(len(got) - 1))
        v = np.arange(-2, span + 45)
        union = brute_mask(v, v, ps, pe)
        assert np.array_equal(union, brute_mask(v, v, [g[0] for g in got], [g[1] for g in got])), t
    assert cleanpets.getAnchors({"a": ["c", 1, 5, "c", 5, 9]}) == [[1, 9]]
    assert cleanpets.getAnchors({"a": ["c", 1, 5, "c", 6, 9]}) == [[1, 5], [6, 9]]


def test_command_line_flags(tmp_path, monkeypatch):
    """-s, -c, -p (no effect), -o created when missing, -f / -d; the output files of the command line are the goldens"""
    from cloops_amd import cleanpets
    brute_backend(monkeypatch)
    dirs = write_jd_dirs(tmp_path)
    loopf = os.path.join(GOLD, "cleanpets_synth.loop")
    for case, extra in (("synth_sig", []), ("synth_all", ["-s"]), ("synth_chroms", ["-s", "-c", "chrA,chrC,chrQ"])):
        for p in ("1", "8"):
            out = os.path.join(str(tmp_path), "o_%s_%s" % (case, p))
            assert not os.path.exists(out)
            assert cleanpets.main(["-d", dirs["synth"], "-f", loopf, "-o", out, "-p", p] + extra) == 0
            _check_case(case, out, "synth")
    out = os.path.join(str(tmp_path), "o_v2")
    cleanpets.main(["-d", dirs["chr21"], "-f", os.path.join(GOLD, "chr21_v2.loop"), "-o", out])
    _check_case("chr21_v2_sig", out, "chr21")
    out = os.path.join(str(tmp_path), "o_none")
    with pytest.raises(ZeroDivisionError):
        cleanpets.main(["-d", dirs["synth"], "-f", loopf, "-o", out, "-c", "chrC,chrD"])
    assert os.path.isdir(out) and os.listdir(out) == []                   # -o is created before the summary raises
    op = cleanpets.help(["-d", "x", "-f", "y", "-o", "z"])
    assert op.significant is True and op.cpu == 1 and op.chroms == ""


def test_log_lines(tmp_path, monkeypatch, caplog):
    import logging
    with caplog.at_level(logging.INFO, logger="cloops_amd.cleanpets"):
        _run_case(tmp_path, "synth_all", monkeypatch)
    msgs = [r.getMessage() for r in caplog.records]
    assert msgs[0].endswith("chrC-chrC.jd not found, however there are loops in that chromosome.")
    assert "('chrA', 'chrA'):" in msgs[1] and "& 8 loops,merged 10 anchors" in msgs[1]
    assert msgs[-2] == "('chrZ', 'chrZ'):0 raw PETs 0 PETs in anchors"                  # a .jd with zero rows
    assert msgs[-1].endswith("loops:12, anchors:17,raw PETs: 1392, PETs in anchors:187, ratio:%s" % (187 / 1.0 / 1392))


@pytest.mark.reference
def test_script_functions_live(tmp_path):
    """the script's own getAnchors / getAnchorPETs (sliced as the golden script does) on random small cases against the brute force"""
    import refload
    if not refload.available():
        pytest.skip("reference checkout absent")
    sys_path = os.path.join(GOLD)
    import sys
    sys.path.insert(0, sys_path)
    try:
        import make_golden_cleanpets as M
    finally:
        sys.path.remove(sys_path)
    from cloops_amd import cleanpets
    rng = np.random.default_rng(77)
    for t in range(20):
        ns = M.script_namespace()
        n = int(rng.integers(1, 400))
        x = rng.integers(0, 3000, n)
        y = x + rng.integers(0, 2000, n)
        jd = os.path.join(str(tmp_path), "c-c.jd")
        joblib.dump(np.stack([np.arange(n), x, y], 1).astype(np.int64), jd)
        a = int(rng.integers(1, 12))
        s = rng.integers(0, 5000, 2 * a)
        e = s + rng.integers(0, 200, 2 * a)
        loops = {"l%d" % k: ["c", int(s[2 * k]), int(e[2 * k]), "c", int(s[2 * k + 1]), int(e[2 * k + 1])] for k in range(a)}
        out = os.path.join(str(tmp_path), "o%d" % t)
        os.mkdir(out)
        l, na, raw, kept = ns["getAnchorPETs"](jd, loops, out)
        assert na == len(cleanpets.getAnchors(loops)) == len(ns["getAnchors"](loops))
        rows = np.sort(joblib.load(os.path.join(out, "c-c.jd"))[:, 0])
        ps, pe = cleanpets._anchor_pool(loops)
        assert np.array_equal(rows, np.flatnonzero(brute_mask(x, y, ps, pe))) and kept == len(rows)
