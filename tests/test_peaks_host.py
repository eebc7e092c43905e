"""CPU: the host side of cloops_amd.peaks and the oracle of kernel K21.  The closed form (tests/peaks_cases.py) against a plain
sequential DBSCAN on seeded small cases; the steps the kernels take (ranks, scans, heads and tails by index) restated in numpy
against the closed form; the interval union, the flank windows, the lambda / ES / p columns on hand-made counts, the bytes of the
three files from fixed inputs, one chromosome's calls in order, argument errors of jd2peaks and the command line."""
import json
import os

import numpy as np
import pytest

import peaks_cases as PC
from cloops_amd import peaks


# ---- the oracle ------------------------------------------------------------------------------------
def random_case(rng):
    n = int(rng.integers(1, 40))
    span = int(rng.integers(1, 60))
    S = np.sort(rng.integers(-span, span + 1, n))                    # duplicates are the rule
    return S, int(rng.integers(1, 8)), int(rng.integers(1, 6))


def test_closed_form_is_sequential_dbscan():
    rng = np.random.default_rng(2021)
    seen_border = seen_many = 0
    for _ in range(400):
        S, eps, minPts = random_case(rng)
        s, e, p, c, ncores = PC.peaks_oracle(S, eps, minPts)
        want = PC.sequential_dbscan(S, eps, minPts)
        assert [a.tolist() for a in (s, e, p, c)] == [list(w) for w in want], (S.tolist(), eps, minPts)
        assert ncores == sum(want[3])
        assert np.all(s[1:] >= e[:-1])                                # ascending and disjoint
        seen_many += len(s) > 1
        seen_border += int((p > c).any())
    assert seen_many > 50 and seen_border > 50                       # the cases are not all trivial


def device_form(S, eps, minPts):
    """the kernels' steps: lo / hi ranks, the scan of the core flags, heads and tails by index, extents from the stored ranks"""
    m = len(S)
    lo, hi = np.searchsorted(S, S - eps, "left"), np.searchsorted(S, S + eps, "right")
    core = (hi - lo) >= minPts
    C = np.concatenate([[0], np.cumsum(core)])
    i = np.arange(m)
    head = core & (C[i] == C[lo])
    tail = core & (C[hi] == C[i + 1])
    a, b = np.flatnonzero(head), np.flatnonzero(tail)
    assert len(a) == len(b) and np.all(a <= b) and np.all(a[1:] > b[:-1])
    i0 = lo[a]
    i0[1:] = np.maximum(i0[1:], hi[b[:-1]])
    i1 = hi[b]
    return S[i0], S[i1 - 1] + 1, i1 - i0, C[b + 1] - C[a], int(C[m])


def test_the_kernels_steps_give_the_closed_form():
    rng = np.random.default_rng(2022)
    for _ in range(600):
        S, eps, minPts = random_case(rng)
        want = PC.peaks_oracle(S, eps, minPts)
        got = device_form(S, eps, minPts)
        assert all(np.array_equal(g, w) for g, w in zip(got[:4], want[:4])) and got[4] == want[4], (S.tolist(), eps, minPts)
    S = PC.ends_of(*PC.seeded_genome()["chr2"])                      # and at a size with hundreds of peaks
    for eps, minPts in ((60, 4), (120, 8), (300, 5)):
        want, got = PC.peaks_oracle(S, eps, minPts), device_form(S, eps, minPts)
        assert len(want[0]) > 100 and all(np.array_equal(g, w) for g, w in zip(got[:4], want[:4]))


def test_border_rule_by_hand():
    # two chains of three cores (minPts 3, eps 2), the point 6 within eps of both: it goes left, the right peak starts after it
    S = np.array([0, 2, 4, 6, 8, 10, 12])
    s, e, p, c, _ = PC.peaks_oracle(S, 2, 3)
    assert (s.tolist(), e.tolist()) == ([0], [13])                    # (every point is a core here: one chain)
    S = np.array([0, 0, 1, 1, 2, 5, 8, 9, 9, 10, 10])                # eps 3, minPts 5: all but 5 are cores; 5 is within 3 of 2 and of 8
    s, e, p, c, ncores = PC.peaks_oracle(S, 3, 5)
    assert (s.tolist(), e.tolist(), p.tolist(), c.tolist(), ncores) == ([0, 8], [6, 11], [6, 5], [5, 5], 10)
    assert PC.sequential_dbscan(S, 3, 5) == ([0, 8], [6, 11], [6, 5], [5, 5])


def test_count_and_summit_oracles():
    S = np.array([-5, 0, 0, 3, 3, 3, 10, 11, 50])
    assert PC.count_oracle(S, [0, 3, -100, 60, 4, 5], [4, 3, 100, 70, 0, 1 << 40]).tolist() == [5, 0, 9, 0, 0, 3]
    for oracle in (PC.summit_oracle, PC.summit_oracle_loop):
        pos, cnt = oracle(S, [-5, 4, 10, 20], [4, 10, 12, 50], 1)
        assert pos.tolist() == [3, -1, 10, -1] and cnt.tolist() == [3, 0, 2, 0]   # 10 and 11 tie at 2: the smaller position
    rng = np.random.default_rng(6)
    for _ in range(200):                                              # the form without a loop against the loop
        S = np.sort(rng.integers(-30, 60, int(rng.integers(1, 50))))
        edges = np.sort(rng.integers(-40, 70, int(rng.integers(2, 12))))
        s, e = edges[:-1], np.minimum(edges[1:], edges[:-1] + rng.integers(0, 30, len(edges) - 1))
        w = int(rng.integers(1, 9))
        assert all(np.array_equal(a, b) for a, b in zip(PC.summit_oracle(S, s, e, w), PC.summit_oracle_loop(S, s, e, w)))


# ---- interval union, flank windows ----------------------------------------------------------------------
def test_merge_intervals():
    m = peaks.merge_intervals
    assert [a.tolist() for a in m([], [])] == [[], []]
    s, e = m([10, 0, 5, 30, 20, 40, 40], [20, 6, 8, 35, 30, 41, 45])
    assert (s.tolist(), e.tolist()) == ([0, 10, 20, 30, 40], [8, 20, 30, 35, 45])     # overlapping merge, abutting stay apart
    s, e = m([0, 1, 2, 50], [100, 3, 4, 60])                                           # nested: the running maximum counts
    assert (s.tolist(), e.tolist()) == ([0], [100])
    s, e = m([5, 5, 5], [6, 9, 7])
    assert (s.tolist(), e.tolist()) == ([5], [9]) and s.dtype == np.int64
    rng = np.random.default_rng(4)
    for _ in range(50):                                                                # against a per-base mask
        a = rng.integers(0, 200, 30)
        b = a + rng.integers(1, 15, 30)
        mask = np.zeros(260, bool)
        for x, y in zip(a, b):
            mask[x:y] = True
        s, e = m(a, b)
        got = np.zeros(260, bool)
        for x, y in zip(s, e):
            got[x:y] = True
        assert np.array_equal(mask, got) and np.all(s[1:] >= e[:-1]) and np.all(e > s)
        starts = set(a.tolist())
        assert all(x in starts for x in s.tolist())


def test_flank_windows():
    w = peaks.flank_windows([100, 1000], [110, 1200], (5, 10))
    assert [[a.tolist() for a in f] for f in w] == [[[50, 0], [160, 2200]], [[0, 0], [210, 3200]]]   # clamped at 0


# ---- significance on hand-made counts -------------------------------------------------------------------
HAND = {"chrA": {"n_ends": 600, "vmin": 1000, "vmax": 60999, "settings": {"100,5": {"n_peaks": 2, "n_cores": 30, "n_clustered": 45}},
                 "candidates": 2, "start": np.array([2000, 30000]), "end": np.array([2010, 30100]), "count": np.array([20, 3]),
                 "bg": [np.array([42, 13]), np.array([60, 23])], "summit": np.array([2004, 30050]), "summit_count": np.array([9, 2])},
        "chrB": {"n_ends": 400, "vmin": 0, "vmax": 39999, "settings": {"100,5": {"n_peaks": 0, "n_cores": 0, "n_clustered": 0}},
                 "candidates": 0, "start": PC.EMPTY, "end": PC.EMPTY, "count": PC.EMPTY, "bg": [PC.EMPTY, PC.EMPTY],
                 "summit": PC.EMPTY, "summit_count": PC.EMPTY}}


def hand_columns():
    from scipy.stats import poisson
    # N = 1000, G = 60000 + 40000; peak 0: L 10, windows of 110 and 210 bp; peak 1: L 100, windows of 1100 and 2100 bp
    lam0 = max(1000 * 10 / 100000, (42 - 20) * 10 / (110 - 10), (60 - 20) * 10 / (210 - 10))
    lam1 = max(1000 * 100 / 100000, (13 - 3) * 100 / (1100 - 100), (23 - 3) * 100 / (2100 - 100))
    assert (lam0, lam1) == (2.2, 1.0)
    p0, p1 = float(poisson.sf(19, lam0)), float(poisson.sf(2, lam1))
    return (lam0, 20 / lam0, p0, min(1.0, p0 * 2), 1), (lam1, 3 / lam1, p1, min(1.0, p1 * 2), 0)


def test_significance_columns():
    assert peaks.genome_of(HAND) == (1000, 100000)
    rows, sig, nsig = peaks.table_of(HAND, (5, 10), 1e-2, 2.0)
    want = hand_columns()
    assert len(rows) == 2 and sig.tolist() == [True, False] and nsig == {"chrA": 1, "chrB": 0}
    assert rows[0] == ("peak-chrA-0", "chrA", 2000, 2010, 10, 20, 2004, 9, 42, 60) + want[0]
    assert rows[1] == ("peak-chrA-1", "chrA", 30000, 30100, 100, 3, 30050, 2, 13, 23) + want[1]
    assert want[1][3] > 1e-2 and want[1][1] == 3.0                                     # ES passes, the corrected p does not
    rows, sig, _ = peaks.table_of(HAND, (5, 10), 1e-2, 10.0)                           # ES 9.09 < 10
    assert sig.tolist() == [False, False]
    rows, sig, _ = peaks.table_of(HAND, (5, 10), 1.0, 2.0)
    assert sig.tolist() == [True, True]
    lam, ES, p = peaks.significance(PC.EMPTY, PC.EMPTY, PC.EMPTY, [], [], 0, 0)
    assert len(lam) == len(ES) == len(p) == 0


def test_file_bytes(tmp_path):
    texts, js = peaks.outputs_of(HAND, [100], [5], 0, "both", [5, 10], 1e-2, 2.0)
    c = hand_columns()
    line = lambda head, cols: "\t".join(str(v) for v in head + cols) + "\n"
    assert texts["_peaks.txt"] == (
        "peakId\tchrom\tstart\tend\tlength\tcount\tsummit\tsummitCount\tflank5Count\tflank10Count\tlambda\tES\tpoisson_p-value\t"
        "poisson_p-value_corrected\tsignificant\n"
        + line(("peak-chrA-0", "chrA", 2000, 2010, 10, 20, 2004, 9, 42, 60), c[0])
        + line(("peak-chrA-1", "chrA", 30000, 30100, 100, 3, 30050, 2, 13, 23), c[1]))
    assert "\t2.2\t9.09090909090909\t" in texts["_peaks.txt"] and texts["_peaks.txt"].endswith("\t1.0\t3.0\t%r\t%r\t0\n" % (c[1][2], c[1][3]))
    assert texts["_peaks.bed"] == "chrA\t2000\t2010\tpeak-chrA-0\t20\n"
    assert json.loads(texts["_peaks.json"]) == js == {
        "eps": [100], "minPts": [5], "cut": 0, "ends": 3, "flank": [5, 10], "pcut": 0.01, "escut": 2.0, "w": 100,
        "chroms": {"chrA": {"n_ends": 600, "vmin": 1000, "vmax": 60999, "settings": HAND["chrA"]["settings"], "candidates": 2, "merged": 2,
                            "significant": 1},
                   "chrB": {"n_ends": 400, "vmin": 0, "vmax": 39999, "settings": HAND["chrB"]["settings"], "candidates": 0, "merged": 0,
                            "significant": 0}},
        "total": {"n_ends": 1000, "span": 100000, "candidates": 2, "merged": 2, "significant": 1}}
    fout = os.path.join(str(tmp_path), "o")
    peaks.write_outputs(fout, texts)
    for suffix in peaks.SUFFIXES:
        with open(fout + suffix) as fh:
            assert fh.read() == texts[suffix]
    assert sorted(os.listdir(str(tmp_path))) == ["o_peaks.bed", "o_peaks.json", "o_peaks.txt"]


def test_a_failure_leaves_no_file(tmp_path):
    fout = os.path.join(str(tmp_path), "o")
    with pytest.raises(TypeError):
        peaks.write_outputs(fout, {"_peaks.txt": "complete\n", "_peaks.bed": None})       # the second write fails
    assert os.listdir(str(tmp_path)) == []
    peaks.write_outputs(fout, {"_peaks.txt": "old\n"})
    with pytest.raises(TypeError):
        peaks.write_outputs(fout, {"_peaks.txt": "new\n", "_peaks.bed": None})
    assert os.listdir(str(tmp_path)) == ["o_peaks.txt"] and open(fout + "_peaks.txt").read() == "old\n"


# ---- one chromosome's calls ------------------------------------------------------------------------------
def test_chrom_peaks_on_the_oracle():
    X, Y = PC.seeded_genome()["chr10"]
    ch = PC.OracleChrom(X, Y)
    d = peaks.chrom_peaks(ch, [60, 120], [4, 8], 0, 3, [5, 10])
    assert ch.calls == ["sort"] + ["call"] * 4 + ["count", "summits", "free"]           # one sort, one count call, one summit call
    S = PC.ends_of(X, Y)
    assert (d["n_ends"], d["vmin"], d["vmax"]) == (len(S), S[0], S[-1])
    cands = [PC.peaks_oracle(S, e, m) for e in (60, 120) for m in (4, 8)]
    assert d["candidates"] == sum(len(c[0]) for c in cands) and list(d["settings"]) == ["60,4", "60,8", "120,4", "120,8"]
    assert d["settings"]["120,4"] == {"n_peaks": len(cands[2][0]), "n_cores": cands[2][4], "n_clustered": int(cands[2][2].sum())}
    ms, me = d["start"], d["end"]
    assert 50 < len(ms) < d["candidates"] and np.all(ms[1:] >= me[:-1])
    assert np.array_equal(d["count"], PC.count_oracle(S, ms, me))
    L = me - ms
    assert np.array_equal(d["bg"][1], PC.count_oracle(S, np.maximum(0, ms - 10 * L), me + 10 * L)) and len(d["bg"]) == 2
    pos, cnt = PC.summit_oracle(S, ms, me, 60)
    assert np.array_equal(d["summit"], pos) and np.array_equal(d["summit_count"], cnt)
    ch = PC.OracleChrom(PC.EMPTY, PC.EMPTY)                                            # a chromosome without PETs
    d = peaks.chrom_peaks(ch, [100], [5], 0, 3, [5])
    assert d["n_ends"] == 0 and len(d["start"]) == 0 and d["settings"]["100,5"] == {"n_peaks": 0, "n_cores": 0, "n_clustered": 0}
    assert peaks.genome_of({"c": d}) == (0, 0)
    texts, js = peaks.outputs_of({"c": d}, [100], [5], 0, "both", [5], 1e-2, 2.0)
    assert texts["_peaks.txt"].count("\n") == 1 and texts["_peaks.bed"] == "" and js["total"]["merged"] == 0


# ---- argument errors --------------------------------------------------------------------------------------
def test_int_list():
    assert peaks.int_list("200,100,100", "eps") == [100, 200] and peaks.int_list((5, 10), "minPts") == [5, 10]
    assert peaks.int_list(7, "eps") == [7] and peaks.int_list(np.int64(7), "eps") == [7]
    for bad in ("", "a,b", "0,5", [-1], [], "1.5", None):
        with pytest.raises(ValueError):
            peaks.int_list(bad, "eps")


@pytest.mark.parametrize("kw", [{"eps": "0"}, {"eps": [1 << 29]}, {"minPts": "0,5"}, {"minPts": "x"}, {"ends": "middle"}, {"ends": 4},
                                {"flank": "0"}, {"flank": []}, {"pcut": 1.5}, {"pcut": -0.1}, {"escut": -1}, {"escut": float("nan")}])
def test_jd2peaks_argument_errors(tmp_path, kw):
    with pytest.raises(ValueError):
        peaks.jd2peaks(str(tmp_path), os.path.join(str(tmp_path), "o"), **kw)
    assert os.listdir(str(tmp_path)) == []


def test_jd2peaks_needs_a_directory(tmp_path):
    with pytest.raises(ValueError):
        peaks.jd2peaks(os.path.join(str(tmp_path), "missing"), os.path.join(str(tmp_path), "o"))


def test_command_line_arguments():
    op = peaks.help(["-d", "jd", "-o", "out"])
    assert (op.d, op.output, op.eps, op.minPts, op.cut, op.ends, op.flank, op.pcut, op.escut, op.chroms) == (
        "jd", "out", "100,200", "5,10", 0, "both", "5,10", 1e-2, 2.0, "")
    op = peaks.help(["-d", "jd", "-o", "out", "-eps", "50", "-minPts", "3,4", "-cut", "1000", "-ends", "left", "-flank", "2", "-pcut", "1e-5",
                     "-escut", "3", "-c", "chr1,chr2"])
    assert (op.eps, op.minPts, op.cut, op.ends, op.flank, op.pcut, op.escut, op.chroms) == ("50", "3,4", 1000, "left", "2", 1e-5, 3.0, "chr1,chr2")
    for bad in (["-o", "out"], ["-d", "jd"], ["-d", "jd", "-o", "out", "-ends", "middle"], ["-d", "jd", "-o", "out", "-cut", "x"]):
        with pytest.raises(SystemExit):
            peaks.help(bad)
    with pytest.raises(ValueError):
        peaks.main(["-d", "jd", "-o", "out", "-eps", "0"])
