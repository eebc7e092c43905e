"""CPU: the host side of cloops_amd.dots against plain loops, the restatement of tests/dots_cases.py against the definitions' own
numbers, the texts of the four files, jd2dots end to end on the restatement's stand-in chromosome, the recovery case, and a check that
the shapes of tests/test_gpu_dots.py reach the edges they are there for."""
import json
import os

import numpy as np
import pytest

import dots_cases as DC
import matrix_cases as MC
from cloops_amd import dots


# ---- the neighbourhoods ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,w", [(0, 1), (1, 3), (2, 5), (4, 7), (0, 16), (15, 16)])
def test_masks_have_the_sizes_the_rules_imply(p, w):
    m = DC.masks(p, w)
    inner_off = (2 * p) ** 2                                                 # entries of the inner square off the pixel's row and column
    assert m[0].sum() == (2 * w) ** 2 - inner_off                            # the box less the cross, less the inner square's part of it
    assert m[1].sum() == w * w - p * p                                       # one quadrant less the inner square's quarter
    assert m[2].sum() == 3 * 2 * (w - p) == m[3].sum()
    assert np.array_equal(m[3], m[2].T) and np.array_equal(m[0], m[0].T) and np.array_equal(m[0], m[0][::-1, ::-1])
    assert not m[:, w, w].any() and not (m[1] & ~m[0]).any()                 # never the pixel itself; lower-left lies inside the donut
    union = m.any(axis=0)
    assert union.sum() == (2 * w + 1) ** 2 - (2 * p + 1) ** 2                # what a walk of the device reads
    a = np.arange(-w, w + 1)
    assert not union[np.ix_(np.abs(a) <= p, np.abs(a) <= p)].any()
    assert m[1][w + 1:, :w].sum() == m[1].sum()                              # towards the diagonal: larger i, smaller j


def test_restatement_on_a_hand_made_matrix():
    """five bins, all valid, p = 0, w = 1, one cell: the sums can be read off"""
    cells = (np.array([0, 1]), np.array([4, 3]), np.array([1, 6]))
    e = np.array([8.0, 4.0, 2.0, 1.0, 0.5])
    la, n_cand, n_full = DC.lambdas_oracle(cells, 0, 5, 0, np.ones(5, bool), np.ones(5), e, 0, 1, 1, 4)
    assert la.shape == (4, 5, 3) and n_cand == 4 + 3 + 2
    # pixel (2, 3), d = 1: its lower-left neighbour is (3, 2) = the mirror of nothing; its donut holds (1, 2), (1, 4), (3, 2), (3, 4)
    assert la[0, 2, 0] == 0.0 and la[1, 2, 0] == 0.0
    # pixel (2, 2) is no candidate (d = 0 < dmin); pixel (1, 2): the vertical neighbourhood (a = +-1, |b| <= 1) holds (0, 1..3), (2, 1..3):
    # V = 0 there; the horizontal one (|a| <= 1, b = +-1) holds (1, 3) = 6: NO = 6, NE = e[1] + e[0] + e[1] + e[3] + e[2] + e[1]
    ne = 4.0 + 8.0 + 4.0 + 1.0 + 2.0 + 4.0                                  # (0,1) (1,1) (2,1) (0,3) (1,3) (2,3)
    assert la[2, 1, 0] == ((6.0 / ne) * e[1]) / 1.0 and la[3, 1, 0] == 0.0
    # pixel (0, 4), d = 4 is outside [1, 4); pixel (0, 3): its donut (a, b = +-1) holds (1, 2), (1, 4): V = 0, E = e[1] + e[3]
    assert la[0, 0, 2] == 0.0 and np.isnan(la[:, 4, :]).all()                # bin 4: every j = 4 + d lies outside
    # an invalid bin empties its row and column of both matrices, and its pixels are no candidates
    valid = np.array([1, 1, 0, 1, 1], bool)
    la2, _, _ = DC.lambdas_oracle(cells, 0, 5, 0, valid, np.ones(5), e, 0, 1, 1, 4)
    assert np.isnan(la2[:, 2, :]).all() and np.isnan(la2[:, 1, 0]).all() and np.isnan(la2[:, 0, 1]).all()
    # pixel (1, 3): of its horizontal neighbourhood (0,2) (1,2) (2,2) (0,4) (1,4) (2,4) only (0,4) = 1 and (1,4) are left
    assert la2[2, 1, 1] == (1.0 / (e[4] + e[3])) * e[2]
    V, E = DC.dense_VE(cells, 0, 5, 2, valid, np.ones(5), e)
    assert V[1, 3] == V[3, 1] == 6.0 and V[0, 4] == 1.0 and V.sum() == 14.0 and E[0, 1] == 0.0 and E[0, 3] == e[3] and not E[2].any()


def test_chunks_histogram_and_call_of_the_restatement():
    edges = np.array([1.0, 2.0, 4.0])
    assert DC.chunk_of([0.0, 1.0, 1.5, 2.0, 2.5, 4.0, 4.5], edges).tolist() == [0, 0, 1, 1, 2, 2, 3]
    la = np.full((4, 2, 2), np.nan)
    la[:, 0, 0] = [0.5, 1.0, 2.0, 4.0]                                       # full, chunks 0 0 1 2
    la[:, 0, 1] = [0.5, 0.5, 0.5, 4.5]                                       # full, beyond in kernel 3
    la[:3, 1, 0] = 1.0                                                       # not full
    la[:, 1, 1] = 3.0                                                        # full, chunk 2, no cell
    counts = np.array([[5000, 7], [9, 0]])
    hist, nbey = DC.hist_oracle(la, counts, edges)
    assert nbey == 1 and hist.sum() == 8
    assert hist[0, 0, DC.CMAX] == hist[1, 0, DC.CMAX] == hist[2, 1, DC.CMAX] == hist[3, 2, DC.CMAX] == 1 and (hist[:, 2, 0] == 1).all()
    cells = (np.array([0, 0, 1, 1]), np.array([0, 1, 1, 2]), np.array([5000, 7, 9, 3]))
    la4 = np.stack([la[:, 0, 0], la[:, 0, 1], la[:, 1, 0], la[:, 1, 1]])
    thr = np.zeros((4, 3), np.uint32)
    assert DC.call_oracle(cells, la4, edges, thr).tolist() == [0, 3]
    thr[2, 1] = 5001
    assert DC.call_oracle(cells, la4, edges, thr).tolist() == [3]
    thr[:, 2] = 4
    assert DC.call_oracle(cells, la4, edges, thr).tolist() == []


# ---- the host rules --------------------------------------------------------------------------------------------------------------
def test_thresholds_match_the_loop_over_t():
    rng = np.random.default_rng(4)
    edges = dots.default_edges(7)
    assert edges[0] == 1.0 and edges[3] == 2.0 and edges[6] == 4.0
    hist = np.zeros((4, 7, DC.CMAX + 1), np.uint64)
    for k in range(4):
        for l in range(7):
            n = int(rng.integers(0, 4000))
            c = np.minimum(rng.poisson(float(edges[l]) * rng.uniform(0.3, 1.0), n), DC.CMAX)
            np.add.at(hist[k, l], c, np.uint64(1))
    hist[0, 1] = 0                                                           # a chunk without pixels
    hist[1, 2] = 0
    hist[1, 2, 0] = 500                                                      # ... with zero counts alone
    hist[2, 3, 40] += np.uint64(3)                                           # a few far outliers: their own threshold
    hist[3, 6, DC.CMAX] = 2
    for fdr in (0.1, 0.01, 1.0):
        thr, n = dots.thresholds(hist, edges, fdr)
        assert thr.dtype == np.uint32 and np.array_equal(thr, DC.thresholds_by_loop(hist, edges, fdr))
        assert np.array_equal(n, hist.astype(np.int64).sum(axis=2))
        assert thr[0, 1] == dots.NO_THRESHOLD and thr[1, 2] == dots.NO_THRESHOLD and thr[2, 3] <= 40 and thr[3, 6] <= DC.CMAX
    thr, _ = dots.thresholds(hist, edges, 0.1)
    assert ((thr >= 1) & ((thr <= DC.CMAX) | (thr == dots.NO_THRESHOLD))).all()


def test_enrichment_filter():
    la = np.array([[1.0, 1.0, 1.0, 1.0], [1.0, 2.0, 1.0, 1.0], [0.0, 1.0, 1.0, 1.0], [1.0, 1.0, np.nan, 1.0], [1.0, 1.0, 1.0, 1.5]])
    cnt = np.array([2, 2, 2, 2, 2])
    assert dots.enrichment_pass(cnt, la, dots.DEFAULT_ENRICH).tolist() == [True, False, True, False, False]
    assert dots.enrichment_pass(cnt, la, (2.0, 1.0, 1.0, 1.0, 2.5)).tolist() == [False, False, True, False, False]
    assert dots.enrichment_pass(np.zeros(0), np.zeros((0, 4)), dots.DEFAULT_ENRICH).shape == (0,)


def test_components_and_ties():
    rng = np.random.default_rng(8)
    for r in (1, 2, 5):
        bx = rng.integers(0, 40, 60)
        by = bx + rng.integers(0, 40, 60)
        cnt = rng.integers(1, 6, 60)
        loops = dots.merge_pixels(bx, by, cnt, r)
        comps = DC.components_by_flood(bx, by, r)
        assert len(loops) == len(comps) and sum(s for _, s, _, _ in loops) == 60
        by_best = {a: (s, cx, cy) for a, s, cx, cy in loops}
        for comp in comps:
            best = min(comp, key=lambda a: (-cnt[a], bx[a], by[a]))           # the largest count, ties to the lowest (bx, by)
            assert by_best[best][0] == len(comp)
            assert by_best[best][1] == float(np.mean(bx[comp])) and by_best[best][2] == float(np.mean(by[comp]))
        assert [(bx[a], by[a]) for a, _, _, _ in loops] == sorted((bx[a], by[a]) for a, _, _, _ in loops)
        small = dots.merge_pixels(bx, by, cnt, r, minpix=3)
        assert [t for t in loops if t[1] >= 3] == small
    # a chain joins through its middle; a diagonal step is one bin away; a tie goes to the lowest (bx, by)
    assert dots.merge_pixels([0, 2, 4, 9], [10, 12, 14, 10], [3, 3, 3, 1], 2) == [(0, 3, 2.0, 12.0), (3, 1, 9.0, 10.0)]
    assert dots.merge_pixels([5, 5], [9, 8], [2, 2], 1) == [(1, 2, 5.0, 8.5)]
    assert dots.merge_pixels([0, 3], [0, 0], [1, 1], 2) == [(0, 1, 0.0, 0.0), (1, 1, 3.0, 0.0)]
    assert dots.merge_pixels([], [], [], 1) == []


def test_argument_checks():
    ok = dict(p=2, w=5, mindist=0, maxdist=2000000, fdr=0.1, chunks=40, merge=20000, minpix=1, enrich="1.75,1.75,1.5,1.5,2.0")
    assert dots.check_dot_args(**ok) == (2, 5, 0, 2000000, 0.1, 40, 20000, 1, dots.DEFAULT_ENRICH)
    for key, bad in (("p", -1), ("p", 5), ("w", 17), ("w", 2.5), ("p", True), ("mindist", -1), ("maxdist", -5), ("fdr", 0.0), ("fdr", 1.5),
                     ("fdr", float("nan")), ("chunks", 0), ("chunks", 65), ("merge", -1), ("minpix", 0), ("enrich", "1,2,3"),
                     ("enrich", "a,b,c,d,e"), ("enrich", (1, 1, 1, 1, -1)), ("enrich", (1, 1, 1, 1, float("nan")))):
        with pytest.raises(ValueError):
            dots.check_dot_args(**dict(ok, **{key: bad}))
    assert dots.band_of(400, 2, 2, 1000, 0, 199000) == (4, 200) and dots.band_of(50, 2, 2, 10000, 0, 2000000) == (4, 50)
    assert dots.band_of(400, 7, 2, 1000, 30500, 10 ** 9) == (30, 400) and dots.band_of(400, 7, 2, 1000, 0, 5000) == (7, 6)
    op = dots.help(["-d", "x", "-o", "y"])
    assert (op.res, op.p, op.w, op.mindist, op.maxdist, op.fdr, op.chunks, op.merge, op.minpix) == (10000, 2, 5, 0, 2000000, 0.1, 40, 20000, 1)
    assert dots.check_dot_args(op.p, op.w, op.mindist, op.maxdist, op.fdr, op.chunks, op.merge, op.minpix, op.enrich)[8] == dots.DEFAULT_ENRICH
    assert not op.raw and op.cut == 0 and op.chroms == "" and op.ignorediags == 2 and op.mad == 5.0 and not op.nosmooth


def test_the_texts():
    bx, by, cnt = np.array([3, 10]), np.array([60, 25]), np.array([41, 7])
    la4 = np.array([[0.1, 2.5, np.nan, 1.0 / 3.0], [1.0, 2.0, 3.0, 4.0]])
    loops = [(1, 3, 10.5, 25.0)]
    assert dots.format_loops("chr1", 1000, bx, by, cnt, la4, loops) == \
        "chr1\t10000\t11000\tchr1\t25000\t26000\t7\t1.0\t2.0\t3.0\t4.0\t3\t11000.0\t25500.0\n"
    assert dots.format_pixels("chr1", 1000, bx, by, cnt, la4, np.array([False, True])) == \
        "chr1\t3000\t4000\tchr1\t60000\t61000\t41\t0.1\t2.5\tnan\t%s\t0\n" % repr(1.0 / 3.0) + \
        "chr1\t10000\t11000\tchr1\t25000\t26000\t7\t1.0\t2.0\t3.0\t4.0\t1\n"
    edges = dots.default_edges(2)
    thr = np.array([[3, dots.NO_THRESHOLD]] * 4, np.uint32)
    n = np.array([[12, 0]] * 4)
    text = dots.format_thresholds("chr1", edges, n, thr)
    assert text.splitlines()[0] == "chr1\tdonut\t0\t1.0\t12\t3" and text.splitlines()[1] == "chr1\tdonut\t1\t%s\t0\tnone" % repr(2.0 ** (1.0 / 3.0))
    assert [l.split("\t")[1] for l in text.splitlines()] == ["donut", "donut", "ll", "ll", "h", "h", "v", "v"]
    assert float(text.splitlines()[1].split("\t")[3]) == edges[1]            # repr reads back to the same bits


# ---- end to end on the stand-in --------------------------------------------------------------------------------------------------
class FakeRecord(object):
    def __init__(self, X, Y):
        import threading
        self.chrom, self.lock = DC.OracleChrom(X, Y), threading.Lock()


def test_jd2dots_end_to_end_on_the_stand_in(tmp_path, monkeypatch):
    from cloops_amd import matrix
    Xa, Ya = MC.scattered(2, 30000, 120000, 40000)
    recs = [("chr1", FakeRecord(Xa, Ya)), ("chr7", FakeRecord(*MC.scattered(3, 200, 90000, 20000))), ("chr9", FakeRecord(np.zeros(0), np.zeros(0)))]
    monkeypatch.setattr(matrix, "_records", lambda jd, chroms=(): [r for r in recs if not chroms or r[0] in chroms])
    out = os.path.join(str(tmp_path), "o")
    js = dots.jd2dots("jd", out, res=2000, w=4, p=1, maxdist=60000, fdr=0.2, chunks=9, minpix=1, enrich=(1.2, 1.2, 1.1, 1.1, 1.3))
    got = {}
    for sfx in dots.SUFFIXES:
        with open(out + sfx) as fh:
            got[sfx] = fh.read()
    assert json.loads(got["_dots.json"]) == js and sorted(js["chroms"]) == ["chr1", "chr7", "chr9"]
    assert js["args"]["w"] == 4 and js["args"]["enrich"] == [1.2, 1.2, 1.1, 1.1, 1.3] and js["args"]["chunks"] == 9
    st = js["chroms"]["chr1"]
    assert st["dmin"] == 3 and st["dmax"] == 31 and st["n_full"] > 1000 and st["n_sig"] >= st["n_kept"] >= st["n_loops"]
    assert js["chroms"]["chr9"]["nb"] == 0 and js["chroms"]["chr9"]["n_cand"] == 0
    # the sparse chromosome: its pixels have a la above ... or none at all; a warning says which
    assert any(w.startswith("chr7") for w in js["warnings"]) or js["chroms"]["chr7"]["n_full"] > 0
    thr_rows = [l.split("\t") for l in got["_dots_thresholds.txt"].splitlines()]
    assert len(thr_rows) == 3 * 4 * 9 and {r[1] for r in thr_rows} == set(dots.KERNELS)
    pix = [l.split("\t") for l in got["_dots_pixels.txt"].splitlines()]
    assert len(pix) == sum(js["chroms"][c]["n_sig"] for c in js["chroms"]) and all(len(r) == 12 for r in pix)
    assert sum(int(r[11]) for r in pix) == sum(js["chroms"][c]["n_kept"] for c in js["chroms"])
    loops = [l.split("\t") for l in got["_dots.bedpe"].splitlines()]
    assert len(loops) == sum(js["chroms"][c]["n_loops"] for c in js["chroms"]) and all(len(r) == 14 for r in loops)
    assert sum(int(r[11]) for r in loops) == sum(int(r[11]) for r in pix)     # minpix 1: every kept pixel lies in one loop
    # every significant pixel reaches its thresholds, recomputed from the texts alone
    edges = dots.default_edges(9)
    thr = {(r[0], r[1], int(r[2])): r[5] for r in thr_rows}
    for r in pix:
        for k, name in enumerate(dots.KERNELS):
            t = thr[(r[0], name, int(DC.chunk_of(float(r[7 + k]), edges)))]
            assert t != "none" and int(r[6]) >= int(t)
    # a chromosome filter, and a refusal before any file is written
    js1 = dots.jd2dots("jd", out + "1", res=2000, chroms={"chr7"})
    assert list(js1["chroms"]) == ["chr7"]
    with pytest.raises(ValueError):
        dots.jd2dots("jd", out + "2", w=3, p=3)
    assert not os.path.exists(out + "2" + dots.SUFFIXES[0])


def test_out_of_order_calls_of_the_stand_in():
    ch = DC.OracleChrom(*MC.scattered(1, 2000, 50000, 9000))
    ch.mat_cells(1000, fold=True)
    b0, nb, _ = ch.bal_marginals(2)
    ch.exp_diagonals(balanced=False)
    with pytest.raises(RuntimeError):
        ch.dot_lambdas(2, 5, 4, 20)                                          # before exp_set
    ch.exp_set(np.ones(nb))
    with pytest.raises(RuntimeError):
        ch.dot_hist([1.0])
    for bad in ((2, 5, 1, 20), (2, 5, 20, 20), (2, 5, 4, nb + 1)):
        with pytest.raises(RuntimeError):
            ch.dot_lambdas(*bad)
    e = np.ones(nb)
    e[9] = np.nan
    ch.exp_set(e)
    with pytest.raises(RuntimeError):
        ch.dot_lambdas(2, 5, 4, 20)
    ch.exp_set(np.ones(nb))
    ch.dot_lambdas(2, 5, 4, 20)
    with pytest.raises(RuntimeError):
        ch.dot_call(np.zeros((4, 1)))
    ch.dot_hist([1.0])
    with pytest.raises(RuntimeError):
        ch.dot_sig()
    assert ch.dot_call(np.zeros((4, 1))) == len(ch.dot_sig())
    ch.exp_set(np.ones(nb))
    with pytest.raises(RuntimeError):
        ch.dot_cells()


# ---- the recovery case -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_recovery_of_the_planted_loops(seed):
    """400 bins of 1000 bp, some 600 k background PETs with log-uniform distances, 40 extra PETs at each of eight bin pairs; raw mode,
    unsmoothed expected, ign 2, p 2, w 5, dmax 200, fdr 0.1, the default edges and filter.  Every bin is valid (`-mad 0`: the window's
    first and last bins have low coverage by construction, not by fault): every planted pair is called at its bins, as one pixel, nothing
    else is called, and the same data without the extra PETs calls nothing."""
    assert DC.RECOVERY_SEED in (1, 2, 3)
    kw = dict(p=2, w=5, maxdist=199000, fdr=0.1, raw=True, nosmooth=True, ignore_diags=2, mad_max=0)
    X, Y = DC.recovery_rows(seed, True)
    assert 480000 < len(X) < 540000                                          # 600 k drawn, those with Y beyond the window dropped
    r = dots.dots_chrom(DC.OracleChrom(X, Y), "chrT", 1000, **kw)
    assert (r["stats"]["dmin"], r["stats"]["dmax"], r["stats"]["nb"]) == (4, 200, 400) and r["warnings"] == []
    assert sorted(r["called"]) == sorted(DC.PLANTED)
    assert r["stats"]["n_sig"] == r["stats"]["n_kept"] == r["stats"]["n_loops"] == len(DC.PLANTED)    # one pixel each
    assert [int(l.split("\t")[11]) for l in r["loops"].splitlines()] == [1] * len(DC.PLANTED)
    X, Y = DC.recovery_rows(seed, False)
    r0 = dots.dots_chrom(DC.OracleChrom(X, Y), "chrT", 1000, **kw)
    assert r0["stats"]["n_sig"] == 0 and r0["called"] == [] and r0["loops"] == "" and r0["stats"]["n_full"] > 50000


# ---- the shapes of the GPU tier reach their edges --------------------------------------------------------------------------------------
def test_gpu_cases_reach_their_edges():
    cases = DC.LA_CASES
    want = {1, 2, 31, 32, 33, 64, 65, 97}
    assert {c["nb"] for c in cases.values()} == want and {c["nd"] for c in cases.values()} == want
    assert {(c["p"], c["w"]) for c in cases.values()} == {(0, 1), (1, 3), (2, 5), (4, 7), (0, 16), (15, 16)}
    assert {c["ign"] for c in cases.values()} >= {0, 2} and any(c["ign"] > 2 * c["w"] for c in cases.values())
    assert any(c["w"] >= c["nb"] for c in cases.values()) and any(c.get("shift", 0) < 0 for c in cases.values())
    assert any(c["raw"] for c in cases.values()) and any(not c["raw"] for c in cases.values())
    T = DC.TILE
    assert any(c["nb"] > T and c["nb"] % T for c in cases.values()) and any(c["nd"] > T and c["nd"] % T for c in cases.values())
    assert any(c["nb"] == 2 * T for c in cases.values()) and any(c["nd"] == 2 * T for c in cases.values())
    crossing = beyond_window = zeros = masked = False
    for name, c in cases.items():
        X, Y = DC.case_rows(name)
        bx, by, cnt = MC.cells_oracle(X, Y, 0, 1, True)[:3]
        b0 = int(bx[0])
        assert b0 == c.get("shift", 0) and int(by.max()) - b0 + 1 == c["nb"]  # the cells span exactly the bins
        dmax = c["dmin"] + c["nd"]
        assert c["ign"] <= c["dmin"] < dmax <= c["nb"]
        d = by - bx
        # a footprint across the diagonal: a pixel nearer the diagonal than 2w whose mirrored half holds a cell
        crossing |= c["dmin"] == c["ign"] == 0 and bool(((d > 0) & (d <= 2 * c["w"])).any())
        beyond_window |= c["w"] > 0 and c["nb"] > 1                          # rows i - w < 0 and i + w >= nb at the first and last bins
        if c["mask"] is not None:
            v = c["mask"](c["nb"])
            run = max(len(s) for s in "".join("01"[int(x)] for x in v).split("1"))
            masked |= bool(run > T and not v[0] and not v[-1])
        if c["expected"] is not None:
            e = c["expected"](c["nb"])
            zeros |= bool((e[c["ign"]:min(c["nb"], dmax + 2 * c["w"])] == 0).any())
    assert crossing and beyond_window and zeros and masked
    # the restatement finds full pixels, not-full candidates and non-candidates in a masked case, on the CPU
    c = cases["nd31_neg"]
    X, Y = DC.case_rows("nd31_neg")
    ch = DC.OracleChrom(X, Y)
    ch.mat_cells(1, fold=True)
    b0, nb, _ = ch.bal_marginals(c["ign"])
    ch.exp_diagonals(valid=c["mask"](nb), balanced=False)
    p, _, vs = ch.exp_diagonals_get()
    from cloops_amd import expected as X26
    ch.exp_set(X26.expected_of(p, vs, c["ign"])[0])
    n_cand, n_full = ch.dot_lambdas(c["p"], c["w"], c["dmin"], c["dmin"] + c["nd"])
    assert 0 < n_full <= n_cand < nb * c["nd"]
    la = np.stack([ch.dot_lambdas_get(k) for k in range(4)])
    hist, nbey = ch.dot_hist(dots.default_edges(3))                          # a pixel beyond the last edge
    assert nbey > 0 and hist.sum() > 0 and np.nanmax(la) > 2.0 ** (2.0 / 3.0)


# ---- the walk down the device state, the options and the clean-up that the commands share -------------------------------------
def test_the_calls_on_the_device_and_no_more():
    head = [("mat_cells", (100,), {"cut": 0, "fold": True}), ("bal_marginals", (2,), {}), ("bal_marginals_get", (0, 5), {})]
    tail = [("exp_diagonals_get", (0, 5), {}), ("exp_set", ("f[5]",), {}), ("dot_lambdas", (2, 5, 4, 5), {}), ("dot_hist", ("f[40]",), {}),
            ("dot_call", ("u[4,40]",), {}), ("dot_sig", (0, 0), {}), ("mat_free", (), {})]
    ch = MC.Recording(DC.OracleChrom(*MC.twelve()))
    dots.dots_chrom(ch, "chr1", 100, ignore_diags=2, min_nnz=1)
    assert ch.log == head + [("bal_iterate", ("b[5]",), {"max_iters": 200, "tol": 1e-5}), ("exp_diagonals", (), {})] + tail   # no bal_weights
    ch = MC.Recording(DC.OracleChrom(*MC.twelve()))
    dots.dots_chrom(ch, "chr1", 100, ignore_diags=2, min_nnz=1, raw=True)
    assert ch.log == head + [("exp_diagonals", (), {"valid": "b[5]", "balanced": False})] + tail


def _two_records(monkeypatch, fail=None):
    from cloops_amd import matrix
    recs = [("chr1", FakeRecord(*MC.scattered(2, 3000, 60000, 20000))), ("chr7", FakeRecord(*MC.scattered(3, 200, 90000, 20000)))]
    recs[0][1].chrom = MC.Recording(recs[0][1].chrom, fail=fail)
    monkeypatch.setattr(matrix, "_records", lambda jd, chroms=(): [r for r in recs if not chroms or r[0] in chroms])
    return recs


def test_main_hands_every_option_on(tmp_path, monkeypatch):
    _two_records(monkeypatch)
    out = os.path.join(str(tmp_path), "o")
    kw = dict(res=2000, cut=20, p=1, w=4, mindist=5, maxdist=60000, fdr=0.3, chunks=11, merge=7, minpix=2, enrich=[1.0, 1.25, 1.5, 1.75, 2.0],
              raw=True, per_decade=4, nosmooth=True, ignore_diags=1, min_nnz=3, min_count=1, mad_max=2.5, tol=1e-8, max_iters=30)
    js = dots.jd2dots("jd", out + "k", chroms={"chr1", "chr7"}, **kw)
    assert js["args"] == kw
    assert dots.main(["-d", "jd", "-o", out + "m", "-res", "2000", "-cut", "20", "-c", "chr1,chr7", "-p", "1", "-w", "4", "-mindist", "5", "-maxdist",
                      "60000", "-fdr", "0.3", "-chunks", "11", "-merge", "7", "-minpix", "2", "-enrich", "1,1.25,1.5,1.75,2", "-raw", "-perdecade",
                      "4", "-nosmooth", "-ignorediags", "1", "-minnnz", "3", "-mincount", "1", "-mad", "2.5", "-tol", "1e-8", "-maxiters", "30"]) == 0
    for sfx in dots.SUFFIXES:
        with open(out + "m" + sfx) as fm, open(out + "k" + sfx) as fk:
            assert fm.read() == fk.read()


@pytest.mark.parametrize("step", ["bal_iterate", "exp_diagonals", "exp_set", "dot_lambdas", "dot_sig"])
def test_a_failing_step_frees_the_cells_once_and_writes_nothing(step, tmp_path, monkeypatch):
    recs = _two_records(monkeypatch, fail=step)
    with pytest.raises(RuntimeError):
        dots.jd2dots("jd", os.path.join(str(tmp_path), "f"), res=2000, maxdist=60000)
    log = recs[0][1].chrom.log
    assert [c[0] for c in log].count("mat_free") == 1 and log[-1][0] == "mat_free" and log[-2][0] == step
    assert os.listdir(str(tmp_path)) == [] and recs[1][1].chrom.calls == []
