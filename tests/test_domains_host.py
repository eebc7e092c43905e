"""CPU: the oracle of kernel K22 and the host side of cloops_amd.domains.  The range form of the three tracks (what the kernel does)
against the brute-force count of the definition on seeded small cases, the count oracle's two paths against each other, the host
rules on hand-made scores, the planted genome (every planted boundary found), the chr21 example's pinned values from the oracle,
the bytes of the files from fixed inputs, argument errors, and write_outputs leaving nothing behind on failure."""
import json
import os

import numpy as np
import pytest

import domains_cases as DC
import golden_util as G
from cloops_amd import domains


# ---- the oracle ------------------------------------------------------------------------------------
def random_case(rng):
    n = int(rng.integers(1, 50))
    span = int(rng.integers(1, 90))
    res = int(rng.choice([1, 1, 2, 3, 7, 10]))
    X = rng.integers(-span, span + 1, n)                                 # negative coordinates: floor is not trunc
    Y = X + rng.integers(-4, span, n)                                    # some rows with Y < X
    return X, Y, int(rng.choice([0, 0, -3, 2, 9])), res, int(rng.integers(1, 7))


def test_range_form_is_the_brute_force_count():
    rng = np.random.default_rng(2201)
    seen_neg = seen_back = seen_res1 = seen_cut = 0
    for _ in range(500):
        X, Y, cut, res, w = random_case(rng)
        a, b = DC.tracks_oracle(X, Y, cut, res, w, "brute"), DC.tracks_oracle(X, Y, cut, res, w, "range")
        assert all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])) and a[3:] == b[3:], (X.tolist(), Y.tolist(), cut, res, w)
        if a[5]:
            assert len(a[0]) == a[3] and a[0][0] == 0 and a[0][-1] == 0  # the two ends of a track have cross = 0 by construction
        seen_neg += int(X.min() < 0 and res > 1)
        seen_back += int((Y < X).any())
        seen_res1 += res == 1
        seen_cut += int(0 < a[5] < len(X))
    assert min(seen_neg, seen_back, seen_res1, seen_cut) > 40           # the cases are not all trivial


def test_tracks_by_hand():
    # res 10, w 2; rows (bx, by): (0, 0), (0, 1), (1, 3), (-1, 0), and one with by < bx
    X, Y = np.array([5, 3, 12, -4, 30]), np.array([7, 15, 33, 2, 21])
    cross, up, down, nb, bmin, kept = DC.tracks_oracle(X, Y, 0, 10, 2, "brute")
    assert (nb, bmin, kept) == (6, -1, 5)                                # bins -1 .. 3 and the entry behind the last
    assert cross.tolist() == [0, 1, 1, 1, 1, 0]                          # (-1, 0) crosses b = 0, (0, 1) b = 1, (1, 3) b = 2 and b = 3
    assert up.tolist() == [0, 0, 2, 2, 0, 0]                             # (0, 0) before b = 1 and 2, (-1, 0) before b = 1, (0, 1) before b = 2
    assert down.tolist() == [2, 2, 0, 0, 0, 0]                           # (-1, 0) and (0, 0) behind b = -1, (0, 0) and (0, 1) behind b = 0
    assert DC.tracks_oracle(X, Y, 0, 10, 2)[0].tolist() == cross.tolist()
    assert DC.tracks_oracle(X, Y, 25, 10, 2)[3:] == (0, 0, 0)            # the cut removes every row
    assert DC.tracks_oracle(X, Y, 12, 10, 2)[3:] == (5, 0, 2)            # (3, 15) and (12, 33) stay: bins 0 .. 3


def test_count_oracle_paths_agree():
    rng = np.random.default_rng(2202)
    X = rng.integers(0, 100000, 3000)
    Y = X + rng.integers(-50, 5000, 3000)
    cuts = np.sort(rng.integers(-100, 101000, 401))
    s, e = cuts[:-1].copy(), cuts[1:].copy()
    e[::3] -= np.minimum(e[::3] - s[::3], 7)                             # gaps, and empty intervals where a piece is short
    a = DC.count_oracle(X, Y, 0, s, e)
    big = DC.count_oracle(np.tile(X, 50), np.tile(Y, 50), 0, s, e)       # 150 000 rows x 400 intervals: the search path
    assert all(np.array_equal(50 * p, q) for p, q in zip(a, big)) and a[0].sum() > 100
    assert [v.tolist() for v in DC.count_oracle([1, 5, 9], [5, 9, 1], 0, [0, 5, 5], [5, 5, 10])] == [[0, 0, 1], [1, 0, 2], [1, 0, 2]]


# ---- the host rules ----------------------------------------------------------------------------------
def test_score_and_boundaries_by_hand():
    s, valid = domains.score_of([3, 5, 1, 5, 5, 0], [10, 5, 9, 5, 0, 2], [7, 10, 10, 10, 5, 0], 10)
    assert valid.tolist() == [True, True, True, True, True, False] and s.tolist() == [0.15, 0.25, 0.05, 0.25, 0.5, 0.0]
    idx, st = domains.boundaries_of(s, valid, 2, 0.05)
    assert idx.tolist() == [2] and np.allclose(st, [0.2])                # the smaller of 0.25 - 0.05 and 0.5 - 0.05; entry 5 is not valid
    assert domains.boundaries_of(s, valid, 2, 0.21)[0].tolist() == []    # delta
    idx, st = domains.boundaries_of([0.0, 0.3], [True, True], 2, 0.05)   # entry 0 has no left side: the right one decides
    assert idx.tolist() == [0] and st.tolist() == [0.3]
    tie = np.array([0.5, 0.1, 0.3, 0.1, 0.5])                            # the leftmost of a tie wins
    assert domains.boundaries_of(tie, np.ones(5, bool), 2, 0.05)[0].tolist() == [1]
    assert domains.boundaries_of(tie, np.ones(5, bool), 1, 0.05)[0].tolist() == [1, 3]
    assert domains.boundaries_of([0.2], [True], 3, 0.0)[0].tolist() == []                # both sides empty
    assert domains.boundaries_of([], [], 3, 0.0)[0].tolist() == []
    valid = np.array([1, 1, 0, 0, 0, 1, 1, 1, 1], bool)
    a, b = domains.domains_of([0, 5, 8], valid, 500)
    assert (a.tolist(), b.tolist()) == ([5], [8])                        # 2 of 5 bins valid: dropped; 3 of 3: kept
    assert domains.domains_of([0, 4, 8], valid, 500)[0].tolist() == [0, 4]               # 2 of 4 is half
    assert domains.domains_of([0, 4, 8], np.ones(9, bool), 3)[0].tolist() == []          # maxbins
    ES, dens = domains.enrichment([10, 0, 4], [12, 3, 4], [14, 0, 4], [0, 0, 100], [100, 10, 300])
    assert ES.tolist() == [10 / 6, 0.0, 4.0] and dens.tolist() == [0.1, 0.0, 0.02]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_genome(seed):
    X, Y, first, end = DC.planted_genome(seed)
    assert len(first) == 12 and 12 * 15 <= end <= 12 * 59
    for delta in (0.05, 0.1):
        ch = DC.OracleChrom(X, Y)
        r = domains.chrom_domains(ch, DC.PLANT_RES, [10], 0, 20, delta, 500)[10]
        found = r["boundary"] + r["bin0"]
        assert set(first.tolist()) <= set(found.tolist()) and len(found) <= len(first) + 1
        planted = np.isin(found, first)
        assert r["strength"][planted].min() > 0.3                       # far above either delta
        assert [c[0] for c in ch.calls] == ["tracks", "count", "free"]
        ES, _ = domains.enrichment(r["intra"], r["nx"], r["ny"], r["start"], r["end"])
        inner = np.isin(r["start"] // DC.PLANT_RES, first) & np.isin(r["end"] // DC.PLANT_RES, np.append(first, end))
        assert inner.sum() >= 11 and ES[inner].min() > 2.0


# (res, w) -> bins, sum(cross), max(cross), boundaries, domains, sum(intra), domains with ES >= 1 at mincov 20, delta 0.05, maxbins 500
CHR21_PINNED = {(10000, 10): (4167, 110425, 395, 55, 50, 80328, 40),
                (5000, 20): (8333, 220078, 395, 65, 59, 73565, 40)}


def pinned_of(r):
    ES, _ = domains.enrichment(r["intra"], r["nx"], r["ny"], r["start"], r["end"])
    return (r["n_bins"], int(r["cross"].sum()), int(r["cross"].max()), len(r["boundary"]), len(r["start"]), int(r["intra"].sum()),
            int((ES >= 1.0).sum()))


@pytest.mark.parametrize("res,w", sorted(CHR21_PINNED))
def test_chr21_pinned_from_the_oracle(res, w):
    X, Y = G.chr21_xy()
    r = domains.chrom_domains(DC.OracleChrom(X, Y), res, [w], 0)[w]
    assert pinned_of(r) == CHR21_PINNED[(res, w)]


# ---- files and arguments -------------------------------------------------------------------------------
def small_result():
    X = np.array([5, 15, 25, 35, 12, 18, 31, 38, 3, 22], np.int64)
    Y = np.array([8, 19, 28, 39, 17, 19, 36, 39, 14, 33], np.int64)
    return {"chrB": domains.chrom_domains(DC.OracleChrom(X, Y), 10, [1, 2], 0, 1, 0.0, 500),
            "chrA": domains.chrom_domains(DC.OracleChrom(X + 100, Y + 100), 10, [1, 2], 0, 1, 0.0, 500)}


def test_outputs_from_fixed_inputs():
    per = small_result()
    texts, js = domains.outputs_of(per, 10, [1, 2], 0, 1, 0.0, 500, 1.0)
    assert list(texts) == list(domains.suffixes_of([1, 2])) and "_insulation_w2.bedGraph" in texts
    lines = texts["_domains.txt"].splitlines()
    assert lines[0].split("\t") == list(domains.DOMAIN_HEAD)
    rows = [l.split("\t") for l in lines[1:]]
    assert [r[1] for r in rows] == sorted(r[1] for r in rows)                             # chrA before chrB
    assert [int(r[5]) for r in rows if r[1] == "chrA"] == sorted(int(r[5]) for r in rows if r[1] == "chrA")   # ascending w
    for r in rows:
        assert int(r[4]) == int(r[3]) - int(r[2]) and r[0].startswith("domain-%s-w%s-" % (r[1], r[5]))
        one = max(1, int(r[7]) + int(r[8]) - 2 * int(r[6]))
        assert r[9] == str(int(r[6]) / one) and r[10] == str(int(r[6]) / int(r[4])) and r[11] == str(int(float(r[9]) >= 1.0))
    assert texts["_domains.bed"].count("\n") == sum(r[11] == "1" for r in rows) == js["total"]["significant"]
    assert js["total"]["domains"] == len(rows) > 0 and js == json.loads(texts["_domains.json"])
    b = [l.split("\t") for l in texts["_boundaries.txt"].splitlines()]
    assert b[0] == list(domains.BOUNDARY_HEAD) and len(b) - 1 == js["total"]["boundaries"]
    for r in b[1:]:
        cov = int(r[3]) + int(r[4]) + int(r[5])
        assert r[6] == str(int(r[3]) / cov) and int(r[1]) % 10 == 0
    g = [l.split("\t") for l in texts["_insulation_w1.bedGraph"].splitlines()]
    assert all(int(r[2]) - int(r[1]) == 10 and int(r[1]) >= 0 and 0.0 <= float(r[3]) <= 1.0 for r in g)
    assert len(g) == sum(js["chroms"][c]["1"]["valid"] for c in js["chroms"])
    assert js["chroms"]["chrA"]["2"]["bins"] == per["chrA"][2]["n_bins"] and js["w"] == [1, 2] and js["res"] == 10


def test_check_args():
    ok = domains.check_args(10000, "20,10,10", 0, 20, 0.05, 500, 1.0)
    assert ok == (10000, [10, 20], 0, 20, 0.05, 500, 1.0)
    assert domains.check_args("5000", 7, -3, 1, 0, 1, 0)[:3] == (5000, [7], -3)
    for bad in ((0, 10), (1 << 29, 1), (10000, 0), (10000, 1025), (10000, ""), (10000, "a"), (1 << 20, 512), ("x", 10)):
        with pytest.raises(ValueError):
            domains.check_args(bad[0], bad[1], 0, 20, 0.05, 500, 1.0)
    for kw in ({"mincov": 0}, {"delta": -0.1}, {"delta": float("nan")}, {"maxbins": 0}, {"escut": -1}):
        args = dict(res=10000, w=10, cut=0, mincov=20, delta=0.05, maxbins=500, escut=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            domains.check_args(**args)
    with pytest.raises(ValueError):
        domains.jd2domains([], "nowhere", res=0)                         # refused before any file is looked at
    op = domains.help(["-d", "x", "-o", "y"])
    assert (op.res, op.w, op.cut, op.mincov, op.delta, op.maxbins, op.escut, op.chroms) == (10000, "10", 0, 20, 0.05, 500, 1.0, "")


def test_write_outputs_leaves_nothing_behind(tmp_path):
    texts, _ = domains.outputs_of(small_result(), 10, [1, 2], 0, 1, 0.0, 500, 1.0)
    out = os.path.join(str(tmp_path), "ok")
    domains.write_outputs(out, texts)
    assert sorted(os.listdir(str(tmp_path))) == sorted("ok" + s for s in texts)
    for s, t in texts.items():
        assert open(out + s).read() == t
    bad = dict(texts)
    bad["_domains.json"] = None                                          # the last file fails to write
    with pytest.raises(TypeError):
        domains.write_outputs(os.path.join(str(tmp_path), "bad"), bad)
    assert sorted(os.listdir(str(tmp_path))) == sorted("ok" + s for s in texts)
