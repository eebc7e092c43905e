"""CPU: the host side of the aggregate analysis (cloops_amd.agg): loop centres, loop selection, the window's origin, the scores with
their x / 0 and 0 / 0 cases, the reading of a `.loop` file and the command line's arguments.  No GPU, no built library."""
import math
import os

import numpy as np
import pytest

import golden_util as G
from cloops_amd import agg

LOOPS = os.path.join(G.GOLD, "chr21_v2.loop")


def test_loop_centres():
    rs = {"a": ["c", 100, 201, "c", 1000, 1003], "b": ["c", 0, 1, "c", 7, 7], "c": ["c", 10, 10, "c", 5, 20]}
    cx, cy = agg.loop_centres(rs)
    assert cx.dtype == np.int64 and cx.tolist() == [150, 0, 10] and cy.tolist() == [1001, 7, 12]
    cx2, cy2 = agg.loop_centres(list(rs.values()))                     # a list of records serves too
    assert cx2.tolist() == cx.tolist() and cy2.tolist() == cy.tolist()
    cx0, cy0 = agg.loop_centres({})
    assert len(cx0) == 0 and len(cy0) == 0


def test_select_loops():
    cx = np.array([0, 0, 0, 100, 500000])
    cy = np.array([21999, 22000, 22001, 90, 400000])
    keep, skipped = agg.select_loops(cx, cy, 1000, 10)                 # default (2 w + 2) res = 22000
    assert agg.default_min_dist(1000, 10) == 22000
    assert keep.tolist() == [False, True, True, False, False] and skipped == 3
    keep, skipped = agg.select_loops(cx, cy, 1000, 10, min_dist=0)
    assert keep.tolist() == [True, True, True, False, False] and skipped == 2
    keep, skipped = agg.select_loops(cx, cy, 1000, 10, min_dist=-10 ** 9)
    assert keep.all() and skipped == 0
    keep, skipped = agg.select_loops(cx, cy, 7, 1, min_dist=None)      # 4 * 7 = 28
    assert keep.tolist() == [True, True, True, False, False] and skipped == 2
    keep, skipped = agg.select_loops([], [], 1000, 10)
    assert len(keep) == 0 and skipped == 0


def test_default_min_dist_keeps_the_window_above_the_diagonal():
    """at cy - cx = (2 w + 2) res the cell nearest the diagonal (last X bin, first Y bin) still has Y > X throughout"""
    for res, w in ((1, 1), (7, 5), (1000, 10), (5000, 20), (2, 3)):
        cx = 12345
        cy = cx + agg.default_min_dist(res, w)
        ox, oy = agg.window_origin(cx, res, w), agg.window_origin(cy, res, w)
        W = 2 * w + 1
        assert oy > ox + W * res - 1                                   # the smallest Y of the window beyond its largest X


def test_window_origin_odd_even_and_one():
    # the centre bin [c - res // 2, c - res // 2 + res) holds c; bins are res wide; Python's floor division on res >= 1 only
    for res in (1, 2, 3, 7, 1000, 1001):
        for w in (1, 5, 20):
            for c in (-5, 0, 3, 1000003):
                o = agg.window_origin(c, res, w)
                assert o == c - w * res - res // 2
                assert (c - o) // res == w                             # the centre falls into bin w
                assert (c - res // 2 - o) // res == w and (c - res // 2 - 1 - o) // res == w - 1
                assert (c - res // 2 + res - 1 - o) // res == w and (c - res // 2 + res - o) // res == w + 1
    assert agg.window_origin(10, 1, 1) == 9                            # res = 1: the window is [c - w, c + w]
    assert agg.window_origin(10, 2, 1) == 7 and agg.window_origin(10, 3, 1) == 6


def test_scores_by_hand():
    S = np.zeros((5, 5), np.int64)
    S[2, 2] = 12
    S[3:, :2] = [[1, 2], [3, 2]]                                       # ll: sum 8, mean 2, std sqrt(0.5)
    S[:2, :2] = [[1, 1], [1, 1]]                                       # ul: sum 4
    S[:2, 3:] = [[0, 0], [0, 0]]                                       # ur: zero corner
    S[3:, 3:] = [[6, 6], [6, 6]]                                       # lr: sum 24
    sc = agg.scores(S, 2)
    assert sc["APA"] == 12 / (8 / 4.0) and sc["P2UL"] == 12 / (4 / 4.0) and sc["P2LR"] == 12 / (24 / 4.0)
    assert sc["P2UR"] == math.inf
    assert sc["ZscoreLL"] == (12 - 2.0) / math.sqrt(0.5)
    assert set(sc) == {"APA", "P2UL", "P2UR", "P2LR", "ZscoreLL"}
    sc1 = agg.scores(S, 1)                                             # corner 1: single cells; std of one cell is 0 -> inf
    assert sc1["APA"] == 12 / 3.0 and sc1["P2UL"] == 12.0 and sc1["P2UR"] == math.inf and sc1["P2LR"] == 2.0
    assert sc1["ZscoreLL"] == math.inf


def test_scores_all_zero_is_nan():
    sc = agg.scores(np.zeros((21, 21), np.int64), 3)
    assert all(math.isnan(v) for v in sc.values())
    S = np.zeros((3, 3), np.int64)
    S[2, 0] = 4                                                        # centre 0 over a non-zero corner: 0, and a negative z
    sc = agg.scores(S, 1)
    assert sc["APA"] == 0.0 and math.isnan(sc["P2UL"]) and sc["ZscoreLL"] == -math.inf


def test_p2ll_per_loop():
    st = np.array([[10, 4, 8, 0, 0, 0], [5, 3, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]], np.int32)
    r = agg.p2ll(st, 2)
    assert r[0] == 4 / (8 / 4.0) and r[1] == math.inf and math.isnan(r[2])


def test_corner_blocks_match_the_definitions():
    M = np.arange(49).reshape(7, 7)
    ll, ul, ur, lr = agg.corner_blocks(M, 2)
    assert np.array_equal(ll, M[5:, :2]) and np.array_equal(ul, M[:2, :2]) and np.array_equal(ur, M[:2, 5:]) and np.array_equal(lr, M[5:, 5:])


def test_read_chr21_loops_and_the_s_flag():
    n_file, n_taken, n_trans, loops = agg.read_loops(LOOPS)            # the default: significant loops only
    assert (n_file, n_taken, n_trans) == (343, 202, 0) and list(loops) == ["chr21"] and len(loops["chr21"]) == 202
    n_file, n_taken, n_trans, every = agg.read_loops(LOOPS, sig=False)
    assert (n_file, n_taken, n_trans) == (343, 343, 0) and len(every["chr21"]) == 343
    assert set(loops["chr21"]) < set(every["chr21"])
    first = every["chr21"]["chr21-chr21-40"]
    assert first == ["chr21", 44800894, 44801696, "chr21", 44911732, 44912078]
    cx, cy = agg.loop_centres({"k": first})
    assert (int(cx[0]), int(cy[0])) == (44801295, 44911905)
    assert agg.read_loops(LOOPS, chroms={"chr1"})[1:] == (0, 0, {})
    assert agg.read_loops(LOOPS, chroms={"chr21"})[1] == 202
    # selection at the default distance: the counts the GPU test pins
    for sig, res, w, used in ((False, 1000, 10, 312), (True, 1000, 10, 193), (False, 5000, 5, 270)):
        cx, cy = agg.loop_centres(agg.read_loops(LOOPS, sig=sig)[3]["chr21"])
        keep, skipped = agg.select_loops(cx, cy, res, w)
        assert int(keep.sum()) == used and skipped == len(cx) - used


def test_trans_loops_are_counted_and_left_out(tmp_path):
    f = os.path.join(str(tmp_path), "t.loop")
    with open(f, "w") as fh:
        fh.write("loopId\tiva\tivb\tsignificant\n")
        fh.write("a\tchr1:10-20\tchr1:100-200\t1.0\n")
        fh.write("b\tchr1:10-20\tchr2:100-200\t1.0\n")
        fh.write("c\tchr2:10-20\tchr2:300-400\t0.0\n")
    assert agg.read_loops(f) == (3, 2, 1, {"chr1": {"a": ["chr1", 10, 20, "chr1", 100, 200]}})
    assert agg.read_loops(f, sig=False)[:3] == (3, 3, 1)


def test_cli_arguments():
    op = agg.help(["-d", "D", "-f", "F", "-o", "O"])
    assert (op.d, op.f, op.output, op.res, op.w, op.corner, op.cut, op.minDist, op.significant, op.chroms, op.plot) == \
        ("D", "F", "O", 1000, 10, 3, 0, None, True, "", False)
    op = agg.help(["-d", "D", "-f", "F", "-o", "O", "-res", "5000", "-w", "5", "-corner", "2", "-cut", "4601", "-minDist", "0", "-s",
                   "-c", "chr1,chr2", "-plot"])
    assert (op.res, op.w, op.corner, op.cut, op.minDist, op.significant, op.chroms, op.plot) == (5000, 5, 2, 4601, 0, False, "chr1,chr2", True)
    with pytest.raises(SystemExit):
        agg.help(["-d", "D", "-f", "F"])                               # -o is required


def test_main_command_has_the_agg_flag():
    import inspect
    from cloops_amd import pipe
    sig = inspect.signature(pipe.pipe)
    assert sig.parameters["agg"].default == 0 and sig.parameters["agg_res"].default == 0
