"""GPU: k_union_c (cloops_amd/csrc/k_lists.hip) searches from undominated cores only -- labels, number of clusters and every row of the
cluster table against the sequential oracle (bit-exact), both variants at traversal level 4, on inputs built around the test's edges:
ties in sp, a linking core at a chain's end, dominators beyond the test's reach, the 512-core tile boundary on either side, strip 0,
the overflow list, q gaps of eps and eps + 1, a tile of more strips than the kernel stages rows of the strip table for.

The constructed sets use the builders of tests/lists_cases.py (rotated coordinates, eps 1000, minPts 3; P0 = strip 0, lines of cores
400 apart in q).  tests/test_union_filter_model.py proves the rule itself on the CPU; `_cores` below restates the core array of a
run so that every case can assert the structure it claims before it is run."""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G
import lists_cases as LC
import oracle
from cloops_amd import api
from table_check import check_table

pytestmark = pytest.mark.gpu

ROT = ("v2", "v1")
EPS, P0, Q0, STEP = LC.EPS, LC.P0, LC.Q0, LC.LADDER_STEP
UNT, HALO = 512, 512             # cores per tile of k_union_c and its halo for these sets (n > 80 S)
K = 4                            # the neighbours on either side the kernel's test looks at
M = LC.LADDER_MIN_PTS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cores(X, Y, m, kinds=None):
    """the core array of the run (eps, m, no cut), variant 2: -> (q, p, strip, kind) in the array's order"""
    p, q = X + Y, Y - X
    core = oracle.neighbor_counts(X, Y, EPS) >= m
    p, q = p[core], q[core]
    kd = (kinds[core] if kinds is not None else np.zeros(len(p), np.int16))
    strip = p // EPS
    o = np.lexsort((p, q, strip))
    return q[o], p[o], strip[o] - P0 // EPS, kd[o]


def _survives(q, p, strip, i, k=K):
    """the kernel's test for core i: the k neighbours on either side that its tile has staged"""
    t0 = (i // UNT) * UNT
    lo, hi = max(t0 - HALO, 0), min(t0 + UNT, len(q))
    left = any(j >= lo and strip[j] == strip[i] and q[i] - q[j] <= EPS and p[j] <= p[i] for j in range(i - k, i))
    right = any(j < hi and strip[j] == strip[i] and q[j] - q[i] <= EPS and p[j] < p[i] for j in range(i + 1, i + k + 1))
    return not (left and right)


def _check_runs(X, Y, eps, runs, tag, variants=ROT):
    ch = api.Chromosome(X, Y)
    try:
        ch.set_traversal(4)
        for variant in variants:
            for m, cut in runs:
                want = oracle.single_dbscan(variant, X, Y, eps, m, cut)["labels"]
                for rep in range(2):                     # (the same answer both times: nothing may depend on the order of atomics)
                    got = ch.cluster(variant, eps, m, cut)
                    assert np.array_equal(got.labels, want), (tag, variant, m, cut, rep, int((got.labels != want).sum()))
                    check_table(X, Y, want, got, (tag, variant, m, cut, rep))
    finally:
        ch.close()


def _zig(i, lo=500, hi=600):
    """p offsets of a line whose odd cores lie higher: every odd core has a lower core on either side"""
    return np.where(np.asarray(i) % 2 == 1, hi, lo)


def _finish(st, name):
    c = LC._case(name, "union_filter", st, [(M, 0)], {})
    assert len(c.X) > 80 * 8                             # (the 512-core halo)
    return c


def test_equal_sp_everywhere():
    """every core of a strip at one p: all keys tie on sp and go by the index, so no core has a dominator behind it and every one
    searches.  The long line of strip 3 is linked with the short lines below and above its middle only through cores of its middle"""
    st = LC._Set(9001)
    st.pad_cores(900)
    i = np.arange(60)
    st.add(P0 + 3 * EPS + 500, Q0 + STEP * i, LC.K_LINE, 3)
    st.add(P0 + 2 * EPS + 500, Q0 + STEP * (28 + np.arange(5)), LC.K_LINE, 2)
    st.add(P0 + 4 * EPS + 500, Q0 + STEP * (28 + np.arange(5)), LC.K_LINE, 4)
    c = _finish(st, "uf-equal-sp")
    q, p, strip, _ = _cores(c.X, c.Y, M)
    line = np.flatnonzero(strip == 3)
    assert len(line) == 60 and all(_survives(q, p, strip, int(a)) for a in line)
    _check_runs(c.X, c.Y, EPS, c.runs, c.name)


def _end_link(dense):
    """strip 3: a chain whose LAST core a is its highest; strip 2: a chain whose first core b lies exactly eps behind a in q and
    exactly eps below it in p -- a is the only core that reaches b, and nothing lies behind a.  dense: the chain's cores are 100
    apart and the eight in front of a lie higher still: a's only dominators in front are beyond the test's reach as well"""
    st = LC._Set(9002 + dense)
    st.pad_cores(900)
    n, step = (30, 100) if dense else (20, STEP)
    i = np.arange(n)
    off = np.where(i == n - 1, 400, np.where(dense & (i >= n - 9), 410, 300 + (0 if dense else 1) * 2 * i))
    st.add(P0 + 3 * EPS + off, Q0 + step * i, LC.K_LINE, 3)
    qa, pa = Q0 + step * (n - 1), P0 + 3 * EPS + 400
    st.add(pa - EPS, qa + EPS + STEP * np.arange(5), LC.K_LINE, 2)
    c = _finish(st, "uf-end-link-%d" % dense)
    q, p, strip, _ = _cores(c.X, c.Y, M)
    a = int(np.flatnonzero((strip == 3) & (q == qa))[0])
    reach = np.flatnonzero((strip == 2) & (np.abs(q - qa) <= EPS) & (p >= pa - EPS))
    assert len(reach) == 1 and q[reach[0]] == qa + EPS
    others = [int(x) for x in np.flatnonzero(strip == 3) if x != a]
    assert not any(((strip == 2) & (np.abs(q - q[x]) <= EPS) & (p >= p[x] - EPS)).any() for x in others)
    assert _survives(q, p, strip, a) and _survives(q, p, strip, a, 16)
    return c, (q, p, strip, a)


def test_link_from_the_highest_core_at_a_chains_end():
    c, _ = _end_link(0)
    want = oracle.single_dbscan("v2", c.X, c.Y, EPS, M, 0)["labels"]
    line = np.flatnonzero(c.grp == 3)
    assert len(np.unique(want[np.isin(c.grp, (2, 3)) & (c.kind == LC.K_LINE)])) == 1 and want[line[0]] >= 0
    _check_runs(c.X, c.Y, EPS, c.runs, c.name)


def test_dominators_beyond_the_tests_reach():
    c, (q, p, strip, a) = _end_link(1)
    near = [j for j in range(a - 8, a)]
    assert all(p[j] > p[a] for j in near) and p[a - 9] < p[a] and q[a] - q[a - 9] <= EPS
    _check_runs(c.X, c.Y, EPS, c.runs, c.name)


@pytest.mark.parametrize("d", [-1, 0])
def test_chain_across_the_tile_boundary(d):
    """a zigzag chain of strip 3 across core rank 1024 = the start of a tile, a high core h of it at rank 1024 + d.  d = -1: h is
    the last core of its tile, the lower core behind it is not staged: h searches.  d = 0: h is the first core of its tile, the lower
    core in front of it lies in the halo: h stays out.  The short chain below lies under h"""
    st = LC._Set(9010 + d)
    ih, nlow = 21, 5
    st.pad_cores(2 * UNT + d - nlow - ih)
    i = np.arange(41)
    st.add(P0 + 3 * EPS + _zig(i), Q0 + STEP * i, LC.K_LINE, 3)
    st.add(P0 + 2 * EPS + 600, Q0 + STEP * (ih - 2 + np.arange(nlow)), LC.K_LINE, 2)
    c = _finish(st, "uf-tile%+d" % d)
    q, p, strip, _ = _cores(c.X, c.Y, M)
    h = 2 * UNT + d
    assert strip[h] == 3 and q[h] == Q0 + STEP * ih and p[h] == P0 + 3 * EPS + 600
    assert _survives(q, p, strip, h) == (d == -1)
    assert not _survives(q, p, strip, h + 2) and not _survives(q, p, strip, h - 2)      # high cores inside a tile stay out
    _check_runs(c.X, c.Y, EPS, c.runs, c.name)


def test_strip_zero():
    """a zigzag chain in strip 0, which has nothing below it, and a line in strip 1 that reaches its high cores only"""
    st = LC._Set(9020)
    st.pad_cores(900)
    i = np.arange(41)
    st.add(P0 + _zig(i), Q0 + STEP * i, LC.K_LINE, 0)
    st.add(P0 + EPS + 600, Q0 + STEP * i, LC.K_LINE, 1)
    c = _finish(st, "uf-strip0")
    q, p, strip, _ = _cores(c.X, c.Y, M)
    assert (strip[(q >= Q0) & (q <= Q0 + STEP * 40)] <= 1).all() and (strip == 0).sum() >= 41
    _check_runs(c.X, c.Y, EPS, c.runs, c.name)


def test_overflow_list():
    """a zigzag strip of 1200 cores over a strip of 1200: the strip below begins in front of what the upper strip's tiles stage --
    their cores go to the overflow list, the dominated ones among them do not"""
    st = LC._Set(9030)
    i = np.arange(1200)
    st.add(P0 + 2 * EPS + 600, Q0 + STEP * i, LC.K_LINE, 2)
    st.add(P0 + 3 * EPS + _zig(i), Q0 + STEP * i, LC.K_LINE, 3)
    c = _finish(st, "uf-overflow")
    q, p, strip, _ = _cores(c.X, c.Y, M)
    up = np.flatnonzero(strip == 3)
    assert len(up) == 1200 and (strip == 2).sum() == 1200
    first_low = int(np.flatnonzero(strip == 2)[0])
    listed = [int(a) for a in up if (a // UNT) * UNT - HALO > first_low]
    assert len(listed) >= 600 and 0 < sum(_survives(q, p, strip, a) for a in listed) < len(listed)
    _check_runs(c.X, c.Y, EPS, c.runs, c.name)


@pytest.mark.parametrize("gap", [EPS, EPS + 1])
def test_q_gap_between_chain_mates(gap):
    """three triple points L, M, R of strip 3, `gap` apart in q, M the highest; below M a cluster exactly eps lower.  gap = eps: L
    and R are M's chain mates and dominate it (they reach the cluster too); gap = eps + 1: three chains, M has to search"""
    st = LC._Set(9040 + gap)
    st.pad_cores(900)
    hi = 600 + gap % 2                                   # (p and q of a PET are both even or both odd)
    for k, off in enumerate((500, hi, 500)):
        st.add(np.full(3, P0 + 3 * EPS + off), Q0 + gap * k, LC.K_LINE, 3)
    st.add(np.full(3, P0 + 2 * EPS + hi), Q0 + gap, LC.K_LINE, 2)
    c = _finish(st, "uf-gap%d" % gap)
    q, p, strip, _ = _cores(c.X, c.Y, M)
    mid = np.flatnonzero((strip == 3) & (q == Q0 + gap))
    assert len(mid) == 3 and [_survives(q, p, strip, int(a)) for a in mid] == [gap > EPS] * 3
    _check_runs(c.X, c.Y, EPS, c.runs, c.name)


def test_a_tile_of_more_strips_than_staged_rows():
    """100 adjacent strips of four cores each, linked from strip to strip: a tile spans more strips than the 64 whose rows of the
    strip table it stages, the cores of the others load theirs"""
    st = LC._Set(9050)
    for s in range(2, 102):
        st.add(P0 + s * EPS + 500, Q0 + 2 * np.arange(4), LC.K_LINE, s)
    c = LC._case("uf-many-strips", "union_filter", st, [(M, 0)], {})
    q, p, strip, _ = _cores(c.X, c.Y, M)
    assert len(q) == 400 and len(np.unique(strip)) == 100
    want = oracle.single_dbscan("v2", c.X, c.Y, EPS, M, 0)["labels"]
    assert len(np.unique(want[want >= 0])) == 1
    _check_runs(c.X, c.Y, EPS, c.runs, c.name)


DENSE_N, DENSE_LEN, DENSE_SEED = 200000, 3000000, 77
_dense = {}


def _dense_xy():
    if not _dense:
        from cloops_amd.synth import synth_chrom
        X, Y = synth_chrom(DENSE_N, DENSE_LEN, DENSE_SEED)
        _dense["xy"] = (X.astype(np.int64), Y.astype(np.int64))
    return _dense["xy"]


@pytest.mark.parametrize("variant", ROT)
def test_random_dense(variant):
    """200 k PETs at the density of the bench genome, eps 5000, minPts 20 and 50, without and with a cut"""
    X, Y = _dense_xy()
    _check_runs(X, Y, 5000, [(50, 0), (20, 0), (50, 5000), (20, 5000)], "dense", (variant,))


@pytest.mark.parametrize("variant", ROT)
def test_chr21_golden(variant):
    X, Y = G.chr21_xy()
    ch = api.Chromosome(X, Y)
    try:
        ch.set_traversal(4)
        for eps, m in ((500, 5), (1000, 5), (2000, 5), (5000, 20)):
            gold = G.chr21_labels(variant, eps, m)
            got = ch.cluster(variant, eps, m, 0)
            assert np.array_equal(got.labels, gold), (variant, eps, m, int((got.labels != gold).sum()))
            check_table(X, Y, gold, got, ("chr21", variant, eps, m))
    finally:
        ch.close()


_COUNTER_SCRIPT = """
import ctypes, os, sys
import numpy as np
from cloops_amd import api, _lib
from cloops_amd.synth import synth_chrom
X, Y = synth_chrom(%d, %d, %d)
ch = api.Chromosome(X, Y)
lib = _lib.load()
out = (ctypes.c_uint64 * 32)()
lib.cl_debug_lstats(out)
ref = None
for dbg2 in (1 << 30, (1 << 30) | (1 << 14)):
    os.environ["CLOOPS_DBG2"] = str(dbg2)
    res = ch.cluster("v2", 5000, 20, 0)
    lib.cl_debug_lstats(out)
    print("COUNT", dbg2, int(out[12]), int(out[23]), res.n_clusters, int(np.asarray(res.labels, np.int64).sum()))
""" % (DENSE_N, DENSE_LEN, DENSE_SEED)


def test_cores_that_searched_counter():
    """devel library only: fewer cores search than there are on the dense set; with ablation bit 14 every core searches, and the
    labels are the same either way"""
    from cloops_amd import _lib
    if not os.path.exists(_lib.SO_PATH.replace(".so", "_devel.so")):
        pytest.skip("no developer library (python -m cloops_amd.build --devel)")
    env = dict(os.environ, CLOOPS_DEVEL_LIB="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _COUNTER_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [[int(v) for v in l.split()[1:]] for l in r.stdout.splitlines() if l.startswith("COUNT")]
    assert len(rows) == 2
    (_, cores, searched, ncl, lsum), (_, cores2, searched2, ncl2, lsum2) = rows
    assert cores == cores2 > 0 and 0 < searched < cores and searched2 == cores2, rows
    assert (ncl, lsum) == (ncl2, lsum2), rows
