"""GPU: the candidate stage of a sweep (K10: k_cand_count / k_step_classify_count, k_cand_append, k_cand_mark, k_cand_emit) against
tests/fake_backend.FakeChromosome (cand_append / cand_finish, i.e. pipe._combine_steps) fed the ORACLE's cluster table.  Exact
equality of counts and of the final rows as arrays, in order.

The inputs are the `classes` families of tests/table_cases.py (conditions: tests/test_table_cases.py): every class of pipe.py:83-97
-- inter, self with max_x == min_y and max_x > min_y, the two degenerate boxes -- interleaved over 2047, 2048, 2049 and 4097 ids
(CAND_BLOCK = 2048), boxes whose floor mid-points are exactly the final cut or one below it apart, negative coordinates for variant 1.
Both append paths run everywhere: cl_cand_append (host-called, scanned block offsets) and the step tail of cl_cluster_step_async
(k_step_classify_count, every block sums the counts in front of it).

Identical boxes inside ONE step ("all stay", as in _combine_steps) are not constructed: no construction was found.  Two clusters whose
chains of CORES reach all four sides of one box cross each other and merge, but a cluster may touch a side with a border PET, which
merges nothing; that case was not examined.  tests/test_pipe_host.py covers the rule of _combine_steps on arrays."""
import ctypes

import numpy as np
import pytest

import oracle
import table_cases as T
from fake_backend import FakeChromosome
from table_check import label_stats, table_from_labels
from cloops_amd import _lib, api

pytestmark = pytest.mark.gpu

PATHS = ("append", "step")
CUTS = (0, T.FINAL_CUT - 1, T.FINAL_CUT, T.FINAL_CUT + 1)
_ref = {}


def _cases():
    return [(n, v) for n in T.CLASS_NAMES for v in T.get(n).variants]


def _fake_sweep(name, variant, steps):
    """the stand-in after the steps, fed the oracle's tables -> (FakeChromosome, [(n_inter, n_self)] per step); once per module"""
    key = (name, variant, steps)
    if key not in _ref:
        c = T.get(name)
        fake = FakeChromosome(c.X, c.Y)
        fake.cand_reset()
        counts = []
        for k, (eps, m, cut) in enumerate(steps):
            lab = oracle.single_dbscan(variant, c.X, c.Y, eps, m, cut)["labels"]
            nc, ml = label_stats(lab)
            fake._last = (api.ClusterResult(lab, nc, ml, table_from_labels(c.X, c.Y, lab, ml + 1), None), cut)
            counts.append(fake.cand_append(k))
        _ref[key] = (fake, counts)
    return _ref[key]


def _gpu_step(ch, path, variant, eps, m, cut, step):
    """one step through one of the two append paths -> (n_inter, n_self)"""
    if path == "append":
        ch.cluster(variant, eps, m, cut)
        return ch.cand_append(step)
    ch.step_async(variant, eps, m, cut, step)
    ch.wait()
    return ch.step_result()[:2]


@pytest.mark.parametrize("name,variant", _cases())
def test_both_append_paths_one_step(name, variant):
    c = T.get(name)
    steps = ((c.eps, c.min_pts, 0),)
    fake, counts = _fake_sweep(name, variant, steps)
    cnt = c.info["counts"]
    assert counts[0] == (cnt["inter"] + cnt["mark_at"] + cnt["mark_below"], cnt["touch"] + cnt["overlap"])
    ch = api.Chromosome(c.X, c.Y)
    try:
        rows = {}
        for path in PATHS:
            ch.cand_reset()
            assert _gpu_step(ch, path, variant, *steps[0], 0) == counts[0], path
            for fc in CUTS:
                want = fake.cand_finish(fc, 0)
                got = ch.cand_finish(fc, len(c.X))
                assert got.dtype == np.int32 and np.array_equal(got, want), (path, fc, len(got), len(want))
                rows[path, fc] = got
        n_at = len(rows["step", T.FINAL_CUT]) - len(rows["step", T.FINAL_CUT + 1])
        n_below = len(rows["step", T.FINAL_CUT - 1]) - len(rows["step", T.FINAL_CUT])
        assert n_at >= cnt["mark_at"] and n_below >= cnt["mark_below"]
    finally:
        ch.close()


@pytest.mark.parametrize("path", PATHS + ("mixed",))
@pytest.mark.parametrize("name,variant", _cases())
def test_three_step_sweep_first_step_wins(name, variant, path):
    """the second step appends nothing, the third brings every box of the first back: each box once, in its first step, in append
    order"""
    c = T.get(name)
    fake, counts = _fake_sweep(name, variant, T.SWEEP_STEPS)
    assert counts[1] == (0, 0) and counts[2][0] > counts[0][0] > 0
    ch = api.Chromosome(c.X, c.Y)
    try:
        ch.cand_reset()
        for k, (eps, m, cut) in enumerate(T.SWEEP_STEPS):
            p = PATHS[k & 1] if path == "mixed" else path
            assert _gpu_step(ch, p, variant, eps, m, cut, k) == counts[k], (k, p)
        for fc in CUTS:
            want = fake.cand_finish(fc, 0)
            got = ch.cand_finish(fc, 2 * len(c.X))
            assert np.array_equal(got, want), (fc, len(got), len(want))
            assert len(np.unique(got, axis=0)) == len(got)
        assert len(ch.cand_finish(0, 2 * len(c.X))) == counts[2][0]      # (every box of step 0 is one of step 2)
        assert np.array_equal(ch.cand_finish(0, 2 * len(c.X))[: counts[0][0]], fake.cand_finish(0, 0)[: counts[0][0]])
    finally:
        ch.close()


@pytest.mark.parametrize("path", PATHS)
def test_capacity_repeat_reset_and_device_form(path):
    c = T.get("classes_2049")
    steps = ((c.eps, c.min_pts, 0),)
    fake, counts = _fake_sweep(c.name, "v2", steps)
    want = fake.cand_finish(T.FINAL_CUT, 0)
    k = len(want)
    assert 100 < k < counts[0][0]
    lib = _lib.load()
    ch = api.Chromosome(c.X, c.Y)
    try:
        ch.cand_reset()
        assert _gpu_step(ch, path, "v2", *steps[0], 0) == counts[0]
        buf = np.full((k, 4), -7, np.int32)
        nout = ctypes.c_int64(-1)
        rc = lib.cl_cand_finish(ch._h, T.FINAL_CUT, buf.ctypes.data_as(ctypes.c_void_p), k - 1, ctypes.byref(nout))
        assert rc == _lib.CL_ERR_ARG and nout.value == k                 # one row too small: refused, the count says what is needed
        assert (buf == -7).all()
        rc = lib.cl_cand_finish(ch._h, T.FINAL_CUT, buf.ctypes.data_as(ctypes.c_void_p), k, ctypes.byref(nout))
        assert rc == _lib.CL_OK and nout.value == k and np.array_equal(buf, want)
        a = ch.cand_finish(T.FINAL_CUT, k)
        b = ch.cand_finish(T.FINAL_CUT, k)
        assert np.array_equal(a, want) and np.array_equal(b, want)
        ptr, rows = ch.cand_finish_device(T.FINAL_CUT)
        assert rows == k and ptr != 0
        ch.cand_reset()
        assert len(ch.cand_finish(0, k)) == 0
        assert ch.cand_finish_device(0) == (0, 0)
    finally:
        ch.close()
