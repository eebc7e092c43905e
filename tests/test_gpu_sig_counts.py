"""GPU: kernel K8 (cl_sig_counts) on the cases of tests/sig_cases.py against `mask_counts`, whole tables and N compared exactly:
every case at three kinds of cut, the table cache and the buffers K8 shares with K11, K8 beside clustering runs and sweep steps,
the arguments of the C entry point, and cModel.getIntSig on the resident chromosome against the same call on the CPU stand-in."""
import ctypes

import numpy as np
import pytest

import sig_cases as S
from test_quant import brute_counts

pytestmark = pytest.mark.gpu

CASE_CUTS = [(name, k) for name in S.NAMES for k in range(3)]


def _chrom(c):
    from cloops_amd import api
    return api.Chromosome(c.X, c.Y)


def _check(ch, name, cut, rows=None):
    """sig_counts of the case's records (or of the records `rows`) at `cut` == the reference"""
    c = S.case(name)
    want, n = S.reference(name, cut)
    got, n2 = ch.sig_counts(c.windows if rows is None else c.windows[rows], cut)
    assert n2 == n
    assert got.dtype == np.int32 and np.array_equal(got, want if rows is None else want[rows])
    return got


def _check_quant(ch, c, wins, cut):
    got, n = ch.quant_counts(wins, cut)
    want, n2 = brute_counts(c.X, c.Y, wins, cut)
    assert n == n2
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name_k", CASE_CUTS, ids=lambda p: "%s-%s" % (p[0], ("cut0", "part", "none")[p[1]]))
def test_cases(name_k):
    name, k = name_k
    c = S.case(name)
    cut = S.cuts_of(c)[k]
    ch = _chrom(c)
    got = _check(ch, name, cut)
    if k == 2:
        assert not got.any() and ch.sig_counts(c.windows, cut)[1] == 0
    ch.close()


def test_extremes_cut_drops_reversed_rows():
    """with rows dropped by the cut the tables end in sentinels: the windows that reach INT32_MAX must stop at the valid rows"""
    c = S.case("extremes")
    assert c.cuts[0] == 1 and ((c.Y - c.X) < 1).sum() > 100 and (c.windows[:, 22:] == S.I32_MAX).sum() >= 5
    ch = _chrom(c)
    _check(ch, "extremes", 1)
    ch.close()


@pytest.mark.parametrize("name", ["hull_with_holes", "pile_up", "extremes"])
def test_same_bytes_twice(name):
    c = S.case(name)
    for cut in S.cuts_of(c)[:2]:
        ch = _chrom(c)
        first = _check(ch, name, cut)
        again = _check(ch, name, cut)
        ch.close()
        fresh = _chrom(c)
        other = _check(fresh, name, cut)
        fresh.close()
        assert first.tobytes() == again.tobytes() == other.tobytes()


@pytest.mark.parametrize("name,b", [("overlapping_sides", 2500), ("directed", 1500), ("duplicates", 2000)])
def test_table_cache(name, b):
    """the sorted tables are cached per cut and shared by K8 and K11: a, b, a, 0, b, then K8 / K11 alternating at different cuts"""
    c = S.case(name)
    a = c.cuts[0]
    kept = [int(((c.Y - c.X) >= cut).sum()) for cut in (a, b)]
    assert 0 < kept[1] < kept[0] < len(c.X)
    want = {cut: S.mask_counts(c.X, c.Y, c.windows, cut) for cut in (a, b, 0)}
    ch = _chrom(c)

    def k8(cut):
        got, n = ch.sig_counts(c.windows, cut)
        assert n == want[cut][1] and np.array_equal(got, want[cut][0])
    for cut in (a, b, a, 0, b):
        k8(cut)
    k8(a)
    _check_quant(ch, c, c.windows, b)
    k8(a)
    _check_quant(ch, c, c.windows, 0)
    _check_quant(ch, c, c.windows, a)
    k8(a)
    k8(0)
    ch.close()


def test_buffer_reuse():
    """3, 5000, then 2 records on one handle; K11 (123 ints per record) then K8 (144) with 5000 in the shared buffers"""
    c = S.case("many_records")
    ch = _chrom(c)
    for cut in (0, c.cuts[0]):
        _check(ch, "many_records", cut, slice(0, 3))
        _check(ch, "many_records", cut)
        _check(ch, "many_records", cut, slice(0, 2))
        _check_quant(ch, c, c.windows, cut)
        _check(ch, "many_records", cut)
        _check_quant(ch, c, c.windows[:7], cut)
        _check(ch, "many_records", cut, slice(0, 9))
    for cut in S.cuts_of(c):
        got, n = ch.sig_counts(np.zeros((0, 44), np.int32), cut)            # n_records == 0
        assert got.shape == (0, 144) and n == S.reference("many_records", cut)[1]
    ch.close()
    fresh = _chrom(c)                                                       # n_records == 0 as the first call of a handle
    got, n = fresh.sig_counts(np.zeros((0, 44), np.int32), c.cuts[0])
    assert got.shape == (0, 144) and n == S.reference("many_records", c.cuts[0])[1]
    _check(fresh, "many_records", c.cuts[0], slice(0, 2))
    fresh.close()


@pytest.mark.parametrize("name", ["many_records", "extremes", "stride_slices"])
def test_record_order(name):
    c = S.case(name)
    p = np.random.default_rng(77).permutation(len(c.windows))
    ch = _chrom(c)
    for cut in S.cuts_of(c)[:2]:
        _check(ch, name, cut, p)
        _check(ch, name, cut, p[::-1][:len(p) // 2 + 1])
    ch.close()


def test_between_sweep_steps():
    """K8 between two sweep steps leaves the steps' results unchanged and is right itself; with a run in flight it is refused"""
    from cloops_amd import _lib
    c = S.case("many_records")
    rows = slice(0, 400)

    def sweep(with_k8):
        ch = _chrom(c)
        ch.set_device_labels(False)
        ch.cand_reset()
        out = []
        for step, (eps, cut) in enumerate(((600, 0), (1200, c.cuts[0]))):
            ch.step_async("v2", eps, 5, cut, step)
            if with_k8 and step == 1:
                with pytest.raises(_lib.CloopsHipError):
                    ch.sig_counts(c.windows[rows])
            ch.wait()
            ni, ns, st = ch.step_result()
            out.append((ni, ns, st["n_all"], st["sumx"], st["loghist"].tolist()))
            if with_k8:
                _check(ch, "many_records", cut, rows)
                _check(ch, "many_records", c.cuts[0] - cut, rows)           # and at the cut the step did not run with
        out.append(ch.cand_finish(c.cuts[0], 100000).tolist())
        ch.close()
        return out
    with_k8, without = sweep(True), sweep(False)
    assert with_k8 == without
    assert without[0][0] > 0 and len(without[-1]) > 0                       # the steps found the blobs


def test_after_cluster_runs():
    """K8 after runs of every variant on the same handle; the runs' labels are those of a handle that never ran K8"""
    c = S.case("many_records")
    rows = slice(0, 400)
    runs = [lambda ch: ch.cluster("v2", 800, 5), lambda ch: ch.cluster("v1", 800, 5, c.cuts[0]), lambda ch: ch.cluster("block", 800, 5),
            lambda ch: ch.cluster_weighted(2000, 5, 3, 1)]
    ch, plain = _chrom(c), _chrom(c)
    _check(ch, "many_records", 0, rows)
    for k, run in enumerate(runs):
        got, want = run(ch), run(plain)
        assert got.n_clusters == want.n_clusters > 0 and np.array_equal(got.labels, want.labels)
        _check(ch, "many_records", (0, c.cuts[0])[k % 2], rows)
        _check(ch, "many_records", (c.cuts[0], 0)[k % 2], rows)
    ch.close()
    plain.close()


def test_entry_point_arguments():
    """cl_sig_counts called as a C caller would: a negative record count, null windows / out with records, an empty chromosome"""
    from cloops_amd import _lib, api
    c = S.case("tiny_2")
    lib = _lib.load()
    w = np.ascontiguousarray(c.windows, np.int32)
    out = np.full((len(w), 144), 7, np.int32)
    n = ctypes.c_int64(-5)
    wp, op = w.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    ch = api.Chromosome(c.X, c.Y)
    for args in ((-1, wp, op), (len(w), None, op), (len(w), wp, None), (len(w), None, None)):
        n.value = -5
        assert lib.cl_sig_counts(ch._h, 0, args[0], args[1], args[2], ctypes.byref(n)) == _lib.CL_ERR_ARG
        assert n.value == 0 and (out == 7).all()                            # refused before anything is written but N
    assert lib.cl_sig_counts(None, 0, len(w), wp, op, ctypes.byref(n)) == _lib.CL_ERR_ARG
    assert lib.cl_sig_counts(ch._h, 0, 0, None, None, ctypes.byref(n)) == _lib.CL_OK and n.value == 2      # no records: nothing to read
    assert lib.cl_sig_counts(ch._h, 0, len(w), wp, op, None) == _lib.CL_OK                                  # N is optional
    assert np.array_equal(out, S.reference("tiny_2", 0)[0])
    _check(ch, "tiny_2", 0)                                                 # the handle is as good as before
    ch.close()
    empty = api.Chromosome(np.zeros(0, np.int64), np.zeros(0, np.int64))
    for cut in (0, 15):
        out[:] = 7
        n.value = -5
        assert lib.cl_sig_counts(empty._h, cut, len(w), wp, op, ctypes.byref(n)) == _lib.CL_OK
        assert n.value == 0 and not out.any()
        assert lib.cl_sig_counts(empty._h, cut, 0, None, None, ctypes.byref(n)) == _lib.CL_OK and n.value == 0
        assert lib.cl_sig_counts(empty._h, cut, -1, wp, op, ctypes.byref(n)) == _lib.CL_ERR_ARG
    got, n0 = empty.sig_counts(c.windows)
    assert got.shape == (2, 144) and not got.any() and n0 == 0
    empty.close()


PRODUCTION = {"overlapping_sides": [(5000, 7000, 5000, 7000), (4000, 9000, 5000, 6000), (4000, 7000, 5500, 8500), (9000, 12000, 3000, 10000),
                                    (0, 40, 10, 300), (2, 10, 30, 60), (200, 800, 1500, 2500), (13000, 13400, 16000, 17500),
                                    (200, 5000, 9000, 14000), (14000, 14999, 14500, 19000)],
              "extremes": [(S.CMAX - 1000, S.CMAX, S.CMAX - 1, S.CMAX), (0, 0, 0, 1), (0, 7, S.CMAX - 1, S.CMAX), S.EXTREME_CLAMPED,
                           (0, 1000, 1000, S.CMAX), (5, 5, 7, 7), (0, S.CMAX, 0, S.CMAX), (1, 1, S.CMAX, S.CMAX)]}


@pytest.mark.parametrize("name", sorted(PRODUCTION))
def test_production_path(name, monkeypatch):
    """cModel.getIntSig on a chromosome registered with pipe.CACHE.put_arrays == the same call on the CPU stand-in, cell by cell"""
    import pandas as pd
    import fake_backend
    from cloops_amd import api, cModel, pipe
    c = S.case(name)
    ok = (c.X >= 0) & (c.Y >= 0)                                            # cModel._windows clamps at 0
    X, Y = c.X[ok], c.Y[ok]
    recs = [["chrT", a, b, "chrT", e, f] for a, b, e, f in PRODUCTION[name]]
    assert len(X) >= 40 and (Y < X).any()

    fed = []                                                                # the count tables getIntSig hands to the statistics
    stats = cModel.getIntSigFromCounts
    monkeypatch.setattr(cModel, "getIntSigFromCounts", lambda r, counts, N, m, d: (fed.append((counts.copy(), N)), stats(r, counts, N, m, d))[1])

    def run(discut):
        pipe.CACHE.clear()
        f = pipe.CACHE.put_arrays("chrT-chrT", X, Y)
        try:
            return cModel.getIntSig(f, recs, [1], discut)
        finally:
            pipe.CACHE.clear()
    got = [run(discut) for discut in (0, 1)]
    with monkeypatch.context() as mp:
        mp.setattr(api, "Chromosome", fake_backend.FakeChromosome)
        want = [run(discut) for discut in (0, 1)]
    assert len(fed) == 4
    for k in (0, 1):
        assert fed[k][1] == fed[2 + k][1] == (int(((Y - X) >= 1).sum()) if k else len(X))
        assert np.array_equal(fed[k][0], fed[2 + k][0])
        assert (fed[k][0][:, 22] > 0).sum() >= 4                            # records that reach the statistics
        # (the duplicate removal keeps the loops that overlap no other one -- and never the last record, as the reference)
        assert want[k] is not None and len(want[k]) >= 1
        pd.testing.assert_frame_equal(got[k], want[k], check_exact=True)
