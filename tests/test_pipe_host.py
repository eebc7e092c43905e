"""CPU: host logic of cloops_amd.pipe (dispatch, record classification, report lines, sweep
chain, combine/filter) against the reference-made golden vectors, with the GPU replaced by
the oracle-backed FakeChromosome (tests/fake_backend.py)."""
import numpy as np
import pytest

import fake_backend
import pipe_checks
import golden_util as G
from cloops_amd import api, pipe


@pytest.fixture()
def cpu_pipe(monkeypatch, tmp_path):
    monkeypatch.setattr(api, "Chromosome", fake_backend.FakeChromosome)
    monkeypatch.setattr(api, "device_count", lambda: 1)
    pipe.CACHE.clear()
    f = pipe_checks.write_chr21_jd(tmp_path)
    yield pipe, f
    pipe.CACHE.clear()


def test_run_dbscan_matches_reference_outputs(cpu_pipe):
    p, f = cpu_pipe
    pipe_checks.check_run_dbscan_chain(p, f)


def test_sweep_chain_combine_filter(cpu_pipe):
    p, f = cpu_pipe
    pipe_checks.check_sweep(p, f)


def test_single_dbscan_all_filtered(cpu_pipe):
    p, f = cpu_pipe
    key, ff, dataI, dataS, dis, dss = p.singleDBSCAN(f, 500, 5, cut=10 ** 9)     # pipe.py:64-65
    assert key == ("chr21", "chr21") and dataI == [] and dataS == [] and dis == []
    assert len(dss) == 99674


def test_filter_uses_floor_division():
    data = {("c", "c"): {"f": "x", "records": [["c", 0, 3, "c", 10, 13], ["c", 0, 3, "c", 10, 12]]}}
    out = pipe.filterClusterByDis(data, 10)          # (10+13)//2 - (0+3)//2 = 10 ; (10+12)//2 - 1 = 10
    assert len(out[("c", "c")]["records"]) == 2
    out = pipe.filterClusterByDis(data, 11)
    assert len(out[("c", "c")]["records"]) == 0


def test_ests_matches_reference_function():
    """estIntSelCutFrag == what the reference's own (cLoops/ests.py:36-61) returned on the same 20 draws
    (tests/golden/reference_checks.npz)"""
    from cloops_amd.ests import estIntSelCutFrag
    z = G.reference_checks()
    draws = G.ests_draws()
    assert G.digest(np.concatenate([np.concatenate([di, ds]) for di, ds in draws])) == str(z["ests_in_sha1"]), "draws drifted"
    for (di, ds), want in zip(draws, z["ests_out"]):
        assert estIntSelCutFrag(di, ds) == tuple(int(v) for v in want)


def test_combine_steps_equals_sequential_combine_twice():
    """the array form used by runSweepFast == repeated combineTwice (pipe.py:155-174), order included"""
    rng = np.random.default_rng(4)
    pool = rng.integers(0, 50, (60, 4)).astype(np.int64)
    steps = []
    for k in range(6):
        idx = rng.integers(0, len(pool), int(rng.integers(0, 30)))
        b = pool[idx]
        if k == 2 and len(b) > 3:
            b = np.concatenate([b, b[:2]])               # duplicates inside one step are all kept
        steps.append(b)
    dataI = {}
    for b in steps:
        if len(b) == 0:
            continue
        d2 = {("c", "c"): {"f": "x", "records": [["c", int(r[0]), int(r[1]), "c", int(r[2]), int(r[3])] for r in b]}}
        dataI = pipe.combineTwice(dataI, d2)
    want = np.asarray([[r[1], r[2], r[4], r[5]] for r in dataI[("c", "c")]["records"]], dtype=np.int64)
    assert np.array_equal(pipe._combine_steps(steps), want)
    # truncated hashes: different boxes share a sort key, the exact repair of those runs must kick in
    for bits in (1, 2, 3, 5):
        assert np.array_equal(pipe._combine_steps(steps, _hash_bits=bits), want)


def test_sweep_fast_host_logic(cpu_pipe):
    """runSweepFast (statistics instead of lists) against the reference-made chain, CPU backend"""
    p, f = cpu_pipe
    pipe_checks.check_sweep_fast(p, f)


def test_filter_candidate_stripes_semantics():
    """scripts/callStripes:75-86: keep records with >= pets PETs whose side lengths differ by more than
    lengthFoldDiff (py2 integer division)"""
    from cloops_amd import stripes
    rs = {("c", "c"): [["c", 0, 1000, "c", 0, 10, 300],       # 100x longer in X: kept
                       ["c", 0, 10, "c", 0, 1000, 300],       # 100x longer in Y: kept
                       ["c", 0, 100, "c", 0, 100, 300],       # square: dropped
                       ["c", 0, 1000, "c", 0, 10, 100],       # too few PETs: dropped
                       ["c", 0, 209, "c", 0, 10, 300]]}       # 209 // 10 = 20, not > 20: dropped
    out = stripes.filterCandidateStripes(rs, pets=200, lengthFoldDiff=20)
    assert out[("c", "c")] == [["c", 0, 1000, "c", 0, 10, 300], ["c", 0, 10, "c", 0, 1000, 300]]


# ---- resident-chromosome cache: a sweep keeps every handle it uses alive ---------------------------
class _ClosableFake(fake_backend.FakeChromosome):
    """like the real handle: close() destroys it, any later call fails"""
    closed_calls = 0

    def close(self):
        self.dead = True

    def cluster_async(self, *a, **kw):
        if getattr(self, "dead", False):
            type(self).closed_calls += 1
            raise RuntimeError("null chromosome handle")
        return fake_backend.FakeChromosome.cluster_async(self, *a, **kw)


def _write_many_jd(tmp_path, n_files, n=400):
    import joblib
    from cloops_amd.synth import synth_chrom
    fs = []
    for k in range(n_files):
        X, Y = synth_chrom(n, 200000, 900 + k)
        f = str(tmp_path / ("c%d-c%d.jd" % (k, k)))
        joblib.dump(np.stack([np.arange(n), X, Y], 1).astype(np.int64), f)
        fs.append(f)
    return fs


def test_sweep_over_more_chromosomes_than_the_cache_keeps(monkeypatch, tmp_path):
    """70 per-chromosome files > max_items = 64 (a scaffold-level assembly): no resident that the sweep
    uses may be evicted / closed while the sweep runs; afterwards the cache shrinks back"""
    monkeypatch.setattr(api, "Chromosome", _ClosableFake)
    monkeypatch.setattr(api, "device_count", lambda: 1)
    pipe.CACHE.clear()
    fs = _write_many_jd(tmp_path, 70)
    _ClosableFake.closed_calls = 0
    dataI, cut, cuts, steps = pipe.runSweepFast(fs, [800], [4, 3], cut=0)
    assert _ClosableFake.closed_calls == 0
    assert len(steps) == 2 and steps[0]["n_in"] == 70 * 400
    assert len(pipe.CACHE._items) <= pipe.CACHE.max_items
    assert all(r.pins == 0 for r in pipe.CACHE._items.values())
    pipe.CACHE.clear()


def test_failed_enqueue_releases_every_lock(monkeypatch, tmp_path):
    """cluster_async raising for chromosome k must not leave chromosomes 0..k-1 locked / in flight"""
    class Failing(fake_backend.FakeChromosome):
        def cluster_async(self, variant, eps, minPts, cut=0, want_labels=True, want_boxes=True):
            if self.n == 403:
                raise RuntimeError("boom")
            return fake_backend.FakeChromosome.cluster_async(self, variant, eps, minPts, cut, want_labels, want_boxes)
    monkeypatch.setattr(api, "Chromosome", Failing)
    monkeypatch.setattr(api, "device_count", lambda: 1)
    pipe.CACHE.clear()
    from cloops_amd.synth import synth_chrom
    fs = [pipe.CACHE.put_arrays("k%d-k%d" % (k, k), *synth_chrom(400 + k, 200000, 70 + k)) for k in range(5)]
    with pytest.raises(RuntimeError):
        pipe.runSweepFast(fs, [800], [4], cut=0)
    for f in fs:
        r = pipe.CACHE.get(f)
        assert not r.lock.locked() and r.pins == 0
        assert not getattr(r.chrom, "_pending", [])
    pipe.CACHE.clear()


def test_cache_get_without_device_preference_keeps_the_resident(monkeypatch, tmp_path):
    """the significance stage asks for a chromosome without a device preference: the resident copy on
    another GPU is reused, not reloaded onto GPU 0"""
    monkeypatch.setattr(api, "Chromosome", fake_backend.FakeChromosome)
    monkeypatch.setattr(api, "device_count", lambda: 2)
    pipe.CACHE.clear()
    f = _write_many_jd(tmp_path, 1)[0]
    r1 = pipe.CACHE.get(f, 1)
    assert r1.device == 1 and pipe.CACHE.get(f) is r1 and pipe.CACHE.get(f, None) is r1
    assert pipe.CACHE.get(f, 0) is not r1
    pipe.CACHE.clear()


def test_cut_on_an_integer_boundary_is_settled_from_the_lists(cpu_pipe, monkeypatch):
    """rcut = int(2 ** cut) truncates: when the statistics-based 2**cut lands within rounding noise of an integer
    the step is re-derived from the distance lists like the reference does -- forced here by a huge margin;
    the chain must not change and the steps say so"""
    p, f = cpu_pipe
    z, meta = pipe_checks.pipe_golden()
    monkeypatch.setattr(p, "CUT_RECHECK_MARGIN", 10.0)
    dataI, cut, cuts, steps = p.runSweepFast([f], [500, 1000, 2000], [5], cut=0)
    assert all(s.get("cut_rechecked") for s in steps)
    assert [s.get("cut_out") for s in steps] == [s.get("cut_out") for s in meta["v2"]["steps"]]
    assert [s.get("frags") for s in steps] == [s.get("frags") for s in meta["v2"]["steps"]]
    assert np.array_equal(dataI[("chr21", "chr21")]["boxes"], z["v2_filtered"])


def test_sweep_fast_key_order_is_first_appearance(monkeypatch):
    """combineTwice (cLoops/pipe.py:155-174) inserts a chromosome's key when it FIRST yields an inter-ligation box;
    runStat walks the dict, so the key order fixes the row order of the .loop file.  A chromosome that comes first in
    file order but gets its first box only in the second step must come second -- in runSweep and runSweepFast alike."""
    monkeypatch.setattr(api, "Chromosome", fake_backend.FakeChromosome)
    monkeypatch.setattr(api, "device_count", lambda: 1)
    pipe.CACHE.clear()
    rng = np.random.RandomState(5)

    def blob(x, y, k):
        return x + rng.randint(0, 300, k), y + rng.randint(0, 300, k)

    ax, ay = blob(100000, 600000, 5)                      # chrA: one inter-ligation cluster of 5 PETs (only minPts 4 sees it)
    sx = 300000 + rng.randint(0, 300, 12)
    bx, by = [np.concatenate(t) for t in zip(blob(150000, 700000, 12), (sx, sx + rng.randint(20, 200, 12)))]   # chrB: inter + self, 12 each
    fa = pipe.CACHE.put_arrays("chrA-chrA", ax, ay)
    fb = pipe.CACHE.put_arrays("chrB-chrB", bx, by)
    try:
        slow = pipe.runSweep([fa, fb], [1000], [8, 4], cut=0)
        fast = pipe.runSweepFast([fa, fb], [1000], [8, 4], cut=0)
        assert [s["n_inter"] for s in slow[3]] == [1, 2] and slow[1] > 0
        assert list(slow[0]) == [("chrB", "chrB"), ("chrA", "chrA")]
        assert list(fast[0]) == list(slow[0])
        assert fast[1] == slow[1] and fast[2] == slow[2]
    finally:
        pipe.CACHE.clear()


def test_two_sweeps_over_the_same_residents_do_not_interleave(monkeypatch, tmp_path):
    """the candidate buffer / layout of a handle belong to one sweep at a time: two threads sweeping the same files get
    the same result as one after the other"""
    import threading
    monkeypatch.setattr(api, "Chromosome", fake_backend.FakeChromosome)
    monkeypatch.setattr(api, "device_count", lambda: 1)
    pipe.CACHE.clear()
    fs = _write_many_jd(tmp_path, 3, n=600)
    try:
        want = pipe.runSweepFast(fs, [800, 1200], [4, 3], cut=0)
        got = [None, None]

        def run(k):
            got[k] = pipe.runSweepFast(fs, [800, 1200], [4, 3], cut=0)
        ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for g in got:
            assert g[1] == want[1] and g[2] == want[2] and g[0].keys() == want[0].keys()
            for k in g[0]:
                assert np.array_equal(g[0][k]["boxes"], want[0][k]["boxes"])
    finally:
        pipe.CACHE.clear()


def test_replaced_resident_is_closed_by_its_last_user(monkeypatch, tmp_path):
    monkeypatch.setattr(api, "Chromosome", _ClosableFake)
    monkeypatch.setattr(api, "device_count", lambda: 1)
    pipe.CACHE.clear()
    X = np.arange(10, dtype=np.int64) * 100
    f = pipe.CACHE.put_arrays("c-c", X, X + 50)
    with pipe.CACHE.pinned([f]) as rs:
        old = rs[0]
        pipe.CACHE.put_arrays("c-c", X, X + 60)          # replaces the resident a sweep still holds
        assert not getattr(old.chrom, "dead", False) and old.replaced
    assert getattr(old.chrom, "dead", False)              # closed when the pin dropped
    pipe.CACHE.clear()


def test_forced_cuts_replace_the_estimated_chain(cpu_pipe):
    """runSweepFast(forced_cuts=...) (bench.py's scaling proxy: one rank's share replays the genome-wide chain): every step
    still runs and estimates, but hands the given cut to the next step"""
    p, f = cpu_pipe
    free = p.runSweepFast([f], [500, 1000], [5], cut=0)
    forced = p.runSweepFast([f], [500, 1000], [5], cut=0, forced_cuts=[3000, 7000])
    assert [s["cut_in"] for s in forced[3]] == [0, 3000] and [s["cut_out"] for s in forced[3]] == [3000, 7000]
    assert forced[2] == [0, 3000, 7000] and forced[1] == 3000
    assert [s["cut_out"] for s in free[3]] != [3000, 7000]
    assert forced[3][0]["n_inter"] == free[3][0]["n_inter"]          # the first step is the same work
    none = p.runSweepFast([f], [500, 1000], [5], cut=0, forced_cuts=[None, None])
    assert none[2] == free[2]


def test_device_tables_are_consumed_under_the_sweeps_locks(monkeypatch, tmp_path):
    """runSweepFast(finish_device=True, device_consumer=...): the consumer sees every chromosome's (pointer, rows) WHILE the residents are
    pinned in the cache and their sweep locks are held -- nothing can evict, free or re-sweep a handle under the gather
    (cLoops/pipe.py:119-127: the parent merges its workers' results; here the merge reads device memory of live handles)"""
    monkeypatch.setattr(api, "Chromosome", fake_backend.FakeChromosome)
    monkeypatch.setattr(api, "device_count", lambda: 1)
    pipe.CACHE.clear()
    fs = _write_many_jd(tmp_path, 3, n=600)
    seen = {}

    def consumer(dataI):
        res = [pipe.CACHE.get(v["f"]) for v in dataI.values()]
        seen["locked"] = all(r.sweep_lock.locked() for r in res)
        seen["pinned"] = all(r.pins > 0 for r in res)
        seen["rows"] = {k: (v["dev_rows"], v["n_rows"]) for k, v in dataI.items()}
        return sum(v["n_rows"] for v in dataI.values())
    try:
        want = pipe.runSweepFast(fs, [800, 1200], [4, 3], cut=0)
        got = pipe.runSweepFast(fs, [800, 1200], [4, 3], cut=0, finish_device=True, device_consumer=consumer)
        assert seen["locked"] and seen["pinned"]
        assert got[0].gathered == sum(len(v["boxes"]) for v in want[0].values())
        assert {k: n for k, (_, n) in seen["rows"].items()} == {k: len(v["boxes"]) for k, v in want[0].items()}
        assert got[1:3] == want[1:3]
        assert not any(pipe.CACHE.get(f).sweep_lock.locked() for f in fs)
    finally:
        pipe.CACHE.clear()


# ---- the sweep driver's stages: the exchange vector, forced cuts without an estimate, a failing wait, the orders ----
def test_exchange_vector_layout(monkeypatch):
    """what a rank hands to `allsum`: per step ONE float64 vector of 8 + DIST_LOGBINS + 2048 + 6 words -- counts, n_all, n_pos, loghist,
    fine, then sumx, sumxx, xshift and the ranks reporting one -- equal, position by position, to the sums of the chromosomes'
    step_result() values (bench.py times an all-reduce of this length); every other call is a refinement histogram of the median"""
    from cloops_amd import _lib
    from cloops_amd.synth import synth_chrom
    results = []

    class Keeping(fake_backend.FakeChromosome):
        def step_result(self):
            out = fake_backend.FakeChromosome.step_result(self)
            results.append((self._step[0], self.n, out[0], out[1], {k: np.copy(v) for k, v in out[2].items()}, self.last_n_in()))
            return out
    monkeypatch.setattr(api, "Chromosome", Keeping)
    monkeypatch.setattr(api, "device_count", lambda: 1)
    pipe.CACHE.clear()
    fs = [pipe.CACHE.put_arrays("k%d-k%d" % (k, k), *synth_chrom(600 + k, 200000, 900 + k)) for k in range(2)]
    sent = []

    def allsum(a):
        sent.append(a.copy())
        return a.copy()
    try:
        _, _, _, steps = pipe.runSweepFast(fs, [800, 1200], [4, 3], cut=0, allsum=allsum)
    finally:
        pipe.CACHE.clear()
    L, F = _lib.DIST_LOGBINS, 2048
    vecs = [a for a in sent if len(a) == 8 + L + F + 6]
    assert len(vecs) == len(steps) == 4
    assert all(a.dtype == np.int64 and a.shape == (F,) for a in sent if len(a) != 8 + L + F + 6)      # the median's refinement
    for k, v in enumerate(vecs):
        assert v.dtype == np.float64 and v.ndim == 1
        mine = sorted((r for r in results if r[0] == k), key=lambda r: r[1])                       # file order
        counted = [r for r in mine if r[2] > 0]
        assert len(mine) == 2 and len(counted) == 2, "both chromosomes must count for the sums to mean something"
        assert list(v[0:4]) == [sum(r[2] for r in mine), sum(r[3] for r in mine), sum(r[5] for r in mine), len(counted)]
        for g in (0, 1):
            assert v[4 + g] == sum(r[4]["n_all"][g] for r in counted) and v[6 + g] == sum(r[4]["n_pos"][g] for r in counted)
            assert v[8 + L + F + g] == counted[0][4]["sumx"][g] + counted[1][4]["sumx"][g]
            assert v[8 + L + F + 2 + g] == counted[0][4]["sumxx"][g] + counted[1][4]["sumxx"][g]
        assert np.array_equal(v[8:8 + L], counted[0][4]["loghist"] + counted[1][4]["loghist"])
        assert np.array_equal(v[8 + L:8 + L + F], counted[0][4]["fine"] + counted[1][4]["fine"])
        assert v[8 + L:8 + L + F].sum() > 0
        assert v[8 + L + F + 4] == counted[-1][4]["xshift"] and v[8 + L + F + 5] == 1.0
        assert (steps[k]["n_inter"], steps[k]["n_self"], steps[k]["n_in"]) == tuple(int(x) for x in v[0:3])


def test_forced_cuts_on_steps_without_an_estimate(monkeypatch):
    """a forced cut also replaces what a step could NOT estimate: step 0 finds no cluster (the "no inter-ligation PETs" branch), step 1
    finds one inter-ligation blob and no self-ligation PET (one distance group empty).  Without forced cuts such a sweep has no
    positive cut and ends in the reference's ValueError"""
    monkeypatch.setattr(api, "Chromosome", fake_backend.FakeChromosome)
    monkeypatch.setattr(api, "device_count", lambda: 1)
    pipe.CACHE.clear()
    rng = np.random.RandomState(5)
    f = pipe.CACHE.put_arrays("chrA-chrA", 100000 + rng.randint(0, 300, 5), 600000 + rng.randint(0, 300, 5))
    log = []
    try:
        with pytest.raises(ValueError, match="zero-size array to reduction operation minimum which has no identity"):
            pipe.runSweepFast([f], [1000], [8, 5], cut=0)
        dataI, cut, cuts, steps = pipe.runSweepFast([f], [1000], [8, 5], cut=0, forced_cuts=[3000, 7000], log=log.append)
    finally:
        pipe.CACHE.clear()
    assert cuts == [0, 3000, 7000] and cut == 3000
    assert [s["cut_in"] for s in steps] == [0, 3000] and [s["cut_out"] for s in steps] == [3000, 7000]
    assert not any("frags" in s for s in steps)
    assert [s["n_inter"] for s in steps] == [0, 1]
    assert list(dataI) == [("chrA", "chrA")] and len(dataI[("chrA", "chrA")]["boxes"]) == 1
    assert len(log) == 1 and log[0].startswith("ERROR: no inter-ligation PETs detected for eps 1000 minPts 8")


class _Watched(fake_backend.FakeChromosome):
    """records the order of the enqueues and every sweep_plan; the wait of the chromosome of `boom` PETs raises"""
    order, plans, boom = [], [], None

    def step_async(self, variant, eps, minPts, cut, step, fine_lo=-1):
        type(self).order.append((step, self.n))
        return fake_backend.FakeChromosome.step_async(self, variant, eps, minPts, cut, step, fine_lo)

    def wait(self, copy=False):
        if self.n == type(self).boom:
            self._pending.pop(0)
            raise RuntimeError("boom")
        return fake_backend.FakeChromosome.wait(self, copy)

    def sweep_plan(self, eps_list, min_pts_list):
        type(self).plans.append((self.n, list(eps_list), list(min_pts_list)))


@pytest.fixture()
def five_watched(monkeypatch):
    from cloops_amd.synth import synth_chrom
    monkeypatch.setattr(api, "Chromosome", _Watched)
    monkeypatch.setattr(api, "device_count", lambda: 1)
    _Watched.order, _Watched.plans, _Watched.boom = [], [], None
    pipe.CACHE.clear()
    yield [pipe.CACHE.put_arrays("k%d-k%d" % (k, k), *synth_chrom(400 + k, 200000, 70 + k)) for k in range(5)]
    pipe.CACHE.clear()


def test_failed_wait_releases_every_lock(five_watched):
    """the wait of the third of five chromosomes raises: runSweepFast raises that error, and no handle stays locked, pinned, with a
    run pending or with the sweep's minPts list announced"""
    fs = five_watched
    _Watched.boom = 402
    with pytest.raises(RuntimeError, match="boom"):
        pipe.runSweepFast(fs, [800], [4, 3], cut=0)
    for f in fs:
        r = pipe.CACHE.get(f)
        assert not r.lock.locked() and not r.sweep_lock.locked() and r.pins == 0
        assert not getattr(r.chrom, "_pending", [])
        assert [p[1:] for p in _Watched.plans if p[0] == r.chrom.n] == [([800], [4, 3]), ([], [])]


def test_enqueue_is_largest_first_and_keys_in_file_order(five_watched):
    fs = five_watched
    dataI, cut, cuts, steps = pipe.runSweepFast(fs, [800], [4, 3], cut=0)
    assert _Watched.order == [(s, n) for s in range(len(steps)) for n in (404, 403, 402, 401, 400)]
    keys = [pipe.CACHE.get(f).key for f in fs]
    assert len(dataI) > 1 and list(dataI) == [k for k in keys if k in dataI]
