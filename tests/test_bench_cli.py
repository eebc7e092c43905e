"""CPU: bench.py's launch contract -- `--gpus N` really starts N ranks (gloo here, RCCL on the GPU box), the 23
chromosomes are LPT-sharded over them, the chained cut comes out of the all-reduced statistics and equals the
single-process chain.  The GPU handle is replaced by the oracle-backed stand-in (tests/bench_cpu_hook.py)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(gpus, extra=()):
    env = dict(os.environ)
    env["CLOOPS_BENCH_PRELOAD"] = "bench_cpu_hook"
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "tests"), ROOT, env.get("PYTHONPATH", "")])
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--backend", "gloo",
                          "--n-total", "400000", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-secondary"] + list(extra),
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines                      # exactly one JSON line on stdout
    return json.loads(lines[0])


def test_bench_gpus_2_spawns_two_ranks_and_matches_single_process():
    one = _bench(1)
    two = _bench(2)
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2
    for j in (one, two):
        assert "configs[3]" in j["config"]["workload"] and j["config"]["chromosomes"] == 23
        assert j["config"]["runs_per_sweep"] == 12 and j["scaling"] == "strong" and j["unit"] == "PETs/s"
    assert any(c is not None for c in one["config"]["cuts"])
    assert two["config"]["cuts"] == one["config"]["cuts"]
    assert two["config"]["final_cut"] == one["config"]["final_cut"]
    assert two["config"]["candidate_loops"] == one["config"]["candidate_loops"]
    assert two["config"]["pets_entering_dbscan_per_sweep"] == one["config"]["pets_entering_dbscan_per_sweep"]


def test_bench_dump_outputs_are_reproducible_and_match_the_json_line(tmp_path):
    """--dump-outputs: float64 .npy files of what the last timed sweep returned, identical from run to run with the same
    arguments, consistent with the JSON line; --steps sets the number of timed sweeps"""
    import numpy as np
    dirs = [str(tmp_path / ("d%d" % k)) for k in range(2)]
    runs = [_bench(1, ["--dump-outputs", d, "--steps", str(k + 1)]) for k, d in enumerate(dirs)]
    assert [j["steps"] for j in runs] == [1, 2]
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1])) and "candidate_boxes.npy" in names
    total = 0
    for name in names:
        a, b = (np.load(os.path.join(d, name)) for d in dirs)
        assert a.dtype == np.float64 and np.array_equal(a, b, equal_nan=True), name
        total += os.path.getsize(os.path.join(dirs[0], name))
    assert total <= 64 << 20
    one = runs[0]
    boxes = np.load(os.path.join(dirs[0], "candidate_boxes.npy"))
    counts = np.load(os.path.join(dirs[0], "candidate_counts.npy"))
    assert boxes.shape == (one["config"]["candidate_loops"], 5) and counts.sum() == one["config"]["candidate_loops"] and len(counts) == 23
    assert np.array_equal(np.load(os.path.join(dirs[0], "candidate_sums.npy")),
                          np.stack([boxes[boxes[:, 0] == i, 1:].sum(0) for i in range(23)]))
    st = np.load(os.path.join(dirs[0], "sweep_steps.npy"))
    assert st.shape == (12, 7) and st[:, 5].sum() == one["config"]["pets_entering_dbscan_per_sweep"]
    assert [None if np.isnan(c) else int(c) for c in st[:, 6]] == one["config"]["cuts"]
    assert int(np.load(os.path.join(dirs[0], "final_cut.npy"))[0]) == one["config"]["final_cut"]


def test_bench_dump_outputs_samples_a_large_table(tmp_path):
    """above the row budget the box table is a fixed sample of the sorted rows; counts and sums still cover every row"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(5)
    tabs = [np.sort(rng.integers(0, 10 ** 6, (n, 4)), axis=1).astype(np.int32) for n in (700, 0, 500)]
    dataI = {("c%d" % i, "c%d" % i): {"f": "f%d" % i, "boxes": t} for i, t in enumerate(tabs) if len(t)}
    steps = [{"eps": 5, "minPts": 3, "cut_in": 0, "n_inter": 2, "n_self": 1, "n_in": 9, "cut_out": 7}]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), ["f0", "f1", "f2"], dataI, 7, [0, 7], steps, max_rows=300)
    a, b = (np.load(str(tmp_path / d / "candidate_boxes.npy")) for d in ("a", "b"))
    assert a.shape == (300, 5) and np.array_equal(a, b)
    full = np.concatenate([np.concatenate([np.full((len(t), 1), i), t], 1) for i, t in enumerate(tabs)])
    assert len(set(map(tuple, a)) - set(map(tuple, full.astype(np.float64)))) == 0
    assert np.array_equal(a, a[np.lexsort(a.T[::-1])])
    assert np.load(str(tmp_path / "a" / "candidate_counts.npy")).tolist() == [700, 0, 500]
    assert np.array_equal(np.load(str(tmp_path / "a" / "candidate_sums.npy")), np.stack([t.astype(np.int64).sum(0) for t in tabs]))


def _preflight_world2(children, timeout):
    """bench.rccl_preflight on two 'ranks' of one launch (two threads: same parent process, i.e. the same launch tag), each
    with a stand-in for the child that would try RCCL -> [(ok, note), (ok, note)]"""
    import threading
    sys.path.insert(0, ROOT)
    import bench
    out = [None, None]

    def run(rank):
        out[rank] = bench.rccl_preflight(rank, 2, rank, timeout=timeout, child=children[rank])
    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    return out


def test_preflight_all_ranks_take_the_same_decision(monkeypatch):
    """the RCCL-direct pre-flight of bench.py: whatever happens to one rank's child (error, hang), every rank reads the same
    verdict -- the ranks cannot split between libcloops_comm.so and torch.distributed"""
    monkeypatch.setenv("MASTER_PORT", "1")
    ok = "import sys"
    bad = "import sys; sys.stderr.write('hipIpcGetMemHandle: invalid argument'); sys.exit(3)"
    hang = "import time; time.sleep(60)"
    monkeypatch.setenv("TORCHELASTIC_RUN_ID", "pf-a")
    a = _preflight_world2([ok, ok], 20.0)
    assert a == [(True, ""), (True, "")], a
    monkeypatch.setenv("TORCHELASTIC_RUN_ID", "pf-b")
    b = _preflight_world2([ok, bad], 20.0)
    assert b[0][0] is False and b[1][0] is False and b[0] == b[1] and "rank 1: exit 3" in b[0][1] and "hipIpcGetMemHandle" in b[0][1], b
    monkeypatch.setenv("TORCHELASTIC_RUN_ID", "pf-c")
    c = _preflight_world2([hang, ok], 2.0)
    assert c[0][0] is False and c[1][0] is False and c[0] == c[1] and "rank 0: no answer" in c[0][1], c


def test_full_is_off_by_default_and_full_cpu_baseline_needs_it():
    """a plain run measures the headline only; what takes runs of its own comes with --full, which --full-cpu-baseline refines"""
    import pytest
    sys.path.insert(0, ROOT)
    import bench
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full", "--full-cpu-baseline"]).full_cpu_baseline is True
    with pytest.raises(SystemExit):
        bench.parse_args(["--full-cpu-baseline"])
