"""GPU: bench.py's two forms on a small genome.  A plain run prints the headline and none of the figures that take runs of their
own; --full adds every one of them and still times the same sweep, with the same outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "cold_sweep_s", "with_labels", "with_labels_sweep_s", "scaling_proxy", "secondary_5M", "secondary_chr21_cli",
             "cpu_baseline")


def _bench(outdir, extra=()):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n-total", "2e6", "--steps", "2", "--warmup", "1",
                          "--dump-outputs", outdir] + list(extra), env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_bench_plain_is_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _bench(str(tmp_path / "plain"))
    full = _bench(str(tmp_path / "full"), ["--full", "--proxy-ranks", "2"])
    for j in (plain, full):
        assert all(k in j for k in HEADLINE) and j["value"] > 0 and j["ms_per_step"] > 0 and j["steps"] == 2
    assert not [k for k in FULL_ONLY if k in plain]
    assert [k for k in FULL_ONLY if k not in full] == []
    assert full["roofline"]["launches"] == 3 * 12 and full["scaling_proxy"]["ranks"] == 2
    assert full["secondary_chr21_cli"]["loop_file_identical_to_golden"] is True
    assert full["cpu_baseline"]["labels_match_gpu"] is True
    assert plain["config"] == dict(full["config"], synthesis_s_rank0=plain["config"]["synthesis_s_rank0"])
    names = sorted(os.listdir(str(tmp_path / "plain")))
    assert names == sorted(os.listdir(str(tmp_path / "full"))) and "candidate_boxes.npy" in names
    for name in names:
        a, b = (np.load(str(tmp_path / d / name)) for d in ("plain", "full"))
        assert np.array_equal(a, b, equal_nan=True), name
