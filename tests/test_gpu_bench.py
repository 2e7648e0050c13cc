"""bench.py without --full: the headline and nothing else — the contract's keys on ONE stdout line, no roofline, baselines or detail file,
and --dump-outputs still written."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_only_the_headline(tmp_path):
    dump = tmp_path / "outputs"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-500:]
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config"):
        assert key in line, key
    assert line["steps"] == 3 and line["warmup"] == 1 and line["higher_is_better"] is True and line["unit"] == "edges/s"
    # value = aggregated edges / step time; ms_per_step is that step time rounded to 3 decimals
    assert abs(1e3 * line["config"]["aggregated_edges_per_step"] / line["value"] - line["ms_per_step"]) <= 0.0005 + 1e-9
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["detail_file"] is None
    # the copy pass before the timed steps reports its rate; eager_ms_per_step: a small window's headline is the faster of the eager
    # forward and its hipGraph replay
    assert set(line["also"]) <= {"bench_wall_s", "hbm_copy_GBps_measured", "eager_ms_per_step"}, line["also"]
    emb = np.load(dump / "embeddings.npy")
    assert emb.dtype == np.float32 and emb.shape[1] == line["config"]["nodes"] and np.isfinite(emb).all()
