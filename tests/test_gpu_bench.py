"""bench.py without --full: the headline figure alone -- set-up, warm-up, the timed steps, --dump-outputs and the result
line, none of the extra measurements or checks (those run behind --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXTRAS = ("steady_state", "hip_graph_replay", "other_engines_extra", "other_configs_extra", "rows_65536_per_gpu_extra",
          "small_shards_extra", "cpu_baseline", "speedup_vs_cpu_baseline")


def test_plain_run_is_the_headline_alone(tmp_path):
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["metric"].startswith("log_prob samples/sec") and r["unit"] == "samples/s" and r["higher_is_better"] is True
    assert r["steps"] == 2 and r["warmup"] == 1 and r["value"] > 0 and r["ms_per_step"] > 0
    assert r["dtype"].startswith("f32") and r["config"]["global_batch"] == 262144
    assert not [k for k in EXTRAS if k in r]
    assert r["roofline_k1_unfused"] is None and r["fwd_inv_max_err"]["composite_32_layers"] is None
    lp = np.load(out_dir / "log_prob.npy")
    sc = np.load(out_dir / "log_likelihood_sum_count.npy")
    assert lp.dtype == np.float32 and np.isfinite(lp).all() and sc[1] == 262144
    assert abs(sc[0] / sc[1] - r["mean_log_likelihood"]) <= 1e-9 * abs(r["mean_log_likelihood"])
