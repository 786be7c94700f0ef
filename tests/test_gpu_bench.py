"""bench.py's plain run, as the benchmark driver starts it: exactly --steps timed steps in one region, the headline fields of the
result line and nothing of --full, and --dump-outputs writing the last step's loss and trained variables as float32 .npy files."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_steps_and_dumps_outputs(tmp_path):
    out = str(tmp_path / "outputs")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RSX_FORCE_DIST")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "24", "--warmup", "5",
                        "--dump-outputs", out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "examples/sec" and d["unit"] == "examples/sec" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 24 and len(d["config"]["timed_repeats_ms_per_step"]) == 1
    assert d["ms_per_step"] > 0 and abs(d["value"] - 256 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    assert not {"roofline", "configs", "cpu_baseline"} & set(d)

    files = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(out, "*.npy"))}
    assert {"loss", "dense", "input_layer.tables", "input_layer.w1"} <= set(files), sorted(files)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in files.values())
    assert sum(os.path.getsize(f) for f in glob.glob(os.path.join(out, "*.npy"))) <= 64 << 20
    assert files["loss"].shape == (1,) and abs(float(files["loss"][0]) - d["config"]["final_loss"]) < 1e-4
    assert files["input_layer.tables"].shape == (65536, 16)
