"""``bench.py`` as later measurements run it (GPU box): a plain run times exactly ``--steps`` steps in one window, prints
the headline keys only, and ``--dump-outputs`` writes the scores of its last timed step -- the same scores again in a
second run with the same arguments, so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _bench(args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_times_k_steps_and_dumps_the_last_step(tmp_path):
    args = ["--gpus", "1", "--config", "tiny", "--steps", "7", "--warmup", "2", "--spinup", "0"]
    runs = [_bench(args + ["--dump-outputs", str(tmp_path / f"run{k}")]) for k in range(2)]
    for d in runs:
        assert d["steps"] == 7 and d["warmup"] == 2 and d["ms_per_step_repeats"]["n"] == 1
        assert d["ms_per_step"] > 0 and d["value"] > 0
        assert d["unit"] == "pairs/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["metric"] == "candidate link-pairs scored/sec (whole node)"
        for k in ("kernels", "rooflines", "cpu_baseline", "trained_weights", "bf16_mode", "encoder_ms"):
            assert k not in d, f"{k} belongs to --full"
    bs = runs[0]["config"]["pairs_per_step_per_gpu"]
    a, b = (np.load(tmp_path / f"run{k}" / "scores.npy") for k in range(2))
    assert a.dtype == np.float32 and a.shape == (bs,)
    assert np.isfinite(a).all() and (a >= 0).all() and (a <= 1).all() and a.std() > 0
    assert np.abs(a - b).max() <= 1e-6
