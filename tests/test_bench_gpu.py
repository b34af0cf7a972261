"""bench.py's plain run: exactly --steps timed steps, the headline fields and nothing of --full; --dump-outputs writes the
last timed step's loss, parameters and BatchNorm running statistics, the same from run to run for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + list(args), cwd=REPO, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_times_its_steps_and_dumps_outputs(tmp_path):
    outs, dumps = [], []
    for run in range(2):
        d = tmp_path / ("run%d" % run)
        outs.append(_bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "32", "--dump-outputs", str(d)))
        dumps.append({k: np.load(d / (k + ".npy")) for k in ("loss", "params", "bn_running")})
        assert sorted(os.listdir(d)) == ["bn_running.npy", "loss.npy", "params.npy"]
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
    out = outs[0]
    assert out["metric"] == "frame-crops/sec (VPD student train)" and out["unit"] == "crops/s" and out["higher_is_better"] is True
    assert out["dtype"] == "bf16" and out["steps"] == 3 and out["repeats"]["n"] == 1 and out["config"]["global_batch"] == 32
    assert out["ms_per_step"] > 0 and abs(out["value"] - 32 * 1e3 / out["ms_per_step"]) <= 1e-6 * out["value"]
    assert not {"roofline", "parity", "apply", "cpu_baseline", "multi_gpu"} & set(out)
    a, b = dumps
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert a["loss"].shape == (1,) and a["params"].shape == (1 << 23,) and a["bn_running"].size > 0
    assert abs(float(a["loss"][0]) - out["config"]["loss_last_step"]) <= 1e-6 * abs(out["config"]["loss_last_step"])
    # same arguments, same inputs: the two runs agree to the rounding of the atomics (first AdamW steps move a weight by <= lr)
    assert abs(float(a["loss"][0]) / float(b["loss"][0]) - 1) < 1e-2
    assert np.abs(a["params"] - b["params"]).max() < 5e-3 and np.allclose(a["bn_running"], b["bn_running"], rtol=1e-2, atol=1e-3)
