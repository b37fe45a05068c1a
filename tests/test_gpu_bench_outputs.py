"""bench.py as later measurements call it: a plain run prints one result line with the headline fields and none of
the --full legs, runs exactly --steps timed steps, and --dump-outputs DIR leaves the last timed step's outputs as
float32 .npy files.  One short run (256 px, 2 + 1 steps) shared by the checks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = tmp_path_factory.mktemp("bench") / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--resolution", "256", "--n-seeds", "8", "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), out


def test_plain_result_line(run):
    line, _ = run
    assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value = 2 images per seed, 4 seeds per step (8 seeds: both batches are full)
    assert line["value"] == pytest.approx(2 * 4 / (line["ms_per_step"] / 1e3), rel=1e-3)
    assert line["config"]["direction_finite"] is True
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["parity"] is None


def test_dumped_outputs(run):
    _, out = run
    assert sorted(os.listdir(out)) == ["direction.npy", "grad.npy", "loss_parts.npy"]
    arrays = {n[:-4]: np.load(out / n, allow_pickle=False) for n in os.listdir(out)}
    assert arrays["direction"].shape == (1, 8, 512) and arrays["grad"].shape == (1, 8, 512)
    assert arrays["loss_parts"].shape == (4,)
    for name, a in arrays.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
    assert np.abs(arrays["grad"]).max() > 0 and np.abs(arrays["direction"]).max() > 0
    assert arrays["loss_parts"][2] == 0   # landmarks loss is off
