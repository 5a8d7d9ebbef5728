"""bench.py's plain single-GPU command, the one every change is measured with: the headline line alone (the side
measurements are --full's), --steps timed steps behind ms_per_step, and --dump-outputs writing what the last timed step
computed -- the same arrays in every run of the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(dump):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(dump)]
    env = {k: v for k, v in os.environ.items() if k not in ("SELAVI_TUNE_CACHE", "SELAVI_BENCHMARK")}
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-6000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"expected ONE JSON line, got {len(lines)}"
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    dump = tmp_path / "dump"
    out = _plain_run(dump)
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["warmup"] == 1
    assert out["unit"] == "clips/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["value"] > 0 and abs(out["value"] - 16 * 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]
    for k in ("roofline", "forward", "comm", "sk", "sk_round", "cfg5_bf16", "cfg2_bf16", "native_fp32_mfma", "cpu_baseline"):
        assert k not in out, k
    assert sorted(os.listdir(dump)) == ["buffers.npy", "grads.npy", "loss.npy", "params.npy"]
    a = {f[:-4]: np.load(dump / f) for f in os.listdir(dump)}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["loss"].shape == (1,) and a["loss"][0] == np.float32(out["config"]["loss_last_step"])
    assert a["params"].shape == a["grads"].shape and a["params"].size > 3_000_000 and np.abs(a["grads"]).max() > 0
    # every conv launch configuration came from bench_tune.json: nothing was chosen by timing in this run ...
    assert out["config"]["launch_configs_timed_this_run"] == 0
    # ... so a second run computes bit for bit the same
    out2 = _plain_run(tmp_path / "dump2")
    assert out2["config"]["loss_last_step"] == out["config"]["loss_last_step"]
    for f in os.listdir(dump):
        assert np.array_equal(np.load(dump / f), np.load(tmp_path / "dump2" / f)), f
