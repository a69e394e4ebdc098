"""bench.py's plain run (no --full): exactly --steps timed steps, the headline fields of the line, and --dump-outputs writing what
the last timed step computed.  The noise of a step is keyed by its index (warm-up steps included), so two runs whose last step has
the same index -- whatever the split between warm-up and timed steps -- must dump the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps, warmup):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith('{"metric"')][-1])


@pytest.mark.gpu
def test_plain_bench_times_the_steps_asked_for_and_dumps_the_last_one(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    line = _bench(a, steps=3, warmup=1)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "frames/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["ms_per_step"] > 0 and np.isfinite(line["value"]) and line["value"] > 0
    # frames per step / seconds per step
    T, B = line["config"]["seq_len"], line["config"]["global_batch"]
    assert abs(line["value"] - B * T / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    # a plain run measures nothing else
    assert line["train"] is None and line["cpu_baseline"] is None and line["streams"] is None and line["slot_chain"] is None
    names = sorted(os.listdir(a))
    for n in ("log_weights_per_timestep.npy", "log_weights.npy", "elbo_iwae.npy", "elbo_iwae_per_example.npy"):
        assert n in names
    assert sum(os.path.getsize(a / n) for n in names) <= 64 << 20
    elbo = np.load(a / "elbo_iwae.npy")
    assert elbo.dtype == np.float32 and abs(float(elbo) - line["elbo_iwae_nats_per_seq"]) <= 1e-6 * abs(float(elbo))
    # same last step index (3), other warm-up / timed split: the same outputs, bit for bit
    _bench(b, steps=2, warmup=2)
    assert sorted(os.listdir(b)) == names
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float32 and x.shape == y.shape and np.array_equal(x, y, equal_nan=True), n
