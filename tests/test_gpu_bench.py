"""bench.py on one GPU: a plain run measures the headline figure alone; --full adds the legs beside it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ("kuf_roofline", "value_and_gradient", "cpu_baseline", "parity", "gpu_over_cpu")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", "C2", *args], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path))
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["unit"] == "evals/s" and plain["dtype"] == "f64"
    assert plain["higher_is_better"] is True and plain["steps"] == 3 and plain["warmup"] == 1
    assert not set(EXTRAS) & set(plain), sorted(set(EXTRAS) & set(plain))
    assert plain["roofline"]["achieved"] > 0 and "traffic_source" not in plain["roofline"]
    assert float(np.load(tmp_path / "elbo.npy")) == plain["config"]["elbo"]

    full = _bench("--full")
    assert set(EXTRAS) <= set(full), sorted(set(EXTRAS) - set(full))
    assert full["parity"]["ok"] and full["value"] > 0
    assert full["kuf_roofline"]["achieved"] > 0 and full["value_and_gradient"]["ms_per_eval"] > 0
    # the same seeded workload either way
    assert abs(full["config"]["elbo"] - plain["config"]["elbo"]) <= 1e-12 * abs(plain["config"]["elbo"])
