"""bench.py's command line on the host simulator (tests/bench_on_hostsim.py runs the unchanged bench.py): a plain run times exactly
--steps steps and carries only the headline fields, --full adds the measurements that moved behind it, and --dump-outputs writes the
last timed step's outputs -- float32 / float64, within 64 MB, the same in every run of the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np

from tests import backends

ARGS = ["--size", "64", "--batch", "1", "--steps", "1", "--warmup", "1"]


def _bench(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SWN_")}
    out = subprocess.run([sys.executable, os.path.join(backends.REPO, "tests", "bench_on_hostsim.py")] + ARGS + extra, env=env,
                         capture_output=True, text=True, timeout=900, cwd=backends.REPO)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_and_full_runs_dump_the_same_outputs(tmp_path):
    backends.build_hostsim()
    a, b = str(tmp_path / "plain"), str(tmp_path / "full")
    plain = _bench(["--dump-outputs", a])
    assert plain["steps"] == 1 and plain["warmup"] == 1 and plain["ms_per_step"] > 0 and plain["losses_finite"] is True
    assert abs(plain["value"] - 1 / (plain["ms_per_step"] * 1e-3)) <= 0.02 * plain["value"]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert "roofline" not in plain and "cpu_baseline" not in plain and "routing" not in plain["config"]
    # --full measures after the dump, on the same model: the routing digest is its part that runs on the simulator
    full = _bench(["--full", "--no-cpu-baseline", "--dump-outputs", b])
    assert full["steps"] == 1 and full["config"]["routing"]["launch_lines"] > 0 and "cpu_baseline" not in full
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"output.npy", "weights_G.npy", "weights_D.npy", "loss_G.npy", "loss_D.npy"} <= set(names)
    assert sum(os.path.getsize(os.path.join(a, n)) for n in names) <= 64 * 10**6
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype in (np.float32, np.float64), (n, x.dtype)
        assert np.isfinite(x).all(), n
        np.testing.assert_array_equal(x, y, err_msg=n)
