"""GPU: bench.py's command line as every change's benchmark run uses it. A plain run times its steps,
writes the last step's digests under --dump-outputs and prints one line; the legs that take runs of
their own (CPU baseline and its parity check, the Zipf size buckets) appear only with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from bench import zipf_index

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *argv], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1  # one result line
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_the_last_steps_digests(gpu, tmp_path):
    n, L = 4099, 4096  # more than one block, not a multiple of the group size
    res = _bench("--steps", "3", "--warmup", "1", "--entries", str(n), "--dump-outputs", str(tmp_path))
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "roofline"):
        assert key in res
    # value is the payload of the timed steps over their wall time, which ms_per_step states per step
    assert res["value"] == pytest.approx(n * L / (res["ms_per_step"] / 1e3) / (1 << 30), rel=0.01)
    assert "cpu_baseline" not in res and "parity_check" not in res
    assert os.listdir(tmp_path) == ["digests.npy"]
    got = np.load(tmp_path / "digests.npy")
    assert got.dtype == np.float64 and got.shape == (n,)
    want = oracle.uniform(oracle.CRC32C, oracle.fill_splitmix64(n * L, 42), L, L, n)
    assert (got == want.astype(np.float64)).all()  # the inputs are seeded: every run dumps exactly these


def test_full_adds_the_legs_a_plain_run_leaves_out(gpu, tmp_path):
    n = 3001
    args = ["--config", "zipf", "--steps", "2", "--warmup", "1", "--entries", str(n), "--no-cpu-baseline"]
    plain = _bench(*args, "--dump-outputs", str(tmp_path))
    full = _bench(*args, "--full")
    assert "buckets" not in plain and set(full["buckets"]) == {"lt_1KiB", "ge_16KiB"}
    for key in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "config"):
        assert plain[key] == full[key]
    offs, lens = zipf_index(n)
    want = oracle.batch(oracle.CRC32C, oracle.fill_splitmix64(int(offs[-1] + lens[-1]), 42), offs, lens)
    assert (np.load(tmp_path / "digests.npy") == want.astype(np.float64)).all()
