"""bench.py on the device: a plain run's line, --dump-outputs, and the legs --full adds (one small
workload, each command run once as a child process and shared by the tests)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ROOTS, SIMS, STEPS = 1000, 10, 3  # the cooperative kernel's batch range; not a multiple of its 16-root tile


def _run(*extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "1", "--roots-per-gpu", str(ROOTS), "--sims", str(SIMS), *extra],
                       capture_output=True, text=True, timeout=280, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return _run("--dump-outputs", str(d)), d


def test_plain_line(plain):
    """the headline fields, --steps timed launches, and none of the --full legs"""
    rec, _ = plain
    assert rec["unit"] == "sims/s" and rec["higher_is_better"] is True and rec["dtype"] == "fp32"
    assert rec["steps"] == STEPS and rec["roofline"]["launch_stats"]["n"] == STEPS
    assert rec["ms_per_step"] > 0
    assert abs(rec["value"] - ROOTS * SIMS / (rec["ms_per_step"] * 1e-3)) <= 1e-6 * rec["value"]
    assert rec["cpu_baseline"] is None and rec["roofline"]["tree"] is None and rec["roofline"]["with_minmax_in"] is None


def test_dumped_outputs_are_the_search_of_the_bench_inputs(plain, oracle):
    """DIR/<name>.npy hold what the timed search returned: equal to the oracle's search of the same
    inputs (bench.random_roots, rng.predraw on RandomState(seed), MuZeroNet after manual_seed(seed))"""
    import torch

    import bench
    from muzero_hanoi_amd import engine, rng
    from muzero_hanoi_amd.networks import MuZeroNet

    _, d = plain
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert {"visits", "action", "root_q", "pi", "minmax", "sel_steps", "latent", "latent_len"} <= set(got)
    assert all(v.dtype in (np.float32, np.float64) and len(v) == ROOTS for v in got.values())
    torch.manual_seed(0)
    flat = engine.flat_weights(MuZeroNet(12, 6, 0.002, "cpu", TD_return=True).state_dict())
    obs = bench.random_roots(4, ROOTS, 0)
    noise, tie, u = rng.predraw(ROOTS, deterministic=False, alpha=0.25, rng=np.random.RandomState(0))
    ref = oracle.search(4, SIMS, obs, flat=flat, support=33, noise=noise, tie_idx=tie, action_u=u, temperature=1.0)
    assert np.array_equal(got["visits"], ref["visits"]) and got["visits"].sum(1).tolist() == [SIMS] * ROOTS
    assert np.array_equal(got["root_q"], ref["rootQ"])
    assert np.array_equal(got["action"], ref["action"])


def test_full_adds_the_other_legs():
    """--full: the device legs a plain run leaves out are measured (the CPU baseline, a pool of host
    processes, switched off here to keep the test short)"""
    rec = _run("--full", "--no-cpu-baseline")
    assert rec["steps"] == STEPS and rec["cpu_baseline"] is None
    assert rec["roofline"]["tree"]["kernel_ms"] > 0 and rec["roofline"]["with_minmax_in"]["kernel_ms"] > 0
