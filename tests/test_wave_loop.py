"""The wave search kernels' simulation loop on ragged waves, bit for bit against the oracle, and the
register budget of every mzh_wave_kernel instantiation.

The loop loads a chain's layer-2 bias fragments before its hidden blocks, keeps the bin-32 chains of its
column tiles apart, and decides the latent normalisation's exactness once per lane.  The cases put
invalid root lanes and invalid columns beside those: one full wave plus a wave with a single valid
root (B = 33 at 32 roots per wave, 17 at 16).
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

DEV = "cuda"
N = 4
CASES = [("wave", 33), ("wave16", 17)]  # one full wave + a wave with one valid root
OUTPUTS = (("visits", "visits"), ("root_q", "rootQ"), ("action", "action"), ("pi", "pi"), ("sel_steps", "sel_steps"),
           ("extra_ties", "extra_ties"), ("latent", "latent"), ("latent_len", "latent_len"))


def _inputs(B, seed, deterministic):
    from muzero_hanoi_amd import rng

    rs = np.random.RandomState(seed)
    st = rs.randint(0, 3, (B, N))
    obs = np.zeros((B, 3 * N), np.float32)
    obs[np.arange(B)[:, None], np.arange(N) * 3 + st] = 1
    noise, tie, u = rng.synthetic_draws(B, deterministic=deterministic, alpha=0.25, seed=seed)
    return obs, noise, tie, u


def _weights(oracle):
    w, in_dim, sup = oracle.load_weights_npz(f"{GOLDEN}/weights_N4_s0.npz")
    return oracle.flat_weights(w), sup


def _tiny_latent_gap(oracle):
    """weights_N4_s0 with the dynamics output layer made constant: h' = its bias, one unit 2^-110 above the
    row minimum, so that unit's numerator in the latent normalisation is below 2^-100 and every expansion
    takes the exact-division rerun (the construction of tests/test_gpu_parity.py)"""
    w, in_dim, sup = oracle.load_weights_npz(f"{GOLDEN}/weights_N4_s0.npz")
    w = {k: v.copy() for k, v in w.items()}
    w["dynamic_net.2.weight"][:] = 0.0
    b = np.random.RandomState(11).uniform(0.25, 1.0, 64).astype(np.float32)
    b[3], b[17] = 0.0, np.float32(2.0 ** -110)
    w["dynamic_net.2.bias"][:] = b
    return oracle.flat_weights(w), sup


def _check(oracle, kernel, B, S, flat, sup, seed, deterministic=False, minmax_in=None):
    from muzero_hanoi_amd import engine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    obs, noise, tie, u = _inputs(B, seed, deterministic)
    tt = lambda a: None if a is None else torch.tensor(np.asarray(a), device=DEV)
    eng = engine.Engine(N, S, B, sup)
    eng.load_weights(flat)
    o = eng.search(S, obs=tt(obs), tie_idx=tt(tie), noise=tt(noise), action_u=tt(u), minmax_in=tt(minmax_in),
                   temperature=1.0, deterministic=deterministic, kernel=kernel)
    want_nt = 2 if kernel == "wave" else 1
    assert o["_plan"]["kernel"].startswith(f"mzh_wave_kernel<{want_nt}, false, true>"), o["_plan"]
    o = {k: v.cpu().numpy() for k, v in o.items() if not k.startswith("_")}
    eng.close()
    ref = oracle.search(N, S, obs, flat=flat, support=sup, noise=noise, tie_idx=tie, action_u=u, temperature=1.0,
                        deterministic=deterministic, minmax_in=minmax_in)
    for k, rk in OUTPUTS:
        assert np.array_equal(o[k], ref[rk]), k
    assert np.array_equal(o["minmax"][:, 0], ref["mm_max"]) and np.array_equal(o["minmax"][:, 1], ref["mm_min"])
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,B", CASES)
def test_wave_loop_ragged_stochastic_vs_oracle(oracle, kernel, B):
    """stochastic search with Dirichlet noise, 20 simulations: every output equals the oracle's"""
    flat, sup = _weights(oracle)
    _check(oracle, kernel, B, 20, flat, sup, seed=500 + B)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,B", CASES)
def test_wave_loop_ragged_caller_bounds_deterministic_vs_oracle(oracle, kernel, B):
    """the same waves with caller-given MinMaxStats bounds (fresh, finite, equal, and spread pairs) and the
    deterministic action"""
    flat, sup = _weights(oracle)
    pairs = np.array([[-np.inf, np.inf], [0.4, -0.2], [0.05, 0.05], [1.5, 0.0], [0.0, -1.0]], np.float64)
    mm = pairs[np.arange(B) % len(pairs)]
    _check(oracle, kernel, B, 20, flat, sup, seed=600 + B, deterministic=True, minmax_in=mm)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,B", CASES)
def test_wave_loop_ragged_exact_rerun_vs_oracle(oracle, kernel, B):
    """a latent unit 2^-110 above the row minimum: the normalisation's once-per-lane exactness decision sends
    every expansion of the ragged waves to the exact-division rerun"""
    flat, sup = _tiny_latent_gap(oracle)
    _check(oracle, kernel, B, 12, flat, sup, seed=700 + B)


def test_wave_kernels_fit_the_register_file():
    """csrc/mzh_wave.hip compiled for gfx950 to assembly: each of the eight mzh_wave_kernel instantiations
    spills no VGPR and stays within the 256 VGPRs that two waves per SIMD leave it"""
    from muzero_hanoi_amd import build as b

    hipcc = b.HIPCC if os.path.exists(b.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc is absent")
    flags = [f for f in b.FLAGS if not f.startswith("--offload-arch")] + b.SOURCE_FLAGS.get("mzh_wave.hip", [])
    r = subprocess.run([hipcc, *flags, "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", "-",
                        os.path.join(ROOT, "muzero-hanoi_amd", "csrc", "mzh_wave.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    meta = {}
    for blk in r.stdout.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "mzh_wave_kernel" in name:
            meta[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                          int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)))
    assert len(meta) == 8, sorted(meta)
    for name, (vgprs, spills) in meta.items():
        assert spills == 0 and vgprs <= 256, (name, vgprs, spills)
