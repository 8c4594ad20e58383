"""The wave kernel's three M-phase forms at their boundaries on the GPU.

The packing permutation, the record / rank bookkeeping of a wave that mixes hits and misses, and the root priors a
wave of state roots takes from the table's depth-0 records: a search must equal the search without the memo and
the oracle bit for bit, and take each form exactly where the oracle's depths say.

Forced forms (N = 3, S = 3, D = 3: a new node's depth is at most s + 1 <= D, so a root whose observation is a
state's hits at every simulation): k roots of the first 32-root wave sit on rows that are no state's (one entry
off by 0.5) and miss always, so that wave takes one form at every simulation -- k = 0 none, 1..16 the packed
tile, 17..32 its own tiles -- and the second wave never runs a chain.  The perturbed roots sit at the lowest, the
highest and scattered lanes of the wave: the packing permutation and the record / rank bookkeeping.

Mixed depths use tests/test_memo_cpu.py's search cases (four discs: the helpers' size) at S = 16, with ragged
last waves of 1 and 8 roots.
"""
import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_memo_cpu import case_inputs, mixed_inputs, predict_paths, scramble_inputs, weights

DEV = "cuda"
OUTPUTS = (("visits", "visits"), ("root_q", "rootQ"), ("action", "action"), ("pi", "pi"), ("sel_steps", "sel_steps"),
           ("extra_ties", "extra_ties"), ("latent", "latent"), ("latent_len", "latent_len"))
RPW = {"wave": 32, "wave16": 16}
N3, S3, D3 = 3, 3, 3
PLACES = ("lowest", "highest", "scattered")
FORCED = [(0, "lowest"), (32, "lowest")] + [(k, pl) for k in (1, 15, 16, 17) for pl in PLACES]


def _tt(a):
    return None if a is None else torch.tensor(np.asarray(a), device=DEV)


def weights3(oracle, other=False):
    """the golden three-disc weights; other: with another policy and value head and a shifted latent"""
    w, in_dim, sup = oracle.load_weights_npz(f"{GOLDEN}/weights_N3_s0.npz")
    assert in_dim == 3 * N3
    if other:
        w = {k: v.copy() for k, v in w.items()}
        w["policy_net.2.weight"] *= np.float32(-3.0)
        w["value_net.2.weight"] *= np.float32(1.5)
        w["dynamic_net.2.bias"] += np.float32(0.125)
    return oracle.flat_weights(w), sup


def inputs3(B, perturbed=(), deterministic=False, seed=0):
    """B three-disc roots with their draws; the rows named in `perturbed` get one entry off by 0.5"""
    from muzero_hanoi_amd import rng

    st = np.random.RandomState(50 + seed).randint(0, 3, (B, N3))
    obs = np.zeros((B, 3 * N3), np.float32)
    obs[np.arange(B)[:, None], np.arange(N3) * 3 + st] = 1
    for r in perturbed:
        obs[r, (5 * r) % (3 * N3)] += np.float32(0.5)
    noise, tie, u = rng.synthetic_draws(B, deterministic=deterministic, alpha=0.25, seed=700 + seed)
    return obs, noise, tie, u, None


def placed(k, place):
    if place == "lowest":
        return tuple(range(k))
    if place == "highest":
        return tuple(range(32 - k, 32))
    return tuple(sorted(np.random.RandomState(k).permutation(32)[:k].tolist()))


@pytest.fixture(scope="module")
def eng3(oracle):
    from muzero_hanoi_amd import engine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    flat, sup = weights3(oracle)
    eng = engine.Engine(N3, 16, 64, sup)
    eng.load_weights(flat)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def eng4(oracle):
    from muzero_hanoi_amd import engine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    flat, sup = weights(oracle)
    eng = engine.Engine(4, 16, 64, sup)
    eng.load_weights(flat)
    yield eng
    eng.close()


def _search(eng, kernel, S, inp, deterministic):
    obs, noise, tie, u, mm = inp
    o = eng.search(S, obs=_tt(obs), tie_idx=_tt(tie), noise=_tt(noise), action_u=_tt(u), minmax_in=_tt(mm),
                   temperature=1.0, deterministic=deterministic, kernel=kernel)
    want_nt = 2 if kernel == "wave" else 1
    assert o["_plan"]["kernel"] == f"mzh_wave_kernel<{want_nt}, false, true>", o["_plan"]
    return {k: v.cpu().numpy() for k, v in o.items() if not k.startswith("_")}


def _counted(eng, fn):
    a = eng.memo_stats()
    out = fn()
    b = eng.memo_stats()
    return out, tuple(int(b[k] - a[k]) for k in ("pairs_skipped", "pairs_packed", "pairs_full"))


def _scramble(eng, kernel, S, inp):
    """a search of other roots with other draws, memo off: other trees' nodes and latents at every workspace slot"""
    eng.set_memo_depth(0)
    _search(eng, kernel, S, inp, False)


def _off_on(eng, kernel, S, D, inp, deterministic, scramble):
    """the search without the memo and, over a scrambled workspace, with it at depth D: every output array equal
    byte for byte; returns the memo leg's outputs and its counted (skipped, packed, full) pairs"""
    eng.set_memo_depth(0)
    off, took_off = _counted(eng, lambda: _search(eng, kernel, S, inp, deterministic))
    assert took_off == (0, 0, 0)
    _scramble(eng, kernel, S, scramble)
    eng.set_memo_depth(D)
    on, took = _counted(eng, lambda: _search(eng, kernel, S, inp, deterministic))
    st = eng.memo_stats()
    assert st["depth"] == D and st["built"] == 1
    assert set(on) == set(off)
    for k in on:
        assert on[k].tobytes() == off[k].tobytes(), k  # the latent outputs and the carried MinMaxStats included
    return on, took


def _equals_oracle(oracle, n, S, inp, deterministic, flat, sup, on):
    obs, noise, tie, u, mm = inp
    ref = oracle.search(n, S, obs, flat=flat, support=sup, noise=noise, tie_idx=tie, action_u=u, temperature=1.0,
                        deterministic=deterministic, minmax_in=mm, depths=True)
    for k, rk in OUTPUTS:
        assert np.array_equal(on[k], ref[rk]), k
    assert np.array_equal(on["minmax"][:, 0], ref["mm_max"]) and np.array_equal(on["minmax"][:, 1], ref["mm_min"])
    return ref["depths"]


@pytest.mark.gpu
@pytest.mark.parametrize("k,place", FORCED)
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_forced_form_boundaries(oracle, eng3, kernel, k, place):
    rows = placed(k, place)
    assert len(rows) == k and all(0 <= r < 32 for r in rows)
    inp = inputs3(64, rows)
    want = predict_paths(np.ones((64, S3), np.int64), inp[0], D3, RPW[kernel])  # known before any search runs
    if kernel == "wave":  # the first wave's form at every simulation; the second wave never runs a chain
        form = 0 if k == 0 else 1 if k <= 16 else 2
        expect = [S3, 0, 0]
        expect[form] += S3
        assert want == tuple(expect)
    flat, sup = weights3(oracle)
    on, took = _off_on(eng3, kernel, S3, D3, inp, False, inputs3(64, (), seed=1))
    depths = _equals_oracle(oracle, N3, S3, inp, False, flat, sup, on)
    assert (np.asarray(depths) <= D3).all()
    print("paths (skipped, packed, full):", took, "predicted:", want)
    assert took == want == predict_paths(depths, inp[0], D3, RPW[kernel])


@pytest.mark.gpu
@pytest.mark.parametrize("B", [33, 40, 64])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("mode", ["noise", "minmax"])
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_mixed_depths_ragged_waves(oracle, eng4, kernel, mode, D, B):
    """stochastic, and deterministic with caller MinMaxStats; last waves of 1, 8 and 32 (16) valid roots"""
    inp, deterministic = case_inputs(mode, B)
    flat, sup = weights(oracle)
    on, took = _off_on(eng4, kernel, 16, D, inp, deterministic, scramble_inputs())
    depths = _equals_oracle(oracle, 4, 16, inp, deterministic, flat, sup, on)
    assert took == predict_paths(depths, inp[0], D, RPW[kernel])


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_mixed_rows(oracle, eng4, kernel):
    """rows that are no state's beside the goal state and equal roots, at depth 3"""
    inp = mixed_inputs()
    flat, sup = weights(oracle)
    on, took = _off_on(eng4, kernel, 16, 3, inp, False, scramble_inputs())
    depths = _equals_oracle(oracle, 4, 16, inp, False, flat, sup, on)
    assert took == predict_paths(depths, inp[0], 3, RPW[kernel])


ROOT_CASES = {"clean": (32, ()), "one_perturbed": (32, (7,)), "ragged": (41, ())}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(ROOT_CASES))
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_root_and_latents_equal_memo_off(oracle, eng3, kernel, case):
    """waves whose every root is a state (no root chain: priors from the table, htree slot 0 unwritten over a
    scrambled workspace), a wave with one root that is none (the root chains) and a ragged wave: every output, the
    latent outputs included, equals the search without the memo"""
    B, rows = ROOT_CASES[case]
    inp = inputs3(B, rows, seed=2)
    flat, sup = weights3(oracle)
    on, took = _off_on(eng3, kernel, 16, D3, inp, False, inputs3(64, (), seed=3))
    depths = _equals_oracle(oracle, N3, 16, inp, False, flat, sup, on)
    assert took == predict_paths(depths, inp[0], D3, RPW[kernel])


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_no_stale_row_after_load_weights(oracle, kernel):
    """other weights through load_weights: the next memo search equals the search without the memo, and the
    oracle, under the new weights"""
    from muzero_hanoi_amd import engine

    flat, sup = weights3(oracle)
    flat2, _ = weights3(oracle, other=True)
    inp = inputs3(40, (3,), seed=4)
    eng = engine.Engine(N3, 16, 64, sup)
    try:
        eng.load_weights(flat)
        eng.set_memo_depth(D3)
        first = _search(eng, kernel, 16, inp, False)
        assert eng.memo_stats()["built"] == 1
        eng.load_weights(flat2)
        assert eng.memo_stats()["built"] == 0
        after = _search(eng, kernel, 16, inp, False)  # the first search under the new weights, memo on
        assert eng.memo_stats()["built"] == 1
        on, took = _off_on(eng, kernel, 16, D3, inp, False, inputs3(64, (), seed=5))
        for k in on:
            assert after[k].tobytes() == on[k].tobytes(), k
        depths = _equals_oracle(oracle, N3, 16, inp, False, flat2, sup, on)
        assert took == predict_paths(depths, inp[0], D3, RPW[kernel])
        assert first["pi"].tobytes() != on["pi"].tobytes()  # the other weights do search other trees
    finally:
        eng.close()
