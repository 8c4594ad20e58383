"""The expansion memo's host side (include/mzh.h): node numbering, table size and the automatic depth's budget
arithmetic -- and the inputs of tests/test_memo_gpu.py, with the oracle's prediction of which M-phase form each
(wave, simulation) pair takes, checked here to reach all three forms without a GPU.
"""
import itertools

import numpy as np
import pytest

from conftest import GOLDEN

N, S = 4, 16
CASE_MODES = ("noise", "deterministic", "minmax")
# tests/test_memo_gpu.py's mixed batch (64 roots = two 32-root waves): rows that are no state's observation sit in
# the first wave only, so the second can still skip; the goal state and a run of equal roots sit in both
MIXED = {"perturbed": (5, 6, 20), "goal": (0, 33), "equal": (10, 11, 12, 13, 40, 41)}


def weights(oracle):
    w, in_dim, sup = oracle.load_weights_npz(f"{GOLDEN}/weights_N4_s0.npz")
    return oracle.flat_weights(w), sup


def invalidation_weights(oracle):
    """the golden weights with another policy and value head (scaled output layers): other priors, other trees"""
    w, in_dim, sup = oracle.load_weights_npz(f"{GOLDEN}/weights_N4_s0.npz")
    w = {k: v.copy() for k, v in w.items()}
    w["policy_net.2.weight"] *= np.float32(-3.0)
    w["value_net.2.weight"] *= np.float32(1.5)
    w["dynamic_net.2.bias"] += np.float32(0.125)
    return oracle.flat_weights(w)


def _states_obs(st):
    B = len(st)
    obs = np.zeros((B, 3 * N), np.float32)
    obs[np.arange(B)[:, None], np.arange(N) * 3 + st] = 1
    return obs


DUP = 20  # the first DUP roots of a search case are one root (equal trees): more than 16 of a wave miss together


def case_inputs(mode, B):
    """(obs, noise, tie, u, minmax_in), deterministic of a search case: B one-hot roots (the first B of 64).  The
    first DUP are copies of root 0 with its draws and bounds, so they walk equal trees and miss in the same
    simulations; the others are random states"""
    from muzero_hanoi_amd import rng

    deterministic = mode != "noise"
    st = np.random.RandomState(41).randint(0, 3, (64, N))[:B]
    noise, tie, u = rng.synthetic_draws(B, deterministic=deterministic, alpha=0.25, seed=900)
    mm = None
    if mode == "minmax":  # caller-given MinMaxStats bounds: fresh, finite, equal and spread pairs
        pairs = np.array([[-np.inf, np.inf], [0.4, -0.2], [0.05, 0.05], [1.5, 0.0], [0.0, -1.0]], np.float64)
        mm = pairs[np.arange(B) % len(pairs)]
    for x in (st, noise, tie, u, mm):
        if x is not None:
            x[:DUP] = x[0]
    return (_states_obs(st), noise, tie, u, mm), deterministic


def scramble_inputs():
    """64 other one-hot roots with other draws: what tests/test_memo_gpu.py searches between a case's legs"""
    from muzero_hanoi_amd import rng

    st = np.random.RandomState(977).randint(0, 3, (64, N))
    noise, tie, u = rng.synthetic_draws(64, deterministic=False, alpha=0.25, seed=978)
    return _states_obs(st), noise, tie, u, None


def mixed_inputs():
    from muzero_hanoi_amd import rng

    st = np.random.RandomState(43).randint(0, 3, (64, N))
    st[list(MIXED["goal"])] = 2
    st[list(MIXED["equal"])] = st[MIXED["equal"][0]]
    obs = _states_obs(st)
    a, b, c = MIXED["perturbed"]
    obs[a, 4] += np.float32(0.25)           # a fourth non-zero entry
    obs[b, np.argmax(obs[b, :3])] = np.float32(1.0 - 2.0 ** -24)  # one ulp below 1
    obs[c, 3:6] = (1.0, 1.0, 0.0)           # two ones on one disc
    noise, tie, u = rng.synthetic_draws(64, deterministic=False, alpha=0.25, seed=901)
    return obs, noise, tie, u, None


def onehot_rows(obs):
    """rows whose every disc has exactly one 1.0 and two +0.0, by bit pattern (what the kernel accepts)"""
    bits = np.ascontiguousarray(obs, np.float32).view(np.uint32).reshape(len(obs), -1, 3)
    one = np.float32(1.0).view(np.uint32)
    return (((bits == one).sum(2) == 1) & ((bits == 0).sum(2) == 2)).all(1)


def predict_paths(depths, obs, D, roots_per_wave):
    """(skipped, packed, full) (wave, simulation) pairs of a search: a root misses where its row is no state's or
    the simulation's new node lies deeper than D; a wave runs no M phase when none misses, the packed tile when
    1..16 of a 32-root wave miss, else its own tiles"""
    miss = (~onehot_rows(obs))[:, None] | (np.asarray(depths) > D)
    took = [0, 0, 0]
    for w0 in range(0, len(obs), roots_per_wave):
        nm = miss[w0:w0 + roots_per_wave].sum(0)
        for n in nm:
            took[0 if n == 0 else 1 if (roots_per_wave == 32 and n <= 16) else 2] += 1
    return tuple(took)


def test_node_numbering():
    from muzero_hanoi_amd import engine

    assert engine.memo_node_id(()) == 0
    assert [engine.memo_node_id((a,)) for a in range(6)] == [1, 2, 3, 4, 5, 6]
    assert engine.memo_node_id((0, 0)) == 7 and engine.memo_node_id((5, 5)) == 42
    for D in range(4):
        ids = sorted(engine.memo_node_id(p) for d in range(D + 1) for p in itertools.product(range(6), repeat=d))
        assert ids == list(range(engine.memo_nodes(D)))  # a bijection onto 0..K(D)-1, level after level
        first = engine.memo_nodes(D - 1) if D else 0
        assert min(engine.memo_node_id(p) for p in itertools.product(range(6), repeat=D)) == first
    assert [engine.memo_nodes(D) for D in range(6)] == [1, 7, 43, 259, 1555, 9331]
    assert engine.memo_state_index((2, 2, 2, 2)) == 80 and engine.memo_state_index((1, 0, 2)) == 19
    with pytest.raises(ValueError):
        engine.memo_node_id((6,))


def test_table_size_and_budget():
    from muzero_hanoi_amd import _lib, build, engine

    build.build()
    for n, d in ((4, 4), (4, 5), (7, 2), (3, 3), (1, 1)):
        pl = _lib.memo_plan(n, d)
        assert pl == {"depth": d, "rows": 3 ** n * engine.memo_nodes(d), "bytes": 288 * 3 ** n * engine.memo_nodes(d)}
    assert _lib.memo_plan(4, 0) == {"depth": 0, "rows": 0, "bytes": 0}
    budget = 256 << 20
    for n in range(1, 17):  # automatic: the deepest table within the budget (none where one level is too much)
        pl = _lib.memo_plan(n, -1)
        d = pl["depth"]
        assert 0 <= d <= 12
        assert d == 0 or pl["bytes"] <= budget
        assert d == 12 or 288 * 3 ** n * engine.memo_nodes(d + 1) > budget
    assert _lib.memo_plan(4, -1)["depth"] == 5 and _lib.memo_plan(7, -1)["depth"] == 3
    assert _lib.memo_plan(16, -1)["depth"] == 0
    with pytest.raises(ValueError):
        _lib.memo_plan(4, -2)
    with pytest.raises(ValueError):
        _lib.memo_plan(4, 13)
    with pytest.raises(RuntimeError, match="rows"):
        _lib.memo_plan(7, 7)  # a forced depth beyond 2^26 rows


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("B", [40, 64])
@pytest.mark.parametrize("mode", CASE_MODES)
def test_gpu_cases_reach_all_three_paths(oracle, mode, B, D):
    """the oracle's selection depths of tests/test_memo_gpu.py's inputs: 32-root waves take every form, 16-root
    waves the skip and the full one"""
    (obs, noise, tie, u, mm), deterministic = case_inputs(mode, B)
    flat, sup = weights(oracle)
    dep = oracle.search(N, S, obs, flat=flat, support=sup, noise=noise, tie_idx=tie, action_u=u, temperature=1.0,
                        deterministic=deterministic, minmax_in=mm, depths=True)["depths"]
    w32, w16 = predict_paths(dep, obs, D, 32), predict_paths(dep, obs, D, 16)
    print(mode, B, D, w32, w16)
    assert min(w32) >= 1 and sum(w32) == S * -(-B // 32)
    assert w16[0] >= 1 and w16[1] == 0 and w16[2] >= 1 and sum(w16) == S * -(-B // 16)


def test_mixed_case_reaches_all_three_paths(oracle):
    obs, noise, tie, u, mm = mixed_inputs()
    assert (~onehot_rows(obs)).nonzero()[0].tolist() == sorted(MIXED["perturbed"])
    flat, sup = weights(oracle)
    dep = oracle.search(N, S, obs, flat=flat, support=sup, noise=noise, tie_idx=tie, action_u=u, temperature=1.0,
                        deterministic=False, depths=True)["depths"]
    w32, w16 = predict_paths(dep, obs, 2, 32), predict_paths(dep, obs, 2, 16)
    print(w32, w16)
    assert min(w32) >= 1 and w16[0] >= 1 and w16[2] >= 1
