"""MuzeroPopulation(overrides=...): agents of different configurations trained abreast, every loop's episodes in one
mzh_play_episodes_sweep launch.  Every agent must end bit for bit as its lone Muzero(selfplay="device") run with its own
configuration ends: parameters, Adam moments and steps, the buffer's arrays, priorities and pointers, MinMaxStats,
tot_accuracy and its NumPy stream.  The env and the loop counts are test_population_equals_the_lone_runs'.
"""
import warnings

import numpy as np
import pytest
import torch

from test_episode_set_gpu import SEEDS, agent_snapshot, assert_same_agent, muzero_kwargs

pytestmark = pytest.mark.gpu

OVERRIDES = ({},
             dict(n_mcts_simulations=10, discount=0.9, dirichlet_alpha=0.5, lr=3e-4, n_TD_step=5),
             dict(n_mcts_simulations=5, batch_s=64, buffer_size=4096))
# what update="set" lets an agent set (its rounds share batch_s and n_update_x_loop)
SET_OVERRIDES = ({}, dict(n_mcts_simulations=10, discount=0.9, lr=3e-4), dict(n_mcts_simulations=5, discount=0.7))


def lone_runs(seeds, kw, overrides, n_loops):
    from muzero_hanoi_amd.muzero import Muzero

    out = []
    for s, over in zip(seeds, overrides):
        torch.manual_seed(s)
        mz = Muzero(selfplay="device", **{**kw, **over})
        np.random.seed(s)
        acc = mz.training_loop(n_loops=n_loops, min_replay_size=0, print_acc=2)
        out.append(agent_snapshot(mz, acc, np.random.get_state()))
    return out


def population_run(seeds, kw, overrides, n_loops, **pop_kw):
    from muzero_hanoi_amd.muzero import MuzeroPopulation

    np.random.seed(12345)
    before = np.random.get_state()
    pop = MuzeroPopulation(seeds, overrides=overrides, **pop_kw, **kw)
    accs = pop.training_loop(n_loops=n_loops, min_replay_size=0, print_acc=2)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:], \
        "the caller's global NumPy stream moved"
    return [agent_snapshot(a, acc, st) for a, acc, st in zip(pop.agents, accs, pop.streams)], pop


def assert_trained(want, seeds):
    for s, w in zip(seeds, want):
        assert w["buffer"][1][2] > 0, f"seed {s}: the lone run's buffer is empty: choose another seed"
        assert min(w["adam_steps"]) > 0, f"seed {s}: the lone run never updated: choose another seed"


@pytest.fixture(scope="module")
def sweep_calls():
    """counts the library's sweep and set launches of episodes (the calls go through _lib.lib()'s attributes)"""
    from muzero_hanoi_amd import _lib

    L = _lib.lib()
    counts = {"sweep": 0, "multi": 0}
    real = {"sweep": L.mzh_play_episodes_sweep, "multi": L.mzh_play_episodes_multi}

    def counted(name):
        def f(*a):
            counts[name] += 1
            return real[name](*a)
        return f

    L.mzh_play_episodes_sweep, L.mzh_play_episodes_multi = counted("sweep"), counted("multi")
    yield counts
    L.mzh_play_episodes_sweep, L.mzh_play_episodes_multi = real["sweep"], real["multi"]


@pytest.mark.parametrize("ingest", ["host", "device"])
def test_population_of_configurations_equals_the_lone_runs(ingest, sweep_calls):
    """three seeds with their own budgets, discounts, Dirichlet alpha, step size, n-step, batch and buffer sizes; four
    loops, an update in every loop whose buffer is not empty"""
    before = dict(sweep_calls)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # n_ep_x_loop = 1 is the parity schedule: no warning
        want = lone_runs(SEEDS, muzero_kwargs(ingest), OVERRIDES, 5)
        got, pop = population_run(SEEDS, muzero_kwargs(ingest), OVERRIDES, 5)
    assert sweep_calls["sweep"] - before["sweep"] == 4 and sweep_calls["multi"] == before["multi"]
    assert_trained(want, SEEDS)
    for s, g, w in zip(SEEDS, got, want):
        assert_same_agent(g, w, f"seed {s}")
    # the agents are what their overrides say
    a = pop.agents
    assert [int(x.mcts.n_simulations) for x in a] == [8, 10, 5] and [x.discount for x in a] == [0.8, 0.9, 0.8]
    assert [x.mcts.root_dirichlet_alpha for x in a] == [0.25, 0.5, 0.25] and [x.n_step for x in a] == [10, 5, 10]
    assert [x.batch_s for x in a] == [16, 16, 64] and [x.buffer.size for x in a] == [500, 500, 4096]
    assert [x.networks.optimiser.param_groups[0]["lr"] for x in a] == [0.002, 3e-4, 0.002]


def test_set_update_equals_its_each_twin():
    """update="set" with overrides of n_mcts_simulations, discount and lr only"""
    kw = muzero_kwargs("device")
    each, _ = population_run(SEEDS, kw, SET_OVERRIDES, 5, update="each")
    got, pop = population_run(SEEDS, kw, SET_OVERRIDES, 5, update="set")
    assert_trained(each, SEEDS)
    for s, g, w in zip(SEEDS, got, each):
        assert_same_agent(g, w, f"seed {s}")
    assert any(pop.active_history)


def test_two_episodes_per_loop():
    seeds, over = SEEDS[:2], OVERRIDES[:2]
    with pytest.warns(RuntimeWarning, match="selfplay='device'.*n_ep_x_loop > 1"):
        want = lone_runs(seeds, muzero_kwargs("device", 2), over, 4)
    with pytest.warns(RuntimeWarning, match="selfplay='device'.*n_ep_x_loop > 1"):
        got, _ = population_run(seeds, muzero_kwargs("device", 2), over, 4)
    assert_trained(want, seeds)
    for s, g, w in zip(seeds, got, want):
        assert_same_agent(g, w, f"seed {s}")


def test_empty_overrides_are_a_population_of_seeds(sweep_calls):
    """overrides=[{}, {}, {}] and overrides=None: the same launches (the set form, not the sweep form), the same agents"""
    kw = muzero_kwargs("device")
    before = dict(sweep_calls)
    none, _ = population_run(SEEDS, kw, None, 5)
    assert sweep_calls["sweep"] == before["sweep"] and sweep_calls["multi"] - before["multi"] == 4
    empty, _ = population_run(SEEDS, kw, [{}, {}, {}], 5)
    assert sweep_calls["sweep"] == before["sweep"] and sweep_calls["multi"] - before["multi"] == 8
    assert_trained(none, SEEDS)
    for s, g, w in zip(SEEDS, empty, none):
        assert_same_agent(g, w, f"seed {s}")
