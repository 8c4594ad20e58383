"""MuzeroPopulation(update="set"): the agents' update rounds as one launch sequence per loop.

Every agent of a "set" population must end bit for bit as its lone Muzero run ends and as its twin in an
update="each" population ends (tests/test_episode_set_gpu.py's configuration, snapshot and comparison): parameters,
Adam moments and step counters, the whole buffer with its priorities, MinMaxStats, tot_accuracy and the NumPy stream.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

from test_episode_set_gpu import agent_snapshot, assert_same_agent, bits, muzero_kwargs

pytestmark = pytest.mark.gpu

SEEDS = (3, 4, 5)
LOOPS = 5
# mixed activity: with this threshold these seeds' buffers cross it in different loops (asserted below)
MIXED_SEEDS, MIXED_MIN_REPLAY = (0, 8, 1), 2


def kwargs(ingest, n_update_x_loop=1):
    kw = muzero_kwargs(ingest)
    kw["n_update_x_loop"] = n_update_x_loop
    return kw


@functools.lru_cache(maxsize=None)
def lone_runs(seeds, ingest, n_update_x_loop, min_replay_size):
    from muzero_hanoi_amd.muzero import Muzero

    out = []
    for s in seeds:
        torch.manual_seed(s)
        mz = Muzero(selfplay="device", **kwargs(ingest, n_update_x_loop))
        np.random.seed(s)
        acc = mz.training_loop(n_loops=LOOPS, min_replay_size=min_replay_size, print_acc=2)
        out.append(agent_snapshot(mz, acc, np.random.get_state()))
    return out


def population_run(seeds, ingest, n_update_x_loop, min_replay_size, update):
    from muzero_hanoi_amd.muzero import MuzeroPopulation

    np.random.seed(12345)
    before = np.random.get_state()
    pop = MuzeroPopulation(seeds, update=update, **kwargs(ingest, n_update_x_loop))
    accs = pop.training_loop(n_loops=LOOPS, min_replay_size=min_replay_size, print_acc=2)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:], \
        "the caller's global NumPy stream moved"
    return pop, [agent_snapshot(a, acc, st) for a, acc, st in zip(pop.agents, accs, pop.streams)]


def check_identity(seeds, ingest, n_update_x_loop, min_replay_size):
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # n_ep_x_loop = 1 is the parity schedule: no warning
        want = lone_runs(seeds, ingest, n_update_x_loop, min_replay_size)
        _, each = population_run(seeds, ingest, n_update_x_loop, min_replay_size, "each")
        pop, got = population_run(seeds, ingest, n_update_x_loop, min_replay_size, "set")
    for s, g, e, w in zip(seeds, got, each, want):
        assert min(w["adam_steps"]) > 0, f"seed {s}: the lone run never updated: choose another seed"
        assert_same_agent(g, w, f"seed {s} against its lone run")
        assert_same_agent(g, e, f"seed {s} against its update='each' twin")
    return pop, want


@pytest.mark.parametrize("ingest", ["host", "device"])
def test_set_population_equals_lone_runs_and_each_twins(ingest):
    pop, want = check_identity(SEEDS, ingest, 1, 0)
    assert len(pop.active_history) == LOOPS - 1
    assert [len(a) for a in pop.active_history][-1] == len(SEEDS)
    for i in range(len(SEEDS)):
        for j in range(i + 1, len(SEEDS)):
            assert any(not torch.equal(a, b) for a, b in zip(want[i]["params"], want[j]["params"])), (i, j)


def test_two_rounds_per_loop():
    pop, want = check_identity(SEEDS, "device", 2, 0)
    for w, active_loops in zip(want, zip(*[[m in a for m in range(len(SEEDS))] for a in pop.active_history])):
        assert w["adam_steps"][0] == 2 * sum(active_loops)


def test_mixed_activity():
    """agents cross min_replay_size in different loops: in some loop the set call runs with inactive networks"""
    pop, _ = check_identity(MIXED_SEEDS, "device", 1, MIXED_MIN_REPLAY)
    M = len(MIXED_SEEDS)
    sizes = [len(a) for a in pop.active_history]
    assert any(0 < n < M for n in sizes), f"no loop with some but not all agents active ({pop.active_history}): " \
                                          "choose another seed or min_replay_size"
    assert set(m for a in pop.active_history for m in a) == set(range(M)), \
        f"an agent never updated ({pop.active_history}): choose another seed or min_replay_size"


def test_state_is_consistent_after_a_set_run():
    """after a "set" run a lone _update of agent 0 and a device refresh of the set's engine behave as after an
    "each" run: the transposed weights and the packed weight set are those of the live parameters"""
    from muzero_hanoi_amd.networks import NetworkSet, engine_for_set

    ends = {}
    for update in ("each", "set"):
        pop, _ = population_run(SEEDS, "device", 1, 0, update)
        a = pop.agents[0]
        np.random.seed(99)
        states, rwds, actions, pi, returns, indx, w = a.buffer.priority_sample(a.batch_s)
        newp, *_ = a._update(states, rwds, actions, pi, returns, w)
        a.buffer.update_priorities(indx, newp)
        fu = a._graphed
        for l, t in enumerate(fu.wt):  # no stale transposed copy
            W = fu.params[2 * l].detach()
            assert torch.equal(bits(t[:, :W.shape[0]]), bits(W.t())), (update, l)
        eng = engine_for_set(pop.networks, 8, 1, weights="device")
        blob = eng.debug_blob(2).clone()
        fresh = engine_for_set(NetworkSet([x.networks for x in pop.agents]), 8, 1, weights="host").debug_blob(2)
        assert torch.equal(bits(blob), bits(fresh)), f"{update}: the device refresh packed stale parameters"
        ends[update] = ([bits(p.detach()) for p in a.networks.parameters()], bits(blob),
                        np.array(a.buffer.priorities).view(np.uint32))
    for k, (x, y) in enumerate(zip(ends["set"][0], ends["each"][0])):
        assert torch.equal(x, y), k
    assert torch.equal(ends["set"][1], ends["each"][1])
    assert np.array_equal(ends["set"][2], ends["each"][2])
