"""Episodes of a network set in one launch (mzh_play_episodes_multi) against mzh_play_episodes.

The reference side is always mzh_play_episodes on an engine holding that one network, on the column slices of the
same [T][B] tables.  Both sides go through the C ABI into buffers of this file's own: every output lies between two
guard regions and is prefilled with a sentinel, so equality of the whole arrays also shows which rows were left
unwritten, and the guards show that nothing was written beside them.  Everything is compared bit for bit.
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -7  # 249 in a uint8 array
GUARD = 64  # elements on either side of an output
GOAL3 = 26  # state_index((2, 2, 2))
# the outputs of mzh_episode_args: field -> (dtype, shape after [T, B] or [B])
RECORD = (("pi", torch.float64, (6,)), ("root_q", torch.float64, ()), ("action", torch.int32, ()),
          ("reward", torch.int8, ()), ("visits", torch.int32, (6,)), ("obs", torch.float32, None))
PER_ENV = (("steps", torch.int32, ()), ("illegal", torch.int32, ()), ("solved", torch.uint8, ()),
           ("final_state", torch.uint8, None), ("minmax_out", torch.float64, (2,)))
KEYS = [k for k, _, _ in RECORD + PER_ENV]


def sentinel(dtype):
    return 249 if dtype == torch.uint8 else SENTINEL


def network(n_disks, support, seed):
    from muzero_hanoi_amd.networks import MuZeroNet

    torch.manual_seed(seed)
    return MuZeroNet(3 * n_disks, 6, 0.002, "cpu", TD_return=support == 33)


def flat(net):
    from muzero_hanoi_amd.engine import flat_weights

    return flat_weights(net.state_dict())


def draw_table(T, B, seed, *, deterministic=False, alpha=0.25, dev="cuda"):
    """(noise [T, B, 6] | None, tie [T, B], u [T, B] | None) on the device: row [t, b] for move t of env b"""
    from muzero_hanoi_amd import rng

    fl = rng.synthetic_draws(T * B, deterministic=deterministic, alpha=alpha, seed=seed)
    return tuple(None if x is None else torch.from_numpy(x).reshape((T, B) + x.shape[1:]).to(dev) for x in fl)


def columns(draws, cols):
    return tuple(None if x is None else x[:, cols].contiguous() for x in draws)


def states_of(start_idx, n_disks, dev="cuda"):
    idx = torch.as_tensor(start_idx, dtype=torch.int64)
    pw = 3 ** torch.arange(n_disks - 1, -1, -1)
    return ((idx[:, None] // pw) % 3).to(torch.uint8).to(dev)


def bits(t):
    """exact comparison of floating point tensors (NaN payloads and signed zeros included)"""
    t = t.contiguous()
    return t.view({torch.float64: torch.int64, torch.float32: torch.int32}.get(t.dtype, t.dtype)).cpu()


def same(got, want, keys, what="", cols=slice(None)):
    """got's envs `cols` equal want's envs (all of them)"""
    for k in keys:
        g = got[k][:, cols] if k in [r for r, _, _ in RECORD] else got[k][cols]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k)
        assert torch.equal(bits(g), bits(want[k])), (what, k)


class Guarded:
    """outputs of one call: each a view into a sentinel-filled buffer with GUARD elements before and after it"""

    def __init__(self, T, B, n_disks, dev="cuda"):
        self.full, self.view = {}, {}
        for group, lead in ((RECORD, (T, B)), (PER_ENV, (B,))):
            for k, dt, tail in group:
                shape = lead + ((3 * n_disks if group is RECORD else n_disks,) if tail is None else tail)
                n = int(np.prod(shape))
                self.full[k] = torch.full((n + 2 * GUARD,), sentinel(dt), dtype=dt, device=dev)
                self.view[k] = self.full[k][GUARD:GUARD + n].view(shape)
        self.full["err"] = torch.full((1 + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.view["err"] = self.full["err"][GUARD:GUARD + 1]
        self.view["err"].zero_()
        self.full["status"] = torch.full((2 + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.view["status"] = self.full["status"][GUARD:GUARD + 2]

    def guards_intact(self):
        for k, f in self.full.items():
            s = sentinel(f.dtype)
            assert bool((f[:GUARD] == s).all()) and bool((f[-GUARD:] == s).all()), k

    def untouched(self, keys):
        for k in keys:
            assert bool((self.full[k] == sentinel(self.full[k].dtype)).all()), k


def call(eng, S, states, draws, *, max_steps=None, minmax=None, net_index=None, n_networks=None, temperature=1.0,
         deterministic=False, np1_ucb=False, expect=0):
    """mzh_play_episodes (net_index None) or mzh_play_episodes_multi through the C ABI into guarded buffers.
    Returns (status code, the outputs by field name + "err" + "status", the Guarded)."""
    from muzero_hanoi_amd import _lib

    noise, tie, u = draws
    T, B = (int(x) for x in tie.shape)
    n_disks = int(states.shape[1])
    g = Guarded(T, B, n_disks)
    a = _lib.EpisodeArgs()
    a.B, a.T, a.n_sims, a.goal_peg, a.max_steps = B, T, int(S), 2, int(T if max_steps is None else max_steps)
    a.deterministic, a.flags = (1 if deterministic else 0), (_lib.MZH_FLAG_NP1_UCB if np1_ucb else 0)
    a.discount, a.eps, a.temperature = 0.8, 0.25, float(temperature)
    pt = eng.pow_table(S, float(temperature))
    keep = [states.contiguous(), tie.contiguous()]
    a.state, a.tie_idx = keep[0].data_ptr(), keep[1].data_ptr()
    for name, t in (("noise", noise), ("action_u", u), ("minmax_in", minmax), ("pow_table", pt)):
        if t is not None:
            keep.append(t.contiguous())
            setattr(a, name, keep[-1].data_ptr())
    for k in KEYS:
        setattr(a, k, g.view[k].data_ptr())
    a.err_count = g.view["err"].data_ptr()
    if net_index is None:
        rc = _lib.lib().mzh_play_episodes(eng._h, ctypes.byref(a), eng._stream())
    else:
        ni = torch.as_tensor(net_index, dtype=torch.int32).to("cuda").contiguous()
        keep.append(ni)
        m = _lib.MultiArgs()
        m.n_networks, m.net_index, m.status = int(n_networks), ni.data_ptr(), g.view["status"].data_ptr()
        rc = _lib.lib().mzh_play_episodes_multi(eng._h, ctypes.byref(a), ctypes.byref(m), eng._stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.last_error())
    g.guards_intact()
    return rc, g.view, g


def lone_engine(net, n_disks, support, S, B):
    from muzero_hanoi_amd.engine import Engine

    eng = Engine(n_disks, S, B, support)
    eng.load_weights(flat(net))
    return eng


def set_engine(nets, n_disks, support, S, B):
    from muzero_hanoi_amd.engine import Engine

    eng = Engine(n_disks, S, B, support)
    eng.load_weight_set([flat(n) for n in nets])
    return eng


def check_set(n_disks, support, S, T, starts, net_index, n_nets, *, seed, minmax=None, eng=None, nets=None, **kw):
    """one set launch against one lone launch per network that has envs"""
    B = len(starts)
    nets = nets or [network(n_disks, support, seed + 10 * m) for m in range(n_nets)]
    draws = draw_table(T, B, seed, deterministic=kw.get("deterministic", False))
    states = states_of(starts, n_disks)
    eng = eng or set_engine(nets, n_disks, support, S, B)
    _, got, _ = call(eng, S, states, draws, minmax=minmax, net_index=net_index, n_networks=n_nets, **kw)
    assert got["status"].tolist() == [0, len(set(net_index))] and int(got["err"]) == 0
    ni = np.asarray(net_index)
    for m in sorted(set(net_index)):
        cols = np.nonzero(ni == m)[0]
        sl = slice(int(cols[0]), int(cols[-1]) + 1)
        lone = lone_engine(nets[m], n_disks, support, S, len(cols))
        _, want, _ = call(lone, S, states[sl], columns(draws, sl), minmax=None if minmax is None else minmax[sl], **kw)
        assert int(want["err"]) == 0
        same(got, want, KEYS, f"network {m}", sl)
        lone.close()
    return got, eng, nets, draws


def test_main_case_equals_three_lone_launches():
    """N=3, S=8, max_steps=12, three random 33-bin networks, B=7 with net_index [0,0,0,1,1,2,2], non-goal starts,
    temperature 1 with noise, carried-in MinMaxStats"""
    starts = [0, 5, 17, 13, 22, 9, 25]
    mm = torch.tensor([[0.9, -0.3], [2.0, 0.1], [-float("inf"), float("inf")], [0.5, 0.5], [1.5, -1.0], [0.2, 0.0],
                       [3.0, -2.0]], dtype=torch.float64, device="cuda")
    got, _, _, _ = check_set(3, 33, 8, 12, starts, [0, 0, 0, 1, 1, 2, 2], 3, seed=1, minmax=mm)
    steps = got["steps"].cpu().numpy()
    assert (steps >= 1).all() and (steps <= 12).all()
    # the three networks do play differently: the same start under each would otherwise hide a wrong network
    a = got["pi"]
    assert not torch.equal(a[0, 0], a[0, 3]) and not torch.equal(a[0, 3], a[0, 5])


def test_a_network_without_envs():
    check_set(3, 33, 8, 6, [3, 17, 11, 20], [0, 0, 2, 2], 3, seed=2)


@pytest.mark.parametrize("case", ["scalar_heads_n4_deterministic", "np1_ucb", "latents_in_hbm"])
def test_variants(case):
    if case == "scalar_heads_n4_deterministic":  # support 1, no noise, no action draw
        check_set(4, 1, 6, 7, [0, 5, 40, 79, 53], [0, 0, 1, 1, 1], 2, seed=3, deterministic=True)
    elif case == "np1_ucb":
        check_set(3, 33, 8, 6, [0, 13, 17, 25], [0, 1, 1, 2], 3, seed=4, np1_ucb=True)
    else:  # an n_sims just above the LDS-resident latent limit, from the plan query
        from muzero_hanoi_amd import _lib

        smem = lambda S: _lib.search_plan(33, 2, S, flags=_lib.MZH_FLAG_KERNEL_ONE, minmax_in=True)["smem_bytes"]
        S = 1
        while smem(S + 1) > smem(S):
            S += 1
            assert S < 4096
        check_set(3, 33, S + 1, 3, [0, 17, 8], [0, 1, 1], 2, seed=5)


def test_two_networks_in_one_workgroup():
    """B=258 on 256 workgroups, the first 129 envs on network 0: workgroups 0 and 1 play env 0 / 1 under network 0
    and env 256 / 257 under network 1, so the weight reload runs"""
    B = 258
    starts = [(7 * b) % 26 for b in range(B)]
    check_set(3, 33, 4, 6, starts, [0] * 129 + [1] * 129, 2, seed=6)


def test_device_refusals():
    """a decreasing net_index, an entry equal to n_networks: status[0] = 1 and no output byte written"""
    nets = [network(3, 33, 70 + m) for m in range(3)]
    eng = set_engine(nets, 3, 33, 8, 4)
    draws = draw_table(6, 4, 7)
    states = states_of([0, 5, 17, 13], 3)
    for ni, n in (([0, 2, 1, 2], 3), ([0, 1, 2, 3], 3), ([0, 0, 1, 2], 2), ([-1, 0, 1, 2], 3)):
        _, got, g = call(eng, 8, states, draws, net_index=ni, n_networks=n)
        assert got["status"].tolist() == [1, 0], ni
        g.untouched(KEYS)
        assert int(got["err"]) == 0
    # and the engine still plays afterwards
    check_set(3, 33, 8, 6, [0, 5, 17, 13], [0, 1, 2, 2], 3, seed=7, eng=eng, nets=nets)


def test_host_refusals_that_need_an_engine():
    from muzero_hanoi_amd import _lib
    from muzero_hanoi_amd.engine import Engine

    eng = Engine(3, 8, 4, 33)
    draws = draw_table(6, 2, 8)
    states = states_of([0, 5], 3)
    kw = dict(net_index=[0, 1], n_networks=2)
    _, _, g = call(eng, 8, states, draws, expect=_lib.MZH_ERR_STATE, **kw)
    assert "no weight set loaded" in _lib.last_error()
    g.untouched(KEYS)
    eng.load_weights(flat(network(3, 33, 80)))  # the single network is not what the call needs
    call(eng, 8, states, draws, expect=_lib.MZH_ERR_STATE, **kw)
    eng.load_weight_set([flat(network(3, 33, 80 + m)) for m in range(2)])
    call(eng, 8, states, draws, net_index=[0, 1], n_networks=3, expect=_lib.MZH_ERR_ARG)
    assert "n_networks=3 outside [1, 2], the loaded set" in _lib.last_error()
    call(eng, 8, states_of([0] * 5, 3), draw_table(6, 5, 8), net_index=[0] * 5, n_networks=2,
         expect=_lib.MZH_ERR_CAPACITY)
    assert "B=5 > max_roots=4" in _lib.last_error()
    call(eng, 8, states, draws, max_steps=7, expect=_lib.MZH_ERR_ARG, **kw)
    assert "T=6 rows cannot hold max_steps=7" in _lib.last_error()
    call(eng, 9, states, draws, expect=_lib.MZH_ERR_CAPACITY, **kw)
    assert "n_sims=9 > max_sims=8" in _lib.last_error()
    # the Python surface says the first of these itself
    with pytest.raises(RuntimeError, match="no weight set loaded"):
        Engine(3, 8, 4, 33).play_episodes(8, states, 6, tie_idx=draws[1], deterministic=True,
                                          net_index=torch.tensor([0, 1]))
    _, got, _ = call(eng, 8, states, draws, **kw)  # and in order, it plays
    assert got["status"].tolist() == [0, 2]


def test_after_a_device_repack():
    """load_weight_set_from of changed parameters gives what load_weight_set of the same values gives"""
    nets = [network(3, 33, 90 + m).to("cuda") for m in range(3)]
    with torch.no_grad():  # the live parameters move away from what any earlier load saw
        for n in nets:
            for p in n.parameters():
                p.mul_(1.25).add_(0.01)
    states, draws = states_of([0, 5, 17, 13, 22], 3), draw_table(6, 5, 9)
    kw = dict(net_index=[0, 0, 1, 2, 2], n_networks=3)
    host = set_engine(nets, 3, 33, 8, 5)
    _, want, _ = call(host, 8, states, draws, **kw)
    dev = set_engine([network(3, 33, 1), network(3, 33, 2), network(3, 33, 3)], 3, 33, 8, 5)  # other weights first
    dev.load_weight_set_from([n.state_dict() for n in nets])
    _, got, _ = call(dev, 8, states, draws, **kw)
    same(got, want, KEYS)
    assert got["status"].tolist() == [0, 3]


PLAY_KEYS = ("action", "reward", "pi", "root_q", "active", "obs", "steps", "illegal", "start_idx", "minmax")


def test_python_surface():
    """BatchedSelfPlay(NetworkSet).play_episodes(net_index=...) is, per network, BatchedSelfPlay(net).play_episodes
    on the sliced table; evaluate_networks(launch="episodes") scores those dicts"""
    from muzero_hanoi_amd.networks import NetworkSet
    from muzero_hanoi_amd import rng
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay, _batch_starts, _new_score, _score_budget, evaluate_networks

    nets = [network(3, 33, 100 + m) for m in range(3)]
    nset, T, S = NetworkSet(nets), 12, 8
    starts, ni = [0, 5, 17, 13, 22, 9], [0, 0, 1, 2, 2, 2]
    table = tuple(x.cpu().numpy() for x in draw_table(T, 6, 10, dev="cpu"))
    got = BatchedSelfPlay(nset, 3, T, S).play_episodes(starts, draws=table, net_index=ni)
    assert set(got) == set(PLAY_KEYS)
    for m, sl in enumerate((slice(0, 2), slice(2, 3), slice(3, 6))):
        want = BatchedSelfPlay(nets[m], 3, T, S).play_episodes(starts[sl], draws=tuple(x[:, sl] for x in table))
        tw = want["action"].shape[0]  # the lone record is trimmed to its own longest episode
        for k in PLAY_KEYS:
            g = got[k][:tw, sl] if got[k].dim() >= 2 and k != "minmax" else got[k][sl]
            assert torch.equal(bits(g), bits(want[k])), (m, k)
        assert not bool(got["active"][tw:, sl].any())
    # evaluate_networks: the batch of a budget is starts tiled over the networks, one synthetic table from `seed`
    E, seed = 4, 3
    res = evaluate_networks(nset, 3, [S], episodes=E, max_steps=T, seed=seed, launch="episodes")
    st = _batch_starts(3, E, None, None, seed, 2)
    fl = rng.synthetic_draws(T * 3 * E, deterministic=False, alpha=0.25, eps=0.25, seed=seed)
    table = tuple(x.reshape((T, 3 * E) + x.shape[1:]) for x in fl)
    for m in range(3):
        sl = slice(m * E, (m + 1) * E)
        lone = BatchedSelfPlay(nets[m], 3, T, S).play_episodes(st, draws=tuple(x[:, sl] for x in table))
        sc = _new_score()
        _score_budget(sc, S, 3, 2, st, lone["steps"].cpu().numpy(), lone["illegal"].cpu().numpy())
        for k, v in sc.items():
            assert np.array_equal(np.asarray(res[m][k]), np.asarray(v)), (m, k)
    # a batch above max_roots is still sliced
    sliced = evaluate_networks(nset, 3, [S], episodes=E, max_steps=T, seed=seed, launch="episodes", max_roots=5)
    assert len(sliced) == 3 and all(len(s["steps"][0]) == E for s in sliced)


def buffer_snapshot(buf):
    raw = lambda x: np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.int64)
    arrays = [t.cpu().numpy() for t in (buf.states, buf.rwds, buf.actions, buf.pi_probs, buf.mc_returns)]
    arrays.append(np.array(buf.priorities, np.float32))
    return [raw(x) for x in arrays], (buf.ptr, buf.is_full, len(buf))


def agent_snapshot(mz, tot_accuracy, stream):
    opt = mz.networks.optimiser
    params = [bits(p.detach()) for p in mz.networks.parameters()]
    moments = [bits(opt.state[p][k]) for p in mz.networks.parameters() for k in ("exp_avg", "exp_avg_sq")]
    adam_steps = [float(opt.state[p]["step"]) for p in mz.networks.parameters()]
    mm = mz.mcts.min_max_stats
    return dict(params=params, moments=moments, adam_steps=adam_steps, buffer=buffer_snapshot(mz.buffer),
                minmax=(mm.maximum, mm.minimum), tot_accuracy=list(tot_accuracy), stream=stream)


def assert_same_agent(got, want, who):
    for k in ("params", "moments"):
        assert len(got[k]) == len(want[k])
        for i, (g, w) in enumerate(zip(got[k], want[k])):
            assert torch.equal(g, w), (who, k, i)
    assert got["adam_steps"] == want["adam_steps"], who
    (ga, gs), (wa, ws) = got["buffer"], want["buffer"]
    assert gs == ws, (who, gs, ws)
    for name, g, w in zip(("states", "rwds", "actions", "pi_probs", "mc_returns", "priorities"), ga, wa):
        assert np.array_equal(g, w), (who, name)
    assert got["minmax"] == want["minmax"], who
    assert got["tot_accuracy"] == want["tot_accuracy"], who
    g, w = got["stream"], want["stream"]
    assert g[0] == w[0] and np.array_equal(g[1], w[1]) and g[2:] == w[2:], who


def muzero_kwargs(ingest, n_ep_x_loop=1):
    from muzero_hanoi_amd.env import TowersOfHanoi

    env = TowersOfHanoi(N=3, max_steps=12, init_state_idx=17)  # (1, 2, 2): one move from the goal
    return dict(env=env, s_space_size=9, n_action=6, discount=0.8, dirichlet_alpha=0.25, n_mcts_simulations=8,
                unroll_n_steps=5, batch_s=16, TD_return=True, n_TD_step=10, lr=0.002, buffer_size=500,
                priority_replay=True, device="cuda", n_ep_x_loop=n_ep_x_loop, update_impl="fused", ingest=ingest)


def lone_runs(seeds, kw, n_loops):
    from muzero_hanoi_amd.muzero import Muzero

    out = []
    for s in seeds:
        torch.manual_seed(s)
        mz = Muzero(selfplay="device", **kw)
        np.random.seed(s)
        acc = mz.training_loop(n_loops=n_loops, min_replay_size=0, print_acc=2)
        out.append(agent_snapshot(mz, acc, np.random.get_state()))
    return out


def population_run(seeds, kw, n_loops):
    from muzero_hanoi_amd.muzero import MuzeroPopulation

    np.random.seed(12345)
    before = np.random.get_state()
    pop = MuzeroPopulation(seeds, **kw)
    accs = pop.training_loop(n_loops=n_loops, min_replay_size=0, print_acc=2)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:], \
        "the caller's global NumPy stream moved"
    return [agent_snapshot(a, acc, st) for a, acc, st in zip(pop.agents, accs, pop.streams)]


SEEDS = (3, 4, 5)


@pytest.mark.parametrize("ingest", ["host", "device"])
def test_population_equals_the_lone_runs(ingest):
    """three seeds, four loops, an update in every loop whose buffer is not empty: every agent of the population
    ends as its lone run ends"""
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # n_ep_x_loop = 1 is the parity schedule: no warning
        want = lone_runs(SEEDS, muzero_kwargs(ingest), 5)
        got = population_run(SEEDS, muzero_kwargs(ingest), 5)
    for s, g, w in zip(SEEDS, got, want):
        assert w["buffer"][1][2] > 0, f"seed {s}: the lone run's buffer is empty: choose another seed"
        assert min(w["adam_steps"]) > 0, f"seed {s}: the lone run never updated: choose another seed"
        assert_same_agent(g, w, f"seed {s}")
    for i in range(len(SEEDS)):
        for j in range(i + 1, len(SEEDS)):
            assert any(not torch.equal(a, b) for a, b in zip(want[i]["params"], want[j]["params"])), (i, j)


def test_population_with_two_episodes_per_loop():
    seeds = SEEDS[:2]
    with pytest.warns(RuntimeWarning, match="selfplay='device'.*n_ep_x_loop > 1"):
        want = lone_runs(seeds, muzero_kwargs("device", 2), 4)
    with pytest.warns(RuntimeWarning, match="selfplay='device'.*n_ep_x_loop > 1"):
        got = population_run(seeds, muzero_kwargs("device", 2), 4)
    for s, g, w in zip(seeds, got, want):
        assert w["buffer"][1][2] > 0 and min(w["adam_steps"]) > 0, f"seed {s}: choose another seed"
        assert_same_agent(g, w, f"seed {s}")
