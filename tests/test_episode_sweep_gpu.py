"""Episodes of envs with their own budgets and discounts in one launch (mzh_play_episodes_sweep) against
mzh_play_episodes.

The reference side is always mzh_play_episodes on an engine holding one network alone, with args.n_sims the env's own
budget and args.discount its own discount, on the env's columns of the same [T][B] tables.  Both sides go through the C
ABI into guarded, sentinel-filled buffers (test_episode_set_gpu.Guarded), so equality of the whole arrays also shows
that rows at and beyond steps[b] were left unwritten.  Everything is compared bit for bit.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_episode_set_gpu import (KEYS, PLAY_KEYS, Guarded, bits, draw_table, flat, network, same, set_engine,
                                  states_of)
from test_episode_set_gpu import call as call_multi

pytestmark = pytest.mark.gpu


def power_table(S, temperature):
    """generate_play_policy's np.power over the visit counts 0..S (Engine.pow_table, also for an integer exponent)"""
    e = max(1.0, min(5.0, 1.0 / temperature))
    return torch.from_numpy(np.power(np.arange(S + 1, dtype=np.int64), e)).to("cuda")


def call(eng, S, states, draws, *, discount=0.8, minmax=None, net_index=None, n_networks=None, sims=None,
         discounts=None, temperature=1.0, deterministic=False, np1_ucb=False, pow_table="auto", expect=0):
    """mzh_play_episodes (net_index None) or mzh_play_episodes_sweep (sims given) through the C ABI into guarded
    buffers.  Returns (the outputs by field name + "err" + "status", the Guarded)."""
    from muzero_hanoi_amd import _lib

    noise, tie, u = draws
    T, B = (int(x) for x in tie.shape)
    n_disks = int(states.shape[1])
    g = Guarded(T, B, n_disks)
    a = _lib.EpisodeArgs()
    a.B, a.T, a.n_sims, a.goal_peg, a.max_steps = B, T, int(S), 2, T
    a.deterministic, a.flags = (1 if deterministic else 0), (_lib.MZH_FLAG_NP1_UCB if np1_ucb else 0)
    a.discount, a.eps, a.temperature = float(discount), 0.25, float(temperature)
    pt = eng.pow_table(S, float(temperature)) if isinstance(pow_table, str) else power_table(S, float(temperature))
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
        assert sims is None and discounts is None
        rc = _lib.lib().mzh_play_episodes(eng._h, ctypes.byref(a), eng._stream())
    else:
        ni = torch.as_tensor(net_index, dtype=torch.int32).to("cuda").contiguous()
        sd = torch.as_tensor(sims, dtype=torch.int32).to("cuda").contiguous()
        dd = None if discounts is None else torch.as_tensor(discounts, dtype=torch.float64).to("cuda").contiguous()
        keep += [ni, sd, dd]
        m = _lib.MultiArgs()
        m.n_networks, m.net_index, m.status = int(n_networks), ni.data_ptr(), g.view["status"].data_ptr()
        w = _lib.EpisodeSweepArgs()
        w.n_sims, w.discount = sd.data_ptr(), (None if dd is None else dd.data_ptr())
        rc = _lib.lib().mzh_play_episodes_sweep(eng._h, ctypes.byref(a), ctypes.byref(m), ctypes.byref(w), eng._stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.last_error())
    g.guards_intact()
    return g.view, g


def lone_engines(nets, n_disks, support, S, B):
    """an engine per network, holding it alone (sized for the largest budget: a call's own n_sims makes its plan)"""
    from muzero_hanoi_amd.engine import Engine

    engs = []
    for n in nets:
        engs.append(Engine(n_disks, S, B, support))
        engs[-1].load_weights(flat(n))
    return engs


def groups_of(net_index, sims, discounts):
    """the envs of each (network, budget, discount), in env order"""
    out = {}
    for b, key in enumerate(zip(net_index, sims, discounts)):
        out.setdefault(key, []).append(b)
    return out


def check_sweep(n_disks, support, S, T, starts, net_index, sims, n_nets, *, seed, discounts=None, minmax=None, eng=None,
                nets=None, lone=None, **kw):
    """one sweep launch of maximum S against one lone launch per (network, budget, discount)"""
    B = len(starts)
    assert len(net_index) == len(sims) == B and max(sims) <= S
    nets = nets or [network(n_disks, support, seed + 10 * m) for m in range(n_nets)]
    draws = draw_table(T, B, seed, deterministic=kw.get("deterministic", False))
    states = states_of(starts, n_disks)
    eng = eng or set_engine(nets, n_disks, support, S, B)
    got, _ = call(eng, S, states, draws, minmax=minmax, net_index=net_index, n_networks=n_nets, sims=sims,
                  discounts=discounts, **kw)
    assert got["status"].tolist() == [0, len(set(net_index))] and int(got["err"]) == 0
    lone = lone or lone_engines(nets, n_disks, support, S, B)
    per_env = [0.8] * B if discounts is None else list(discounts)
    for (m, s, d), cols in groups_of(net_index, sims, per_env).items():
        ct = torch.tensor(cols, device="cuda")
        sub = tuple(None if x is None else x.index_select(1, ct) for x in draws)
        want, _ = call(lone[m], s, states[ct], sub, discount=d, minmax=None if minmax is None else minmax[ct], **kw)
        assert int(want["err"]) == 0
        same(got, want, KEYS, f"network {m}, {s} simulations, discount {d}", cols)
    # rows at and beyond steps[b] keep the canary: `same` compared them with the lone launches' untouched rows, and
    # here directly
    steps = got["steps"].cpu().numpy()
    for b in range(B):
        for k in ("pi", "root_q", "action", "reward", "visits", "obs"):
            tail = got[k][int(steps[b]):, b]
            assert bool((tail == (-7 if tail.dtype != torch.uint8 else 249)).all()), (b, k)
    return got, eng, nets, lone


MAIN = dict(starts=[0, 5, 17, 13, 22, 9, 25], net_index=[0, 0, 0, 1, 1, 2, 2], sims=[8, 3, 8, 1, 5, 5, 2],
            discounts=[0.8, 0.9, 0.8, 0.5, 0.8, 0.97, 0.8])


def test_main_case_equals_lone_launches():
    """N=3, 33-bin heads, max_steps=12, B=7 on three random networks, budgets [8,3,8,1,5,5,2] of maximum 8 with their
    own discounts, stochastic with root noise, T=1"""
    got, _, _, _ = check_sweep(3, 33, 8, 12, MAIN["starts"], MAIN["net_index"], MAIN["sims"], 3, seed=1,
                               discounts=MAIN["discounts"])
    steps = got["steps"].cpu().numpy()
    assert (steps >= 1).all() and (steps <= 12).all()
    vis = got["visits"][0].sum(-1).cpu().tolist()  # the first move's visits are the env's own budget
    assert vis == MAIN["sims"]


def latent_limit():
    """the smallest n_sims whose latency-kernel plan keeps the latents in HBM (the non-LATL instantiation)"""
    from muzero_hanoi_amd import _lib

    kernel = lambda S: _lib.search_plan(33, 2, S, flags=_lib.MZH_FLAG_KERNEL_ONE, minmax_in=True)["kernel"]
    S = 1
    while kernel(S) == "mzh_search_one_kernel<true, true, true>":
        S += 1
        assert S < 4096
    assert kernel(S) == "mzh_search_one_kernel<true, true, false>" and S > 5
    return S


@pytest.mark.parametrize("case", ["discount_null", "deterministic_t0_budget0", "np1_ucb", "scalar_heads_n4",
                                  "carried_minmax", "t05_pow_table", "t04_pow_table", "latents_in_hbm"])
def test_variants(case):
    if case == "discount_null":  # every env under args.discount
        check_sweep(3, 33, 8, 6, [0, 5, 17, 13], [0, 0, 1, 1], [8, 2, 5, 8], 2, seed=2)
    elif case == "deterministic_t0_budget0":  # no noise, no action draw; a budget of 0 never selects
        check_sweep(3, 33, 6, 6, [0, 5, 17, 13, 22], [0, 0, 0, 1, 1], [6, 0, 3, 0, 4], 2, seed=3,
                    discounts=[0.8, 0.9, 0.7, 0.8, 0.95], deterministic=True, temperature=0.0)
    elif case == "np1_ucb":
        check_sweep(3, 33, 8, 6, [0, 13, 17, 25], [0, 1, 1, 2], [3, 8, 4, 6], 3, seed=4,
                    discounts=[0.8, 0.6, 0.9, 0.8], np1_ucb=True)
    elif case == "scalar_heads_n4":  # support 1
        check_sweep(4, 1, 6, 7, [0, 5, 40, 79, 53], [0, 0, 1, 1, 1], [6, 2, 4, 6, 1], 2, seed=5,
                    discounts=[0.8, 0.9, 0.8, 0.7, 0.8])
    elif case == "carried_minmax":
        mm = torch.tensor([[0.9, -0.3], [2.0, 0.1], [-float("inf"), float("inf")], [0.5, 0.5], [1.5, -1.0]],
                          dtype=torch.float64, device="cuda")
        check_sweep(3, 33, 8, 6, [0, 5, 17, 13, 22], [0, 0, 1, 1, 2], [8, 3, 8, 5, 2], 3, seed=6,
                    discounts=[0.8, 0.9, 0.8, 0.5, 0.97], minmax=mm)
    elif case == "t05_pow_table":  # a table of args.n_sims + 1 entries on either side (exponent 2: x * x in the kernel)
        check_sweep(3, 33, 8, 6, [0, 5, 17, 13], [0, 0, 1, 1], [8, 3, 5, 8], 2, seed=7, discounts=[0.8, 0.9, 0.8, 0.7],
                    temperature=0.5, pow_table="given")
    elif case == "t04_pow_table":  # exponent 2.5: the kernel reads the table, the sweep launch's longer than a twin's
        check_sweep(3, 33, 8, 6, [0, 5, 17, 13], [0, 0, 1, 1], [8, 3, 5, 8], 2, seed=8, discounts=[0.8, 0.9, 0.8, 0.7],
                    temperature=0.4)
    else:  # the sweep launch keeps every env's latents in HBM, the lone twin of budget 5 its own in LDS
        S = latent_limit()
        check_sweep(3, 33, S, 3, [0, 17, 8, 22], [0, 0, 1, 1], [5, S, S, 5], 2, seed=9, discounts=[0.8, 0.9, 0.8, 0.9])


def test_more_envs_than_workgroups():
    """B=260 on 256 workgroups, budgets cycling 1, 2, 3 inside two networks: workgroup w < 4 plays env w, then env
    256 + w under the other network with another budget (the weight reload and the budget read both run)"""
    B = 260
    net_index = [0] * 130 + [1] * 130
    sims = [1 + b % 3 for b in range(B)]
    discounts = [0.8 if b % 2 else 0.9 for b in range(B)]
    for w in range(B - 256):
        assert net_index[w] != net_index[256 + w] and sims[w] != sims[256 + w]
    starts = [(7 * b) % 26 for b in range(B)]
    check_sweep(3, 33, 3, 4, starts, net_index, sims, 2, seed=10, discounts=discounts)


def test_device_refusals():
    """a budget of -1 or args.n_sims + 1, and a bad net_index: status[0] = 1, no output byte written (err_count
    included); the engine plays afterwards"""
    nets = [network(3, 33, 70 + m) for m in range(3)]
    eng = set_engine(nets, 3, 33, 8, 7)
    draws = draw_table(6, 4, 11)
    states = states_of([0, 5, 17, 13], 3)
    ok_ni, ok_sims = [0, 1, 2, 2], [8, 3, 0, 5]
    for ni, n, sims in ((ok_ni, 3, [8, -1, 0, 5]), (ok_ni, 3, [8, 3, 0, 9]), (ok_ni, 3, [9, 9, 9, 9]),
                        ([0, 2, 1, 2], 3, ok_sims), ([0, 1, 2, 3], 3, ok_sims), ([-1, 0, 1, 2], 3, ok_sims)):
        for discounts in (None, [0.8, 0.9, 0.8, 0.7]):
            got, g = call(eng, 8, states, draws, net_index=ni, n_networks=n, sims=sims, discounts=discounts)
            assert got["status"].tolist() == [1, 0], (ni, sims)
            g.untouched(KEYS)
            assert int(got["err"]) == 0
            assert bool((g.full["err"][:64] == -7).all()) and bool((g.full["err"][65:] == -7).all())
    check_sweep(3, 33, 8, 12, MAIN["starts"], MAIN["net_index"], MAIN["sims"], 3, seed=12, discounts=MAIN["discounts"],
                eng=eng, nets=nets)


def test_equal_budgets_equal_the_set_launch():
    """every budget args.n_sims and discount NULL: the outputs of mzh_play_episodes_multi"""
    nets = [network(3, 33, 90 + m) for m in range(3)]
    eng = set_engine(nets, 3, 33, 8, 5)
    states, draws = states_of([0, 5, 17, 13, 22], 3), draw_table(6, 5, 13)
    ni = [0, 0, 1, 2, 2]
    _, want, _ = call_multi(eng, 8, states, draws, net_index=ni, n_networks=3)
    got, _ = call(eng, 8, states, draws, net_index=ni, n_networks=3, sims=[8] * 5)
    same(got, want, KEYS)
    assert got["status"].tolist() == want["status"].tolist() == [0, 3]


def test_python_surface():
    """BatchedSelfPlay(NetworkSet).play_episodes(net_index=, sims=, discounts=) returns play_episodes' dict and is, per
    env, BatchedSelfPlay(net, n_simulations=sims[b], discount=discounts[b]).play_episodes on the env's column"""
    from muzero_hanoi_amd.networks import NetworkSet
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay

    nets = [network(3, 33, 100 + m) for m in range(3)]
    nset, T, S = NetworkSet(nets), 12, 8
    starts, ni = [0, 5, 17, 13, 22, 9], [0, 0, 1, 2, 2, 2]
    sims, discounts = [8, 3, 5, 1, 8, 4], [0.8, 0.9, 0.8, 0.5, 0.97, 0.8]
    table = tuple(x.cpu().numpy() for x in draw_table(T, 6, 14, dev="cpu"))
    sp = BatchedSelfPlay(nset, 3, T, S)
    got = sp.play_episodes(starts, draws=table, net_index=ni, sims=sims, discounts=discounts)
    assert set(got) == set(PLAY_KEYS)
    for b in range(6):
        sl = slice(b, b + 1)
        want = BatchedSelfPlay(nets[ni[b]], 3, T, sims[b], discount=discounts[b]).play_episodes(
            starts[sl], draws=tuple(x[:, sl] for x in table))
        tw = want["action"].shape[0]  # the lone record is trimmed to its own episode
        for k in PLAY_KEYS:
            g = got[k][:tw, sl] if got[k].dim() >= 2 and k != "minmax" else got[k][sl]
            assert torch.equal(bits(g), bits(want[k])), (b, k)
        assert not bool(got["active"][tw:, sl].any())
    # sims alone plays under the play's discount, discounts alone with n_simulations for every env
    only_s = sp.play_episodes(starts, draws=table, net_index=ni, sims=sims)
    only_d = sp.play_episodes(starts, draws=table, net_index=ni, discounts=discounts)
    for b, (res, s, d) in enumerate([(only_s, sims[1], 0.8), (only_d, S, discounts[1])]):
        want = BatchedSelfPlay(nets[0], 3, T, s, discount=d).play_episodes(starts[1:2],
                                                                           draws=tuple(x[:, 1:2] for x in table))
        tw = want["action"].shape[0]
        for k in ("action", "pi", "root_q"):
            assert torch.equal(bits(res[k][:tw, 1:2]), bits(want[k])), (b, k)
    # without either, the set launch as before
    plain = sp.play_episodes(starts, draws=table, net_index=ni)
    full = sp.play_episodes(starts, draws=table, net_index=ni, sims=[S] * 6)
    for k in PLAY_KEYS:
        assert torch.equal(bits(plain[k]), bits(full[k])), k
