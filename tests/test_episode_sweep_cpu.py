"""Episodes of agents of different configurations in one launch (mzh_play_episodes_sweep, Engine /
BatchedSelfPlay.play_episodes with sims / discounts, MuzeroPopulation(overrides=...)): what holds without a GPU -- the
symbol and its struct, every refusal the library makes before it touches an engine or a device, and the Python
surface's argument errors.
"""
import ctypes

import pytest

from test_abi_cpu import _c_offsets, declared_symbols, lib  # noqa: F401  (lib: the built library's fixture)
from test_episode_set_cpu import MUZERO_KW, REQUIRED, _net, _valid_args, _valid_multi


def test_symbol_is_declared_and_exported(lib):
    assert "mzh_play_episodes_sweep" in declared_symbols()
    assert hasattr(lib.lib(), "mzh_play_episodes_sweep")
    assert "mzh_play_episodes_sweep" in lib.SIGNATURES


def test_abi_version_stays_6(lib):
    assert lib.lib().mzh_abi_version() == lib.ABI_VERSION == 6


def test_sweep_args_layout_matches_header(lib, tmp_path):
    """ctypes EpisodeSweepArgs == struct mzh_episode_sweep_args as the C compiler lays out include/mzh.h"""
    fields = [f[0] for f in lib.EpisodeSweepArgs._fields_]
    assert fields == ["n_sims", "discount"]
    want = [getattr(lib.EpisodeSweepArgs, f).offset for f in fields] + [ctypes.sizeof(lib.EpisodeSweepArgs)]
    assert _c_offsets("mzh_episode_sweep_args", fields, tmp_path) == want


def _valid_sweep(lib):
    w = lib.EpisodeSweepArgs()
    w.n_sims, w.discount = 0x1000, 0x1000
    return w


def _refused(lib, a, m, w, status, text):
    """the call on a NULL engine and stream: the refusal must come before either is used"""
    ref = lambda x: None if x is None else ctypes.byref(x)
    got = lib.lib().mzh_play_episodes_sweep(None, ref(a), ref(m), ref(w), None)
    assert got == status, (text, got, lib.last_error())
    assert text in lib.last_error(), (text, lib.last_error())


def test_engine_free_refusals_in_order(lib):
    """mzh_play_episodes_multi's engine-free refusals first (with a valid, a NULL and a half-empty sweep block), then
    the sweep block's own, then the engine"""
    half = _valid_sweep(lib)
    half.n_sims = None
    for w in (_valid_sweep(lib), None, half):
        _refused(lib, None, _valid_multi(lib), w, lib.MZH_ERR_ARG, "args is NULL")
        for field, value, text in (("B", 0, "B=0"), ("n_sims", -1, "n_sims=-1"), ("goal_peg", 3, "goal_peg=3"),
                                   ("max_steps", 0, "max_steps=0"), ("T", 11, "T=11"),
                                   ("flags", lib.MZH_FLAG_KERNEL_ONE | lib.MZH_FLAG_NP1_UCB, "flags=0x81")):
            a = _valid_args(lib)
            setattr(a, field, value)
            _refused(lib, a, _valid_multi(lib), w, lib.MZH_ERR_ARG, text)
        a = _valid_args(lib)
        a.temperature = 1.5
        _refused(lib, a, _valid_multi(lib), w, lib.MZH_ERR_TEMPERATURE, "Expect `temperature` to be in the range")
        for f in REQUIRED:
            a = _valid_args(lib)
            setattr(a, f, None)
            _refused(lib, a, _valid_multi(lib), w, lib.MZH_ERR_ARG, "required buffer is NULL")
        a = _valid_args(lib)
        a.action_u = None
        _refused(lib, a, _valid_multi(lib), w, lib.MZH_ERR_ARG, "needs action_u")
        a = _valid_args(lib)
        _refused(lib, a, None, w, lib.MZH_ERR_ARG, "multi is NULL")
        m = _valid_multi(lib)
        m.net_index = None
        _refused(lib, a, m, w, lib.MZH_ERR_ARG, "net_index is NULL")
        m = _valid_multi(lib)
        m.n_networks = 0
        _refused(lib, a, m, w, lib.MZH_ERR_ARG, "n_networks=0")
    # the sweep block's own, before "engine is NULL"
    a, m = _valid_args(lib), _valid_multi(lib)
    _refused(lib, a, m, None, lib.MZH_ERR_ARG, "sweep is NULL")
    _refused(lib, a, m, half, lib.MZH_ERR_ARG, "n_sims is NULL")
    # everything in order (a NULL discount is fine): the engine is what is missing
    w = _valid_sweep(lib)
    w.discount = None
    _refused(lib, a, m, w, lib.MZH_ERR_ARG, "engine is NULL")
    _refused(lib, a, m, _valid_sweep(lib), lib.MZH_ERR_ARG, "engine is NULL")


def test_play_episodes_takes_sims_only_with_a_set():
    """refused before any engine is made"""
    from muzero_hanoi_amd.networks import NetworkSet
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay

    one, nset = _net(0), NetworkSet([_net(0), _net(1)])
    for kw in (dict(sims=[8, 3]), dict(discounts=[0.8, 0.9]), dict(sims=[8, 3], discounts=[0.8, 0.9])):
        with pytest.raises(ValueError, match="sims / discounts .* need a NetworkSet"):
            BatchedSelfPlay(one, 3, 12, 8).play_episodes([0, 1], **kw)
    for bad in ([8], [9, 3], [-1, 3], [1.5, 2.0]):
        with pytest.raises(ValueError, match=r"sims must be 2 integer budgets in \[0, 8\]"):
            BatchedSelfPlay(nset, 3, 12, 8).play_episodes([0, 1], net_index=[0, 1], sims=bad)
    with pytest.raises(ValueError, match="discounts must be 2 floats"):
        BatchedSelfPlay(nset, 3, 12, 8).play_episodes([0, 1], net_index=[0, 1], sims=[8, 3], discounts=[0.8])


def test_population_override_errors_need_no_device():
    """each names the agent and the key, and is raised before any agent is built (device='cpu' would refuse the
    first agent with the lone class's message)"""
    from muzero_hanoi_amd.muzero import MuzeroPopulation

    P = lambda seeds, overrides, **kw: MuzeroPopulation(seeds, device="cpu", overrides=overrides, **{**MUZERO_KW, **kw})
    with pytest.raises(ValueError, match="overrides has 1 entries for 2 seeds"):
        P([1, 2], [{}])
    with pytest.raises(ValueError, match="overrides has 3 entries for 2 seeds"):
        P([1, 2], [{}, {}, {}])
    for key, value in (("unroll_n_steps", 3), ("TD_return", False), ("n_ep_x_loop", 2), ("env", None),
                       ("device", "cuda"), ("selfplay", "device"), ("ingest", "device"), ("update_impl", "fused"),
                       ("priority_replay", False), ("s_space_size", 12)):
        with pytest.raises(ValueError, match=f"agent 1 overrides '{key}'"):
            P([1, 2], [{"lr": 1e-3}, {key: value}])
    # root noise for some agents only
    with pytest.raises(ValueError, match="agent 2 with 'dirichlet_alpha'=0.0 searches without root noise and agent 0 "
                                         "with 0.25 with:"):
        P([1, 2, 3], [{}, {"dirichlet_alpha": 0.5}, {"dirichlet_alpha": 0.0}])
    with pytest.raises(ValueError, match="agent 1 with 'dirichlet_alpha'=0.25 searches with root noise and agent 0 "
                                         "with 0.0 without:"):
        P([1, 2], [{"dirichlet_alpha": 0.0}, {}])
    # the set update's rounds share one shape
    for key in ("batch_s", "n_update_x_loop"):
        with pytest.raises(ValueError, match=f"update='set'.*agent 0 overrides '{key}'"):
            P([1, 2], [{key: 32}, {}], update="set", update_impl="fused")
    # every key an agent may set passes these checks: the first agent is what then refuses the CPU device
    ok = dict(n_mcts_simulations=5, discount=0.9, dirichlet_alpha=0.5, lr=3e-4, n_TD_step=5, buffer_size=64,
              batch_s=8, n_update_x_loop=2)
    assert set(ok) == set(MuzeroPopulation.SWEEP_KEYS)
    with pytest.raises(ValueError, match="selfplay='device'.*GPU device"):
        P([1, 2], [ok, {}])
    with pytest.raises(ValueError, match="selfplay='device'.*GPU device"):  # all agents noise-free is fine too
        P([1, 2], [{"dirichlet_alpha": 0.0}, {"dirichlet_alpha": 0.0}])
