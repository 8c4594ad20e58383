"""Episodes of a network set in one launch (mzh_play_episodes_multi, Engine / BatchedSelfPlay.play_episodes with
net_index, evaluate_networks(launch="episodes"), MuzeroPopulation): what holds without a GPU -- every refusal the
library makes before it touches an engine or a device, and the Python surface's argument errors.
"""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from muzero_hanoi_amd import build

    build.build()
    from muzero_hanoi_amd import _lib

    return _lib


def test_abi_version_stays_6(lib):
    assert lib.lib().mzh_abi_version() == lib.ABI_VERSION == 6


REQUIRED = ("state", "tie_idx", "pi", "root_q", "action", "reward", "steps", "illegal", "solved", "final_state",
            "minmax_out")


def _valid_args(lib):
    """values in range and every pointer non-null (never dereferenced: each test breaks one field)"""
    a = lib.EpisodeArgs()
    a.B, a.T, a.n_sims, a.goal_peg, a.max_steps, a.deterministic, a.flags = 4, 12, 8, 2, 12, 0, 0
    a.discount, a.eps, a.temperature = 0.8, 0.25, 1.0
    for f, t in lib.EpisodeArgs._fields_:
        if t is ctypes.c_void_p:
            setattr(a, f, 0x1000)
    return a


def _valid_multi(lib):
    m = lib.MultiArgs()
    m.n_networks, m.net_index, m.status = 3, 0x1000, 0x1000
    return m


def _refused(lib, a, m, status, text):
    """the call on a NULL engine and stream: the refusal must come before either is used"""
    got = lib.lib().mzh_play_episodes_multi(None, None if a is None else ctypes.byref(a),
                                            None if m is None else ctypes.byref(m), None)
    assert got == status, (text, got, lib.last_error())
    assert text in lib.last_error(), (text, lib.last_error())


def test_everything_play_episodes_refuses_before_the_engine(lib):
    """with a valid and with a NULL `multi`: the episode arguments' refusals come first, in mzh_play_episodes' order"""
    for multi in (_valid_multi(lib), None):
        _refused(lib, None, multi, lib.MZH_ERR_ARG, "args is NULL")
        for field, value, text in (("B", 0, "B=0"), ("B", -3, "B=-3"), ("n_sims", -1, "n_sims=-1"),
                                   ("goal_peg", 3, "goal_peg=3"), ("goal_peg", -1, "goal_peg=-1"),
                                   ("max_steps", 0, "max_steps=0"), ("T", 11, "T=11"),
                                   ("flags", lib.MZH_FLAG_KERNEL_COOP, "flags=0x2"),
                                   ("flags", lib.MZH_FLAG_KERNEL_ONE | lib.MZH_FLAG_NP1_UCB, "flags=0x81")):
            a = _valid_args(lib)
            setattr(a, field, value)
            _refused(lib, a, multi, lib.MZH_ERR_ARG, text)
        a = _valid_args(lib)
        a.B, a.T, a.max_steps = 1 << 20, 1 << 12, 1 << 12
        _refused(lib, a, multi, lib.MZH_ERR_ARG, "exceed int32")
        for temperature in (-0.5, 1.5, float("nan")):
            a = _valid_args(lib)
            a.temperature = temperature
            _refused(lib, a, multi, lib.MZH_ERR_TEMPERATURE, "Expect `temperature` to be in the range [0.0, 1.0]")
        for f in REQUIRED:
            a = _valid_args(lib)
            setattr(a, f, None)
            _refused(lib, a, multi, lib.MZH_ERR_ARG, "required buffer is NULL")
        a = _valid_args(lib)
        a.action_u = None
        _refused(lib, a, multi, lib.MZH_ERR_ARG, "needs action_u")
    # an earlier refusal wins over a later one: T < max_steps and a NULL net_index
    a, m = _valid_args(lib), _valid_multi(lib)
    a.T, m.net_index = 11, None
    _refused(lib, a, m, lib.MZH_ERR_ARG, "T=11")


def test_multi_refusals_precede_the_engine(lib):
    a = _valid_args(lib)
    _refused(lib, a, None, lib.MZH_ERR_ARG, "multi is NULL")
    m = _valid_multi(lib)
    m.net_index = None
    _refused(lib, a, m, lib.MZH_ERR_ARG, "net_index is NULL")
    for n in (0, -2):
        m = _valid_multi(lib)
        m.n_networks = n
        _refused(lib, a, m, lib.MZH_ERR_ARG, f"n_networks={n}")
    # everything in order (a NULL status is fine): the engine is what is missing
    m = _valid_multi(lib)
    m.status = None
    _refused(lib, a, m, lib.MZH_ERR_ARG, "engine is NULL")


def _net(seed=0):
    from muzero_hanoi_amd.networks import MuZeroNet

    torch.manual_seed(seed)
    return MuZeroNet(9, 6, 0.002, "cpu", TD_return=True)


def test_play_episodes_wants_net_index_exactly_with_a_set():
    """both refusals come before any engine is made"""
    from muzero_hanoi_amd.networks import NetworkSet
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay, RecordedNetwork

    one, nset = _net(0), NetworkSet([_net(0), _net(1)])
    with pytest.raises(ValueError, match="net_index .* required with a NetworkSet"):
        BatchedSelfPlay(nset, 3, 12, 8).play_episodes([0, 1])
    with pytest.raises(ValueError, match="net_index .* only accepted with one"):
        BatchedSelfPlay(one, 3, 12, 8).play_episodes([0, 1], net_index=[0, 0])
    for bad in ([0], [1, 0], [0, 2], [-1, 0]):
        with pytest.raises(ValueError, match="net_index must be 2 non-decreasing indices into the set of 2"):
            BatchedSelfPlay(nset, 3, 12, 8).play_episodes([0, 1], net_index=bad)
    with pytest.raises(ValueError, match="no RecordedNetwork"):
        BatchedSelfPlay(RecordedNetwork.__new__(RecordedNetwork), 3, 12, 8).play_episodes([0])


def test_evaluate_networks_launch_argument():
    from muzero_hanoi_amd.selfplay import evaluate_networks

    nets = [_net(0), _net(1)]
    with pytest.raises(ValueError, match="launch='episodes' .* no max_plan_len form"):
        evaluate_networks(nets, 3, [8], launch="episodes", max_plan_len=2)
    with pytest.raises(ValueError, match="launch must be 'lockstep' or 'episodes', not 'graph'"):
        evaluate_networks(nets, 3, [8], launch="graph")


MUZERO_KW = dict(env=None, s_space_size=9, n_action=6, discount=0.8, dirichlet_alpha=0.25, n_mcts_simulations=8,
                 unroll_n_steps=5, batch_s=16, TD_return=True, n_TD_step=10, lr=0.002, buffer_size=100,
                 priority_replay=True)


def test_population_needs_a_gpu_and_device_selfplay():
    from muzero_hanoi_amd.muzero import MuzeroPopulation

    with pytest.raises(ValueError, match="selfplay='device'.*GPU device"):  # the lone class's message
        MuzeroPopulation([1, 2], device="cpu", **MUZERO_KW)
    with pytest.raises(ValueError, match="selfplay must be 'device', not 'batched'"):
        MuzeroPopulation([1, 2], device="cpu", selfplay="batched", **MUZERO_KW)
    with pytest.raises(ValueError, match="no seeds"):
        MuzeroPopulation([], device="cpu", **MUZERO_KW)
