"""Whole episodes in one launch (mzh_play_episodes, Engine.play_episodes, BatchedSelfPlay.play_episodes,
Muzero(selfplay="device")): what holds without a GPU -- the argument block's layout, every refusal the library
makes before it touches an engine or a device, and the Python surface's argument errors.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mzh.h")


@pytest.fixture(scope="module")
def lib():
    from muzero_hanoi_amd import build

    build.build()
    from muzero_hanoi_amd import _lib

    return _lib


def test_abi_version_stays_6(lib):
    assert lib.lib().mzh_abi_version() == lib.ABI_VERSION == 6


def test_episode_args_layout_matches_header(lib, tmp_path):
    """ctypes EpisodeArgs == struct mzh_episode_args as the C compiler lays it out"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [f[0] for f in lib.EpisodeArgs._fields_]
    want = [getattr(lib.EpisodeArgs, f).offset for f in fields] + [ctypes.sizeof(lib.EpisodeArgs)]
    src = tmp_path / "episode_args.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mzh.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof(mzh_episode_args, {f}));\n' for f in fields)
                   + 'printf("%zu\\n", sizeof(mzh_episode_args)); return 0; }\n')
    exe = tmp_path / "episode_args"
    subprocess.run([cc, "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert len(fields) == 28


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


def _refused(lib, a, status, text):
    """the call on a NULL engine and stream: the refusal must come before either is used"""
    assert lib.lib().mzh_play_episodes(None, None if a is None else ctypes.byref(a), None) == status, text
    assert text in lib.last_error(), (text, lib.last_error())


def test_play_episodes_refusals_precede_the_engine(lib):
    _refused(lib, None, lib.MZH_ERR_ARG, "args is NULL")
    for field, value, text in (("B", 0, "B=0"), ("B", -3, "B=-3"), ("n_sims", -1, "n_sims=-1"),
                               ("goal_peg", 3, "goal_peg=3"), ("goal_peg", -1, "goal_peg=-1"),
                               ("max_steps", 0, "max_steps=0"), ("T", 11, "T=11"),
                               ("flags", lib.MZH_FLAG_KERNEL_COOP, "flags=0x2"),
                               ("flags", lib.MZH_FLAG_KERNEL_ONE | lib.MZH_FLAG_NP1_UCB, "flags=0x81")):
        a = _valid_args(lib)
        setattr(a, field, value)
        _refused(lib, a, lib.MZH_ERR_ARG, text)
    a = _valid_args(lib)
    a.B, a.T, a.max_steps = 1 << 20, 1 << 12, 1 << 12
    _refused(lib, a, lib.MZH_ERR_ARG, "exceed int32")
    for temperature in (-0.5, 1.5, float("nan")):
        a = _valid_args(lib)
        a.temperature = temperature
        _refused(lib, a, lib.MZH_ERR_TEMPERATURE, "Expect `temperature` to be in the range [0.0, 1.0]")
    for f in REQUIRED:
        a = _valid_args(lib)
        setattr(a, f, None)
        _refused(lib, a, lib.MZH_ERR_ARG, "required buffer is NULL")
    a = _valid_args(lib)
    a.action_u = None
    _refused(lib, a, lib.MZH_ERR_ARG, "needs action_u")
    # everything in order: the engine is what is missing (the nullable pointers may all be NULL; the MZH_FLAG_NP1_UCB
    # flag and a deterministic call without action_u pass)
    a = _valid_args(lib)
    a.flags, a.deterministic = lib.MZH_FLAG_NP1_UCB, 1
    for f in ("noise", "action_u", "minmax_in", "pow_table", "visits", "obs", "err_count"):
        setattr(a, f, None)
    _refused(lib, a, lib.MZH_ERR_ARG, "engine is NULL")


def _selfplay(max_steps=12):
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay

    return BatchedSelfPlay(None, 3, max_steps, 8)  # the network is not reached: every error below precedes it


def _table(T, B, rng=np.random.default_rng(0)):
    return (rng.dirichlet(np.full(6, 0.25), size=(T, B)), rng.integers(0, 6, size=(T, B), dtype=np.int32),
            rng.random((T, B)))


def test_play_episodes_legacy_rng_is_the_one_env_schedule():
    sp = _selfplay()
    with pytest.raises(ValueError, match="legacy_rng=True .* B = 1"):
        sp.play_episodes([0, 1], legacy_rng=True)
    with pytest.raises(ValueError, match="legacy_rng=True .* draws=None"):
        sp.play_episodes([0], legacy_rng=True, draws=_table(12, 1))


def test_play_episodes_refuses_a_wrong_draw_table():
    sp = _selfplay()
    T, B = 12, 3
    noise, tie, u = _table(T, B)
    starts = [0, 1, 2]
    bad = {
        "not a triple": (noise, tie),
        "tie rows": (noise, tie[:-1], u),
        "tie envs": (noise, tie[:, :2], u),
        "tie flat": (noise, tie.reshape(-1), u),
        "tie dtype": (noise, tie.astype(np.int64), u),
        "noise shape": (noise[:, :, :5], tie, u),
        "noise dtype": (noise.astype(np.float32), tie, u),
        "noise missing": (None, tie, u),
        "u shape": (noise, tie, u[:, :, None]),
        "u dtype": (noise, tie, u.astype(np.float32)),
        "u missing": (noise, tie, None),
    }
    for what, draws in bad.items():
        with pytest.raises(ValueError, match="play_episodes: draws"):
            sp.play_episodes(starts, draws=draws)
    # deterministic searches draw neither noise nor an action: a table that has them is as wrong
    with pytest.raises(ValueError, match="draws' noise must be None"):
        sp.play_episodes(starts, deterministic=True, draws=(noise, tie, None))
    with pytest.raises(ValueError, match="draws' u must be None"):
        sp.play_episodes(starts, deterministic=True, draws=(None, tie, u))


MUZERO_KW = dict(env=None, s_space_size=9, n_action=6, discount=0.8, dirichlet_alpha=0.25, n_mcts_simulations=8,
                 unroll_n_steps=5, batch_s=16, TD_return=True, n_TD_step=10, lr=0.002, buffer_size=100,
                 priority_replay=True)


def test_muzero_device_selfplay_needs_a_gpu():
    from muzero_hanoi_amd.muzero import Muzero

    with pytest.raises(ValueError, match="selfplay='device'.*GPU device"):
        Muzero(device="cpu", selfplay="device", **MUZERO_KW)
    with pytest.raises(ValueError, match="selfplay='device'.*GPU device"):
        Muzero(device="cpu", selfplay="device", ingest="host", n_ep_x_loop=4, **MUZERO_KW)


def test_muzero_device_selfplay_warns_about_several_episodes_per_loop():
    """n_ep_x_loop > 1 is not the reference's schedule: the RuntimeWarning comes before anything needs the GPU"""
    from muzero_hanoi_amd.muzero import Muzero

    with pytest.warns(RuntimeWarning, match="selfplay='device'.*n_ep_x_loop > 1.*not the reference's"):
        try:
            Muzero(device="cuda", selfplay="device", n_ep_x_loop=4, **MUZERO_KW)
        except (RuntimeError, AssertionError):  # without a GPU the construction ends at the first device use
            pass


def test_muzero_unknown_selfplay_keeps_its_message():
    from muzero_hanoi_amd.muzero import Muzero

    with pytest.raises(ValueError, match="selfplay must be 'sequential' or 'batched', not 'gpu'.*'sequential', "
                                         "'batched' and 'device'"):
        Muzero(device="cpu", selfplay="gpu", **MUZERO_KW)
