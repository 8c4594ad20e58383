"""Episode ingest on the device (csrc/mzh_ingest.hip, Buffer.add_episodes, selfplay.ingest_records,
Muzero(ingest="device")) against the host path it replaces: selfplay.episode_records, the
`returns[-1, 0] > 0` filter and Buffer.add per episode, on the same record and NumPy seed.  Every
comparison is bit for bit: the five ring arrays in full (prefilled with a sentinel, so untouched rows
show), the priorities, ptr / is_full / len and the next draws of the NumPy stream.

The records are synthetic (no search runs): steps[b] in [1, T], rewards -0.1 with the last either 100 or
-0.1, Dirichlet pi, normal root values, one-hot observations, and NaN / -1 / 7 in everything past steps[b].
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mzh.h")


@pytest.fixture(scope="module")
def lib():
    from muzero_hanoi_amd import build

    build.build()
    from muzero_hanoi_amd import _lib

    return _lib


# ------------------------------------------------------------------------------------------------ CPU
def test_abi_version_stays_6(lib):
    assert lib.lib().mzh_abi_version() == lib.ABI_VERSION == 6


def test_ingest_args_layout_matches_header(lib, tmp_path):
    """ctypes IngestArgs == struct mzh_ingest_args as the C compiler lays it out"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [f[0] for f in lib.IngestArgs._fields_]
    want = [getattr(lib.IngestArgs, f).offset for f in fields] + [ctypes.sizeof(lib.IngestArgs)]
    src = tmp_path / "ingest_args.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mzh.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof(mzh_ingest_args, {f}));\n' for f in fields)
                   + 'printf("%zu\\n", sizeof(mzh_ingest_args)); return 0; }\n')
    exe = tmp_path / "ingest_args"
    subprocess.run([cc, "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert len(fields) == 24


def _valid_args(lib):
    """dimensions in range and every pointer non-null (never dereferenced: each test breaks one field)"""
    a = lib.IngestArgs()
    a.B, a.T, a.d_state, a.U, a.A, a.n_step, a.size, a.ptr = 4, 3, 9, 5, 6, 10, 100, 7
    for f, t in lib.IngestArgs._fields_:
        if t is ctypes.c_void_p:
            setattr(a, f, 0x1000)
    return a


def test_ingest_argument_errors_are_loud(lib):
    """mzh_episode_ingest refuses bad arguments on the host, before any device call"""
    L = lib.lib()
    assert L.mzh_episode_ingest(None, None) == lib.MZH_ERR_ARG and "null args" in lib.last_error()
    for f in ("B", "T", "d_state", "U", "A", "n_step", "size"):
        a = _valid_args(lib)
        setattr(a, f, 0)
        if f == "size":
            a.ptr = 0
        assert L.mzh_episode_ingest(ctypes.byref(a), None) == lib.MZH_ERR_ARG, f
        assert f"{f}=0" in lib.last_error(), (f, lib.last_error())
    for ptr in (-1, 100, 101):
        a = _valid_args(lib)
        a.ptr = ptr
        assert L.mzh_episode_ingest(ctypes.byref(a), None) == lib.MZH_ERR_ARG
        assert f"ptr={ptr}" in lib.last_error()
    for f, t in lib.IngestArgs._fields_:
        if t is ctypes.c_void_p:
            a = _valid_args(lib)
            setattr(a, f, None)
            assert L.mzh_episode_ingest(ctypes.byref(a), None) == lib.MZH_ERR_ARG, f
            assert "null pointer" in lib.last_error()


def test_muzero_device_ingest_requirements():
    """ingest="device" needs the batched self-play, n-step TD returns and a GPU device"""
    from muzero_hanoi_amd.muzero import Muzero

    kw = dict(env=None, s_space_size=9, n_action=6, discount=0.8, dirichlet_alpha=0.25, n_mcts_simulations=8,
              unroll_n_steps=5, batch_s=16, n_TD_step=10, lr=0.002, buffer_size=100, priority_replay=True)
    with pytest.raises(ValueError, match="selfplay='batched'"):
        Muzero(TD_return=True, device="cuda", selfplay="sequential", ingest="device", **kw)
    with pytest.raises(ValueError, match="TD_return=True"):
        Muzero(TD_return=False, device="cuda", selfplay="batched", ingest="device", **kw)
    with pytest.raises(ValueError, match="GPU device"):
        Muzero(TD_return=True, device="cpu", selfplay="batched", ingest="device", **kw)
    with pytest.raises(ValueError, match="ingest must be"):
        Muzero(TD_return=True, device="cpu", ingest="gpu", **kw)


def test_add_episodes_needs_a_gpu_buffer():
    from muzero_hanoi_amd.buffer import Buffer

    buf = Buffer(10, 5, 9, 6, "cpu")
    with pytest.raises(ValueError, match="GPU buffer"):
        buf.add_episodes({}, discount=0.8, n_step=10, pad_action=[0])


# ------------------------------------------------------------------------------------------------ GPU
U, N_STEP, A, D = 5, 10, 6, 9


def make_record(seed, B, T, *, A=A, D=D, success="mixed", steps=None, dev="cuda"):
    """a BatchedSelfPlay.play(record_obs=True) result with garbage past every episode's end"""
    g = np.random.default_rng(seed)
    steps = g.integers(1, T + 1, size=B) if steps is None else np.asarray(steps)
    steps = steps.astype(np.int32)
    win = {"mixed": g.random(B) < 0.6, "all": np.ones(B, bool), "none": np.zeros(B, bool)}[success]
    live = np.arange(T)[:, None] < steps[None, :]  # [T][B]
    reward = np.where(live, -0.1, np.nan)
    last = steps - 1
    reward[last[win], np.nonzero(win)[0]] = 100.0
    pi = np.where(live[..., None], g.dirichlet(np.ones(A), size=(T, B)), np.nan)
    root_q = np.where(live, g.normal(size=(T, B)), np.nan)
    obs = np.full((T, B, D), 7.0, np.float32)
    hot = g.integers(0, D, size=(T, B))
    obs[live] = np.eye(D, dtype=np.float32)[hot[live]]
    action = np.where(live, g.integers(0, A, size=(T, B)), -1).astype(np.int32)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return dict(obs=t(obs), action=t(action), reward=t(reward), pi=t(pi), root_q=t(root_q), active=t(live),
                steps=t(steps))


SENTINEL = -7.0


def make_buffer(size, device_sampling, *, ptr=0, is_full=False, U=U, A=A, D=D):
    from muzero_hanoi_amd.buffer import Buffer

    buf = Buffer(size, U, D, A, "cuda", device_sampling=device_sampling)
    for t in (buf.states, buf.rwds, buf.pi_probs, buf.mc_returns):
        t.fill_(SENTINEL)
    buf.actions.fill_(-7)
    buf.priorities = np.full(size, 3.0, np.float32)
    buf.ptr, buf.is_full = ptr, is_full
    return buf


def snapshot(buf):
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.int64)
    arrays = [t.cpu().numpy() for t in (buf.states, buf.rwds, buf.actions, buf.pi_probs, buf.mc_returns)]
    arrays.append(np.array(buf.priorities, np.float32))
    return [bits(x) for x in arrays], (buf.ptr, buf.is_full, len(buf))


def host_ingest(res, buf, *, n_step=N_STEP, unroll=U, n_action=A):
    """the path the device call replaces"""
    from muzero_hanoi_amd.selfplay import episode_records

    for _, states, rwds, actions, pi_probs, returns, prio in episode_records(
            res, discount=0.8, TD_return=True, n_step=n_step, unroll_n_steps=unroll, n_action=n_action):
        if returns[-1, 0] > 0:
            buf.add(states, rwds, actions, pi_probs, returns, prio)


def device_ingest(res, buf, *, n_step=N_STEP, unroll=U, n_action=A):
    from muzero_hanoi_amd.selfplay import ingest_records

    steps = ingest_records(res, buf, discount=0.8, n_step=n_step, unroll_n_steps=unroll, n_action=n_action)
    assert np.array_equal(steps, res["steps"].cpu().numpy())


NAMES = ("states", "rwds", "actions", "pi_probs", "mc_returns", "priorities")


def check_equal(records, size, device_sampling, *, ptr=0, is_full=False, n_step=N_STEP, unroll=U, n_action=A, D=D):
    """the same records through both paths from the same NumPy seed: equal buffers and streams"""
    out = []
    for path in (host_ingest, device_ingest):
        buf = make_buffer(size, device_sampling, ptr=ptr, is_full=is_full, U=unroll, A=n_action, D=D)
        np.random.seed(11)
        for res in records:
            path(res, buf, n_step=n_step, unroll=unroll, n_action=n_action)
        out.append((*snapshot(buf), np.random.random_sample(3)))
    (ha, hs, hr), (da, ds, dr) = out
    assert ds == hs, f"(ptr, is_full, len): device {ds}, host {hs}"
    for name, h, d in zip(NAMES, ha, da):
        assert np.array_equal(h, d), f"{name}: {int((h != d).sum())} words differ"
    assert np.array_equal(hr, dr), "the NumPy stream ends elsewhere"
    return hs


MODES = pytest.mark.parametrize("device_sampling", [False, True], ids=["host_prio", "device_prio"])


@pytest.mark.gpu
@MODES
def test_minimal(device_sampling):
    ptr, is_full, n = check_equal([make_record(1, 1, 1, success="all")], 16, device_sampling)
    assert (ptr, is_full, n) == (1, False, 1)


@pytest.mark.gpu
@MODES
def test_realistic(device_sampling):
    """B=37, T=23, U=5, n_step=10, A=6, d_state=9 into an empty ring with room to spare"""
    ptr, is_full, n = check_equal([make_record(2, 37, 23)], 1000, device_sampling)
    assert 0 < n < 1000 and not is_full


@pytest.mark.gpu
@MODES
def test_windows_longer_than_the_episode(device_sampling):
    """n_step > T and U > T (T=3), with envs of one step"""
    res = make_record(3, 9, 3, steps=[1, 3, 2, 1, 3, 3, 1, 2, 3], success="all")
    _, _, n = check_equal([res], 64, device_sampling)
    assert n == 19


@pytest.mark.gpu
@MODES
def test_no_episode_succeeds(device_sampling):
    ptr, is_full, n = check_equal([make_record(4, 37, 23, success="none")], 300, device_sampling, ptr=5)
    assert (ptr, is_full, n) == (5, False, 5)


@pytest.mark.gpu
@MODES
def test_every_episode_succeeds(device_sampling):
    res = make_record(5, 37, 23, success="all")
    _, _, n = check_equal([res], 1000, device_sampling)
    assert n == int(res["steps"].sum())


@pytest.mark.gpu
def test_scan_over_more_envs_than_one_pass():
    """B=3,077 > the 1,024 envs of one scan pass (three full passes and a partial one)"""
    _, _, n = check_equal([make_record(6, 3077, 12)], 40000, True)
    assert n > 3 * 1024


@pytest.mark.gpu
@MODES
def test_episode_wraps_at_the_ring_end(device_sampling):
    """ptr near the end: an episode's rows continue at row 0; rows never written keep the sentinel"""
    ptr, is_full, n = check_equal([make_record(7, 5, 23, success="all", steps=[23, 20, 4, 23, 9])], 300,
                                  device_sampling, ptr=290)
    assert (ptr, is_full, n) == ((290 + 79) % 300, True, 300)


@pytest.mark.gpu
@MODES
def test_more_rows_than_the_ring(device_sampling):
    """size=50 < G: only the last 50 rows of the sequential order stay (the overwrite rule)"""
    res = make_record(8, 37, 23)
    ptr, is_full, n = check_equal([res], 50, device_sampling, ptr=13)
    assert is_full and n == 50


@pytest.mark.gpu
@MODES
def test_second_ingest_onto_a_full_ring(device_sampling):
    ptr, is_full, n = check_equal([make_record(9, 37, 23), make_record(10, 21, 17)], 120, device_sampling)
    assert is_full and n == 120


@pytest.mark.gpu
@MODES
def test_episode_longer_than_the_ring(device_sampling):
    """an entering episode with steps > size: Buffer.add's AssertionError, every array unchanged"""
    res = make_record(12, 6, 23, success="all", steps=[3, 5, 23, 2, 7, 4])
    buf = make_buffer(20, device_sampling, ptr=4)
    before = snapshot(buf)
    np.random.seed(11)
    with pytest.raises(AssertionError):
        device_ingest(res, buf)
    after = snapshot(buf)
    assert after[1] == before[1]
    for name, x, y in zip(NAMES, before[0], after[0]):
        assert np.array_equal(x, y), name
    with pytest.raises(AssertionError):
        host_ingest(res, make_buffer(20, device_sampling, ptr=4))
    # the same batch without the long episode's success goes in
    res = make_record(12, 6, 23, success="all", steps=[3, 5, 20, 2, 7, 4])
    check_equal([res], 20, device_sampling, ptr=4)


@pytest.mark.gpu
def test_other_widths():
    """row widths that are no multiple of anything: A=4, d_state=12, U=3, n_step=2; and the observation widths
    of 1 and 16 discs, d_state 3 and 48"""
    check_equal([make_record(13, 19, 11, A=4, D=12)], 90, False, ptr=80, n_step=2, unroll=3, n_action=4, D=12)
    check_equal([make_record(14, 19, 11, D=3)], 90, False, ptr=80, D=3)
    check_equal([make_record(15, 19, 11, D=48)], 90, True, ptr=80, D=48)


@pytest.mark.gpu
def test_muzero_device_ingest_end_to_end():
    """two agents seeded identically, ingest="host" and "device": equal buffers, MinMaxStats and NumPy
    stream after three loops of four lockstep episodes; then a loop with fused updates on the device-ingest
    agent's buffer runs with finite losses"""
    import warnings

    from muzero_hanoi_amd.env import TowersOfHanoi
    from muzero_hanoi_amd.muzero import Muzero

    def agent(ingest):
        torch.manual_seed(3)
        env = TowersOfHanoi(N=3, max_steps=200)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # n_ep_x_loop > 1: not the reference's schedule
            return Muzero(env=env, s_space_size=9, n_action=6, discount=0.8, dirichlet_alpha=0.25,
                          n_mcts_simulations=8, unroll_n_steps=5, batch_s=16, TD_return=True, n_TD_step=10, lr=0.002,
                          buffer_size=5000, priority_replay=True, device="cuda", n_ep_x_loop=4, selfplay="batched",
                          update_impl="fused", ingest=ingest)

    outs, agents = [], []
    for ingest in ("host", "device"):
        mz = agent(ingest)
        np.random.seed(9)
        mz.training_loop(n_loops=4, min_replay_size=10**9, print_acc=1000)
        mm = mz.mcts.min_max_stats
        outs.append((*snapshot(mz.buffer), (mm.maximum, mm.minimum), np.random.random_sample(3)))
        agents.append(mz)
    (ha, hs, hm, hr), (da, ds, dm, dr) = outs
    assert ds == hs and hs[2] > 0, (hs, ds)  # some episode reached the goal: the buffers are not empty
    for name, h, d in zip(NAMES, ha, da):
        assert np.array_equal(h, d), name
    assert dm == hm and np.array_equal(hr, dr)

    mz = agents[1]
    losses = []
    inner = mz._update

    def recording(*args):
        out = inner(*args)
        losses.append([float(x) for x in out[1:]])
        return out

    mz._update = recording
    mz.training_loop(n_loops=2, min_replay_size=0, print_acc=1000)
    assert len(losses) == 1 and np.isfinite(losses[0]).all(), losses
    assert np.isfinite(mz.buffer.priorities).all()
