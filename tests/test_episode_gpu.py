"""Whole episodes in one launch (mzh_play_episodes) against the lockstep pieces it fuses.

The reference is driven here, move by move, from the same [T][B] draw table: Engine.search over the unfinished
rows with their MinMaxStats carried (minmax_out -> minmax_in), HanoiBatch.step_observe on the chosen actions, env b
taking row b of move t's draws.  Everything is compared bit for bit.  Both sides write into record arrays prefilled
with a sentinel, so equality of the whole arrays also shows that the kernel left the rows past each episode's end
unwritten.
"""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -7
RECORD = (("pi", torch.float64, (6,)), ("root_q", torch.float64, ()), ("action", torch.int32, ()),
          ("reward", torch.int8, ()), ("obs", torch.float32, None))
PER_ENV = ("steps", "illegal", "solved", "final_state", "minmax")
GOAL3 = 26  # state_index((2, 2, 2))


def network(n_disks, support, seed):
    from muzero_hanoi_amd.networks import MuZeroNet

    torch.manual_seed(seed)
    return MuZeroNet(3 * n_disks, 6, 0.002, "cpu", TD_return=support == 33)


def draw_table(T, B, seed, *, deterministic=False, alpha=0.25, dev="cuda"):
    """(noise [T, B, 6] | None, tie [T, B], u [T, B] | None) on the device: row [t, b] for move t of env b"""
    from muzero_hanoi_amd import rng

    flat = rng.synthetic_draws(T * B, deterministic=deterministic, alpha=alpha, seed=seed)
    return tuple(None if x is None else torch.from_numpy(x).reshape((T, B) + x.shape[1:]).to(dev) for x in flat)


def blank_record(T, B, n_disks, dev="cuda"):
    return {k: torch.full((T, B) + ((3 * n_disks,) if tail is None else tail), SENTINEL, dtype=dt, device=dev)
            for k, dt, tail in RECORD}


def bits(t):
    """exact comparison of floating point tensors (NaN payloads and signed zeros included)"""
    t = t.contiguous()
    return t.view({torch.float64: torch.int64, torch.float32: torch.int32}.get(t.dtype, t.dtype)).cpu()


def same(got, want, keys, what=""):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert torch.equal(bits(got[k]), bits(want[k])), (what, k)


def lockstep_reference(eng, n_disks, S, max_steps, start_idx, draws, minmax=None, *, goal_peg=2, **kw):
    """the episodes of mzh_play_episodes from the existing launches: one search and one env step per move"""
    from muzero_hanoi_amd.env import HanoiBatch

    noise, tie, u = draws
    T, B = tie.shape
    dev = tie.device
    env = HanoiBatch(n_disks, max_steps, B, goal_peg=goal_peg, device=dev)
    env.reset(torch.as_tensor(start_idx))
    env._tallies()
    mm = torch.empty((B, 2), dtype=torch.float64, device=dev)
    if minmax is None:
        mm[:, 0], mm[:, 1] = -float("inf"), float("inf")
    else:
        mm.copy_(minmax)
    rec = blank_record(T, B, n_disks, dev)
    idx, t = torch.arange(B, device=dev), 0
    while idx.numel():
        row = lambda x: None if x is None else x[t].index_select(0, idx)
        obs = env.last_obs.index_select(0, idx)
        out = eng.search(S, obs=obs, tie_idx=row(tie), noise=row(noise), action_u=row(u),
                         minmax_in=mm.index_select(0, idx), **kw)
        mm.index_copy_(0, idx, out["minmax"])
        r = env.step_observe(out["action"], idx.to(torch.int32))
        for k, v in (("pi", out["pi"]), ("root_q", out["root_q"]), ("action", out["action"]), ("reward", r["reward"]),
                     ("obs", obs)):
            rec[k][t].index_copy_(0, idx, v)
        idx = torch.nonzero(env.active).reshape(-1)
        t += 1
    assert int(env.err.item()) == 0
    return dict(rec, steps=env.steps_total, illegal=env.illegal_total, solved=env.solved, final_state=env.state, minmax=mm)


def states_of(start_idx, n_disks, dev="cuda"):
    idx = torch.as_tensor(start_idx, dtype=torch.int64)
    pw = 3 ** torch.arange(n_disks - 1, -1, -1)
    return ((idx[:, None] // pw) % 3).to(torch.uint8).to(dev)


def run_episodes(eng, n_disks, S, max_steps, start_idx, draws, minmax=None, **kw):
    noise, tie, u = draws
    T, B = tie.shape
    out = eng.play_episodes(S, states_of(start_idx, n_disks), max_steps, tie_idx=tie, noise=noise, action_u=u,
                            minmax_in=minmax, out=blank_record(T, B, n_disks), **kw)
    assert int(out["err"].item()) == 0
    return out


def check_case(n_disks, support, S, max_steps, start_idx, *, seed, deterministic=False, np1_ucb=False, temperature=1.0,
               max_sims=None):
    from muzero_hanoi_amd.networks import engine_for

    B = len(start_idx)
    eng = engine_for(network(n_disks, support, seed), max_sims or S, B)
    draws = draw_table(max_steps, B, seed, deterministic=deterministic)
    kw = dict(temperature=temperature, deterministic=deterministic, np1_ucb=np1_ucb)
    want = lockstep_reference(eng, n_disks, S, max_steps, start_idx, draws, **kw)
    got = run_episodes(eng, n_disks, S, max_steps, start_idx, draws, **kw)
    same(got, want, [k for k, _, _ in RECORD] + list(PER_ENV))
    return got, want, eng, draws


def test_main_case_equals_the_lockstep_pieces():
    """N=3, S=8, max_steps=12, the 26 non-goal starts plus one repeat, a random 33-bin network, temperature 1,
    Dirichlet noise; the batch must hold an env that reaches the goal early, one that runs to max_steps and one
    that plays an illegal move"""
    starts = [i for i in range(27) if i != GOAL3] + [17]
    got, _, _, _ = check_case(3, 33, 8, 12, starts, seed=1)
    steps, solved, illegal = (got[k].cpu().numpy() for k in ("steps", "solved", "illegal"))
    assert ((solved == 1) & (steps < 12)).any(), "no env reached the goal before max_steps: choose another seed"
    assert ((solved == 0) & (steps == 12)).any(), "no env ran to max_steps: choose another seed"
    assert (illegal > 0).any(), "no env played an illegal move: choose another seed"
    assert (steps >= 1).all() and (steps <= 12).all()


@pytest.mark.parametrize("case", ["scalar_heads_n4_deterministic", "np1_ucb"])
def test_variants_equal_the_lockstep_pieces(case):
    if case == "scalar_heads_n4_deterministic":  # support 1, no noise, no action draw
        check_case(4, 1, 6, 7, [0, 5, 40, 79, 53], seed=2, deterministic=True)
    else:
        check_case(3, 33, 8, 6, [0, 13, 17, 25], seed=3, np1_ucb=True)


def test_fresh_minmax_equals_explicit_infinities():
    """minmax_in NULL and an explicit (-inf, +inf) give the same episodes"""
    starts = [0, 9, 17, 23]
    got, _, eng, draws = check_case(3, 33, 8, 6, starts, seed=4)
    mm = torch.tensor([[-float("inf"), float("inf")]] * len(starts), dtype=torch.float64, device="cuda")
    explicit = run_episodes(eng, 3, 8, 6, starts, draws, minmax=mm)
    same(explicit, got, [k for k, _, _ in RECORD] + list(PER_ENV))
    assert torch.isfinite(got["minmax"]).all()  # the carried bounds moved


def lds_latent_limit(support):
    """the largest n_sims whose latents the latency kernel keeps in LDS, from the plan query"""
    from muzero_hanoi_amd import _lib

    smem = lambda S: _lib.search_plan(support, 2, S, flags=_lib.MZH_FLAG_KERNEL_ONE, minmax_in=True)["smem_bytes"]
    S = 1  # a simulation more adds LDS (its tree block, and its latent while the latents are there): the first
    while smem(S + 1) > smem(S):  # n_sims whose LDS is smaller than the one before has moved the latents out
        S += 1
        assert S < 4096
    return S


def test_latents_in_hbm():
    """an n_sims just above the LDS-resident limit: the latents live in the engine's workspace, indexed by env"""
    S = lds_latent_limit(33) + 1
    check_case(3, 33, S, 3, [0, 17], seed=5, max_sims=S)


def test_several_envs_per_workgroup():
    """B = 257 on 256 workgroups: the last env is its workgroup's second, and plays as it does alone"""
    B, S, T = 257, 2, 3
    starts = [(7 * b) % 26 for b in range(B)]
    got, _, eng, draws = check_case(3, 33, S, T, starts, seed=6)
    alone = run_episodes(eng, 3, S, T, starts[-1:], tuple(None if x is None else x[:, -1:].contiguous() for x in draws))
    last = {k: got[k][:, -1:] for k, _, _ in RECORD}
    last.update({k: got[k][-1:] for k in PER_ENV})
    same(alone, last, [k for k, _, _ in RECORD] + list(PER_ENV))


PLAY_KEYS = ("action", "reward", "pi", "root_q", "active", "obs", "steps", "illegal", "start_idx", "minmax")


def selfplay(S=8, max_steps=12, seed=7):
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay

    return BatchedSelfPlay(network(3, 33, seed), 3, max_steps, S)


def test_equals_play_with_synthetic_draws():
    """B = 1: play_episodes on the table of play's own per-move draws returns play(record_obs=True)'s dict"""
    from muzero_hanoi_amd import rng

    sp, T, seed = selfplay(), 12, 21
    gen = np.random.default_rng(seed)  # _Lockstep: one seed per move from default_rng(seed)
    moves = [rng.synthetic_draws(1, deterministic=False, alpha=sp.alpha, eps=sp.eps, seed=int(gen.integers(2**31)))
             for _ in range(T)]
    table = tuple(np.stack([m[i] for m in moves]) for i in range(3))
    want = sp.play([3], temperature=1.0, seed=seed, record_obs=True)
    got = sp.play_episodes([3], temperature=1.0, draws=table)
    assert set(got) == set(want) == set(PLAY_KEYS)
    same(got, want, PLAY_KEYS)


def test_equals_play_on_the_legacy_stream():
    """B = 1, legacy_rng: the same dict, and NumPy's global stream is left where play leaves it"""
    sp = selfplay()
    out = []
    for play in (lambda: sp.play([16], temperature=0.5, legacy_rng=True, record_obs=True),
                 lambda: sp.play_episodes([16], temperature=0.5, legacy_rng=True)):
        np.random.seed(13)
        res = play()
        out.append((res, np.random.get_state()))
    (want, sw), (got, sg) = out
    same(got, want, PLAY_KEYS)
    assert sw[0] == sg[0] and np.array_equal(sw[1], sg[1]) and sw[2:] == sg[2:]


def buffer_snapshot(buf):
    raw = lambda x: np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.int64)
    arrays = [t.cpu().numpy() for t in (buf.states, buf.rwds, buf.actions, buf.pi_probs, buf.mc_returns)]
    arrays.append(np.array(buf.priorities, np.float32))
    return [raw(x) for x in arrays], (buf.ptr, buf.is_full, len(buf))


@pytest.mark.parametrize("ingest", ["host", "device"])
def test_training_loops_equal_the_batched_selfplay(ingest):
    """Muzero(selfplay="device") against selfplay="batched", one episode per loop, three loops from one seed: the
    same buffer arrays, priorities, ptr, MinMaxStats and NumPy stream"""
    from muzero_hanoi_amd.env import TowersOfHanoi
    from muzero_hanoi_amd.muzero import Muzero

    out = []
    for selfplay_mode in ("batched", "device"):
        torch.manual_seed(3)
        env = TowersOfHanoi(N=3, max_steps=12, init_state_idx=17)  # (1, 2, 2): one move from the goal
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)  # n_ep_x_loop = 1 is the parity schedule: no warning
            mz = Muzero(env=env, s_space_size=9, n_action=6, discount=0.8, dirichlet_alpha=0.25, n_mcts_simulations=8,
                        unroll_n_steps=5, batch_s=16, TD_return=True, n_TD_step=10, lr=0.002, buffer_size=500,
                        priority_replay=True, device="cuda", n_ep_x_loop=1, selfplay=selfplay_mode, ingest=ingest)
        np.random.seed(9)
        mz.training_loop(n_loops=4, min_replay_size=10**9, print_acc=1000)
        mm = mz.mcts.min_max_stats
        out.append((*buffer_snapshot(mz.buffer), (mm.maximum, mm.minimum), np.random.random_sample(3)))
    (ba, bs, bm, br), (da, ds, dm, dr) = out
    assert ds == bs and bs[2] > 0, (bs, ds)  # some episode reached the goal: the buffers are not empty
    for name, b, d in zip(("states", "rwds", "actions", "pi_probs", "mc_returns", "priorities"), ba, da):
        assert np.array_equal(b, d), name
    assert dm == bm and np.array_equal(br, dr)


def test_several_episodes_per_loop_take_a_move_major_legacy_table():
    """Muzero(selfplay="device", n_ep_x_loop=3): the loop's episodes are play_episodes on rng.predraw(T * 3) from
    the global stream, reshaped move-major -- the same record, MinMaxStats union and stream as that explicit call"""
    from muzero_hanoi_amd import rng
    from muzero_hanoi_amd.env import TowersOfHanoi
    from muzero_hanoi_amd.muzero import Muzero
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay, episode_records
    from muzero_hanoi_amd.utils import adjust_temperature

    G, T, episode = 3, 12, 7
    torch.manual_seed(3)
    env = TowersOfHanoi(N=3, max_steps=T, init_state_idx=17)
    with pytest.warns(RuntimeWarning, match="selfplay='device'.*n_ep_x_loop > 1"):
        mz = Muzero(env=env, s_space_size=9, n_action=6, discount=0.8, dirichlet_alpha=0.25, n_mcts_simulations=8,
                    unroll_n_steps=5, batch_s=16, TD_return=True, n_TD_step=10, lr=0.002, buffer_size=500,
                    priority_replay=True, device="cuda", n_ep_x_loop=G, selfplay="device")
    np.random.seed(21)
    got = mz._play_games(G, episode=episode)
    mm, after = mz.mcts.min_max_stats, np.random.random_sample(3)

    np.random.seed(21)
    flat = rng.predraw(T * G, deterministic=False, alpha=0.25, eps=mz.mcts.root_exploration_eps)
    table = tuple(x.reshape((T, G) + x.shape[1:]) for x in flat)
    sp = BatchedSelfPlay(mz.networks, 3, T, 8, discount=0.8, dirichlet_alpha=0.25,
                         root_exploration_eps=mz.mcts.root_exploration_eps, np1_ucb=mz.mcts.np1_ucb)
    res = sp.play_episodes([17] * G, temperature=adjust_temperature(episode), draws=table,
                           minmax=[[-float("inf"), float("inf")]] * G)
    want = episode_records(res, discount=0.8, TD_return=True, n_step=10, unroll_n_steps=5, n_action=6)
    assert np.array_equal(after, np.random.random_sample(3))  # one organise_transitions draw per episode on both sides
    fin = res["minmax"].cpu().numpy()
    assert (mm.maximum, mm.minimum) == (float(fin[:, 0].max()), float(fin[:, 1].min()))
    assert len(got) == len(want) == G
    for g, w in zip(got, want):
        assert g[0] == w[0]
        for x, y in zip(g[1:], w[1:]):
            assert np.array_equal(np.asarray(x), np.asarray(y))


def test_bad_start_state_is_skipped():
    """a start state with peg 3: that env plays nothing and is counted; the other envs are unaffected"""
    from muzero_hanoi_amd.networks import engine_for

    S, T, starts = 8, 6, [5, 17, 22]
    eng = engine_for(network(3, 33, 8), S, 3)
    draws = draw_table(T, 3, 8)
    want = lockstep_reference(eng, 3, S, T, starts, draws, temperature=1.0)
    state = states_of(starts, 3)
    state[1, 2] = 3
    noise, tie, u = draws
    got = eng.play_episodes(S, state, T, tie_idx=tie, noise=noise, action_u=u, out=blank_record(T, 3, 3))
    assert int(got["err"].item()) == 1
    for k, _, _ in RECORD:
        assert torch.equal(bits(got[k][:, [0, 2]]), bits(want[k][:, [0, 2]])), k
        assert (got[k][:, 1] == SENTINEL).all(), k
    for k in PER_ENV:
        assert torch.equal(bits(got[k][[0, 2]]), bits(want[k][[0, 2]])), k
    assert got["steps"][1] == 0 and got["illegal"][1] == 0 and got["solved"][1] == 0
    assert torch.equal(got["final_state"][1], state[1])
    assert got["minmax"][1].tolist() == [-float("inf"), float("inf")]


def test_engine_side_refusals():
    """the refusals that need an engine: capacity, the latency kernel's LDS, weights not loaded, T < max_steps"""
    from muzero_hanoi_amd import _lib
    from muzero_hanoi_amd.engine import Engine, flat_weights

    eng = Engine(3, 2000, 4, 33)
    tie = torch.zeros((6, 2), dtype=torch.int32, device="cuda")
    kw = dict(tie_idx=tie, deterministic=True)
    with pytest.raises(RuntimeError, match="weights not loaded"):
        eng.play_episodes(8, states_of([0, 1], 3), 6, **kw)
    eng.load_weights(flat_weights(network(3, 33, 9).state_dict()))
    with pytest.raises(RuntimeError, match="n_sims=2001 > max_sims=2000"):
        eng.play_episodes(2001, states_of([0, 1], 3), 6, **kw)
    with pytest.raises(RuntimeError, match="B=5 > max_roots=4"):
        eng.play_episodes(8, states_of([0] * 5, 3), 6, tie_idx=torch.zeros((6, 5), dtype=torch.int32, device="cuda"),
                          deterministic=True)
    with pytest.raises(ValueError, match="T=6 rows cannot hold max_steps=7"):
        eng.play_episodes(8, states_of([0, 1], 3), 7, **kw)
    S = 64  # the first n_sims the latency kernel's LDS cannot hold (MZH_FLAG_KERNEL_ONE is an error there)
    fits = lambda s: _lib.lib().mzh_search_plan_query(33, 2, s, _lib.MZH_FLAG_KERNEL_ONE, 0, 1, _lib.SearchPlan()) == 0
    while fits(S):
        S += 64
        assert S <= 2000
    with pytest.raises(RuntimeError, match="MZH_FLAG_KERNEL_ONE: n_sims=.* of LDS"):
        eng.play_episodes(S, states_of([0, 1], 3), 6, **kw)
    eng.close()
