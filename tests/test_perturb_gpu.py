"""Acting on perturbed observations on the GPU (noise_injection_comparison.py, permutation_importance.py).

  kernel    mzh_env_step_observe against a NumPy statement of its contract on oracle.env_step: every 3-disk
            state x action x permuted disc x replacement peg, counters next to max_steps, with and without
            noise, through a shuffled env_index with sentinel padding around every array; observe-only calls,
            inactive rows, every error row, N = 1 and N = 32;
  batched   BatchedSelfPlay.play_perturbed without a perturbation against play, with mixed conditions against
            the same episodes simulated with oracle.search + oracle.env_step on NumPy-built observations (one
            network and a set of three), evaluate_perturbed's scores and its slicing;
  drop-in   acting.noise_play_game / permutation_play_game on the reference's recorded games
            (tests/golden/perturb_*.npz) and, with a real network, against the loops restated on the oracle.
All comparisons are exact: integers, and float bit patterns as uint32 / uint64 views.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
from muzero_hanoi_amd import rng as mrng
from test_plan_cpu import recorded_calls
from test_plan_gpu import _fresh_net, _padded, _pads_intact

FILLS = dict(env_index=-9, action=99, state=77, step_ctr=-7, active=9, steps_total=-3, illegal_total=-4, solved=66,
             perm_disc=-99, perm_peg=98, noise=-123.0, obs=-5.0, reward=55, done=44, err_count=-2)
DTYPES = dict(env_index=np.int32, action=np.int32, state=np.uint8, step_ctr=np.int32, active=np.uint8,
              steps_total=np.int32, illegal_total=np.int32, solved=np.uint8, perm_disc=np.int32, perm_peg=np.int32,
              noise=np.float64, obs=np.float32, reward=np.int8, done=np.uint8, err_count=np.int32)
SPECIAL_NOISE = np.array([-1.0, 2.0 ** -30, -2.0 ** -30, 1e-8, -1e-8, 1e10, -1e10, 0.0, -0.0])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _onehot64(st):
    hot = np.zeros(3 * len(st), np.float64)
    hot[np.arange(len(st)) * 3 + st] = 1
    return hot


def contract(oracle, n_disks, max_steps, inp):
    """mzh_env_step_observe's contract in NumPy on oracle.env_step: the expected value of every array.
    inp: env_index / action / perm_disc / perm_peg / noise may be None; the rest as the kernel takes them."""
    B = len(inp["state"])
    rows = len(next(inp[k] for k in ("env_index", "action", "perm_peg", "noise", "state") if inp[k] is not None))
    out = {k: inp[k].copy() for k in ("state", "step_ctr", "active", "steps_total", "illegal_total", "solved", "obs")}
    reward, done, errors = np.zeros(rows, np.int8), np.zeros(rows, np.uint8), 0
    for j in range(rows):
        e = j if inp["env_index"] is None else int(inp["env_index"][j])
        if not 0 <= e < B:
            errors += 1
            continue
        if not out["active"][e]:
            continue
        pd = -1 if inp["perm_disc"] is None else int(inp["perm_disc"][e])
        if (not -1 <= pd < n_disks or (pd >= 0 and not 0 <= inp["perm_peg"][j] <= 2)
                or (inp["action"] is not None and not 0 <= inp["action"][j] < 6)):
            errors += 1
            continue
        if inp["action"] is not None:
            code, s2, _, c2, a2, d, ill = oracle.env_step(out["state"][e], int(inp["action"][j]),
                                                          int(out["step_ctr"][e]), 1, max_steps)
            out["state"][e], out["step_ctr"][e], out["active"][e] = s2, c2, a2
            out["steps_total"][e] += 1
            out["illegal_total"][e] += ill
            out["solved"][e] |= code == 1
            reward[j], done[j] = code, d
        if out["active"][e]:
            seen = out["state"][e].copy()
            if pd >= 0:
                seen[pd] = inp["perm_peg"][j]
            hot = _onehot64(seen)
            out["obs"][e] = (hot if inp["noise"] is None else hot + inp["noise"][j]).astype(np.float32)
    return dict(out, reward=reward, done=done, err_count=np.array([errors], np.int32))


def run_kernel(n_disks, max_steps, inp, dev):
    """mzh_env_step_observe through the C ABI on padded copies of `inp`; returns name -> (buffer, view)"""
    from muzero_hanoi_amd import _lib

    rows = len(next(inp[k] for k in ("env_index", "action", "perm_peg", "noise", "state") if inp[k] is not None))
    arrays = dict(inp, reward=np.full(rows, 55, np.int8), done=np.full(rows, 44, np.uint8),
                  err_count=np.zeros(1, np.int32))
    bufs = {k: _padded(np.asarray(v, DTYPES[k]), FILLS[k], dev) for k, v in arrays.items() if v is not None}
    a = _lib.ObserveArgs()
    a.n_disks, a.goal_peg, a.max_steps, a.B, a.n = n_disks, 2, max_steps, len(inp["state"]), rows
    for k, (_, view) in bufs.items():
        setattr(a, k, view.data_ptr())
    _lib.check(_lib.lib().mzh_env_step_observe(ctypes.byref(a), _lib.stream_handle(dev)), "mzh_env_step_observe")
    torch.cuda.synchronize(dev)
    return bufs


def check_kernel(oracle, n_disks, max_steps, inp, dev=None):
    dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else dev
    want = contract(oracle, n_disks, max_steps, inp)
    bufs = run_kernel(n_disks, max_steps, inp, dev)
    for k, (buf, view) in bufs.items():
        assert _pads_intact(buf, FILLS[k]), f"padding of {k} overwritten"
        exp = want[k] if k in want else np.asarray(inp[k], DTYPES[k])  # the inputs are left as they were
        got = view.cpu().numpy()
        assert np.array_equal(_bits(got.reshape(np.shape(exp))), _bits(np.asarray(exp, DTYPES[k]))), k
    return want


def _noise_rows(rs, rows, n_obs):
    """standard normals scaled by 0.3 with the special values sprinkled in: exact cancellation (-1), sums that
    need rounding (2^-30, 1e-8), large values (1e10) and both zeros"""
    z = 0.3 * rs.standard_normal((rows, n_obs))
    mask = rs.random_sample((rows, n_obs)) < 0.35
    z[mask] = SPECIAL_NOISE[rs.randint(0, len(SPECIAL_NOISE), int(mask.sum()))]
    z[0, :len(SPECIAL_NOISE)] = SPECIAL_NOISE[:n_obs]  # each at least once
    return z


# ---------------------------------------------------------------------------- every state x action x disc x peg
ALL_MAX_STEPS = 9


def _all_inputs(ctr0, noisy, spare=56):
    n = 3
    states = np.array(list(itertools.product(range(3), repeat=n)), np.uint8)
    grid = np.array(list(itertools.product(range(len(states)), range(6), (-1, 0, 1, 2), range(3))))
    rows = len(grid)
    assert rows == 27 * 6 * 4 * 3
    B = rows + spare
    rs = np.random.RandomState(100 + ctr0)
    env_index = rs.permutation(B)[:rows].astype(np.int32)
    state = np.full((B, n), 200, np.uint8)  # the envs no row names keep this
    state[env_index] = states[grid[:, 0]]
    perm_disc = np.full(B, 7, np.int32)  # out of range where no row looks
    perm_disc[env_index] = grid[:, 2]
    return dict(env_index=env_index, action=grid[:, 1].astype(np.int32), state=state,
                step_ctr=np.full(B, ctr0, np.int32), active=np.ones(B, np.uint8),
                steps_total=rs.randint(0, 50, B).astype(np.int32), illegal_total=rs.randint(0, 50, B).astype(np.int32),
                solved=np.zeros(B, np.uint8), perm_disc=perm_disc, perm_peg=grid[:, 3].astype(np.int32),
                noise=_noise_rows(rs, rows, 3 * n) if noisy else None,
                obs=rs.random_sample((B, 3 * n)).astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("ctr0", [0, ALL_MAX_STEPS - 1, ALL_MAX_STEPS - 2])
def test_kernel_all_states_actions_discs_pegs(oracle, ctr0, noisy):
    inp = _all_inputs(ctr0, noisy)
    want = check_kernel(oracle, 3, ALL_MAX_STEPS, inp)
    rows = inp["env_index"]
    assert want["err_count"][0] == 0 and set(want["reward"].tolist()) == {-1, 0, 1}
    assert want["solved"][rows].sum() == (want["reward"] == 1).sum() > 0
    ended = want["done"].astype(bool)
    assert ended.all() if ctr0 == ALL_MAX_STEPS - 1 else (ended.any() and not ended.all())
    # an env whose step ended the episode keeps its obs row; the others got a new one
    assert np.array_equal(want["obs"][rows[ended]], inp["obs"][rows[ended]])
    assert not (want["obs"][rows[~ended]] == inp["obs"][rows[~ended]]).all(1).any()
    if not noisy and not ended.all():  # a permuted observation is one-hot and differs from the true state's
        live = rows[~ended]
        assert np.isin(want["obs"][live], (0.0, 1.0)).all()
        true = np.stack([_onehot64(s) for s in want["state"][live]])
        assert (want["obs"][live] != true).any(1).sum() > 0 and (want["obs"][live] == true).all(1).sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("noisy", [False, True])
def test_kernel_observe_only_and_inactive_rows(oracle, noisy):
    """action NULL: nothing is stepped, no tally changes, the active envs get their (perturbed) observation and
    the finished ones keep theirs; without env_index row j is env j"""
    n, B = 3, 300
    rs = np.random.RandomState(5)
    inp = dict(env_index=None, action=None, state=rs.randint(0, 3, (B, n)).astype(np.uint8),
               step_ctr=rs.randint(0, 9, B).astype(np.int32), active=(rs.random_sample(B) < 0.7).astype(np.uint8),
               steps_total=rs.randint(0, 50, B).astype(np.int32), illegal_total=rs.randint(0, 50, B).astype(np.int32),
               solved=rs.randint(0, 2, B).astype(np.uint8), perm_disc=rs.randint(-1, n, B).astype(np.int32),
               perm_peg=rs.randint(0, 3, B).astype(np.int32), noise=_noise_rows(rs, B, 3 * n) if noisy else None,
               obs=rs.random_sample((B, 3 * n)).astype(np.float32))
    inp["perm_peg"][inp["perm_disc"] < 0] = 7  # never read there
    want = check_kernel(oracle, n, 9, inp)
    off = inp["active"] == 0
    assert off.any() and np.array_equal(want["obs"][off], inp["obs"][off]) and want["err_count"][0] == 0
    for k in ("state", "step_ctr", "active", "steps_total", "illegal_total", "solved"):
        assert np.array_equal(want[k], inp[k]), k
    assert not want["reward"].any() and not want["done"].any()
    # the same through an env_index over a third of the envs, with a step: finished envs stay untouched
    idx = rs.permutation(B)[:100].astype(np.int32)
    inp2 = dict(inp, env_index=idx, action=rs.randint(0, 6, 100).astype(np.int32), perm_peg=inp["perm_peg"][idx],
                noise=None if inp["noise"] is None else inp["noise"][idx])
    want2 = check_kernel(oracle, n, 9, inp2)
    named_off = idx[inp["active"][idx] == 0]
    assert len(named_off) and np.array_equal(want2["steps_total"][named_off], inp["steps_total"][named_off])
    assert (want2["steps_total"].astype(int) - inp["steps_total"]).sum() == int(inp["active"][idx].sum())


@pytest.mark.gpu
def test_kernel_error_rows(oracle):
    """each error adds 1 to err_count and skips its row entirely (env, tallies, obs, reward, done); what is not
    needed is not checked (perm_peg without a disc, anything on a finished env); the neighbours are correct"""
    n, B = 3, 10
    state = np.zeros((B, n), np.uint8)
    state[3] = (0, 2, 2)
    inp = dict(
        env_index=np.array([0, 1, 2, 3, 4, 5, 6, 7, 10, -1, 8], np.int32),
        #              ok  a=6 a=-1 goal pd=3 pd=-2 peg=3 peg=-1 e=10 e=-1 off
        action=np.array([0, 6, -1, 1, 0, 0, 0, 0, 0, 0, 6], np.int32),
        perm_peg=np.array([9, 0, 0, 0, 0, 0, 3, -1, 0, 0, 5], np.int32),  # row 0 has no disc: the 9 is not read
        state=state, step_ctr=np.zeros(B, np.int32), active=np.array([1] * 8 + [0, 1], np.uint8),
        steps_total=np.zeros(B, np.int32), illegal_total=np.zeros(B, np.int32), solved=np.zeros(B, np.uint8),
        perm_disc=np.array([-1, 0, 0, 2, 3, -2, 1, 1, 7, 0], np.int32),  # env 8 is finished: its 7 is not read
        noise=None, obs=np.full((B, 3 * n), 0.25, np.float32))
    want = check_kernel(oracle, n, 30, inp)
    assert want["err_count"][0] == 8
    assert want["steps_total"].tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 0, 0] and want["solved"].tolist() == [0, 0, 0, 1] + [0] * 6
    assert want["reward"].tolist() == [0, 0, 0, 1] + [0] * 7 and want["done"].tolist() == [0, 0, 0, 1] + [0] * 7
    assert (want["obs"][1:] == 0.25).all() and want["obs"][0].tolist() == [0, 1, 0, 1, 0, 0, 1, 0, 0]
    # observe-only: the action checks do not apply, the perturbation checks do
    inp2 = dict(inp, action=None)
    want2 = check_kernel(oracle, n, 30, inp2)
    assert want2["err_count"][0] == 6 and not want2["steps_total"].any()
    assert (want2["obs"][[4, 5, 6, 7, 8, 9]] == 0.25).all() and (want2["obs"][[0, 1, 2, 3]] != 0.25).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 32])
def test_kernel_smallest_and_largest_disc_count(oracle, n):
    """N = 1 (every state and action; the goal is one move away) and N = 32 (random states, some a move from
    the goal), discs and pegs at random, noise on, counters next to max_steps"""
    rs = np.random.RandomState(n)
    B = 18 if n == 1 else 40
    if n == 1:
        state = np.repeat(np.arange(3, dtype=np.uint8), 6)[:, None]
        action = np.tile(np.arange(6, dtype=np.int32), 3)
    else:
        state = rs.randint(0, 3, (B, n)).astype(np.uint8)
        action = rs.randint(0, 6, B).astype(np.int32)
        state[:8, 1:] = 2  # disc 0 alone decides: its move to peg 2 reaches the goal, another one misses it
        state[:8, 0] = [0, 0, 1, 1, 0, 1, 0, 1]
        action[:8] = [1, 0, 3, 2, 1, 3, 4, 5]
    idx = rs.permutation(B).astype(np.int32)
    inp = dict(env_index=idx, action=action[idx], state=state, step_ctr=rs.randint(6, 9, B).astype(np.int32),
               active=np.ones(B, np.uint8), steps_total=np.zeros(B, np.int32), illegal_total=np.zeros(B, np.int32),
               solved=np.zeros(B, np.uint8), perm_disc=rs.randint(-1, n, B).astype(np.int32),
               perm_peg=rs.randint(0, 3, B).astype(np.int32), noise=_noise_rows(rs, B, 3 * n)[:, :3 * n],
               obs=rs.random_sample((B, 3 * n)).astype(np.float32))
    want = check_kernel(oracle, n, 9, inp)
    assert want["err_count"][0] == 0 and want["solved"].any() and not want["solved"].all()
    assert want["done"].any() and not want["done"].all() and want["illegal_total"].any()


# ---------------------------------------------------------------------------- play_perturbed == play
@pytest.mark.gpu
@pytest.mark.parametrize("B,kernel", [(48, "mzh_search_one_kernel"), (600, "mzh_search_kernel")])
@pytest.mark.parametrize("temperature,deterministic", [(1.0, False), (0.0, True)])
def test_play_perturbed_without_perturbation_equals_play(B, kernel, temperature, deterministic):
    from muzero_hanoi_amd import _lib
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay

    n, S, max_steps = 3, 25, 20
    assert _lib.search_plan(33, B, S, minmax_in=True)["kernel"].startswith(kernel)
    sp = BatchedSelfPlay(_fresh_net(n), n, max_steps, S)
    starts = np.random.RandomState(2).randint(0, 3 ** n - 1, B)
    mm0 = np.stack([np.linspace(-2.0, 0.0, B), np.linspace(0.5, 3.0, B)], 1)
    mm0[::3] = (-np.inf, np.inf)
    kw = dict(temperature=temperature, deterministic=deterministic, seed=9, minmax=mm0)
    ref = sp.play(starts, **kw)
    steps = ref["steps"].cpu().numpy()
    assert steps.min() < max_steps and steps.max() == max_steps  # episodes end at different moves
    for extra in (dict(), dict(noise_std=0.0, permute_disc=-1), dict(noise_std=np.zeros(B), permute_disc=[None] * B)):
        got = sp.play_perturbed(starts, **kw, **extra)
        for k in ("steps", "illegal", "start_idx"):
            assert torch.equal(got[k], ref[k]), k
        assert np.array_equal(_bits(got["minmax"].cpu().numpy()), _bits(ref["minmax"].cpu().numpy()))
        solved = got["solved"].cpu().numpy()  # an episode shorter than max_steps ended on the goal
        assert solved.dtype == np.uint8 and np.array_equal(solved[steps < max_steps], np.ones((steps < max_steps).sum()))


# ---------------------------------------------------------------------------- mixed conditions against the oracle
def oracle_play_perturbed(oracle, flats, net_index, n, S, max_steps, starts, std, disc, seed, mm0=None,
                          temperature=0.0, deterministic=True, alpha=0.25, draw_index=None):
    """play_perturbed's episodes on oracle.search (carried bounds) + oracle.env_step, the observations built in
    NumPy from the same synthetic_draws / perturbation_draws: row j of a draw for the j-th unfinished env, or,
    with draw_index, row draw_index[b] of a draw of max(draw_index) + 1 rows for env b"""
    B = len(starts)
    n_draw = lambda idx: len(idx) if draw_index is None else int(np.max(draw_index)) + 1
    rows = lambda x, idx: None if x is None else (x[:len(idx)] if draw_index is None else x[np.asarray(draw_index)[idx]])
    gen, pgen = np.random.default_rng(seed), mrng.perturbation_seeds(seed)
    st = np.stack([(np.asarray(starts) // 3 ** (n - 1 - d)) % 3 for d in range(n)], 1).astype(np.uint8)
    ctr, alive = np.zeros(B, int), np.ones(B, bool)
    obs = np.zeros((B, 3 * n), np.float32)
    mm = np.tile([-np.inf, np.inf], (B, 1)) if mm0 is None else np.array(mm0, np.float64)
    steps, illegal, solved = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.uint8)

    def observe(idx):
        peg, z = (rows(x, idx) for x in mrng.perturbation_draws(n_draw(idx), 3 * n, int(pgen.integers(2**31))))
        for j, b in enumerate(idx):
            if alive[b]:
                seen = st[b].copy()
                if disc[b] >= 0:
                    seen[disc[b]] = peg[j]
                obs[b] = (_onehot64(seen) + std[b] * z[j]).astype(np.float32)

    observe(np.arange(B))
    first = dict(obs=obs.copy())
    while alive.any():
        idx = np.nonzero(alive)[0]
        noise, tie, u = (rows(x, idx) for x in mrng.synthetic_draws(
            n_draw(idx), deterministic=deterministic, alpha=alpha, seed=int(gen.integers(2**31))))
        action = np.zeros(len(idx), np.int32)
        for m in range(len(flats)):
            sel = np.nonzero(net_index[idx] == m)[0]
            if len(sel):
                o = oracle.search(n, S, obs[idx[sel]], flat=flats[m], support=33,
                                  noise=None if noise is None else noise[sel], tie_idx=tie[sel],
                                  action_u=None if u is None else u[sel], temperature=temperature,
                                  deterministic=deterministic, minmax_in=mm[idx[sel]])
                mm[idx[sel]] = np.stack([o["mm_max"], o["mm_min"]], 1)
                action[sel] = o["action"]
        if "tie" not in first:
            first.update(tie=tie, action=action.copy())
        for j, b in enumerate(idx):
            code, s2, _, c2, _, d, ill = oracle.env_step(st[b], int(action[j]), int(ctr[b]), 1, max_steps)
            st[b], ctr[b] = s2, c2
            steps[b] += 1
            illegal[b] += ill
            solved[b] |= code == 1
            alive[b] = not d
        observe(idx)
    return dict(steps=steps, illegal=illegal, solved=solved, minmax=mm), first


MIXED = [("baseline",), ("noise", 0.1), ("noise", 0.5), ("permute", 0), ("permute", 1), ("permute", 2)]
# permutation_importance.py:143-156's twelve starts
STARTS12 = [(0, 0, 0), (1, 1, 1), (0, 1, 2), (2, 1, 0), (0, 0, 1), (1, 0, 0), (2, 2, 0), (1, 2, 1), (0, 2, 2), (2, 0, 1),
            (1, 1, 0), (0, 2, 1)]


def _s0_net(oracle):
    from muzero_hanoi_amd.networks import MuZeroNet

    w, in_dim, sup = oracle.load_weights_npz(f"{GOLDEN}/weights_N3_s0.npz")
    net = MuZeroNet(in_dim, 6, 0.002, "cpu", TD_return=sup == 33)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in w.items()})
    return net


def _three_nets(oracle):
    """weights_N3_s0 and two copies with a re-initialised head (policy, value)"""
    from muzero_hanoi_amd import acting

    base = _s0_net(oracle)
    torch.manual_seed(17)
    nets = [base, acting.get_ablated_network(base, ablate_policy=True),
            acting.get_ablated_network(base, ablate_value=True)]
    sd = [n.state_dict() for n in nets]
    assert not torch.equal(sd[0]["policy_net.0.weight"], sd[1]["policy_net.0.weight"])
    assert torch.equal(sd[0]["value_net.0.weight"], sd[1]["value_net.0.weight"])
    assert not torch.equal(sd[0]["value_net.2.weight"], sd[2]["value_net.2.weight"])
    assert torch.equal(sd[0]["policy_net.2.bias"], sd[2]["policy_net.2.bias"])
    return nets


def _mixed_case(oracle, nets, S, max_steps, seed):
    from muzero_hanoi_amd.engine import flat_weights
    from muzero_hanoi_amd.networks import NetworkSet
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay, perturbed_layout, state_index

    n = 3
    lay = perturbed_layout(len(nets), MIXED, [state_index(s) for s in STARTS12], n)
    B = len(lay["start_idx"])
    assert B == len(nets) * 72
    multi = len(nets) > 1
    sp = BatchedSelfPlay(NetworkSet(nets) if multi else nets[0], n, max_steps, S)
    got = sp.play_perturbed(lay["start_idx"], noise_std=lay["noise_std"], permute_disc=lay["permute_disc"], seed=seed,
                            net_index=lay["net_index"] if multi else None)
    want, first = oracle_play_perturbed(oracle, [flat_weights(x.state_dict()) for x in nets], lay["net_index"], n, S,
                                        max_steps, lay["start_idx"], lay["noise_std"], lay["permute_disc"], seed)
    for k in ("steps", "illegal", "solved"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert np.array_equal(_bits(got["minmax"].cpu().numpy()), _bits(want["minmax"]))
    assert np.array_equal(got["start_idx"].cpu().numpy(), lay["start_idx"])
    return lay, want, first


@pytest.mark.gpu
def test_play_perturbed_mixed_conditions_vs_oracle(oracle):
    """72 agents of one network (S = 25, the latency kernel), episodes of at most 6 moves"""
    from muzero_hanoi_amd.engine import flat_weights
    from muzero_hanoi_amd.selfplay import index_state

    net = _s0_net(oracle)
    lay, want, first = _mixed_case(oracle, [net], 25, 6, 3)
    assert 0 < want["solved"].sum() < 72 and want["steps"].min() < 6 and want["illegal"].any()
    # precondition: the perturbations change decisions (a kernel that ignored them would not pass) -- the first
    # move searched from the true observations, under the same draws, differs on perturbed rows only
    true = np.stack([_onehot64(np.array(index_state(int(i), 3))) for i in lay["start_idx"]]).astype(np.float32)
    o = oracle.search(3, 25, true, flat=flat_weights(net.state_dict()), support=33, tie_idx=first["tie"],
                      temperature=0.0, deterministic=True)
    changed = o["action"] != first["action"]
    assert np.array_equal(first["obs"][:12], true[:12]) and not changed[:12].any()
    assert changed[12:36].any() and changed[36:].any()  # under noise, and under a permuted disc


@pytest.mark.gpu
def test_play_perturbed_mixed_conditions_network_set_vs_oracle(oracle):
    """216 agents of three networks (S = 10, one mzh_search_multi launch per move), at most 6 moves"""
    lay, want, _ = _mixed_case(oracle, _three_nets(oracle), 10, 6, 4)
    per_net = want["illegal"].reshape(3, -1)
    assert not np.array_equal(per_net[0], per_net[1]) and not np.array_equal(per_net[0], per_net[2])


@pytest.mark.gpu
def test_play_perturbed_draw_index_vs_oracle(oracle):
    """draw_index: every env takes its own row of each draw whatever its rank among the unfinished (what lets
    evaluate_perturbed slice a batch); stochastic searches, so all three search draws are indexed too"""
    from muzero_hanoi_amd.engine import flat_weights
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay, state_index

    n, S, max_steps, seed = 3, 10, 6, 8
    net = _s0_net(oracle)
    starts = np.array([state_index(s) for s in STARTS12] * 2)
    B = len(starts)
    std = np.where(np.arange(B) % 3 == 1, 0.4, 0.0)
    disc = np.where(np.arange(B) % 3 == 2, (np.arange(B) // 3) % 3, -1).astype(np.int32)
    draw_index = np.random.RandomState(4).permutation(60)[:B] + 7  # scattered rows of a draw of up to 67
    kw = dict(temperature=1.0, deterministic=False)
    got = BatchedSelfPlay(net, n, max_steps, S).play_perturbed(starts, noise_std=std, permute_disc=disc, seed=seed,
                                                               draw_index=draw_index, **kw)
    flat = [flat_weights(net.state_dict())]
    want, _ = oracle_play_perturbed(oracle, flat, np.zeros(B, int), n, S, max_steps, starts, std, disc, seed,
                                    draw_index=draw_index, **kw)
    for k in ("steps", "illegal", "solved"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert np.array_equal(_bits(got["minmax"].cpu().numpy()), _bits(want["minmax"]))
    ranked, _ = oracle_play_perturbed(oracle, flat, np.zeros(B, int), n, S, max_steps, starts, std, disc, seed, **kw)
    assert not np.array_equal(ranked["illegal"], want["illegal"])  # precondition: the rows taken matter
    assert want["steps"].min() < max_steps  # some env leaves early: ranks and rows then part ways


# ---------------------------------------------------------------------------- evaluate_perturbed
@pytest.mark.gpu
def test_evaluate_perturbed_scores_and_slicing(oracle):
    from muzero_hanoi_amd.selfplay import evaluate_perturbed

    nets = _three_nets(oracle)[:2]
    conds = [("baseline",), ("noise", 0.3), ("permute", 0), ("permute", 2)]
    starts = STARTS12[:9] + [(1, 2, 2), (2, 1, 2), (2, 2, 1)]  # three of them a move or three from the goal
    kw = dict(conditions=conds, starts=starts, n_sims=25, max_steps=10, seed=6)
    one = evaluate_perturbed(nets, 3, **kw)
    M, C, E = 2, 4, 12
    assert one["solve_rate"].shape == one["importance"].shape == (M, C) and one["solved"].shape == (M * C * E,)
    s = one["solved"].reshape(M, C, E)
    assert np.array_equal(one["solve_rate"], s.sum(2) / E) and 0 < s.sum() < s.size
    assert np.isnan(one["importance"][:, :2]).all()
    assert np.array_equal(one["importance"][:, 2:], one["solve_rate"][:, :1] - one["solve_rate"][:, 2:])
    assert np.all(np.diff(one["net_index"]) >= 0) and one["steps"].max() == 10 and one["steps"].min() >= 1
    sliced = evaluate_perturbed(nets, 3, max_roots=40, **kw)  # 96 rows as 40 + 40 + 16, the cuts inside a network
    for k in ("solved", "steps", "illegal", "net_index", "cond_index", "start_idx"):
        assert np.array_equal(sliced[k], one[k]), k
    assert np.array_equal(_bits(sliced["solve_rate"]), _bits(one["solve_rate"]))
    single = evaluate_perturbed(nets[1], 3, **kw)  # one network alone: its rows take other draws, the layout holds
    assert single["solved"].shape == (C * E,) and np.array_equal(single["start_idx"], one["start_idx"][:C * E])


# ---------------------------------------------------------------------------- the drop-ins on the fixtures
def _dropin(n, max_steps, n_sims):
    from muzero_hanoi_amd import acting
    from muzero_hanoi_amd.env import TowersOfHanoi
    from muzero_hanoi_amd.mcts import MCTS

    env = TowersOfHanoi(N=n, max_steps=max_steps)
    mcts = MCTS(discount=0.8, root_dirichlet_alpha=0.25, n_simulations=n_sims, batch_s=1, device="cpu")
    seen, inner = [], mcts.run_mcts

    def run_mcts(state, network, temperature, deterministic):
        assert temperature == 0 and deterministic is True
        seen.append(np.array(state, copy=True))
        out = inner(state, network, temperature, deterministic)
        seen.append(int(out[0]))
        return out

    mcts.run_mcts = run_mcts
    return acting, env, mcts, seen


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["noise", "permute"])
def test_dropins_on_the_reference_fixtures(name):
    """the reference's recorded games replayed through a RecordedNetwork: the observation handed to run_mcts at
    every decision == the float32 the reference's network saw, bit for bit; actions, solved flags, RNG position"""
    from muzero_hanoi_amd.mcts import RecordedNetwork

    g = golden(f"perturb_{name}.npz")
    n = int(g["n"])
    acting, env, mcts, seen = _dropin(n, int(g["max_game_steps"]), int(g["n_sims"]))
    net = RecordedNetwork(recorded_calls(g), n)
    np.random.seed(int(g["seed"]))
    solved = []
    for cond, start in zip(g["cond"], g["start"]):
        s = tuple(int(x) for x in start)
        if name == "noise":
            solved.append(acting.noise_play_game(net, env, s, int(g["max_game_steps"]), mcts, noise_std=float(cond)))
        else:
            solved.append(acting.permutation_play_game(net, env, s, int(g["max_game_steps"]), mcts,
                                                       permute_feature=None if cond < 0 else int(cond)))
    post = np.random.random_sample(3)
    assert np.array_equal(np.array(solved, np.uint8), g["solved"]) and net.cursor == len(g["run_S"])
    obs = np.stack([x.astype(np.float32) for x in seen[0::2]])
    assert all(x.dtype == np.float64 for x in seen[0::2])  # oneHot_encoding's float64, rounded by the search
    assert np.array_equal(_bits(obs), _bits(g["run_obs"]))
    assert np.array_equal(seen[1::2], g["actions"])
    assert (mcts.min_max_stats.maximum, mcts.min_max_stats.minimum) == tuple(g["mm"][-1])
    assert np.array_equal(post, g["post_rng"]), "RNG stream position differs"


def _oracle_games(oracle, flat, kind, values, starts, n, S, max_steps):
    """both play_game loops restated on oracle.search + oracle.env_step, draws from the global NumPy stream
    in the reference's order (the perturbation's draw, then the search's), one MinMaxStats chain"""
    mm = np.array([[-np.inf, np.inf]])
    actions, solved = [], []
    for v in values:
        for start in starts:
            st, ctr, won = np.array(start, np.uint8), 0, False
            for _ in range(max_steps):
                seen = st.copy()
                if kind == "permute" and v is not None:
                    seen[v] = np.random.randint(0, 3)
                obs = _onehot64(seen)
                if kind == "noise" and v > 0:
                    obs = obs + np.random.normal(0.0, v, size=obs.shape)
                _, tie, _ = mrng.predraw(1, deterministic=True, alpha=0.25)
                o = oracle.search(n, S, obs[None].astype(np.float32), flat=flat, support=33, tie_idx=tie,
                                  temperature=0.0, deterministic=True, minmax_in=mm)
                mm = np.stack([o["mm_max"], o["mm_min"]], 1)
                actions.append(int(o["action"][0]))
                code, st, _, ctr, _, d, _ = oracle.env_step(st, actions[-1], ctr, 1, max_steps)
                won = code == 1
                if d:
                    break
            solved.append(won)
    return actions, solved, mm


@pytest.mark.gpu
@pytest.mark.parametrize("kind,values", [("noise", [0.0, 0.4]), ("permute", [None, 0, 2])])
def test_dropins_with_a_network_vs_oracle(oracle, kind, values):
    from muzero_hanoi_amd.engine import flat_weights

    n, S, max_steps = 3, 25, 8
    net = _s0_net(oracle)
    starts = [(1, 2, 2), (2, 1, 0), (0, 0, 0)]
    acting, env, mcts, seen = _dropin(n, max_steps, S)
    np.random.seed(31)
    solved = []
    for v in values:
        for s in starts:
            if kind == "noise":
                solved.append(acting.noise_play_game(net, env, s, max_steps, mcts, noise_std=v))
            else:
                solved.append(acting.permutation_play_game(net, env, s, max_steps, mcts, permute_feature=v))
    post = np.random.random_sample(3)
    np.random.seed(31)
    want_a, want_s, want_mm = _oracle_games(oracle, flat_weights(net.state_dict()), kind, values, starts, n, S, max_steps)
    assert seen[1::2] == want_a and solved == want_s
    assert (mcts.min_max_stats.maximum, mcts.min_max_stats.minimum) == tuple(want_mm[0])
    assert np.array_equal(np.random.random_sample(3), post), "RNG stream position differs"


@pytest.mark.gpu
@pytest.mark.parametrize("kind,value", [("noise", 0.4), ("permute", 1)])
def test_run_evaluation_is_the_rate_of_its_games(oracle, kind, value):
    net = _s0_net(oracle)
    starts = [(1, 2, 2), (2, 1, 0), (0, 0, 0), (0, 2, 2)]
    acting, env, mcts, _ = _dropin(3, 8, 25)
    play, rate = ((acting.noise_play_game, acting.noise_run_evaluation) if kind == "noise" else
                  (acting.permutation_play_game, acting.permutation_run_evaluation))
    np.random.seed(32)
    games = [play(net, env, s, 8, mcts, value) for s in starts]
    post = np.random.random_sample(3)
    acting, env, mcts, _ = _dropin(3, 8, 25)  # a fresh MinMaxStats chain, the same stream
    np.random.seed(32)
    assert rate(net, env, starts, 8, mcts, value) == sum(games) / len(games)
    assert np.array_equal(np.random.random_sample(3), post)
