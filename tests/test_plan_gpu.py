"""Plan-ahead acting on the GPU (acting_experiments/planning_multiple_actions.py:111-183).

  kernel    mzh_env_run_plan against k applications of mzh_env_step and against oracle.env_step (every
            3-disk state x every ordered pair of moves, counters next to max_steps), random plans through
            env_index with sentinel padding around every array, error rows;
  batched   BatchedSelfPlay.play_plans against the same episodes simulated with oracle.search (its latent
            path) + oracle.env_step, on the latency kernel's and the cooperative kernel's paths;
  drop-in   acting.plan_multiple_actions on the reference's recorded runs (tests/golden/plan_*.npz), and the
            sequential / batched forms against each other.
All comparisons are exact (integers and float64 bit patterns).
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from conftest import golden
from muzero_hanoi_amd import rng as mrng
from test_plan_cpu import PLAN, recorded_calls

PAD = 64  # sentinel elements before and after every array handed to the kernel


def _padded(arr, fill, dev):
    """a device copy of `arr` inside a buffer with PAD sentinel elements on both sides: (buffer, view)"""
    a = np.ascontiguousarray(arr)
    buf = torch.full((a.size + 2 * PAD,), fill, dtype=torch.from_numpy(a).dtype, device=dev)
    view = buf[PAD:PAD + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return buf, view


def _pads_intact(buf, fill):
    return bool((buf[:PAD] == fill).all() and (buf[-PAD:] == fill).all())


def run_plan_raw(n_disks, max_steps, L, stride, bufs, n_rows, B, env_index=True):
    """mzh_env_run_plan through the C ABI on the views of `bufs` (name -> (buffer, view))"""
    from muzero_hanoi_amd import _lib

    a = _lib.PlanArgs()
    a.n_disks, a.goal_peg, a.max_steps, a.B, a.n, a.max_plan_len, a.plan_stride = n_disks, 2, max_steps, B, n_rows, L, stride
    for k in ("plan", "plan_len", "state", "step_ctr", "active", "obs", "executed", "steps_total", "illegal_total",
              "rec_action", "rec_reward", "err_count"):
        setattr(a, k, bufs[k][1].data_ptr())
    if env_index:
        a.env_index = bufs["env_index"][1].data_ptr()
    dev = bufs["state"][1].device
    _lib.check(_lib.lib().mzh_env_run_plan(ctypes.byref(a), _lib.stream_handle(dev)), "mzh_env_run_plan")
    torch.cuda.synchronize(dev)


def oracle_run_plan(oracle, n_disks, max_steps, L, env_index, plan, plan_len, state, ctr, active, obs, steps_total,
                    illegal_total):
    """the kernel's contract on oracle.env_step; returns the expected value of every array"""
    n = len(env_index)
    state, ctr, active, obs = state.copy(), ctr.copy(), active.copy(), obs.copy()
    steps_total, illegal_total = steps_total.copy(), illegal_total.copy()
    executed = np.zeros(n, np.int32)
    rec_a = np.full((L, n), -1, np.int32)
    rec_r = np.zeros((L, n), np.int8)
    errors = 0
    for j, e in enumerate(env_index):
        if not active[e]:
            continue
        if plan_len[j] < 1:
            errors += 1
            continue
        k = 0
        while k < min(plan_len[j], L) and active[e]:
            a = int(plan[j, k])
            if not 0 <= a < 6:
                errors += 1
                break
            code, s2, moved, c2, a2, _, ill = oracle.env_step(state[e], a, int(ctr[e]), 1, max_steps)
            state[e], ctr[e], active[e] = s2, c2, a2
            obs[e] = 0
            obs[e, np.arange(n_disks) * 3 + moved] = 1
            rec_a[k, j], rec_r[k, j] = a, code
            illegal_total[e] += ill
            steps_total[e] += 1
            k += 1
        executed[j] = k
    return dict(state=state, step_ctr=ctr, active=active, obs=obs, steps_total=steps_total,
                illegal_total=illegal_total, executed=executed, rec_action=rec_a, rec_reward=rec_r, err_count=errors)


def _make_bufs(dev, n_disks, L, env_index, plan, plan_len, state, ctr, active, obs, steps_total, illegal_total):
    n = len(plan_len)
    return dict(
        env_index=_padded(np.asarray(env_index, np.int32), -9, dev), plan=_padded(plan.astype(np.int32), 99, dev),
        plan_len=_padded(plan_len.astype(np.int32), 99, dev), state=_padded(state.astype(np.uint8), 77, dev),
        step_ctr=_padded(ctr.astype(np.int32), -7, dev), active=_padded(active.astype(np.uint8), 9, dev),
        obs=_padded(obs.astype(np.float32), -5.0, dev), steps_total=_padded(steps_total.astype(np.int32), -3, dev),
        illegal_total=_padded(illegal_total.astype(np.int32), -4, dev),
        executed=_padded(np.full(n, -8, np.int32), -8, dev), rec_action=_padded(np.full((L, n), -6, np.int32), -6, dev),
        rec_reward=_padded(np.full((L, n), 55, np.int8), 55, dev), err_count=_padded(np.zeros(1, np.int32), -2, dev))


FILLS = dict(env_index=-9, plan=99, plan_len=99, state=77, step_ctr=-7, active=9, obs=-5.0, steps_total=-3,
             illegal_total=-4, executed=-8, rec_action=-6, rec_reward=55, err_count=-2)


def _check_against(bufs, want, inputs):
    for k, (buf, view) in bufs.items():
        assert _pads_intact(buf, FILLS[k]), f"padding of {k} overwritten"
        got = view.cpu().numpy()
        exp = want[k] if k in want else inputs[k]
        assert np.array_equal(got.reshape(np.shape(exp)), exp), k


# ---------------------------------------------------------------------------- every state x every pair of moves
PAIRS_MAX_STEPS = 9


def _pairs_inputs(ctr0):
    n = 3
    states = np.array(list(itertools.product(range(3), repeat=n)), np.uint8)
    pairs = np.array(list(itertools.product(range(6), repeat=2)), np.int32)
    state = np.repeat(states, len(pairs), 0)
    plan = np.tile(pairs, (len(states), 1))
    B = len(plan)
    assert B == 972
    obs = np.zeros((B, 3 * n), np.float32)
    obs[np.arange(B)[:, None], np.arange(n) * 3 + state] = 1
    return dict(env_index=np.arange(B, dtype=np.int32), plan=plan, plan_len=np.full(B, 2, np.int32), state=state,
                step_ctr=np.full(B, ctr0, np.int32), active=np.ones(B, np.uint8), obs=obs,
                steps_total=np.zeros(B, np.int32), illegal_total=np.zeros(B, np.int32))


def _pairs_oracle(oracle, ctr0, L):
    i = _pairs_inputs(ctr0)
    return oracle_run_plan(oracle, 3, PAIRS_MAX_STEPS, L, i["env_index"], i["plan"], i["plan_len"], i["state"],
                           i["step_ctr"], i["active"], i["obs"], i["steps_total"], i["illegal_total"])


@pytest.mark.gpu
@pytest.mark.parametrize("L", [2, 1])
@pytest.mark.parametrize("ctr0", [0, PAIRS_MAX_STEPS - 1, PAIRS_MAX_STEPS - 2])
def test_kernel_all_states_all_move_pairs(oracle, ctr0, L):
    """legal-then-illegal, goal on the first move, the dropped second move, max_steps on the first or second
    move: the kernel == L applications of mzh_env_step == L applications of oracle.env_step"""
    from muzero_hanoi_amd import engine

    dev = torch.device("cuda", torch.cuda.current_device())
    i = _pairs_inputs(ctr0)
    B = 972
    bufs = _make_bufs(dev, 3, L, i["env_index"], i["plan"], i["plan_len"], i["state"], i["step_ctr"], i["active"],
                      i["obs"], i["steps_total"], i["illegal_total"])
    run_plan_raw(3, PAIRS_MAX_STEPS, L, 2, bufs, B, B, env_index=False)
    want = _pairs_oracle(oracle, ctr0, L)
    two = L == 2 and ctr0 != PAIRS_MAX_STEPS - 1  # at max_steps - 1 every first move ends the episode
    assert want["err_count"] == 0 and set(np.unique(want["executed"])) == ({1, 2} if two else {1})
    _check_against(bufs, want, i)
    # the existing step kernel, applied L times (a second step on a finished env is refused and leaves it untouched)
    t = lambda k, dt: torch.tensor(i[k], dtype=dt, device=dev)
    st, ctr, act = t("state", torch.uint8), t("step_ctr", torch.int32), t("active", torch.uint8)
    obs = t("obs", torch.float32)
    executed = torch.zeros(B, dtype=torch.int32, device=dev)
    illegal = torch.zeros(B, dtype=torch.int32, device=dev)
    rec_a = torch.full((L, B), -1, dtype=torch.int32, device=dev)
    rec_r = torch.zeros((L, B), dtype=torch.int8, device=dev)
    for k in range(L):
        was = act.clone().bool()
        o = torch.empty_like(obs)
        a = torch.tensor(i["plan"][:, k].copy(), device=dev)
        code, _, ill = engine.env_step(3, PAIRS_MAX_STEPS, st, a, ctr, act, obs=o)
        obs = torch.where(was[:, None], o, obs)
        executed += was.int()
        illegal += (ill.bool() & was).int()
        rec_a[k] = torch.where(was, a, rec_a[k])
        rec_r[k] = torch.where(was, code, rec_r[k])
    for k, v in (("state", st), ("step_ctr", ctr), ("active", act), ("obs", obs), ("executed", executed),
                 ("illegal_total", illegal), ("steps_total", executed), ("rec_action", rec_a), ("rec_reward", rec_r)):
        assert torch.equal(bufs[k][1].reshape(v.shape), v), k


# ---------------------------------------------------------------------------- random plans through env_index
@pytest.mark.gpu
def test_kernel_random_plans_through_env_index(oracle):
    """N = 4, 400 envs of which a shuffled 300 are rows (a ragged last workgroup), plan lengths 1..9 cut at 7,
    stride 12, some envs finished on entry, counters near max_steps, plan entries beyond plan_len = 99 (an
    error if read), sentinels around every array and in the 100 envs no row names"""
    n, B, rows, L, stride, max_steps = 4, 400, 300, 7, 12, 10
    rs = np.random.RandomState(7)
    dev = torch.device("cuda", torch.cuda.current_device())
    env_index = rs.permutation(B)[:rows].astype(np.int32)
    plan_len = rs.randint(1, 10, rows).astype(np.int32)
    plan = np.full((rows, stride), 99, np.int32)
    for j in range(rows):
        plan[j, :plan_len[j]] = rs.randint(0, 6, plan_len[j])
    state = rs.randint(0, 3, (B, n)).astype(np.uint8)
    ctr = rs.randint(0, max_steps, B).astype(np.int32)
    active = (rs.random_sample(B) < 0.85).astype(np.uint8)
    obs = rs.random_sample((B, 3 * n)).astype(np.float32)  # untouched where nothing executes
    steps_total = rs.randint(0, 50, B).astype(np.int32)
    illegal_total = rs.randint(0, 50, B).astype(np.int32)
    untouched = np.setdiff1d(np.arange(B), env_index)
    assert len(untouched) == 100
    state[untouched], ctr[untouched], active[untouched], obs[untouched] = 200, -77, 1, -1.5
    inputs = dict(env_index=env_index, plan=plan, plan_len=plan_len, state=state, step_ctr=ctr, active=active, obs=obs,
                  steps_total=steps_total, illegal_total=illegal_total)
    want = oracle_run_plan(oracle, n, max_steps, L, env_index, plan, plan_len, state, ctr, active, obs, steps_total,
                           illegal_total)
    ex = want["executed"]
    assert want["err_count"] == 0 and ex.min() == 0 and ex.max() == 7 and (ex[plan_len > 7] < 7).any()
    assert (active[env_index] == 0).any() and (want["active"][env_index] != active[env_index]).any()
    bufs = _make_bufs(dev, n, L, env_index, plan, plan_len, state, ctr, active, obs, steps_total, illegal_total)
    run_plan_raw(n, max_steps, L, stride, bufs, rows, B)
    _check_against(bufs, want, inputs)
    for k in ("state", "step_ctr", "active", "obs", "steps_total", "illegal_total"):
        assert np.array_equal(bufs[k][1].cpu().numpy()[untouched], inputs[k][untouched]), k


# ---------------------------------------------------------------------------- error rows
@pytest.mark.gpu
def test_kernel_error_rows(oracle):
    """plan_len 0 on an active env and an action of 6 where it would execute add to err_count and end the row;
    a 6 behind the cut, behind the end of an episode or on a finished env is never read as an action; an env
    index outside the batch is an error that touches nothing; the neighbours are correct"""
    n, B, L, stride, max_steps = 3, 8, 3, 5, 30
    dev = torch.device("cuda", torch.cuda.current_device())
    state = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 2, 2], [0, 0, 0], [0, 0, 0], [1, 1, 1], [0, 0, 0]], np.uint8)
    plan = np.array([[0, 1, 3, 6, 6],    # three legal moves; the 6 is behind the cut
                     [0, 0, 0, 0, 0],    # plan_len 0, active: error
                     [0, 6, 1, 0, 0],    # one move, then the 6 would execute: error after 1 step
                     [1, 6, 6, 6, 6],    # reaches the goal on the first move: the 6 is dropped with the plan
                     [6, 6, 6, 6, 6],    # finished env: nothing read
                     [1, 1, 0, 0, 0],    # legal, illegal (disc 0 already there)
                     [2, 0, 0, 0, 0],    # plan_len 1
                     [0, 0, 0, 0, 0]], np.int32)  # env index outside the batch
    plan_len = np.array([5, 0, 3, 4, 0, 2, 1, 2], np.int32)
    active = np.array([1, 1, 1, 1, 0, 1, 1, 1], np.uint8)
    env_index = np.array([0, 1, 2, 3, 4, 5, 6, 8], np.int32)
    ctr = np.zeros(B, np.int32)
    obs = np.full((B, 3 * n), 0.25, np.float32)
    tot = np.zeros(B, np.int32)
    inputs = dict(env_index=env_index, plan=plan, plan_len=plan_len, state=state, step_ctr=ctr, active=active, obs=obs,
                  steps_total=tot, illegal_total=tot)
    ok = env_index < B
    want = oracle_run_plan(oracle, n, max_steps, L, env_index[ok], plan[ok], plan_len[ok], state, ctr, active, obs,
                           tot, tot)
    for k, fill in (("executed", 0), ("rec_action", -1), ("rec_reward", 0)):  # the out-of-batch row: nothing ran
        want[k] = np.concatenate([want[k], np.full(want[k].shape[:-1] + (1,), fill, want[k].dtype)], -1)
    want["err_count"] += 1
    assert want["err_count"] == 3 and want["executed"].tolist() == [3, 0, 1, 1, 0, 2, 1, 0]
    assert want["illegal_total"].tolist() == [0, 0, 0, 0, 0, 1, 0, 0] and want["active"].tolist() == [1, 1, 1, 0, 0, 1, 1, 1]
    bufs = _make_bufs(dev, n, L, env_index, plan, plan_len, state, ctr, active, obs, tot, tot)
    run_plan_raw(n, max_steps, L, stride, bufs, 8, B)
    _check_against(bufs, want, inputs)


# ---------------------------------------------------------------------------- play_plans against the oracle
def _fresh_net(n, seed=0):
    from muzero_hanoi_amd.networks import MuZeroNet

    torch.manual_seed(seed)
    return MuZeroNet(3 * n, 6, 0.002, "cpu", TD_return=True)


def _oracle_play_plans(oracle, flat, n, S, max_steps, L, starts, mm0, seed, temperature=1.0):
    B = len(starts)
    gen = np.random.default_rng(seed)
    st = np.stack([(starts // 3 ** (n - 1 - d)) % 3 for d in range(n)], 1).astype(np.uint8)
    ctr = np.zeros(B, int)
    alive = np.ones(B, bool)
    obs = np.zeros((B, 3 * n), np.float32)
    obs[np.arange(B)[:, None], np.arange(n) * 3 + st] = 1
    mm = mm0.copy()
    steps, illegal, plans = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    acts, rwds, rootq, sact = [], [], [], []
    while alive.any():
        idx = np.nonzero(alive)[0]
        noise, tie, u = mrng.synthetic_draws(len(idx), deterministic=False, alpha=0.25, seed=int(gen.integers(2**31)))
        o = oracle.search(n, S, obs[idx], flat=flat, support=33, noise=noise, tie_idx=tie, action_u=u,
                          temperature=temperature, minmax_in=mm[idx])
        mm[idx] = np.stack([o["mm_max"], o["mm_min"]], 1)
        plans[idx] += 1
        ra, rr = np.full((L, B), -1, np.int32), np.zeros((L, B), np.int8)
        rq, sa = np.zeros(B), np.full(B, -1, np.int32)
        rq[idx], sa[idx] = o["rootQ"], o["action"]
        for j, b in enumerate(idx):
            seq = o["latent"][j, :int(o["latent_len"][j])][:L]
            assert len(seq) >= 1
            for k, a in enumerate(seq):
                code, s2, moved, c2, _, d, ill = oracle.env_step(st[b], int(a), int(ctr[b]), 1, max_steps)
                st[b], ctr[b] = s2, c2
                obs[b] = 0
                obs[b, np.arange(n) * 3 + moved] = 1
                ra[k, b], rr[k, b] = a, code
                steps[b] += 1
                illegal[b] += ill
                if d:
                    alive[b] = False
                    break
        acts.append(ra), rwds.append(rr), rootq.append(rq), sact.append(sa)
    return dict(action=np.stack(acts), reward=np.stack(rwds), root_q=np.stack(rootq), search_action=np.stack(sact),
                steps=steps, illegal=illegal, plans=plans, minmax=mm)


def _play_plans_case(oracle, S, B, L, max_steps, seed, kernel_prefix):
    from muzero_hanoi_amd import _lib
    from muzero_hanoi_amd.engine import flat_weights
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay

    n = 3
    net = _fresh_net(n)
    flat = flat_weights(net.state_dict())
    assert _lib.search_plan(33, B, S, minmax_in=True)["kernel"].startswith(kernel_prefix)
    starts = np.random.RandomState(1).randint(0, 3 ** n - 1, B)
    mm0 = np.stack([np.linspace(-2.0, 0.0, B), np.linspace(0.5, 3.0, B)], 1)  # agents with history
    mm0[::3] = (-np.inf, np.inf)  # and fresh ones
    res = BatchedSelfPlay(net, n, max_steps, S).play_plans(starts, L, temperature=1.0, seed=seed, minmax=mm0)
    want = _oracle_play_plans(oracle, flat, n, S, max_steps, L, starts, mm0, seed)
    for k, v in want.items():
        got = res[k].cpu().numpy()
        assert got.shape == v.shape and np.array_equal(got, v), k
    assert np.array_equal(res["steps"].cpu().numpy(), (want["action"] >= 0).sum((0, 1)))
    assert np.array_equal(res["start_idx"].cpu().numpy(), starts)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 3, 7])
def test_play_plans_vs_oracle(oracle, L):
    """48 agents (with and without MinMaxStats history), the latency kernel writing the paths"""
    want = _play_plans_case(oracle, 12, 48, L, 15, 5, "mzh_search_one_kernel")
    assert want["plans"].max() > 1 and (want["action"][:, :L] >= 0).any()
    if L == 1:  # a plan of one move: a search per step, the executed move being the last simulation's first
        assert np.array_equal(want["plans"], want["steps"])


@pytest.mark.gpu
def test_play_plans_vs_oracle_cooperative_kernel(oracle):
    """S = 200: the tree does not fit the latency kernel, the cooperative kernel writes the paths"""
    _play_plans_case(oracle, 200, 3, 7, 15, 6, "mzh_search_kernel")


# ---------------------------------------------------------------------------- the drop-in on the fixtures
def _dropin(g, alpha):
    from muzero_hanoi_amd import acting
    from muzero_hanoi_amd.env import TowersOfHanoi
    from muzero_hanoi_amd.mcts import MCTS

    env = TowersOfHanoi(N=int(g["n"]) if g is not None else 3, max_steps=int(g["max_steps"]) if g is not None else 30)
    return acting, env, MCTS(discount=0.8, root_dirichlet_alpha=alpha, n_simulations=1, batch_s=1, device="cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", PLAN)
def test_plan_multiple_actions_dropin_on_fixture(name):
    from muzero_hanoi_amd.mcts import RecordedNetwork

    g = golden(f"plan_{name}.npz")
    acting, env, mcts = _dropin(g, float(g["alpha"]))
    start = None if int(g["start"]) < 0 else int(g["start"])
    assert acting.get_starting_state(env, start) == str(g["start_label"])
    net = RecordedNetwork(recorded_calls(g), int(g["n"]))
    trace = []
    np.random.seed(int(g["seed"]))
    data = acting.plan_multiple_actions(env, start, net, mcts, int(g["episodes"]), [int(b) for b in g["budgets"]],
                                        float(g["temperature"]), max_plan_len=int(g["max_plan_len"]), trace=trace)
    assert data == g["data"].tolist()
    assert net.cursor == len(g["run_S"])
    assert np.array_equal(np.concatenate([t[1] for t in trace]), g["actions"])
    assert np.array_equal(np.concatenate([t[2] for t in trace]), g["plan_lens"])
    assert np.array_equal(np.array([t[0] for t in trace]), g["ep_start"])
    assert (mcts.min_max_stats.maximum, mcts.min_max_stats.minimum) == tuple(g["mm"][-1])
    assert np.array_equal(np.random.random_sample(3), g["post_rng"]), "RNG stream position differs"


@pytest.mark.gpu
@pytest.mark.parametrize("name", PLAN)
def test_evaluate_sequential_on_fixture(name):
    """the batched evaluator in the reference's schedule (B = 1 play_plans per episode, RecordedNetwork)"""
    from muzero_hanoi_amd.mcts import RecordedNetwork
    from muzero_hanoi_amd.selfplay import evaluate

    g = golden(f"plan_{name}.npz")
    net = RecordedNetwork(recorded_calls(g), int(g["n"]))
    np.random.seed(int(g["seed"]))
    start = None if int(g["start"]) < 0 else str(g["start_label"])
    out = evaluate(net, int(g["n"]), [int(b) for b in g["budgets"]], episodes=int(g["episodes"]), start=start,
                   max_steps=int(g["max_steps"]), temperature=float(g["temperature"]), sequential=True,
                   max_plan_len=int(g["max_plan_len"]), dirichlet_alpha=float(g["alpha"]))
    assert out["data"] == g["data"].tolist()
    assert np.array_equal(np.concatenate(out["steps"]), g["ep_steps"])
    assert np.array_equal(np.concatenate(out["errors"]), g["ep_error"])
    ill, p = [], 0
    for s in g["ep_steps"]:
        ill.append(int(g["env_illegal"][p:p + s].sum()) / int(s))
        p += s
    assert np.array_equal(np.concatenate(out["illegal_rates"]), np.array(ill))
    assert tuple(out["minmax"][0]) == tuple(g["mm"][-1])
    assert np.array_equal(np.random.random_sample(3), g["post_rng"]), "RNG stream position differs"


@pytest.mark.gpu
def test_play_plans_one_env_on_fixture():
    """the fixed-start fixture's episodes one by one through play_plans (B = 1, the global stream, the
    MinMaxStats chain carried by hand): executed moves, reward codes, plans, illegal counts, each search's
    action and root Q"""
    from muzero_hanoi_amd.mcts import RecordedNetwork
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay, state_index

    g = golden("plan_es_l7.npz")
    net = RecordedNetwork(recorded_calls(g), int(g["n"]))
    sp = BatchedSelfPlay(net, int(g["n"]), int(g["max_steps"]), int(g["budgets"][0]), dirichlet_alpha=float(g["alpha"]))
    code = {0.0: 0, 100.0: 1, -0.1: -1}
    np.random.seed(int(g["seed"]))
    mm, p, q = None, 0, 0
    for ep in range(int(g["episodes"])):
        res = sp.play_plans([state_index(g["ep_start"][ep])], int(g["max_plan_len"]),
                            temperature=float(g["temperature"]), legacy_rng=True, minmax=mm)
        mm = res["minmax"].cpu().numpy()
        s, k = int(g["ep_steps"][ep]), int(g["ep_nplans"][ep])
        a = res["action"].cpu().numpy()[:, :, 0].reshape(-1)
        r = res["reward"].cpu().numpy()[:, :, 0].reshape(-1)
        assert np.array_equal(a[a >= 0], g["actions"][p:p + s])
        assert np.array_equal(r[a >= 0], [code[float(x)] for x in g["env_rwd"][p:p + s]])
        assert (int(res["steps"][0]), int(res["plans"][0])) == (s, k)
        assert int(res["illegal"][0]) == int(g["env_illegal"][p:p + s].sum())
        assert np.array_equal((res["action"].cpu().numpy()[:, :, 0] >= 0).sum(1)[:-1], g["plan_lens"][q:q + k - 1])
        assert np.array_equal(res["search_action"].cpu().numpy()[:, 0], g["search_action"][q:q + k])
        assert np.array_equal(res["root_q"].cpu().numpy()[:, 0], g["root_q"][q:q + k])
        p, q = p + s, q + k
    assert tuple(mm[0]) == tuple(g["mm"][-1])
    assert np.array_equal(np.random.random_sample(3), g["post_rng"]), "RNG stream position differs"


# ---------------------------------------------------------------------------- sequential and batched forms
@pytest.mark.gpu
def test_evaluate_sequential_equals_dropin_on_a_network():
    from muzero_hanoi_amd.selfplay import evaluate

    net = _fresh_net(3)
    acting, env, mcts = _dropin(None, 0.25)
    env.max_steps = 20
    budgets, L = [5, 20], 3
    np.random.seed(11)
    trace = []
    data = acting.plan_multiple_actions(env, None, net, mcts, 3, budgets, 0.5, max_plan_len=L, trace=trace)
    post = np.random.random_sample(3)
    np.random.seed(11)
    out = evaluate(net, 3, budgets, episodes=3, start=None, max_steps=20, temperature=0.5, sequential=True,
                   max_plan_len=L)
    assert out["data"] == data
    assert np.array_equal(np.concatenate(out["steps"]), [len(t[1]) for t in trace])
    assert tuple(out["minmax"][0]) == (mcts.min_max_stats.maximum, mcts.min_max_stats.minimum)
    assert np.array_equal(np.random.random_sample(3), post), "RNG stream position differs"


@pytest.mark.gpu
def test_play_plans_one_env_equals_one_dropin_episode():
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay, state_index

    net = _fresh_net(3)
    acting, env, mcts = _dropin(None, 0.25)
    env.max_steps = 25
    assert acting.get_starting_state(env, 0) == "ES"
    mcts.min_max_stats.maximum, mcts.min_max_stats.minimum = 0.25, -0.5
    np.random.seed(123)
    trace = []
    data = acting.plan_multiple_actions(env, 0, net, mcts, 1, [30], 1.0, max_plan_len=7, trace=trace)
    post = np.random.random_sample(3)
    np.random.seed(123)
    res = BatchedSelfPlay(net, 3, 25, 30).play_plans([state_index((2, 2, 0))], 7, temperature=1.0, legacy_rng=True,
                                                     minmax=[[0.25, -0.5]])
    a = res["action"].cpu().numpy()
    assert a.shape[1:] == (7, 1)
    a = a[:, :, 0].reshape(-1)
    assert np.array_equal(a[a >= 0], trace[0][1])
    assert int(res["plans"][0]) == len(trace[0][2]) and int(res["steps"][0]) == len(trace[0][1])
    assert data == [[30, int(res["steps"][0]) - 7]]
    assert tuple(res["minmax"].cpu().numpy()[0]) == (mcts.min_max_stats.maximum, mcts.min_max_stats.minimum)
    assert np.array_equal(np.random.random_sample(3), post), "RNG stream position differs"


# ---------------------------------------------------------------------------- argument errors (before any device use)
def test_argument_errors():
    from muzero_hanoi_amd import acting
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay, evaluate

    with pytest.raises(ValueError, match="max_plan_len"):
        evaluate(None, 3, [25], episodes=1, max_plan_len=0)
    with pytest.raises(ValueError, match="n_simulations >= 1"):
        evaluate(None, 3, [25, 0], episodes=1, max_plan_len=7)
    with pytest.raises(ValueError, match="n_simulations >= 1"):
        acting.plan_multiple_actions(None, 0, None, None, 1, [0], 0.0)
    with pytest.raises(ValueError, match="n_simulations >= 1"):
        BatchedSelfPlay(None, 3, 30, 0).play_plans([0], 7)
    with pytest.raises(ValueError, match="max_plan_len"):
        BatchedSelfPlay(None, 3, 30, 5).play_plans([0], 0)
