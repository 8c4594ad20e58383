"""Acting / evaluation drop-ins: the functions the reference's acting scripts are built from, with
the same signatures, running on the drop-in TowersOfHanoi / MCTS / MuZeroNet (every search one
fused kernel launch, every env step the integer kernel).

  get_starting_state   acting_experiments/acting_ablations.py:49-68 (ES / MS / LS / random)
  ablate_networks      acting_experiments/acting_ablations.py:29-45 (head re-initialisation)
  get_results          acting_experiments/acting_ablations.py:72-128 (error vs the optimal move count
                       per simulation budget; one MCTS instance, MinMaxStats carried throughout)
  illegal_move_rate    illegal_move_rate_comparison.py:27-50 (per-episode rates: mean, std error)
  plan_multiple_actions  acting_experiments/planning_multiple_actions.py:111-183 (one search, then its
                       latent path executed open loop; a new search only when the plan ran out)

  noise_play_game / noise_run_evaluation              noise_injection_comparison.py:17-37 / 40-46 (solve rate with
                       Gaussian noise added to the observation the agent searches from)
  permutation_play_game / permutation_run_evaluation  permutation_importance.py:27-76 / 79-91 (solve rate with one
                       disc's peg replaced by a random peg in that observation)
  get_ablated_network  permutation_importance.py:17-24 (a copy with re-initialised heads)
  ablate_network / legality_evaluate_network  legal_illegal_preds.py:16-23 / 26-80 (the predicted reward and value
                       of the six moves at every decision, legal minus illegal; one mzh_probe_actions launch per
                       decision); legality_summary is its statistics, shared with selfplay.evaluate_legality

  compute_saliency / aggregate_saliency_per_disk  monosemanticity_analysis/gradient_analysis.py:354-391 / 569-592
                       (d(policy logit at its argmax)/d(obs) and d(value)/d(obs) of one state: one mzh_saliency
                       launch; selfplay.evaluate_saliency is the batched form over states and networks)
  gradient_get_results  monosemanticity_analysis/gradient_analysis.py:274-338, that script's get_results (the
                       parameter gradients of the five sub-networks for one state and action: one mzh_param_grads
                       call; selfplay.evaluate_gradients is the batched form over networks, states and actions)

They run one decision at a time, exactly as the reference does (same RNG stream, same MinMaxStats
chain); selfplay.evaluate is the batched form (sequential=True reproduces get_results, and with
max_plan_len plan_multiple_actions; selfplay.evaluate_perturbed batches the two perturbation scripts).
"""
import copy
import ctypes
import logging

import numpy as np
import torch

from . import _lib
from . import engine as _engine
from .checkpoint import ablate_networks  # noqa: F401  (acting_ablations.py:29-45; one implementation)
from .hanoi_utils import hanoi_solver
from .mcts import RecordedNetwork
from .networks import engine_for
from .selfplay import GRADIENT_NETS, START_STATES
from .staging import Packed
from .utils import oneHot_encoding

_LABELS = {0: "ES", 1: "MS", 2: "LS"}


def get_starting_state(env, start=None):
    """Point env.init_state_idx at the named start (0 = ES, 1 = MS, 2 = LS; 3-disk states chosen
    off the training trajectory) and return its file label; None leaves the env for random_reset."""
    if start is None:
        return "RandState"
    label = _LABELS[start]
    env.init_state_idx = env.states.index(START_STATES[label])
    return label


def _episode(env, start, networks, mcts, temperature, deterministic=False):
    """one episode: reset (fixed or random start), search + step until done; returns
    (start state, steps, illegal moves)"""
    c_state = env.reset() if start else env.random_reset()
    s0 = tuple(env.current_state())
    steps = illegal = 0
    done = False
    while not done:
        action, _, _ = mcts.run_mcts(c_state, networks, temperature=temperature, deterministic=deterministic)
        c_state, _, done, illegal_move = env.step(action)
        steps += 1
        illegal += int(illegal_move)
    return s0, steps, illegal


@torch.no_grad()
def get_results(env, start, networks, mcts, episode, n_mcts_simulations_range, temperature):
    """[[n_simulations, mean(steps - optimal moves)]] over `episode` episodes per budget."""
    data = []
    for n in n_mcts_simulations_range:
        mcts.n_simulations = n
        errors = []
        for _ in range(episode):
            s0, steps, _ = _episode(env, start is not None, networks, mcts, temperature)
            errors.append(steps - hanoi_solver(s0))
        data.append([n, sum(errors) / len(errors)])
    logging.info(data)
    return data


def _plan(mcts, c_state, networks, temperature, max_plan_len):
    """one search; the plan is the last simulation's selection path, cut to max_plan_len moves.  The action
    run_mcts returns is drawn (deterministic=False, as the script calls it) but not executed."""
    mcts.run_mcts(c_state, networks, temperature=temperature, deterministic=False)
    return [int(a.item()) if hasattr(a, "item") else int(a) for a in mcts.return_latent_actions()[:max_plan_len]]


@torch.no_grad()
def plan_multiple_actions(env, start, networks, mcts, episode, n_mcts_simulations_range, temperature, max_plan_len=7,
                          trace=None):
    """planning_multiple_actions.py:111-183 with get_results' arguments and return value: per episode one
    search whose latent path (mcts.return_latent_actions()[:max_plan_len]) is executed open loop, illegal
    moves included, with a new search from the current observation only when the plan ran out before the
    episode ended; reaching the goal or max_steps inside a plan drops the rest of it.  One MCTS instance
    (its MinMaxStats chain) serves every episode and budget.  Returns [[n_simulations, mean(steps - optimal
    moves)]].  A budget below 1 would execute a stale path in the reference: ValueError.
    trace: a list that receives (start state, executed actions, plan lengths) per episode."""
    if int(max_plan_len) < 1:
        raise ValueError(f"plan_multiple_actions: max_plan_len must be >= 1, got {max_plan_len}")
    if any(int(n) < 1 for n in n_mcts_simulations_range):
        raise ValueError("plan_multiple_actions: a plan needs n_simulations >= 1 in every budget")
    data = []
    for n in n_mcts_simulations_range:
        mcts.n_simulations = n
        errors = []
        for _ in range(episode):
            c_state = env.reset() if start is not None else env.random_reset()
            s0 = tuple(env.current_state())
            action_seq = _plan(mcts, c_state, networks, temperature, max_plan_len)
            executed, plan_lens = [], [len(action_seq)]
            done = False
            t = 0
            while not done:
                c_state, _, done, _ = env.step(action_seq[t])
                executed.append(action_seq[t])
                t += 1
                if t >= len(action_seq) and not done:
                    action_seq = _plan(mcts, c_state, networks, temperature, max_plan_len)
                    plan_lens.append(len(action_seq))
                    t = 0
            errors.append(len(executed) - hanoi_solver(s0))
            if trace is not None:
                trace.append((s0, executed, plan_lens))
        data.append([n, sum(errors) / len(errors)])
    logging.info(data)
    return data


def illegal_move_rate(env, networks, mcts, episodes=100, temperature=0.0, fixed_start=False):
    """(mean, standard error) of the per-episode illegal-move rates (illegal moves / moves)."""
    rates = []
    for _ in range(episodes):
        _, steps, illegal = _episode(env, fixed_start, networks, mcts, temperature)
        if steps > 0:
            rates.append(illegal / steps)
    if not rates:
        return 0.0, 0.0
    return float(np.mean(rates)), float(np.std(rates, ddof=1) / np.sqrt(len(rates)))


def get_ablated_network(networks, ablate_policy=False, ablate_value=False):
    """permutation_importance.py:17-24: a deep copy of `networks` with the policy and / or value head
    re-initialised (ablate_networks on the copy: the same draws from the global torch RNG)."""
    return ablate_networks(ablate_policy, ablate_value, False, copy.deepcopy(networks))


def ablate_network(networks, ablate_policy=False, ablate_value=False):
    """legal_illegal_preds.py:16-23: a deep copy of `networks` with the policy and / or value head re-initialised
    (policy first: the same draws from the global torch RNG)."""
    net_copy = copy.deepcopy(networks)
    if ablate_policy:
        net_copy.policy_net.apply(net_copy.reset_param)
    if ablate_value:
        net_copy.value_net.apply(net_copy.reset_param)
    return net_copy


def legality_summary(reward, value, legal, steps):
    """legal_illegal_preds.py:60-80 from the probes of every decision: reward / value [T][B][6] float32 (the
    predicted reward and value of move a at decision t of episode b), legal [T][B] uint8 (bit a: move a allowed),
    steps [B] decisions of episode b (rows t >= steps[b] are not read).  Per episode the means of its legal and
    illegal lists in the reference's append order (decision-major, move ascending), np.mean over the float64 of
    the float32 values as the reference's lists of Python floats give, 0.0 for an empty list; then the mean and
    the standard error np.std(ddof=1) / sqrt(n) of the per-episode (legal - illegal) differences, 0.0 without
    episodes.  Returns evaluate_network's dict."""
    reward, value = np.asarray(reward, np.float32), np.asarray(value, np.float32)
    legal, steps = np.asarray(legal, np.uint8), np.asarray(steps, np.int64).reshape(-1)
    mean = lambda xs: np.mean(xs) if xs else 0.0
    reward_diffs, value_diffs = [], []
    for b in range(steps.shape[0]):
        T = int(steps[b])
        ok = ((legal[:T, b, None] >> np.arange(6)) & 1).astype(bool).reshape(-1)  # decision-major, move ascending
        r = [float(x) for x in reward[:T, b].reshape(-1)]
        v = [float(x) for x in value[:T, b].reshape(-1)]
        pick = lambda xs, keep: [x for x, k in zip(xs, ok) if k == keep]
        reward_diffs.append(mean(pick(r, True)) - mean(pick(r, False)))
        value_diffs.append(mean(pick(v, True)) - mean(pick(v, False)))
    n_r, n_v = len(reward_diffs), len(value_diffs)
    return {
        "reward_diff_mean": float(np.mean(reward_diffs)) if reward_diffs else 0.0,
        "reward_diff_std": float(np.std(reward_diffs, ddof=1) / np.sqrt(n_r)) if reward_diffs else 0.0,
        "value_diff_mean": float(np.mean(value_diffs)) if value_diffs else 0.0,
        "value_diff_std": float(np.std(value_diffs, ddof=1) / np.sqrt(n_v)) if value_diffs else 0.0,
    }


class _OneRootProbe:
    """the host side of a probe of one root on `eng`: its observation and state in, the six (reward, value) pairs
    and the legal mask out, in pinned host memory the kernel addresses where the device can (one launch and one
    synchronisation per decision, as the one-root search)"""

    def __init__(self, eng):
        n = eng.n_disks
        self.eng = eng
        self.pin = Packed.mapped([("obs", torch.float32, (1, 3 * n)), ("state", torch.uint8, (1, n))], eng.device)
        self.pout = Packed.mapped([("reward", torch.float32, (1, 6)), ("value", torch.float32, (1, 6)),
                                   ("legal", torch.uint8, (1,))], eng.device)
        a = self.args = _lib.ProbeArgs()
        a.B = a.n = 1
        a.obs, a.state = self.pin.dptr["obs"], self.pin.dptr["state"]
        a.reward, a.value, a.legal = (self.pout.dptr[k] for k in ("reward", "value", "legal"))

    def __call__(self, obs, c_state):
        h = self.pin.h
        h["obs"][0] = obs  # torch.tensor(state, dtype=torch.float32), legal_illegal_preds.py:39
        h["state"][0] = c_state
        self.pin.to_device()
        _lib.check(_lib.lib().mzh_probe_actions(self.eng._h, ctypes.byref(self.args), None,
                                                _lib.stream_handle(self.eng.device)), "mzh_probe_actions")
        self.pout.to_host()
        o = self.pout.h
        return o["reward"][0].copy(), o["value"][0].copy(), int(o["legal"][0])


def _probe_decision(env, mcts, networks, state):
    """one decision's probe after its search: (reward [6], value [6] float32, legal mask).  A RecordedNetwork
    carries the probe in its recording (no probe launch; the mask is mzh_legal_mask's on the env's state)."""
    if isinstance(networks, RecordedNetwork):
        p = networks.last_probe()
        st = torch.tensor([list(env.c_state)], dtype=torch.uint8, device=env._dev)
        return (np.asarray(p["reward"], np.float32), np.asarray(p["value"], np.float32),
                int(_engine.legal_mask(env.discs, st).item()))
    eng = engine_for(networks, int(mcts.n_simulations), 1)  # the engine the search just ran on
    probe = eng.__dict__.get("_one_probe")
    if probe is None:
        probe = eng._one_probe = _OneRootProbe(eng)
    return probe(np.asarray(state).reshape(-1), env.c_state)


@torch.no_grad()
def legality_evaluate_network(env, mcts, networks, episodes, device, trace=None):
    """legal_illegal_preds.py:26-80 evaluate_network, with its signature and its dict: episodes from
    random_reset, at every decision run_mcts(temperature=0.0, deterministic=False) and then the model's predicted
    reward and value of each of the six moves from the current state, filed under legal or illegal by
    env._move_allowed; per episode the means' difference, over episodes its mean and standard error.  The same
    draws from NumPy's global stream as the reference.  The reference's seven network calls per decision
    (represent, six recurrent_inference) are one mzh_probe_actions launch of one row.  `device` is accepted as
    the reference takes it (the probe runs on the network's engine).
    trace: a list that receives per decision (reward [6] float32, value [6] float32, legal mask, action)."""
    rec_r, rec_v, rec_l, steps = [], [], [], []
    for _ in range(episodes):
        state = env.random_reset()
        done = False
        ep_r, ep_v, ep_l = [], [], []
        while not done:
            action, _, _ = mcts.run_mcts(state, networks, temperature=0.0, deterministic=False)
            r6, v6, mask = _probe_decision(env, mcts, networks, state)
            ep_r.append(r6)
            ep_v.append(v6)
            ep_l.append(mask)
            if trace is not None:
                trace.append((r6, v6, mask, int(action)))
            state, _, done, _ = env.step(action)
        rec_r.append(ep_r)
        rec_v.append(ep_v)
        rec_l.append(ep_l)
        steps.append(len(ep_l))
    T, B = max(steps, default=0), len(steps)
    reward, value = np.zeros((T, B, 6), np.float32), np.zeros((T, B, 6), np.float32)
    legal = np.zeros((T, B), np.uint8)
    for b in range(B):
        reward[:steps[b], b], value[:steps[b], b], legal[:steps[b], b] = rec_r[b], rec_v[b], rec_l[b]
    return legality_summary(reward, value, legal, steps)


def _start_game(env, start_state):
    """both play_game functions' first lines: reset, then put the env on start_state"""
    env.reset()
    env.c_state = start_state
    env.oneH_c_state = oneHot_encoding(env.c_state, n_integers=env.n_pegs)


def noise_play_game(networks, env, start_state, max_game_steps, mcts, noise_std=0.0):
    """noise_injection_comparison.py:17-37: one game from start_state; before every search the one-hot
    observation gets np.random.normal(0, noise_std) added (drawn only for noise_std > 0, before the search's
    own draws), the action is applied to the true env.  True if a step returned reward 100."""
    _start_game(env, start_state)
    for _ in range(max_game_steps):
        state_one_hot = oneHot_encoding(env.c_state, n_integers=env.n_pegs)
        if noise_std > 0:
            noise = np.random.normal(0.0, noise_std, size=state_one_hot.shape)
            state_one_hot = state_one_hot + noise
        action, _, _ = mcts.run_mcts(state_one_hot, networks, temperature=0, deterministic=True)
        _, reward, done, _ = env.step(action)
        if reward == 100:
            return True
        if done:
            return False
    return False


def noise_run_evaluation(networks, env, test_states, max_game_steps, mcts, noise_std=0.0):
    """noise_injection_comparison.py:40-46: the solve rate of `networks` over test_states under noise."""
    solved = 0
    for start_state in test_states:
        if noise_play_game(networks, env, start_state, max_game_steps, mcts, noise_std):
            solved += 1
    return solved / len(test_states)


def permutation_play_game(networks, env, start_state, max_game_steps, mcts, permute_feature=None):
    """permutation_importance.py:27-76: one game from start_state; with permute_feature the agent searches from
    the state with that disc's peg replaced by np.random.randint(0, n_pegs) (drawn before the search's own
    draws), the action is applied to the true env.  True if a step returned reward 100."""
    _start_game(env, start_state)
    for _ in range(max_game_steps):
        state_to_feed_model = env.c_state
        if permute_feature is not None:
            permuted_state_list = list(env.c_state)
            permuted_state_list[permute_feature] = np.random.randint(0, env.n_pegs)
            state_to_feed_model = tuple(permuted_state_list)
        state_one_hot = oneHot_encoding(state_to_feed_model, n_integers=env.n_pegs)
        action, _, _ = mcts.run_mcts(state_one_hot, networks, temperature=0, deterministic=True)
        _, reward, done, _ = env.step(action)
        if reward == 100:
            return True
        if done:
            return False
    return False


def permutation_run_evaluation(networks, env, test_states, max_game_steps, mcts, permute_feature=None):
    """permutation_importance.py:79-91: the solve rate of `networks` over test_states with a permuted disc."""
    solved_count = 0
    for start_state in test_states:
        if permutation_play_game(networks, env, start_state, max_game_steps, mcts, permute_feature):
            solved_count += 1
    return solved_count / len(test_states)


# ---------------------------------------------------------------------- gradient_analysis.py
def compute_saliency(state, N, networks, action):
    """gradient_analysis.py:354-391: {"policy": d(policy logit at its argmax)/d(obs), "value": d(value)/d(obs)},
    float32 [3N] each, through represent + prediction -- forward and backward one mzh_saliency launch.  `action`
    is accepted and unused, as in the reference (its dummy action only feeds the commented-out heads)."""
    eng = engine_for(networks, 0, 1)
    obs = torch.as_tensor(oneHot_encoding(state, n_integers=3), dtype=torch.float32)[None].to(eng.device)
    if obs.shape[1] != 3 * N or eng.n_disks != N:
        raise ValueError(f"compute_saliency: a state of {len(state)} discs on a {eng.n_disks}-disc network, N={N}")
    out = eng.saliency(obs)
    return {"policy": out["policy"][0].cpu().numpy(), "value": out["value"][0].cpu().numpy()}


def gradient_get_results(networks, state, action):
    """gradient_analysis.py get_results (:274-338; acting.get_results is acting_ablations.py's): {"representation", "dynamic", "reward", "policy", "value"}, each the tuple of
    four float32 tensors (Linear0 weight and bias, Linear2 weight and bias, parameters() order and shapes) the
    reference's autograd.grad of h0.mean() / h1.mean() / reward / softmax(pi_logits).mean() / value returns for that
    sub-network -- forward, backward and the dense expansion one mzh_param_grads call.  The tensors are on the CPU
    and carry no graph (the reference's create_graph=True graph is never used by the script)."""
    eng = engine_for(networks, 0, 1)
    if len(state) != eng.n_disks or any(int(p) not in (0, 1, 2) for p in state):
        raise ValueError(f"gradient_get_results: state {tuple(state)} on a {eng.n_disks}-disc network")
    if int(action) != action or not 0 <= int(action) < 6:
        raise ValueError(f"gradient_get_results: action {action} outside 0..5")
    obs = torch.as_tensor(oneHot_encoding(state, n_integers=3), dtype=torch.float32)[None].to(eng.device)
    act = torch.tensor([int(action)], dtype=torch.int32, device=eng.device)
    flat = eng.param_grads(obs, act, dense=True)["grad"][0].cpu()
    shapes = _engine.weight_shapes(eng.n_disks, eng.support)
    data, lo = {}, 0
    for i, name in enumerate(GRADIENT_NETS):
        ts = []
        for shp in shapes[4 * i: 4 * i + 4]:
            size = int(np.prod(shp))
            ts.append(flat[lo: lo + size].reshape(shp).clone())
            lo += size
        data[name] = tuple(ts)
    return data


def aggregate_saliency_per_disk(saliency_vector, num_disks=3, num_rods=3):
    """gradient_analysis.py:569-592: sum of |.| over each disc's `num_rods` elements, a list ordered small to
    large (the kernel's disc_policy / disc_value outputs are this sum in fp32, (|s0| + |s1|) + |s2|)."""
    if len(saliency_vector) != num_disks * num_rods:
        raise ValueError("Saliency vector length does not match num_disks * num_rods.")
    v = np.asarray(saliency_vector)
    return [np.sum(np.abs(v[i * num_rods:(i + 1) * num_rods])) for i in range(num_disks)]
