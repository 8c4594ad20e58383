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

They run one decision at a time, exactly as the reference does (same RNG stream, same MinMaxStats
chain); selfplay.evaluate is the batched form (sequential=True reproduces get_results, and with
max_plan_len plan_multiple_actions; selfplay.evaluate_perturbed batches the two perturbation scripts).
"""
import copy
import logging

import numpy as np
import torch

from .checkpoint import ablate_networks  # noqa: F401  (acting_ablations.py:29-45; one implementation)
from .hanoi_utils import hanoi_solver
from .selfplay import START_STATES
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
