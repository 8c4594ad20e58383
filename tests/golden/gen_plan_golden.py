"""Generate the plan-ahead acting fixtures tests/golden/plan_<case>.npz from the reference itself.

    python tests/golden/gen_plan_golden.py

Like gen_golden.py (whose import set-up and recording helpers it uses) it runs only where the reference
is present, never writes into the reference tree and saves inputs and outputs only.

The reference has the experiment as a script, acting_experiments/planning_multiple_actions.py, not as a
function; its loop (:111-183) is restated here on the reference's own MCTS, TowersOfHanoi and MuZeroNet:
per episode one run_mcts, the plan = mcts.return_latent_actions()[:max_plan_len] executed with env.step
entry by entry, a new run_mcts from the current observation only when the plan ran out before the episode
ended, error = steps - hanoi_solver(start).  One MCTS instance for every episode and budget.  The
network is the reference-written checkpoint tests/golden/muzero_model_N3.pt.

Each fixture holds: the configuration and seed; every network output per run_mcts call (run_*, the format
of the acting_<case>.npz fixtures); per search its returned action, root Q and the MinMaxStats after it;
per env.step its reward, done and illegal flag; per episode the start state, steps, error and number of
plans; the executed actions and plan lengths of all episodes concatenated; the returned data; three
np.random.random_sample() values drawn after the run.
"""
import os

import numpy as np
import torch

from gen_golden import (HERE, MuZeroNet, Recorder, _ActingMCTS, _pack_runs, _split_calls, _traced_env,
                        hanoi_solver)

START_STATES = {0: ("ES", (2, 2, 0)), 1: ("MS", (0, 0, 2)), 2: ("LS", (1, 2, 2))}  # planning_multiple_actions.py:87-101

PLAN_CASES = [
    # name, budgets, max_plan_len, episodes, start, alpha, temperature, max_steps, seed
    ("es_l7", [25], 7, 4, 0, 0.0, 0.0, 30, 91),  # the script's setting at a small budget
    ("rand_l3", [10, 50], 3, 4, None, 0.25, 0.5, 12, 92),
]


def load_net(n=3):
    net = MuZeroNet(rpr_input_s=3 * n, action_s=6, lr=0, device="cpu", TD_return=True)
    ck = torch.load(os.path.join(HERE, "muzero_model_N3.pt"), map_location="cpu", weights_only=True)
    net.load_state_dict(ck["Muzero_net"])
    return net


def gen_plan(name, budgets, max_plan_len, episodes, start, alpha, temperature, max_steps, seed, n=3):
    rec = Recorder(load_net(n))
    env = _traced_env(n, max_steps)
    label = "RandState"
    if start is not None:
        label, init_state = START_STATES[start]
        env.init_state_idx = env.states.index(init_state)
    mcts = _ActingMCTS(discount=0.8, root_dirichlet_alpha=alpha, n_simulations=budgets[0], batch_s=1, device="cpu")
    mcts.trace = []

    def plan(c_state):
        mcts.run_mcts(c_state, rec, temperature=temperature, deterministic=False)
        return mcts.return_latent_actions()[:max_plan_len]

    np.random.seed(seed)
    data, ep_start, ep_steps, ep_error, ep_nplans, actions, plan_lens = [], [], [], [], [], [], []
    for n_sims in budgets:
        mcts.n_simulations = n_sims
        errors = []
        for _ in range(episodes):
            c_state = env.reset() if start is not None else env.random_reset()
            s0 = tuple(env.current_state())  # hanoi_solver is lru_cached: a hashable state
            min_n_moves = hanoi_solver(s0)
            action_seq = plan(c_state)
            lens = [len(action_seq)]
            done = False
            step = t = 0
            while not done:
                a = action_seq[t].item()
                c_state, _, done, _ = env.step(a)
                actions.append(a)
                step += 1
                t += 1
                if t >= len(action_seq) and not done:
                    action_seq = plan(c_state)
                    lens.append(len(action_seq))
                    t = 0
            errors.append(step - min_n_moves)
            ep_start.append(s0)
            ep_steps.append(step)
            ep_error.append(step - min_n_moves)
            ep_nplans.append(len(lens))
            plan_lens += lens
        data.append([n_sims, sum(errors) / len(errors)])
    post = np.random.random_sample(3)
    tr = np.array(mcts.trace, np.float64).reshape(-1, 4)
    et = np.array(env.trace, np.float64).reshape(-1, 4)
    assert [int(x) for x in et[:, 0]] == actions and len(plan_lens) == len(tr)
    np.savez_compressed(
        os.path.join(HERE, f"plan_{name}.npz"), n=n, budgets=np.array(budgets, np.int32), episodes=episodes,
        start=-1 if start is None else start, start_label=label, init_state_idx=env.init_state_idx,
        alpha=alpha, temperature=temperature, max_plan_len=max_plan_len, max_steps=max_steps, seed=seed,
        data=np.array(data, np.float64), ep_start=np.array(ep_start, np.uint8), ep_steps=np.array(ep_steps, np.int32),
        ep_error=np.array(ep_error, np.int32), ep_nplans=np.array(ep_nplans, np.int32),
        actions=np.array(actions, np.int32), plan_lens=np.array(plan_lens, np.int32),
        search_action=tr[:, 0].astype(np.int32), root_q=tr[:, 1], mm=tr[:, 2:], env_rwd=et[:, 1],
        env_done=et[:, 2].astype(np.int32), env_illegal=et[:, 3].astype(np.int32), **_pack_runs(_split_calls(rec.calls)),
        post_rng=post)
    return ep_steps, ep_nplans, plan_lens


if __name__ == "__main__":
    for c in PLAN_CASES:
        print(c[0], gen_plan(*c))
