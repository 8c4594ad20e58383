"""Generate the perturbed-observation acting fixtures tests/golden/perturb_<case>.npz from the reference itself.

    python tests/golden/gen_perturb_golden.py

Like gen_golden.py (whose import set-up and recording helpers it uses) it runs only where the reference
is present, never writes into the reference tree and saves inputs and outputs only.

It calls the reference's own noise_injection_comparison.play_game (:17-37) and permutation_importance.play_game
(:27-76) on the reference's MCTS, TowersOfHanoi and MuZeroNet, game after game as the scripts' run_evaluation
loops do: one MCTS instance (its MinMaxStats chain) and one env for every game of a fixture, the global NumPy
stream seeded once.  The network is the reference-written checkpoint tests/golden/muzero_model_N3.pt.

Each fixture holds: the configuration and seed; per game its condition (the noise std, or the permuted disc
with -1 for None), start state, number of decisions and the returned solved flag; per decision the float32
observation the reference handed to initial_inference (run_obs) and every network output (run_*, the format of
the acting_<case>.npz fixtures), the returned action, root Q and the MinMaxStats after it, and env.step's
reward, done and illegal flag; three np.random.random_sample() values drawn after the run.
"""
import os

import numpy as np

from gen_golden import HERE, Recorder, _ActingMCTS, _pack_runs, _split_calls, _traced_env
from gen_plan_golden import load_net

import noise_injection_comparison as nic  # noqa: E402  (the reference's, on gen_golden's sys.path)
import permutation_importance as pim  # noqa: E402

# one and three moves from the goal (this checkpoint solves few states within 12 steps) and the far corner
STARTS = [(1, 2, 2), (2, 1, 2), (0, 0, 0)]

PERTURB_CASES = [
    # name, the reference's play_game, its keyword, the keyword's values, n_simulations, max_game_steps, seed
    ("noise", nic.play_game, "noise_std", [0.0, 0.3], 25, 12, 101),
    ("permute", pim.play_game, "permute_feature", [None, 0, 2], 10, 12, 102),
]


def gen_perturb(name, play_game, key, values, n_sims, max_game_steps, seed, n=3):
    rec = Recorder(load_net(n))
    env = _traced_env(n, max_game_steps)  # both scripts: TowersOfHanoi(N, max_steps=max_game_steps)
    mcts = _ActingMCTS(discount=0.8, root_dirichlet_alpha=0.25, n_simulations=n_sims, batch_s=1, device="cpu")
    mcts.trace = []
    np.random.seed(seed)
    cond, start, solved, decisions = [], [], [], []
    for v in values:
        for s in STARTS:
            before = len(mcts.trace)
            solved.append(bool(play_game(rec, env, s, max_game_steps, mcts, **{key: v})))
            cond.append(-1.0 if v is None else float(v))
            start.append(s)
            decisions.append(len(mcts.trace) - before)
    post = np.random.random_sample(3)
    runs = _split_calls(rec.calls)
    tr = np.array(mcts.trace, np.float64).reshape(-1, 4)
    et = np.array(env.trace, np.float64).reshape(-1, 4)
    assert len(runs) == len(tr) == len(et) == sum(decisions)
    packed = _pack_runs(runs)
    obs32 = np.array([x for kind, x, _, _ in rec.calls if kind == "i"])
    assert obs32.dtype == np.float32 and np.array_equal(obs32.astype(np.float64), packed["run_obs"])
    packed["run_obs"] = obs32
    np.savez_compressed(
        os.path.join(HERE, f"perturb_{name}.npz"), n=n, n_sims=n_sims, max_game_steps=max_game_steps, seed=seed,
        kind=name, cond=np.array(cond, np.float64), start=np.array(start, np.uint8),
        solved=np.array(solved, np.uint8), decisions=np.array(decisions, np.int32),
        actions=tr[:, 0].astype(np.int32), root_q=tr[:, 1], mm=tr[:, 2:], env_rwd=et[:, 1],
        env_done=et[:, 2].astype(np.int32), env_illegal=et[:, 3].astype(np.int32), **packed, post_rng=post)
    return solved, decisions


if __name__ == "__main__":
    for c in PERTURB_CASES:
        print(c[0], gen_perturb(*c))
