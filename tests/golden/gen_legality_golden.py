"""Generate the legal-versus-illegal prediction fixture tests/golden/legality_n3.npz from the reference itself.

    python tests/golden/gen_legality_golden.py

Like gen_perturb_golden.py (whose import set-up and recording helpers it uses, through gen_golden.py) it runs
only where the reference is present, never writes into the reference tree and saves inputs and outputs only.

It calls the reference's own legal_illegal_preds.evaluate_network (:26-80) on the reference's MCTS, TowersOfHanoi
and MuZeroNet, as the script's main does: one env and one MCTS instance (its MinMaxStats chain) for every
network, the global NumPy stream seeded once.  The networks are the reference-written checkpoint
tests/golden/muzero_model_N3.pt and legal_illegal_preds.ablate_network(net, ablate_policy=True) of it under
torch.manual_seed(seed).  N = 3, max_steps = 12, 25 simulations, 4 episodes per network.

The fixture holds: the configuration and seed; the re-initialised policy_net tensors of the ablated copy (its
other tensors are the checkpoint's); per network its number of decisions and the returned dict (KEYS order);
per episode its start state and number of decisions; per decision every network output of the search (run_*,
the format of the acting_<case>.npz fixtures), the float32 observation handed to represent, the six predicted
(reward, value) pairs and env._move_allowed of the six moves as a bit mask (bit a: move a allowed), the returned
action, root Q and the MinMaxStats after it, and env.step's reward, done and illegal flag; three
np.random.random_sample() values drawn after the run.
"""
import os

import numpy as np
import torch

from gen_golden import HERE, Recorder, _ActingMCTS, _pack_runs, _split_calls, _traced_env
from gen_plan_golden import load_net

import legal_illegal_preds as lip  # noqa: E402  (the reference's, on gen_golden's sys.path)

KEYS = ("reward_diff_mean", "reward_diff_std", "value_diff_mean", "value_diff_std")
POLICY_KEYS = ("policy_net.0.weight", "policy_net.0.bias", "policy_net.2.weight", "policy_net.2.bias")


class ProbeRecorder(Recorder):
    """Recorder that also serves evaluate_network's direct calls: represent(state) opens a probe, the next six
    recurrent_inference calls (a = 0..5) belong to it and are recorded apart from the search's"""

    def __init__(self, net, env):
        super().__init__(net)
        self.env = env
        self.probes = []
        self._left = 0

    def represent(self, x):
        env = self.env
        mask = sum(int(bool(env._move_allowed(env.moves[a]))) << a for a in range(self.num_actions))
        self.probes.append(dict(obs=x.detach().numpy()[0].copy(), reward=[], value=[], legal=mask))
        self._left = self.num_actions
        return self.net.represent(x)

    def recurrent_inference(self, h, a):
        if not self._left:
            return super().recurrent_inference(h, a)
        out = self.net.recurrent_inference(h, a)
        p = self.probes[-1]
        assert int(a.argmax()) == len(p["reward"])
        p["reward"].append(np.float32(out[1]))
        p["value"].append(np.float32(out[3]))
        self._left -= 1
        return out


def gen_legality(n=3, n_sims=25, max_steps=12, episodes=4, seed=117):
    base = load_net(n)
    torch.manual_seed(seed)
    ablated = lip.ablate_network(base, ablate_policy=True)
    env = _traced_env(n, max_steps)
    starts = []
    reset = env.random_reset

    def random_reset():
        out = reset()
        starts.append(tuple(env.c_state))
        return out

    env.random_reset = random_reset
    mcts = _ActingMCTS(discount=0.8, root_dirichlet_alpha=0.25, n_simulations=n_sims, batch_s=1, device="cpu")
    mcts.trace = []
    np.random.seed(seed)
    dicts, calls, probes, net_decisions = [], [], [], []
    for net in (base, ablated):
        net.eval()
        rec = ProbeRecorder(net, env)
        d = lip.evaluate_network(env, mcts, rec, episodes, "cpu")
        dicts.append([d[k] for k in KEYS])
        calls += rec.calls
        probes += rec.probes
        net_decisions.append(len(rec.probes))
    post = np.random.random_sample(3)
    runs = _split_calls(calls)
    tr = np.array(mcts.trace, np.float64).reshape(-1, 4)
    et = np.array(env.trace, np.float64).reshape(-1, 4)
    assert len(runs) == len(tr) == len(et) == len(probes) == sum(net_decisions) and len(starts) == 2 * episodes
    done = et[:, 2].astype(np.int32)
    ep_steps = np.diff(np.concatenate([[0], np.nonzero(done)[0] + 1]))
    assert len(ep_steps) == 2 * episodes and ep_steps.sum() == len(probes)
    packed = _pack_runs(runs)
    obs32 = np.array([p["obs"] for p in probes])
    assert obs32.dtype == np.float32 and np.array_equal(obs32.astype(np.float64), packed["run_obs"])
    packed["run_obs"] = obs32
    sd = ablated.state_dict()
    np.savez_compressed(
        os.path.join(HERE, "legality_n3.npz"), n=n, n_sims=n_sims, max_steps=max_steps, episodes=episodes, seed=seed,
        dicts=np.array(dicts, np.float64), net_decisions=np.array(net_decisions, np.int32),
        ep_start=np.array(starts, np.uint8), ep_steps=ep_steps.astype(np.int32),
        probe_reward=np.array([p["reward"] for p in probes], np.float32),
        probe_value=np.array([p["value"] for p in probes], np.float32),
        probe_legal=np.array([p["legal"] for p in probes], np.uint8),
        actions=tr[:, 0].astype(np.int32), root_q=tr[:, 1], mm=tr[:, 2:], env_rwd=et[:, 1], env_done=done,
        env_illegal=et[:, 3].astype(np.int32), **packed, post_rng=post,
        **{"ablated." + k: sd[k].numpy() for k in POLICY_KEYS})
    return dicts, ep_steps


if __name__ == "__main__":
    print(gen_legality())
