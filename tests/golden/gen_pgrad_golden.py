"""Generate the parameter-gradient fixture tests/golden/pgrad_n3.npz from the reference itself.

    python tests/golden/gen_pgrad_golden.py

Like gen_saliency_golden.py (whose import set-up it uses, through gen_golden.py) it runs only where the reference
is present, never writes into the reference tree and saves inputs and outputs only.

It calls the reference's own gradient_analysis.get_results (:274-338) under the three networks of
saliency_n3.npz -- the reference-written checkpoint tests/golden/muzero_model_N3.pt and the policy-ablated and
value-ablated copies stored there, loaded, not drawn again -- for all 27 states of N = 3 (TowersOfHanoi.states
order, selfplay.state_index's) with action s % 6.  The module reads a global `env` (for env.n_pegs), which is set
here as the script's main sets it.

The fixture holds: the states and actions; per (network, state) the reference's bias gradients of the five
sub-networks, which are the deltas -- delta1 [3][27][5][256] (the Linear0 biases) and delta2 [3][27][5][64] (the
Linear2 biases, zero beyond the net's outputs); and the full 20 gradient tensors of the script's default pair
(state 0_0_0, action 0) under the checkpoint, under their state_dict keys with the prefix "grad.".
"""
import copy
import os

import numpy as np
import torch

from gen_golden import HERE, TowersOfHanoi
from gen_plan_golden import load_net

import gradient_analysis as ga  # noqa: E402  (the reference's, on gen_golden's sys.path)

NETS = ("representation", "dynamic", "reward", "policy", "value")
MODULES = ("representation_net", "dynamic_net", "rwd_net", "policy_net", "value_net")


def fixture_networks(n):
    base = load_net(n)
    g = np.load(os.path.join(HERE, "saliency_n3.npz"))
    nets = [base]
    for prefix in ("policy_ablated.", "value_ablated."):
        net = copy.deepcopy(base)
        sd = net.state_dict()
        for k in g.files:
            if k.startswith(prefix):
                sd[k[len(prefix):]] = torch.from_numpy(g[k].copy())
        net.load_state_dict(sd)
        nets.append(net)
    return nets


def gen_pgrad(n=3):
    env = TowersOfHanoi(N=n, max_steps=200)
    ga.env = env
    states = [tuple(s) for s in env.states]
    assert len(states) == 3 ** n
    actions = np.arange(len(states), dtype=np.int32) % 6
    delta1 = np.zeros((3, len(states), 5, 256), np.float32)
    delta2 = np.zeros((3, len(states), 5, 64), np.float32)
    full = {}
    for m, net in enumerate(fixture_networks(n)):
        net.eval()
        for s, st in enumerate(states):
            res = ga.get_results(net, st, int(actions[s]))
            for i, name in enumerate(NETS):
                w0, b0, w2, b2 = (t.detach().numpy() for t in res[name])
                assert b0.dtype == np.float32 and b0.shape == (256,) and w0.shape[0] == 256 and w2.shape == (len(b2), 256)
                delta1[m, s, i] = b0
                delta2[m, s, i, :len(b2)] = b2
                if m == 0 and s == 0:
                    for key, t in zip(("0.weight", "0.bias", "2.weight", "2.bias"), (w0, b0, w2, b2)):
                        full[f"grad.{MODULES[i]}.{key}"] = t.copy()
    assert states[0] == (0,) * n and actions[0] == 0
    path = os.path.join(HERE, "pgrad_n3.npz")
    np.savez_compressed(path, n=n, states=np.array(states, np.uint8), actions=actions, delta1=delta1, delta2=delta2, **full)
    return delta1.shape, os.path.getsize(path)


if __name__ == "__main__":
    print(gen_pgrad())
