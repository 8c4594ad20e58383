"""Generate the input-saliency fixture tests/golden/saliency_n3.npz from the reference itself.

    python tests/golden/gen_saliency_golden.py

Like gen_legality_golden.py (whose import set-up it uses, through gen_golden.py) it runs only where the reference
is present, never writes into the reference tree and saves inputs and outputs only.

It calls the reference's own gradient_analysis.compute_saliency (:354-391) for all 27 states of N = 3 (in
TowersOfHanoi.states order, which is selfplay.state_index's) under three networks: the reference-written
checkpoint tests/golden/muzero_model_N3.pt, gradient_analysis.ablate_networks(net, policy=True) and
ablate_networks(net, value=True) of it, both drawn in that order under one torch.manual_seed(seed).  The module
reads a global `env` (for env.n_pegs), which is set here as the script's main sets it.

The fixture holds: the seed; the re-initialised policy_net tensors of the policy-ablated copy and value_net tensors
of the value-ablated copy (their other tensors are the checkpoint's); the states; per (network, state) the two
float32 saliency vectors and the index of the policy logit the reference differentiated (its argmax).
"""
import os

import numpy as np
import torch

from gen_golden import HERE, TowersOfHanoi
from gen_plan_golden import load_net

import gradient_analysis as ga  # noqa: E402  (the reference's, on gen_golden's sys.path)

POLICY_KEYS = ("policy_net.0.weight", "policy_net.0.bias", "policy_net.2.weight", "policy_net.2.bias")
VALUE_KEYS = ("value_net.0.weight", "value_net.0.bias", "value_net.2.weight", "value_net.2.bias")


def gen_saliency(n=3, seed=211):
    base = load_net(n)
    torch.manual_seed(seed)
    pol = ga.ablate_networks(base, policy=True)
    val = ga.ablate_networks(base, value=True)
    env = TowersOfHanoi(N=n, max_steps=200)
    ga.env = env
    states = [tuple(s) for s in env.states]
    assert len(states) == 3 ** n
    policy = np.zeros((3, len(states), 3 * n), np.float32)
    value = np.zeros_like(policy)
    picked = np.zeros((3, len(states)), np.int32)
    for m, net in enumerate((base, pol, val)):
        net.eval()
        for s, st in enumerate(states):
            sal = ga.compute_saliency(st, n, net, 0)
            assert sal["policy"].dtype == np.float32 and sal["value"].dtype == np.float32
            policy[m, s], value[m, s] = sal["policy"], sal["value"]
            with torch.no_grad():
                x = torch.tensor(ga.oneHot_encoding(st, n_integers=env.n_pegs), dtype=torch.float32)[None]
                picked[m, s] = int(net.prediction(net.represent(x))[0].argmax(dim=1).item())
    psd, vsd = pol.state_dict(), val.state_dict()
    np.savez_compressed(
        os.path.join(HERE, "saliency_n3.npz"), n=n, seed=seed, states=np.array(states, np.uint8),
        policy=policy, value=value, picked=picked,
        **{"policy_ablated." + k: psd[k].numpy() for k in POLICY_KEYS},
        **{"value_ablated." + k: vsd[k].numpy() for k in VALUE_KEYS})
    return policy.shape, picked


if __name__ == "__main__":
    print(gen_saliency())
