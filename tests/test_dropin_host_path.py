"""The drop-in's one-root host path (MCTS.run_mcts: staging record, draws by rng.predraw_into, the cached argument
block, the result reader) against the generic one (Engine.search at B = 1 fed rng.predraw draws and the carried
MinMaxStats): the same kernel instantiation, so every result must agree bit for bit.  This pins the host path; it
is no oracle comparison of the latency kernel."""
import numpy as np
import pytest
import torch

STATES = [(0, 0, 0), (2, 2, 0), (0, 0, 2), (1, 2, 2)]


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


@pytest.mark.gpu
@pytest.mark.parametrize("temperature,deterministic", [(1.0, False), (0.5, True)])
def test_run_mcts_equals_engine_search(temperature, deterministic):
    from muzero_hanoi_amd import rng as mrng
    from muzero_hanoi_amd.mcts import MCTS
    from muzero_hanoi_amd.networks import MuZeroNet, engine_for

    n, S = 3, 25
    torch.manual_seed(0)
    net = MuZeroNet(3 * n, 6, 0.002, "cuda", TD_return=True)
    mcts = MCTS(discount=0.8, root_dirichlet_alpha=0.25, n_simulations=S, batch_s=256, device="cpu")
    eng = engine_for(net, S, 1)
    saved = np.random.get_state()
    try:
        np.random.seed(41)
        rs = np.random.RandomState(41)
        mm = torch.tensor([[-float("inf"), float("inf")]], dtype=torch.float64, device=eng.device)
        for call, state in enumerate(STATES):
            obs = np.zeros(3 * n)
            obs[np.arange(n) * 3 + np.array(state)] = 1
            noise, tie, u = mrng.predraw(1, deterministic=deterministic, alpha=0.25, eps=0.25, rng=rs)
            t = lambda a: None if a is None else torch.as_tensor(a).to(eng.device)
            want = eng.search(S, obs=torch.as_tensor(obs[None], dtype=torch.float32).to(eng.device), tie_idx=t(tie),
                              noise=t(noise), action_u=t(u), minmax_in=mm, temperature=temperature,
                              deterministic=deterministic, discount=0.8, eps=0.25)
            assert want["_plan"]["kernel"] == "mzh_search_one_kernel<true, true, true>"
            mm = want["minmax"]
            w = {k: v.cpu().numpy() for k, v in want.items() if not k.startswith("_")}
            action, pi, root_q = mcts.run_mcts(obs, net, temperature, deterministic)
            assert isinstance(action, int) and action == int(w["action"][0]), call
            assert pi.dtype == np.float64 and np.array_equal(pi, w["pi"][0]), call
            assert isinstance(root_q, float) and root_q == float(w["root_q"][0]), call
            assert (mcts.min_max_stats.maximum, mcts.min_max_stats.minimum) == tuple(w["minmax"][0].tolist()), call
            path = [int(x) for x in mcts.return_latent_actions()]
            assert path == w["latent"][0, :int(w["latent_len"][0])].tolist() and len(path) >= 1, call
            assert mcts.last_extra_ties == int(w["extra_ties"][0]), call
            assert _same_state(np.random.mtrand._rand, rs), f"NumPy global stream position after call {call}"
    finally:
        np.random.set_state(saved)
