"""The action probe on the GPU (mzh_probe_actions: mzh_probe_kernel / mzh_probe_multi_kernel, Engine.probe_actions),
the drop-in acting.legality_evaluate_network and the batched selfplay.evaluate_legality.  Expected values come
from the calls the probe fuses (mzh_initial_inference + six mzh_recurrent_inference on the same engine), from the
C oracle composed the same way, from mzh_legal_mask, and from the reference's own run
(tests/golden/legality_n3.npz).  Every comparison is bit for bit.  The single-network tests come first in the
file, the multi-network ones after them."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
from test_legality_cpu import KEYS, fixture_flats, oracle_probe

pytestmark = pytest.mark.gpu

DEV = "cuda"
OUTPUTS = ("reward", "value", "h0", "pi0", "value0", "h1", "pi1")
WEIGHTS = [("weights_N3_s0", 3, 33), ("weights_N4_s0", 4, 33), ("weights_N3_s0_mc", 3, 1)]
NROWS = 37
FLOAT_ROWS = (1, 7, 15, 16, 36)  # rows whose observation is not a one-hot encoding


@pytest.fixture(scope="module")
def mzh():
    from muzero_hanoi_amd import _lib, engine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return engine


def tt(a):
    return torch.tensor(np.asarray(a), device=DEV)


def _states_obs(n, rows, seed):
    rs = np.random.RandomState(seed)
    st = rs.randint(0, 3, (rows, n)).astype(np.uint8)
    obs = np.zeros((rows, 3 * n), np.float32)
    obs[np.arange(rows)[:, None], np.arange(n) * 3 + st] = 1
    return st, obs, rs


def _nan_outputs(B, legal=False):
    shapes = dict(reward=(B, 6), value=(B, 6), h0=(B, 64), pi0=(B, 6), value0=(B,), h1=(B, 6, 64), pi1=(B, 6, 6))
    out = {k: torch.full(s, float("nan"), dtype=torch.float32, device=DEV) for k, s in shapes.items()}
    if legal:
        out["legal"] = torch.full((B,), 255, dtype=torch.uint8, device=DEV)
    return out


def _composition(eng, obs):
    """what the probe fuses, on the same engine: one initial_inference + six recurrent_inference calls"""
    B = obs.shape[0]
    ii = eng.initial_inference(tt(obs))
    out = dict(h0=ii["h"], pi0=ii["pi"], value0=ii["value"])
    parts = [eng.recurrent_inference(ii["h"], torch.full((B,), a, dtype=torch.int32, device=DEV)) for a in range(6)]
    out["reward"] = torch.stack([p["reward"] for p in parts], 1)
    out["value"] = torch.stack([p["value"] for p in parts], 1)
    out["h1"] = torch.stack([p["h"] for p in parts], 1)
    out["pi1"] = torch.stack([p["pi"] for p in parts], 1)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(a, b):
    """bit for bit (NaN patterns included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32 if a.itemsize == 4 else np.uint8),
                                                                        b.view(np.uint32 if b.itemsize == 4 else np.uint8))


@pytest.fixture(scope="module", params=WEIGHTS, ids=[w[0] for w in WEIGHTS])
def probe_case(request, mzh, oracle):
    """per weight fixture, computed once: the engine, 37 observations (5 of them arbitrary floats), the seven-call
    composition on the engine and the oracle composition"""
    name, n, sup = request.param
    w, in_dim, s = oracle.load_weights_npz(f"{GOLDEN}/{name}.npz")
    assert (in_dim, s) == (3 * n, sup)
    flat = oracle.flat_weights(w)
    _, obs, rs = _states_obs(n, NROWS, 31)
    for r in FLOAT_ROWS:
        obs[r] = rs.uniform(-0.5, 1.5, 3 * n).astype(np.float32)
    eng = mzh.Engine(n, 1, 64, sup)
    eng.load_weights(flat)
    comp = _composition(eng, obs)
    orc = oracle_probe(oracle, flat, n, sup, obs)
    for k in OUTPUTS:  # the two references agree with each other
        assert _same(comp[k], orc[k]), f"{name}: composition vs oracle {k}"
    assert not _same(comp["reward"][:, 0], comp["reward"][:, 1])  # the action matters
    return eng, obs, comp, orc


# ------------------------------------------------------------------------------------ single network
@pytest.mark.parametrize("tile", [16, 32])
def test_probe_equals_composition_and_oracle(probe_case, tile):
    """n in {1, 16, 17, 37} rows of a batch of 40 on both forced tiles: every output of every row equals the
    seven-call composition and the oracle; rows outside the call keep their NaN prefill"""
    eng, obs, comp, orc = probe_case
    B = 40
    full = np.zeros((B, obs.shape[1]), np.float32)
    full[:NROWS] = obs
    for n in (1, 16, 17, 37):
        out = _nan_outputs(B)
        eng.probe_actions(tt(full), env_index=torch.arange(n, dtype=torch.int32, device=DEV), out=out, tile=tile)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        for k in OUTPUTS:
            assert _same(got[k][:n], comp[k][:n]), f"tile {tile} n {n}: {k} vs the composition"
            assert _same(got[k][:n], orc[k][:n]), f"tile {tile} n {n}: {k} vs the oracle"
            assert np.isnan(got[k][n:]).all(), f"tile {tile} n {n}: {k} written outside the call"


@pytest.mark.parametrize("tile", [16, 32])
def test_gather_scatter_and_skipped_row(probe_case, tile):
    """B = 40, n = 9 with a shuffled env_index that holds one index >= B: that row is skipped, err_count == 1, the
    other eight equal the dense call's rows; only reward / value are given"""
    eng, obs, comp, _ = probe_case
    B = 40
    full = np.zeros((B, obs.shape[1]), np.float32)
    full[:NROWS] = obs
    dense = eng.probe_actions(tt(full), tile=tile)  # env_index NULL: row j is env j
    dense = {k: v.cpu().numpy() for k, v in dense.items()}
    assert sorted(dense) == ["reward", "value"]
    for k in ("reward", "value"):
        assert _same(dense[k][:NROWS], comp[k])
    env_index = np.array([36, 2, 17, 40, 0, 16, 39, 15, 7], np.int32)  # 40 is outside [0, B)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = {k: torch.full((B, 6), float("nan"), dtype=torch.float32, device=DEV) for k in ("reward", "value")}
    eng.probe_actions(tt(full), env_index=tt(env_index), out=out, err=err, tile=tile)
    assert int(err.item()) == 1
    rows = env_index[env_index < B]
    rest = np.setdiff1d(np.arange(B), rows)
    for k in ("reward", "value"):
        got = out[k].cpu().numpy()
        assert _same(got[rows], dense[k][rows]), k
        assert np.isnan(got[rest]).all(), k
    eng.probe_actions(tt(full), env_index=tt(np.array([-1, 3], np.int32)), out=out, err=err, tile=tile)
    assert int(err.item()) == 2  # the count accumulates; a negative index is outside too


@pytest.mark.parametrize("n", [3, 4])
def test_legal_mask_equals_mzh_legal_mask_on_every_state(mzh, oracle, n):
    name = f"weights_N{n}_s0"
    w, _, sup = oracle.load_weights_npz(f"{GOLDEN}/{name}.npz")
    B = 3 ** n
    states = np.array([[(i // 3 ** (n - 1 - d)) % 3 for d in range(n)] for i in range(B)], np.uint8)
    obs = np.zeros((B, 3 * n), np.float32)
    obs[np.arange(B)[:, None], np.arange(n) * 3 + states] = 1
    eng = mzh.Engine(n, 1, B, sup)
    eng.load_weights(oracle.flat_weights(w))
    want = mzh.legal_mask(n, tt(states)).cpu().numpy()
    assert np.array_equal(want, [oracle.legal_mask(s) for s in states])
    for tile in (16, 32):
        out = eng.probe_actions(tt(obs), state=tt(states), tile=tile)
        assert np.array_equal(out["legal"].cpu().numpy(), want), f"tile {tile}"
    # through env_index: only the rows of the call are written
    legal = torch.full((B,), 255, dtype=torch.uint8, device=DEV)
    idx = np.arange(B - 1, -1, -2).astype(np.int32)
    eng.probe_actions(tt(obs), state=tt(states), env_index=tt(idx), out=dict(legal=legal))
    got = legal.cpu().numpy()
    assert np.array_equal(got[idx], want[idx]) and (np.delete(got, idx) == 255).all()


def test_engine_refusals(mzh, oracle):
    """MZH_ERR_STATE without weights / without a set, MZH_ERR_CAPACITY above max_roots, n_networks above the set"""
    import ctypes

    from muzero_hanoi_amd import _lib

    eng = mzh.Engine(3, 1, 8, 33)
    obs = torch.zeros((9, 9), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="weights not loaded"):
        eng.probe_actions(obs[:4])
    w, _, _ = oracle.load_weights_npz(f"{GOLDEN}/weights_N3_s0.npz")
    eng.load_weights(oracle.flat_weights(w))
    with pytest.raises(RuntimeError, match="max_roots"):
        eng.probe_actions(obs)
    ni = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="no weight set loaded"):
        eng.probe_actions(obs[:4], net_index=ni)
    a, m = _lib.ProbeArgs(), _lib.MultiArgs()
    a.B = a.n = 4
    out = torch.zeros((2, 4, 6), dtype=torch.float32, device=DEV)
    a.obs, a.reward, a.value = obs.data_ptr(), out[0].data_ptr(), out[1].data_ptr()
    m.n_networks, m.net_index = 1, ni.data_ptr()
    L = _lib.lib()
    assert L.mzh_probe_actions(eng._h, ctypes.byref(a), ctypes.byref(m), None) == _lib.MZH_ERR_STATE
    eng.load_weight_set([oracle.flat_weights(w)] * 2)
    m.n_networks = 3
    assert L.mzh_probe_actions(eng._h, ctypes.byref(a), ctypes.byref(m), None) == _lib.MZH_ERR_ARG
    assert "n_networks=3" in _lib.last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ the fixture's networks
def _fixture_nets(oracle, g):
    """the fixture's two networks as drop-in MuZeroNets (the checkpoint and its policy-ablated copy)"""
    from muzero_hanoi_amd.networks import MuZeroNet

    nets = []
    for flat in fixture_flats(oracle, g):
        net = MuZeroNet(9, 6, 0.0, "cpu", TD_return=True)
        sd, off = {}, 0
        for k, v in net.state_dict().items():
            sd[k] = torch.from_numpy(flat[off:off + v.numel()].reshape(tuple(v.shape)).copy())
            off += v.numel()
        assert off == flat.size
        net.load_state_dict(sd)
        nets.append(net.eval())
    return nets


def _dropin(g):
    from muzero_hanoi_amd.env import TowersOfHanoi
    from muzero_hanoi_amd.mcts import MCTS

    env = TowersOfHanoi(N=int(g["n"]), max_steps=int(g["max_steps"]))
    mcts = MCTS(discount=0.8, root_dirichlet_alpha=0.25, n_simulations=int(g["n_sims"]), batch_s=1, device="cpu")
    return env, mcts


def test_dropin_replays_the_reference_run():
    """acting.legality_evaluate_network with the fixture's RecordedNetwork (search outputs and probes from the
    recording): the reference's dicts for both networks, its actions and legality, its stream position"""
    from muzero_hanoi_amd import acting
    from muzero_hanoi_amd.mcts import RecordedNetwork

    g = golden("legality_n3.npz")
    S, calls = int(g["n_sims"]), []
    for k in range(len(g["actions"])):
        sl = slice(k * S, (k + 1) * S)
        calls.append(dict(root_pi=g["run_root_pi"][k], pi=g["run_pi"][sl], reward=g["run_reward"][sl],
                          value=g["run_value"][sl], probe=dict(reward=g["probe_reward"][k], value=g["probe_value"][k])))
    net = RecordedNetwork(calls, int(g["n"]))
    env, mcts = _dropin(g)
    np.random.seed(int(g["seed"]))
    trace = []
    for m in range(2):  # one env and one MCTS instance for both networks, as the script's main
        d = acting.legality_evaluate_network(env, mcts, net, int(g["episodes"]), DEV, trace=trace)
        assert [d[k] for k in KEYS] == g["dicts"][m].tolist(), m
        assert net.cursor == int(np.cumsum(g["net_decisions"])[m])
    assert [t[3] for t in trace] == g["actions"].tolist()
    assert [t[2] for t in trace] == g["probe_legal"].tolist()
    assert (mcts.min_max_stats.maximum, mcts.min_max_stats.minimum) == tuple(g["mm"][-1])
    assert np.array_equal(np.random.random_sample(3), g["post_rng"]), "RNG stream position differs"


def test_dropin_live_equals_batched_record_per_decision(oracle):
    """per fixture start and network: the drop-in with the live network (a fresh MCTS, the start forced) and
    evaluate_legality of that one start on the same legacy draws give the same probes, masks and actions at every
    decision, the same dict; the probes also equal the oracle's on the visited states"""
    from muzero_hanoi_amd import acting
    from muzero_hanoi_amd.selfplay import evaluate_legality, state_index

    g = golden("legality_n3.npz")
    flats = fixture_flats(oracle, g)
    for m, net in enumerate(_fixture_nets(oracle, g)):
        for e, s in enumerate(g["ep_start"][:int(g["episodes"])]):
            env, mcts = _dropin(g)
            env.init_state_idx = state_index(tuple(int(x) for x in s))
            env.random_reset = env.reset  # the episode starts at s, no start draw
            trace = []
            np.random.seed(500 + e)
            d = acting.legality_evaluate_network(env, mcts, net, 1, DEV, trace=trace)
            after = np.random.random_sample(2)
            np.random.seed(500 + e)
            b = evaluate_legality(net, 3, starts=[tuple(int(x) for x in s)], n_sims=int(g["n_sims"]),
                                  max_steps=int(g["max_steps"]), legacy_rng=True, record=True)[0]
            assert np.array_equal(np.random.random_sample(2), after)
            T = int(b["steps"][0])
            assert T == len(trace) >= 1 and b["reward"].shape == (T, 1, 6)
            for t, (r6, v6, mask, action) in enumerate(trace):
                assert _same(r6, b["reward"][t, 0]) and _same(v6, b["value"][t, 0]), (m, e, t)
                assert mask == int(b["legal"][t, 0]) and action == int(b["action"][t, 0]), (m, e, t)
            assert all(np.array_equal(d[k], b[k], equal_nan=True) for k in KEYS)
            # the visited states from the start and the actions, through the oracle env
            st, ctr, active, states = np.array(s, np.uint8), 0, 1, []
            for t in range(T):
                states.append(st.copy())
                _, st, _, ctr, active, _, _ = oracle.env_step(st, trace[t][3], ctr, active, int(g["max_steps"]))
            states = np.array(states, np.uint8)
            o = oracle_probe(oracle, flats[m], 3, 33, np.eye(3, dtype=np.float32)[states].reshape(T, 9), states)
            assert _same(o["reward"], b["reward"][:, 0]) and _same(o["value"], b["value"][:, 0])
            assert np.array_equal(o["legal"], b["legal"][:, 0])


# ------------------------------------------------------------------------------------ several networks
@pytest.fixture(scope="module")
def set_case(mzh, oracle):
    """three N = 3 networks -- the fixture's checkpoint, its policy-ablated copy and another seed's weights
    (weights_N3_s0) -- as a set on one engine and alone on one engine each, with 37 + 3 probe rows"""
    g = golden("legality_n3.npz")
    w, _, _ = oracle.load_weights_npz(f"{GOLDEN}/weights_N3_s0.npz")
    flats = fixture_flats(oracle, g) + [oracle.flat_weights(w)]
    eng = mzh.Engine(3, 1, 64, 33)
    eng.load_weight_set(flats)
    singles = []
    for f in flats:
        e1 = mzh.Engine(3, 1, 64, 33)
        e1.load_weights(f)
        singles.append(e1)
    states, obs, rs = _states_obs(3, 40, 41)
    obs[5] = rs.uniform(-0.5, 1.5, 9).astype(np.float32)
    return eng, singles, states, obs


@pytest.mark.parametrize("tile", [16, 32])
@pytest.mark.parametrize("counts", [(5, 0, 20), (17, 16, 1)], ids=lambda c: "-".join(map(str, c)))
def test_multi_probe_equals_single_network_probes(set_case, counts, tile):
    eng, singles, states, obs = set_case
    n = sum(counts)
    net_index = np.repeat(np.arange(3), counts).astype(np.int32)
    B = 40
    out = _nan_outputs(B, legal=True)
    eng.probe_actions(tt(obs), env_index=torch.arange(n, dtype=torch.int32, device=DEV), state=tt(states),
                      net_index=tt(net_index), out=out, tile=tile)
    res = {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}
    status = eng.probe_actions(tt(obs[:n]), net_index=tt(net_index), tile=tile)["_status"]
    assert status.tolist() == [0, sum(-(-c // tile) for c in counts)]
    lo = 0
    for m, c in enumerate(counts):
        if c:
            one = singles[m].probe_actions(tt(obs[lo:lo + c]), state=tt(states[lo:lo + c]), full=True, tile=tile)
            for k in OUTPUTS + ("legal",):
                assert _same(res[k][lo:lo + c], one[k].cpu().numpy()), f"counts {counts} tile {tile} network {m}: {k}"
            if m:  # a kernel that ignored net_index would not pass (network 1 differs in its policy head only)
                other = singles[0].probe_actions(tt(obs[lo:lo + c]), full=True, tile=tile)
                assert not _same(res["pi1"][lo:lo + c], other["pi1"].cpu().numpy())
        lo += c
    for k in OUTPUTS:
        assert np.isnan(res[k][n:]).all(), k
    assert (res["legal"][n:] == 255).all()


@pytest.mark.parametrize("tile", [16, 32])
def test_multi_probe_refuses_a_bad_net_index_on_the_device(set_case, tile):
    """a decreasing net_index and an entry equal to M: nothing is written, status[0] == 1"""
    eng, _, states, obs = set_case
    for bad in ([0] * 10 + [2] * 5 + [1] * 6, [0] * 20 + [3]):
        ni = np.array(bad, np.int32)
        out = _nan_outputs(len(ni), legal=True)
        r = eng.probe_actions(tt(obs[:len(ni)]), state=tt(states[:len(ni)]), net_index=tt(ni), out=out, tile=tile)
        assert r["_status"].tolist() == [1, 0]
        for k in OUTPUTS:
            assert np.isnan(out[k].cpu().numpy()).all(), k
        assert (out["legal"].cpu().numpy() == 255).all()


def test_evaluate_legality_batch_equals_single_network_runs(oracle):
    """2 networks x 4 episodes as one batch == the two single-network runs (same starts, same seed)"""
    from muzero_hanoi_amd.selfplay import evaluate_legality

    g = golden("legality_n3.npz")
    nets = _fixture_nets(oracle, g)
    starts = [tuple(int(x) for x in s) for s in g["ep_start"][:int(g["episodes"])]]
    kw = dict(starts=starts, n_sims=int(g["n_sims"]), max_steps=int(g["max_steps"]), seed=7, record=True)
    both = evaluate_legality(nets, 3, **kw)
    assert len(both) == 2
    for m, net in enumerate(nets):
        one = evaluate_legality(net, 3, **kw)[0]
        assert sorted(one) == sorted(both[m]) and set(KEYS) <= set(one)
        T = int(one["steps"].max())
        for k in one:
            a, b = np.asarray(one[k]), np.asarray(both[m][k])
            if a.ndim >= 2:  # the record: the batch runs until its last episode ends
                a, b = a[:T], b[:T]
                assert both[m][k].shape[0] >= T
            assert np.array_equal(a, b, equal_nan=True), (m, k)
        assert one["steps"].min() >= 1 and all(np.isfinite(one[k]) for k in KEYS)
    assert not np.array_equal(both[0]["action"], both[1]["action"]) or not _same(both[0]["value"], both[1]["value"])
