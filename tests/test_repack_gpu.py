"""The device repack on the GPU (mzh_load_weights_device / mzh_load_weight_set_device, Engine.load_weights_from /
load_weight_set_from, engine_for(weights=...)): an engine refreshed from the live parameter tensors must be the
engine the host path (flat_weights + load_weights) makes for the same values -- the same blob bytes, and the same
bits out of every kernel afterwards.  Every comparison is bit equality on an int32 view; no tolerance is involved."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (golden weights, n_disks, support): a 33-bin head, a 1-bin head (no by-value scalars), the ragged in_dim of 21
WEIGHTS = [("weights_N3_s0", 3, 33), ("weights_N3_s0_mc", 3, 1), ("weights_N7_s0", 7, 33)]
IDS = [w[0] for w in WEIGHTS]


@pytest.fixture(scope="module")
def mzh():
    from muzero_hanoi_amd import _lib, engine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return engine


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _npz(oracle, name):
    w, in_dim, sup = oracle.load_weights_npz(f"{GOLDEN}/{name}.npz")
    return {k: np.ascontiguousarray(v, np.float32).copy() for k, v in w.items()}


def _variant(w, seed, support):
    """other values for every tensor; with a 33-bin head both bin-32 biases at +5, so that the two scalars the
    kernels take by value decide the reward and the value"""
    rs = np.random.RandomState(seed)
    out = {k: (v * np.float32(1.0 + 0.05 * rs.standard_normal()) + (0.02 * rs.standard_normal(v.shape)).astype(np.float32))
           for k, v in w.items()}
    if support == 33:
        out["rwd_net.2.bias"][32] = np.float32(5.0)
        out["value_net.2.bias"][32] = np.float32(5.0)
    return {k: np.ascontiguousarray(v, np.float32) for k, v in out.items()}


def _cuda_params(mzh, w):
    return [torch.tensor(w[k], device=DEV) for k in mzh.WEIGHT_KEYS]


def _write(params, mzh, w):
    """the new values into the live tensors, in place"""
    with torch.no_grad():
        for t, k in zip(params, mzh.WEIGHT_KEYS):
            t.copy_(torch.tensor(w[k], device=DEV))


def _host_engine(mzh, oracle, w, n, sup, max_sims=0, max_roots=64):
    eng = mzh.Engine(n, max_sims, max_roots, sup)
    eng.load_weights(oracle.flat_weights(w))
    return eng


def _all_states(n):
    st = np.array(np.unravel_index(np.arange(3 ** n), (3,) * n)).T
    obs = np.zeros((3 ** n, 3 * n), np.float32)
    obs[np.arange(3 ** n)[:, None], np.arange(n) * 3 + st] = 1
    return torch.tensor(obs, device=DEV)


def _infer(eng, obs):
    """initial inference of every row and a recurrent step of each (move = row % 6): every output tensor"""
    a = eng.initial_inference(obs)
    b = eng.recurrent_inference(a["h"], torch.arange(obs.shape[0], device=DEV, dtype=torch.int32) % 6)
    return {**{f"i_{k}": v for k, v in a.items()}, **{f"r_{k}": v for k, v in b.items()}}


def _assert_same_outputs(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert _same(got[k], want[k]), f"{what}: {k}"


# ------------------------------------------------------------------------------------------ 1. blob identity
@pytest.mark.parametrize("name,n,sup", WEIGHTS, ids=IDS)
def test_blob_identity_single_network(mzh, oracle, name, n, sup):
    w = _npz(oracle, name)
    A = _host_engine(mzh, oracle, w, n, sup)
    B = mzh.Engine(n, 0, 64, sup)
    with pytest.raises(RuntimeError, match="not loaded"):
        B.debug_blob(0)
    B.load_weights_from(_cuda_params(mzh, w))
    for which in (0, 1):
        a, b = A.debug_blob(which), B.debug_blob(which)
        assert a.numel() > 0 and _same(a, b), f"blob {which} of a device load differs from the host load's"
    # either kind of load may follow the other, on the same engine
    w2 = _variant(w, 5, sup)
    B.load_weights(oracle.flat_weights(w2))
    assert not _same(A.debug_blob(0), B.debug_blob(0))
    B.load_weights_from(_cuda_params(mzh, w))
    A2 = _host_engine(mzh, oracle, w2, n, sup)
    A2.load_weights_from(dict(zip(mzh.WEIGHT_KEYS, _cuda_params(mzh, w))))  # a state_dict is accepted
    for which in (0, 1):
        assert _same(A.debug_blob(which), B.debug_blob(which)) and _same(A.debug_blob(which), A2.debug_blob(which))
    obs = _all_states(n)[:64]
    _assert_same_outputs(_infer(B, obs), _infer(A, obs), name)
    _assert_same_outputs(_infer(A2, obs), _infer(A, obs), name)


@pytest.mark.parametrize("name,n,sup", WEIGHTS, ids=IDS)
def test_blob_identity_set_of_three(mzh, oracle, name, n, sup):
    w0 = _npz(oracle, name)
    ws = [w0, _variant(w0, 1, sup), _variant(w0, 2, 1)]  # the third keeps its own bin-32 biases
    A = mzh.Engine(n, 0, 64, sup)
    A.load_weight_set([oracle.flat_weights(w) for w in ws])
    B = mzh.Engine(n, 0, 64, sup)
    with pytest.raises(RuntimeError, match="no weight set"):
        B.debug_blob(2)
    B.load_weight_set_from([_cuda_params(mzh, w) for w in ws])
    assert B.set_size == 3
    for which in (2, 3):
        a, b = A.debug_blob(which), B.debug_blob(which)
        assert a.numel() > 0 and _same(a, b), f"set blob {which} of a device load differs from the host load's"
    tail = B.debug_blob(2)[-6:].cpu().numpy()
    want = [w[k][32] if sup == 33 else 0.0 for w in ws for k in ("rwd_net.2.bias", "value_net.2.bias")]
    assert np.array_equal(tail.view(np.int32), np.array(want, np.float32).view(np.int32))
    # a refresh of the same M reuses the buffers; another M reallocates them; a host load may follow
    c0 = B.debug_counters()
    B.load_weight_set_from([_cuda_params(mzh, w) for w in ws[::-1]])
    assert B.debug_counters() == c0
    A.load_weight_set([oracle.flat_weights(w) for w in ws[::-1]])
    assert _same(A.debug_blob(2), B.debug_blob(2)) and _same(A.debug_blob(3), B.debug_blob(3))
    B.load_weight_set_from([_cuda_params(mzh, w) for w in ws[:2]])
    A.load_weight_set([oracle.flat_weights(w) for w in ws[:2]])
    assert B.debug_counters()["allocs"] == c0["allocs"] + 2 and B.debug_counters()["frees"] == c0["frees"] + 2
    assert _same(A.debug_blob(2), B.debug_blob(2)) and _same(A.debug_blob(3), B.debug_blob(3))
    B.load_weight_set([oracle.flat_weights(w) for w in ws])
    A.load_weight_set_from([_cuda_params(mzh, w) for w in ws])
    assert _same(A.debug_blob(2), B.debug_blob(2)) and _same(A.debug_blob(3), B.debug_blob(3))


# ------------------------------------------------------------------------------------------ 2. refresh in place
@pytest.mark.parametrize("name,n,sup", WEIGHTS[:2], ids=IDS[:2])
def test_refresh_follows_in_place_changes(mzh, oracle, name, n, sup):
    w = _npz(oracle, name)
    obs = _all_states(n)
    params = _cuda_params(mzh, w)
    eng = mzh.Engine(n, 0, 64, sup)
    eng.load_weights_from(params)
    before = _infer(eng, obs)
    _assert_same_outputs(before, _infer(_host_engine(mzh, oracle, w, n, sup), obs), "first device load")
    counters = eng.debug_counters()
    # every parameter changes in place; both bin-32 biases to +5
    with torch.no_grad():
        for i, t in enumerate(params):
            t.mul_(1.0 + 0.01 * (i + 1)).add_(0.003 * (i % 3 - 1))
        if sup == 33:
            params[mzh.WEIGHT_KEYS.index("rwd_net.2.bias")][32] = 5.0
            params[mzh.WEIGHT_KEYS.index("value_net.2.bias")][32] = 5.0
    w_new = {k: t.cpu().numpy() for k, t in zip(mzh.WEIGHT_KEYS, params)}
    eng.load_weights_from(params)
    after = _infer(eng, obs)
    _assert_same_outputs(after, _infer(_host_engine(mzh, oracle, w_new, n, sup), obs), "refresh")
    for k in ("i_h", "i_pi", "i_value", "r_h", "r_reward", "r_value"):
        assert not _same(after[k], before[k]), f"{k} did not change with the weights"
    assert eng.debug_counters() == counters, "a refresh allocated, freed or waited for the device"


# ------------------------------------------------------------------------------------------ 3. every search kernel
def _search_inputs(B, n, seed):
    from muzero_hanoi_amd import rng

    st = np.random.RandomState(seed).randint(0, 3, (B, n))
    obs = np.zeros((B, 3 * n), np.float32)
    obs[np.arange(B)[:, None], np.arange(n) * 3 + st] = 1
    noise, tie, u = rng.synthetic_draws(B, deterministic=False, alpha=0.25, seed=300 + seed)
    tt = lambda a: torch.tensor(np.asarray(a), device=DEV)
    return dict(obs=tt(obs), noise=tt(noise), tie_idx=tt(tie), action_u=tt(u), temperature=1.0)


@pytest.mark.parametrize("kernel,B,prefix", [("one", 3, "mzh_search_one_kernel"), ("coop", 40, "mzh_search_kernel"),
                                             ("wave16", 64, "mzh_wave_kernel<1")], ids=["latency", "coop", "wave16"])
def test_every_search_kernel_after_a_refresh(mzh, oracle, kernel, B, prefix):
    n, sup, S, D = 3, 33, 10, 3
    w1 = _npz(oracle, "weights_N3_s0")
    w2 = _variant(w1, 7, sup)
    inp = _search_inputs(B, n, 11)
    keys = ("visits", "root_q", "action", "minmax")

    def search(e):
        o = e.search(S, kernel=kernel, **inp)
        assert o["_plan"]["kernel"].startswith(prefix), o["_plan"]
        return {k: o[k] for k in keys}

    params = _cuda_params(mzh, w1)
    eng = mzh.Engine(n, S, B, sup)
    eng.set_memo_depth(D)  # the wave kernel's expansion memo (the other kernels have none)
    eng.load_weights_from(params)
    first = search(eng)
    if kernel == "wave16":
        assert eng.memo_stats()["built"] == 1
    _write(params, mzh, w2)
    eng.load_weights_from(params)
    if kernel == "wave16":
        assert eng.memo_stats()["built"] == 0, "the refresh kept a table built from the old weights"
    second = search(eng)
    fresh1, fresh2 = (_host_engine(mzh, oracle, w, n, sup, S, B) for w in (w1, w2))
    for e in (fresh1, fresh2):
        e.set_memo_depth(D)
    want1, want2 = search(fresh1), search(fresh2)
    for k in keys:
        assert _same(first[k], want1[k]), f"{kernel}: {k} after the first device load"
        assert _same(second[k], want2[k]), f"{kernel}: {k} after the refresh"
    assert not _same(want1["visits"], want2["visits"]), "the two weight sets search alike: choose another variant"
    if kernel == "wave16":
        st = eng.memo_stats()
        assert st["built"] == 1 and st["depth"] == D, st
        (h, rec, d), (hw, recw, dw) = eng.memo_table(), fresh2.memo_table()
        assert d == dw == D and _same(h, hw) and _same(rec, recw), "the table was not rebuilt from the new weights"


# ------------------------------------------------------------------------------------------ 4. stream order
@pytest.mark.parametrize("name,n,sup", WEIGHTS[:2], ids=IDS[:2])
def test_refresh_is_stream_ordered(mzh, oracle, name, n, sup):
    w1 = _npz(oracle, name)
    w2 = _variant(w1, 9, sup)
    obs = _all_states(n)
    params = _cuda_params(mzh, w1)
    new = _cuda_params(mzh, w2)
    eng = mzh.Engine(n, 0, 64, sup)
    eng.load_weights_from(params)
    old = eng.initial_inference(obs)
    big = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(8):  # work ahead of the writes: a refresh on another stream would read the old values
            big = big @ big * 1e-3
        for t, v in zip(params, new):
            t.copy_(v)
        eng.load_weights_from(params)
        out = eng.initial_inference(obs)
    side.synchronize()
    want = _host_engine(mzh, oracle, w2, n, sup).initial_inference(obs)
    for k in want:
        assert _same(out[k], want[k]), f"{k} is not the final parameters' result"
    assert not _same(out["h"], old["h"])


# ------------------------------------------------------------------------------------------ 5. engine_for
def _fused_agent():
    from muzero_hanoi_amd.muzero import Muzero

    torch.manual_seed(4)
    return Muzero(env=None, s_space_size=9, n_action=6, discount=0.8, dirichlet_alpha=0.25, n_mcts_simulations=10,
                  unroll_n_steps=5, batch_s=8, TD_return=True, n_TD_step=10, lr=0.002, buffer_size=100,
                  priority_replay=True, device=DEV, update_impl="fused")


def _fused_step(mz, seed):
    g = np.random.default_rng(seed)
    B, U = 8, 5
    states = np.zeros((B, 9), np.float32)
    states[np.arange(B)[:, None], np.arange(3) * 3 + g.integers(0, 3, (B, 3))] = 1
    tt = lambda a, dt: torch.tensor(a, dtype=dt, device=DEV)
    mz._update(tt(states, torch.float32), tt(g.normal(0, 1, (B, U)), torch.float32), tt(g.integers(0, 6, (B, U)), torch.long),
               tt(g.dirichlet(np.ones(6), size=(B, U)), torch.float32), tt(g.normal(0, 5, (B, U)), torch.float32),
               tt(g.random(B) + 0.1, torch.float32))


def test_engine_for_weights_modes(mzh, oracle):
    from muzero_hanoi_amd import networks

    mz = _fused_agent()
    net = mz.networks
    obs = _all_states(3)

    def fresh():
        e = mzh.Engine(3, 10, 27, 33)
        e.load_weights(mzh.flat_weights(net.state_dict()))
        return e.initial_inference(obs)

    def cached_how():
        return networks._CACHE[net]["how"]

    start = fresh()
    _fused_step(mz, 0)  # writes the 20 parameters in place and bumps their versions
    eng = networks.engine_for(net, 10, 27, weights="device")
    assert cached_how() == "device"
    got, want = eng.initial_inference(obs), fresh()
    for k in want:
        assert _same(got[k], want[k]), f"weights='device': {k}"
    assert not _same(want["h"], start["h"]), "the update changed nothing"
    counters = eng.debug_counters()
    _fused_step(mz, 1)
    assert networks.engine_for(net, 10, 27, weights="device") is eng and eng.debug_counters() == counters
    got, want = eng.initial_inference(obs), fresh()
    for k in want:
        assert _same(got[k], want[k]), f"second refresh: {k}"
    _fused_step(mz, 2)
    assert networks.engine_for(net, 10, 27, weights="host") is eng and cached_how() == "host"
    got, want = eng.initial_inference(obs), fresh()
    for k in want:
        assert _same(got[k], want[k]), f"weights='host': {k}"
    _fused_step(mz, 3)
    assert networks.engine_for(net, 10, 27) is eng  # "auto": eligible parameters take the path the benchmark chose
    assert cached_how() == ("device" if networks.AUTO_DEVICE_RELOAD else "host")
    got, want = eng.initial_inference(obs), fresh()
    for k in want:
        assert _same(got[k], want[k]), f"weights='auto': {k}"
    with pytest.raises(ValueError, match="weights must be"):
        networks.engine_for(net, 10, 27, weights="gpu")
    # a CPU-resident parameter: "device" refuses, "auto" falls back to the host path
    with torch.no_grad():
        net.policy_net[2].bias.data = (net.policy_net[2].bias.data + 0.25).cpu()
    with pytest.raises(ValueError, match="policy_net.2.bias"):
        networks.engine_for(net, 10, 27, weights="device")
    assert networks.engine_for(net, 10, 27, weights="auto") is eng and cached_how() == "host"
    got, want = eng.initial_inference(obs), fresh()
    for k in want:
        assert _same(got[k], want[k]), f"host fallback: {k}"
    with pytest.raises(ValueError, match="policy_net.2.bias"):  # the cached host load does not serve a "device" request
        networks.engine_for(net, 10, 27, weights="device")


def test_engine_for_set_weights_modes(mzh, oracle):
    from muzero_hanoi_amd import networks
    from muzero_hanoi_amd.networks import MuZeroNet, NetworkSet

    nets = []
    for seed in (1, 2, 3):
        torch.manual_seed(seed)
        nets.append(MuZeroNet(rpr_input_s=9, action_s=6, lr=0.002, device=DEV, TD_return=True).to(DEV))
    nset = NetworkSet(nets)
    want = mzh.Engine(3, 0, 8, 33)
    want.load_weight_set([mzh.flat_weights(n.state_dict()) for n in nets])
    eng = networks.engine_for_set(nset, 0, 8, weights="device")
    assert nset._cache["how"] == "device"
    assert _same(eng.debug_blob(2), want.debug_blob(2)) and _same(eng.debug_blob(3), want.debug_blob(3))
    with torch.no_grad():
        nets[1].value_net[2].bias.add_(1.0)
    assert networks.engine_for_set(nset, 0, 8, weights="host") is eng and nset._cache["how"] == "host"
    want.load_weight_set([mzh.flat_weights(n.state_dict()) for n in nets])
    assert _same(eng.debug_blob(2), want.debug_blob(2)) and _same(eng.debug_blob(3), want.debug_blob(3))
    nets[2].cpu()
    with pytest.raises(ValueError, match="weights='device'"):
        networks.engine_for_set(nset, 0, 8, weights="device")
    assert networks.engine_for_set(nset, 0, 8, weights="auto") is eng and nset._cache["how"] == "host"


# ------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_launch_nothing(mzh, oracle):
    w = _npz(oracle, "weights_N3_s0")
    eng = mzh.Engine(3, 0, 8, 33)
    good = _cuda_params(mzh, w)
    i = mzh.WEIGHT_KEYS.index("dynamic_net.0.weight")

    def swapped(t):
        return good[:i] + [t] + good[i + 1:]

    cases = {
        "19 tensors": good[:19],
        "a wrong shape": swapped(good[i][:, :64].contiguous()),
        "fp64": swapped(good[i].double()),
        "a non-contiguous view": swapped(torch.empty(70, 256, device=DEV).t()),
        "a CPU tensor": swapped(good[i].cpu()),
        "a wrong network": _cuda_params(mzh, _npz(oracle, "weights_N3_s0_mc")),
    }
    assert cases["a non-contiguous view"][i].shape == good[i].shape and not cases["a non-contiguous view"][i].is_contiguous()
    for what, params in cases.items():
        with pytest.raises(ValueError, match="load_weights_from"):
            eng.load_weights_from(params)
        with pytest.raises(ValueError, match="load_weight_set_from: network 1"):
            eng.load_weight_set_from([good, params])
    with pytest.raises(ValueError, match="1 to 256 networks, got 257"):
        eng.load_weight_set_from([good] * 257)
    with pytest.raises(ValueError, match="1 to 256 networks, got 0"):
        eng.load_weight_set_from([])
    # nothing was launched, allocated or loaded
    assert eng.debug_counters() == {"allocs": 0, "frees": 0, "device_waits": 0}
    assert not eng.weights_loaded and getattr(eng, "set_size", 0) == 0
    with pytest.raises(RuntimeError, match="not loaded"):
        eng.initial_inference(_all_states(3)[:8])
    eng.load_weight_set_from([good] * 256)  # the largest set is accepted
    assert eng.set_size == 256 and eng.debug_counters() == {"allocs": 2, "frees": 0, "device_waits": 0}
