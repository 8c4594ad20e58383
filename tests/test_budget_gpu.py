"""A simulation budget per root on the GPU (mzh_search_multi_budget, Engine.search_multi(sims=...),
BatchedSelfPlay.play(sims=...), evaluate_networks(budgets="fused")).  The reference of every comparison is the
same engine's search_multi at one budget on the same rows and draws (itself checked against the C oracle in
test_multi_gpu.py); every comparison is bit for bit, floats compared as integers."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from muzero_hanoi_amd import rng as mrng

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 3
LO = 0  # the smallest n_sims mzh_search_multi accepts (search_args_check refuses n_sims < 0)
# (network, budget, roots) of the consecutive runs: runs of 1, 17 and 33 roots, budgets from {LO, 5, 25}; inside
# network 0 and network 1 the budgets are not monotone, and 25 (network 0), LO (network 1) come in two separate runs;
# network 3 of the set gets no root
RUNS = ((0, 5, 17), (0, 25, 1), (0, LO, 33), (0, 25, 17),
        (1, LO, 1), (1, 25, 33), (1, LO, 17), (1, 5, 1),
        (2, 25, 17), (2, 5, 33))
OUT_KEYS = ("visits", "root_q", "minmax", "extra_ties", "action", "pi", "latent_len", "sel_steps")


@pytest.fixture(scope="module")
def mzh():
    from muzero_hanoi_amd import _lib, engine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return engine


@pytest.fixture(scope="module")
def nets33():
    """the N = 3 checkpoint, two ablated copies of it, and a fourth network that gets no root"""
    from muzero_hanoi_amd.checkpoint import ablation_variants, load_model

    torch.manual_seed(3)
    v = ablation_variants(load_model(os.path.join(GOLDEN, "muzero_model_N3.pt")))
    return [v[i][1] for i in (0, 4, 3, 7)]  # as trained; policy head reset; value and reward heads reset; all three


@pytest.fixture(scope="module")
def flats(mzh, nets33):
    """support -> the four flat weight vectors"""
    f33 = [mzh.flat_weights(n.state_dict()) for n in nets33]
    z = np.load(os.path.join(GOLDEN, "weights_N3_s0_mc.npz"))
    w0 = {k: z[k].astype(np.float32) for k in z.files if k in mzh.WEIGHT_KEYS}
    assert w0["value_net.2.bias"].shape[0] == 1
    f1 = []
    for shift in range(4):  # the policy head's rows rolled: four networks that do not search alike
        w = {k: v.copy() for k, v in w0.items()}
        for k in ("policy_net.2.weight", "policy_net.2.bias"):
            w[k] = np.roll(w0[k], shift, axis=0)
        f1.append(mzh.flat_weights(w))
    return {33: f33, 1: f1}


def _inputs(B, seed):
    rs = np.random.RandomState(seed)
    st = rs.randint(0, 3, (B, N))
    obs = np.zeros((B, 3 * N), np.float32)
    obs[np.arange(B)[:, None], np.arange(N) * 3 + st] = 1
    noise, tie, u = mrng.synthetic_draws(B, deterministic=False, alpha=0.25, seed=seed)
    mm = np.stack([rs.uniform(-1.0, 0.5, B), rs.uniform(0.6, 3.0, B)], 1)  # minmax_in given
    mm[::3] = (-np.inf, np.inf)  # every third root fresh
    tt = lambda a: torch.tensor(np.asarray(a), device=DEV)
    return dict(obs=tt(obs), noise=tt(noise), tie_idx=tt(tie), action_u=tt(u), minmax_in=tt(mm))


def _bits(t):
    """a tensor as integers: floats by their bit pattern"""
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _layout():
    net = np.concatenate([np.full(c, m, np.int32) for m, _, c in RUNS])
    sims = np.concatenate([np.full(c, b, np.int32) for _, b, c in RUNS])
    edges = np.cumsum([0] + [c for _, _, c in RUNS])
    return net, sims, [slice(int(edges[i]), int(edges[i + 1])) for i in range(len(RUNS))]


@pytest.fixture(scope="module")
def engines(mzh, flats):
    """(support, max_sims) -> an engine with the four networks loaded, made once"""
    cache = {}

    def get(support, max_sims):
        if (support, max_sims) not in cache:
            eng = mzh.Engine(N, max_sims, 256, support)
            eng.load_weight_set(flats[support])
            cache[support, max_sims] = eng
        return cache[support, max_sims]

    return get


# 25 is the engine's max_sims in one case; in the other the launch's maximum (30) is above every budget
@pytest.mark.parametrize("max_sims,n_sims", [(25, 25), (64, 30)], ids=["cap25", "launch30"])
@pytest.mark.parametrize("support", [33, 1])
@pytest.mark.parametrize("tile", [16, 32])
def test_each_run_equals_search_multi_at_its_budget(engines, tile, support, max_sims, n_sims):
    eng = engines(support, max_sims)
    net, sims, runs = _layout()
    B = len(net)
    kw = _inputs(B, seed=41)
    tt = lambda a: torch.tensor(a, device=DEV)
    o = eng.search_multi(n_sims, net_index=tt(net), sims=tt(sims), max_runs=len(RUNS), tile=tile, **kw)
    assert o["_plan"]["kernel"].startswith(f"mzh_search_multi_kernel<{tile}, ")
    assert o["_plan"]["workgroups"] == -(-B // tile) + len(RUNS) - 1
    assert o["_status"].tolist() == [0, sum(-(-c // tile) for _, _, c in RUNS)]
    assert o["latent"].shape == (B, n_sims + 1)
    differ = 0
    for (m, b, c), sl in zip(RUNS, runs):
        ref = eng.search_multi(b, net_index=tt(net[sl]), tile=tile, **{k: v[sl] for k, v in kw.items()})
        assert ref["_status"].tolist()[0] == 0
        what = f"run of {c} roots, network {m}, budget {b}"
        for k in OUT_KEYS:
            assert torch.equal(_bits(o[k][sl]), _bits(ref[k])), f"{what}: {k}"
        assert int(o["visits"][sl].sum()) == b * c, what
        L = ref["latent_len"].cpu().numpy()
        got, want = o["latent"][sl].cpu().numpy(), ref["latent"].cpu().numpy()
        for j in range(c):
            assert np.array_equal(got[j, :L[j]], want[j, :L[j]]), f"{what}: latent of root {j}"
            if b > 0:
                assert (got[j, L[j]:] == -1).all(), f"{what}: latent row {j} past its path"
        if b == 25:  # precondition: the budgets matter (a kernel running n_sims for every root would not pass)
            other = eng.search_multi(5, net_index=tt(net[sl]), tile=tile, **{k: v[sl] for k, v in kw.items()})
            differ += int(not torch.equal(other["visits"], ref["visits"]))
    assert differ > 0
    # the default max_runs (here B, the most there can be) gives the same results on a larger grid
    o2 = eng.search_multi(n_sims, net_index=tt(net), sims=tt(sims), tile=tile, **kw)
    assert o2["_plan"]["workgroups"] == -(-B // tile) + B - 1 and o2["_status"].tolist() == o["_status"].tolist()
    for k in OUT_KEYS:
        assert torch.equal(_bits(o2[k]), _bits(o[k])), k


@pytest.mark.parametrize("tile", [16, 32])
def test_every_budget_at_n_sims_equals_search_multi(engines, tile):
    eng = engines(33, 25)
    net, _, _ = _layout()
    B, S = len(net), 25
    kw = _inputs(B, seed=42)
    tt = lambda a: torch.tensor(a, device=DEV)
    ref = eng.search_multi(S, net_index=tt(net), tile=tile, **kw)
    o = eng.search_multi(S, net_index=tt(net), sims=tt(np.full(B, S, np.int32)), max_runs=3, tile=tile, **kw)
    assert o["_status"].tolist() == ref["_status"].tolist() and ref["_status"].tolist()[0] == 0
    for k in OUT_KEYS + ("latent",):
        assert torch.equal(_bits(o[k]), _bits(ref[k])), k


# ------------------------------------------------------------------------------------------ device refusals
CANARY = -77


def test_device_refusals_write_nothing(mzh, engines):
    from muzero_hanoi_amd import _lib

    L = _lib.lib()
    eng = engines(33, 64)
    S = 25  # the launch's n_sims, below the engine's 64: a budget of 26 fits the engine and is still refused
    net, sims, _ = _layout()
    B = len(net)
    kw = _inputs(B, seed=43)
    tt = lambda a: torch.tensor(np.asarray(a, np.int32), device=DEV)

    def raw(net_index, n_sims, max_runs):
        """mzh_search_multi_budget called directly -> (status code, device verdict, outputs prefilled with the canary)"""
        out = eng.alloc_search_outputs(B, S, lockstep=True)
        for v in out.values():
            v.fill_(CANARY)
        a, out = eng._search_args(S, replay=None, temperature=1.0, deterministic=False, discount=0.8, eps=0.25,
                                  out=out, flags=0, **kw)
        ni, ns = tt(net_index), tt(n_sims)
        status = torch.full((2,), CANARY, dtype=torch.int32, device=DEV)
        m, b = _lib.MultiArgs(), _lib.BudgetArgs()
        m.n_networks, m.net_index, m.status = 4, _lib.ptr(ni), _lib.ptr(status)
        b.n_sims, b.max_runs = _lib.ptr(ns), max_runs
        st = L.mzh_search_multi_budget(eng._h, ctypes.byref(a), ctypes.byref(m), ctypes.byref(b), eng._stream())
        torch.cuda.synchronize()
        return st, status.tolist(), out

    untouched = lambda out: all(bool((v == CANARY).all()) for k, v in out.items() if not k.startswith("_"))

    def edited(arr, i, v):
        arr = arr.copy()
        arr[i] = v
        return arr

    R = len(RUNS)
    decreasing = net.copy()
    decreasing[-1] = 1  # a root of network 1 after network 2's
    cases = {"one budget below lo": (net, edited(sims, 40, LO - 1), B),
             "one budget above n_sims": (net, edited(sims, 40, S + 1), B),
             "the last root's budget above n_sims": (net, edited(sims, B - 1, 2 ** 30), B),
             "one run more than max_runs": (net, sims, R - 1),
             "a decreasing net_index": (decreasing, sims, B)}
    for what, (ni, ns, max_runs) in cases.items():
        st, verdict, out = raw(ni, ns, max_runs)
        assert st == _lib.MZH_OK, (what, _lib.last_error())
        assert verdict == [1, 0], what
        assert untouched(out), what
    # and with exactly as many runs as max_runs the batch is searched
    st, verdict, out = raw(net, sims, R)
    assert st == _lib.MZH_OK and verdict[0] == 0 and not untouched(out)
    # refused on the host: a NULL n_sims and max_runs < 1 (the engine at hand this time), n_sims beyond the engine
    m, b = _lib.MultiArgs(), _lib.BudgetArgs()
    a, _ = eng._search_args(S, replay=None, temperature=1.0, deterministic=False, discount=0.8, eps=0.25, out=None,
                            flags=0, **kw)
    ni = tt(net)
    m.n_networks, m.net_index = 4, _lib.ptr(ni)
    b.n_sims, b.max_runs = None, 3
    assert L.mzh_search_multi_budget(eng._h, ctypes.byref(a), ctypes.byref(m), ctypes.byref(b), None) == _lib.MZH_ERR_ARG
    b.n_sims, b.max_runs = _lib.ptr(ni), 0
    assert L.mzh_search_multi_budget(eng._h, ctypes.byref(a), ctypes.byref(m), ctypes.byref(b), None) == _lib.MZH_ERR_ARG
    a.n_sims = 65  # beyond the engine, as in mzh_search_multi
    b.max_runs = 3
    assert L.mzh_search_multi_budget(eng._h, ctypes.byref(a), ctypes.byref(m), ctypes.byref(b), None) == _lib.MZH_ERR_CAPACITY


def test_max_runs_beyond_the_tile_workspace_is_refused_on_the_host(mzh, flats):
    """an engine of 1,024 roots holds ceil(1024 / 16) + 255 = 319 tiles: 1,024 roots in up to 1,024 runs could make
    64 + 1,023; the default max_runs stays inside the workspace"""
    from muzero_hanoi_amd import _lib

    B, S = 1024, 5
    eng = mzh.Engine(N, S, B, 33)
    eng.load_weight_set(flats[33])
    kw = _inputs(B, seed=44)
    ni = torch.zeros(B, dtype=torch.int32, device=DEV)
    sims = torch.full((B,), S, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="tile workspace"):
        eng.search_multi(S, net_index=ni, sims=sims, max_runs=B, tile=16, **kw)
    assert _lib.last_error().startswith("max_runs=1024")
    o = eng.search_multi(S, net_index=ni, sims=sims, tile=16, **kw)  # default: 64 + 256 - 64 = 256 runs allowed
    assert o["_plan"]["workgroups"] == 64 + 256 - 1 and o["_status"].tolist() == [0, 64]
    ref = eng.search_multi(S, net_index=ni, tile=16, **kw)
    for k in OUT_KEYS + ("latent",):
        assert torch.equal(_bits(o[k]), _bits(ref[k])), k
    eng.close()


# ------------------------------------------------------------------------------------------ play
def test_play_budget_groups_equal_their_own_plays(nets33):
    """six envs, two budgets over two networks, draw_index = arange(6): each budget group replayed alone -- play on
    the same seed with draw_index at the group's positions and no sims -- gives its envs the same episodes (a move's
    synthetic draws for n rows are the first n rows of a larger draw)"""
    from muzero_hanoi_amd.networks import NetworkSet
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay

    nset = NetworkSet(nets33[:2])
    max_steps, seed = 12, 9
    starts = np.array([5, 0, 17, 25, 12, 5])
    net_index = np.array([0, 0, 0, 1, 1, 1])
    sims = np.array([12, 5, 12, 5, 5, 12])  # not monotone inside either network
    mm0 = np.stack([np.linspace(-2.0, 0.0, 6), np.linspace(0.5, 3.0, 6)], 1)
    mm0[::2] = (-np.inf, np.inf)
    kw = dict(temperature=1.0, deterministic=False, seed=seed)
    res = BatchedSelfPlay(nset, N, max_steps, 12).play(starts, net_index=net_index, sims=sims, minmax=mm0,
                                                       draw_index=np.arange(6), **kw)
    T = res["action"].shape[0]
    played = []
    for b in (5, 12):
        pos = np.nonzero(sims == b)[0]
        alone = BatchedSelfPlay(nset, N, max_steps, b).play(starts[pos], net_index=net_index[pos], minmax=mm0[pos],
                                                            draw_index=pos, **kw)
        Tg = alone["action"].shape[0]
        assert Tg <= T
        p = torch.as_tensor(pos, device=res["action"].device)
        for k in ("action", "pi", "root_q"):
            assert torch.equal(_bits(res[k][:Tg].index_select(1, p)), _bits(alone[k])), (b, k)
        assert bool((res["action"][Tg:].index_select(1, p) == -1).all()), b
        for k in ("steps", "minmax"):
            assert torch.equal(_bits(res[k].index_select(0, p)), _bits(alone[k])), (b, k)
        played.append(alone["action"].cpu().numpy())
    assert max(a.shape[0] for a in played) == T
    with pytest.raises(ValueError):
        BatchedSelfPlay(nset, N, max_steps, 12).play(starts, net_index=net_index, sims=sims + 1, **kw)


# ------------------------------------------------------------------------------------------ evaluate_networks
def _same_scores(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert set(ra) == set(rb)
        assert ra["data"] == rb["data"] and ra["minmax"] is None and rb["minmax"] is None
        assert np.array_equal(np.array(ra["illegal"]), np.array(rb["illegal"]), equal_nan=True)
        for k in ("errors", "steps", "illegal_rates"):
            assert len(ra[k]) == len(rb[k])
            for x, y in zip(ra[k], rb[k]):
                assert np.array_equal(x, y), k


def test_evaluate_networks_fused(nets33):
    from muzero_hanoi_amd.selfplay import evaluate_networks

    nets = nets33[:2]
    starts = np.array([5, 0, 17, 25, 12])
    kw = dict(start_idx=starts, max_steps=15, seed=3)
    # one budget: the fused batch is the per-budget batch, also where max_roots splits it
    for max_roots in (65536, 7):
        each = evaluate_networks(nets, N, [6], max_roots=max_roots, **kw)
        fused = evaluate_networks(nets, N, [6], budgets="fused", max_roots=max_roots, **kw)
        _same_scores(each, fused)
    # two budgets: the same structure under the same labels (the draws are the fused batch's own)
    each = evaluate_networks(nets, N, [4, 9], **kw)
    fused = evaluate_networks(nets, N, [4, 9], budgets="fused", **kw)
    assert len(fused) == len(each) == 2
    for rf, re_ in zip(fused, each):
        assert set(rf) == set(re_) and rf["minmax"] is None
        assert [d[0] for d in rf["data"]] == [d[0] for d in re_["data"]] == [4, 9]
        assert [d[0] for d in rf["illegal"]] == [4, 9]
        for k in ("errors", "steps", "illegal_rates"):
            assert [np.shape(x) for x in rf[k]] == [np.shape(x) for x in re_[k]] == [(5,), (5,)]
        assert all((s >= 1).all() and (s <= 15).all() for s in rf["steps"])
    # a fused plan-ahead sweep plays too (every budget >= 1)
    plans = evaluate_networks(nets, N, [4, 9], budgets="fused", max_plan_len=2, **kw)
    assert [d[0] for d in plans[0]["data"]] == [4, 9]
