"""Search over a set of networks on the GPU (mzh_load_weight_set / mzh_search_multi, Engine.search_multi,
BatchedSelfPlay with a NetworkSet, evaluate_networks).  Expected values come from the C oracle run per network
(oracle.search(..., flat=flat_m)), and a multi search is also compared with Engine.search on an engine that
holds only that root's network.  Every comparison is bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from muzero_hanoi_amd import rng as mrng

pytestmark = pytest.mark.gpu

DEV = "cuda"
# search result name -> oracle result name(s)
ORACLE_KEYS = (("visits", "visits"), ("root_q", "rootQ"), ("extra_ties", "extra_ties"), ("action", "action"),
               ("pi", "pi"), ("latent_len", "latent_len"), ("sel_steps", "sel_steps"))
MODES = [(1.0, False), (0.5, False), (1.0, True), (0.5, True)]  # (temperature, deterministic)


@pytest.fixture(scope="module")
def mzh():
    from muzero_hanoi_amd import _lib, engine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return engine


def _npz_weights(oracle, name):
    w, in_dim, sup = oracle.load_weights_npz(f"{GOLDEN}/{name}.npz")
    return {k: v.copy() for k, v in w.items()}, in_dim, sup


@pytest.fixture(scope="module")
def dicts_n3(oracle):
    """the three N = 3 networks as state-dict arrays: weights_N3_s0, the same with ablated_N3.npz's tensors
    substituted, and the reference-written checkpoint muzero_model_N3.pt"""
    w0, _, _ = _npz_weights(oracle, "weights_N3_s0")
    ab = np.load(os.path.join(GOLDEN, "ablated_N3.npz"))
    w1 = {k: (ab[k].copy() if k in ab.files else v.copy()) for k, v in w0.items()}
    assert any(not np.array_equal(w0[k], w1[k]) for k in w0)
    ck = torch.load(os.path.join(GOLDEN, "muzero_model_N3.pt"), map_location="cpu", weights_only=True)["Muzero_net"]
    w2 = {k: ck[k].numpy().astype(np.float32) for k in w0}
    return [w0, w1, w2]


def _inputs(B, n, seed):
    rs = np.random.RandomState(seed)
    st = rs.randint(0, 3, (B, n))
    obs = np.zeros((B, 3 * n), np.float32)
    obs[np.arange(B)[:, None], np.arange(n) * 3 + st] = 1
    noise, tie, u = mrng.synthetic_draws(B, deterministic=False, alpha=0.25, seed=seed)
    # MinMaxStats: every third root fresh, the others with bounds given by the caller
    mm = np.stack([rs.uniform(-1.0, 0.5, B), rs.uniform(0.6, 3.0, B)], 1)
    mm[::3] = (-np.inf, np.inf)
    return obs, noise, tie, u, mm


def _host(o):
    return {k: v.cpu().numpy() for k, v in o.items() if not k.startswith("_")}


def _assert_equals_oracle(got, ref, rows, what):
    """rows of a GPU search result == the oracle's result for those rows, every output"""
    for k, rk in ORACLE_KEYS:
        assert np.array_equal(got[k][rows], ref[rk]), f"{what}: {k}"
    assert np.array_equal(got["minmax"][rows], np.stack([ref["mm_max"], ref["mm_min"]], 1)), f"{what}: minmax"
    for j, b in enumerate(np.arange(len(got["visits"]))[rows]):
        L = ref["latent_len"][j]
        assert np.array_equal(got["latent"][b, :L], ref["latent"][j, :L]), f"{what}: latent of root {b}"


def _check_multi(mzh, oracle, n, S, sup, flats, counts, seed):
    """multi searches of sum(counts) roots, counts[m] of them under network m, at both tiles and in every mode
    == the oracle per network == Engine.search on a single-network engine of that network"""
    M, B = len(flats), int(sum(counts))
    net_index = np.repeat(np.arange(M), counts).astype(np.int32)
    seg = [slice(int(np.sum(counts[:m])), int(np.sum(counts[:m + 1]))) for m in range(M)]
    obs, noise, tie, u, mm = _inputs(B, n, seed)
    tt = lambda a: torch.tensor(np.asarray(a), device=DEV)
    eng = mzh.Engine(n, S, B, sup)
    eng.load_weight_set(flats)
    singles = []
    for f in flats:
        e1 = mzh.Engine(n, S, max(counts), sup)
        e1.load_weights(f)
        singles.append(e1)
    for T, det in MODES:
        kw = dict(noise=noise, tie_idx=tie, action_u=None if det else u, temperature=T, deterministic=det, minmax_in=mm)
        sub = lambda sl: {k: (v[sl] if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        refs = [oracle.search(n, S, obs[seg[m]], flat=flats[m], support=sup, **sub(seg[m])) if counts[m] else None
                for m in range(M)]
        # precondition: a kernel that ignored net_index (network 0 for every root) would not pass
        for m in range(1, M):
            if counts[m]:
                under0 = oracle.search(n, S, obs[seg[m]], flat=flats[0], support=sup, **sub(seg[m]))
                assert not np.array_equal(under0["visits"], refs[m]["visits"]), \
                    f"network {m}'s roots have network 0's visits: choose another seed"
        one = []
        for m in range(M):
            if not counts[m]:
                one.append(None)
                continue
            k1 = {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in sub(seg[m]).items()}
            one.append(_host(singles[m].search(S, obs=tt(obs[seg[m]]), **k1)))
        for tile in (16, 32):
            kg = {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
            o = eng.search_multi(S, net_index=tt(net_index), obs=tt(obs), tile=tile, **kg)
            assert o["_plan"]["kernel"].startswith(f"mzh_search_multi_kernel<{tile}, ")
            assert o["_plan"]["workgroups"] == -(-B // tile) + min(M, B) - 1
            tiles = sum(-(-c // tile) for c in counts)
            assert o["_status"].tolist() == [0, tiles]
            got = _host(o)
            for m in range(M):
                if not counts[m]:
                    continue
                what = f"counts {list(counts)} tile {tile} T {T} det {det} network {m}"
                _assert_equals_oracle(got, refs[m], seg[m], what)
                for k in one[m]:
                    if k == "latent":
                        for j in range(counts[m]):
                            L = one[m]["latent_len"][j]
                            assert np.array_equal(got[k][seg[m]][j, :L], one[m][k][j, :L]), f"{what}: single {k}"
                    else:
                        assert np.array_equal(got[k][seg[m]], one[m][k]), f"{what}: single-network engine {k}"


# a one-root network, a 16 + 1 split and an exact tile; 32 + 1 on the 32-root tile and an empty network
@pytest.mark.parametrize("counts", [(1, 17, 16), (33, 0, 31)], ids=lambda c: "-".join(map(str, c)))
def test_multi_search_n3_vs_oracle_and_single(mzh, oracle, dicts_n3, counts):
    flats = [oracle.flat_weights(w) for w in dicts_n3]
    _check_multi(mzh, oracle, 3, 8, 33, flats, np.array(counts), seed=21)


def test_multi_search_n4_s50(mzh, oracle):
    flats = [oracle.flat_weights(_npz_weights(oracle, f"weights_N4_s{s}")[0]) for s in (0, 1)]
    _check_multi(mzh, oracle, 4, 50, 33, flats, np.array([5, 40]), seed=22)


def test_multi_search_support_1(mzh, oracle):
    w0, in_dim, sup = _npz_weights(oracle, "weights_N3_s0_mc")
    assert (in_dim, sup) == (9, 1)
    w1 = {k: v.copy() for k, v in w0.items()}
    for k in ("policy_net.2.weight", "policy_net.2.bias"):  # the policy head's rows rolled by one action
        w1[k] = np.roll(w0[k], 1, axis=0)
    _check_multi(mzh, oracle, 3, 8, 1, [oracle.flat_weights(w0), oracle.flat_weights(w1)], np.array([3, 20]), seed=23)


# ------------------------------------------------------------------------------------------ refusals
SENTINEL = -77


def _sentinel_outputs(eng, B, S):
    out = eng.alloc_search_outputs(B, S, lockstep=True)
    for v in out.values():
        v.fill_(SENTINEL)
    return out


def _untouched(out):
    return all(bool((v == SENTINEL).all()) for k, v in out.items() if not k.startswith("_"))


def test_refusals(mzh, oracle, dicts_n3):
    from muzero_hanoi_amd import _lib

    L = _lib.lib()
    n, S, B, M = 3, 8, 40, 3
    flats = [oracle.flat_weights(w) for w in dicts_n3]
    obs, noise, tie, u, mm = _inputs(B, n, 31)
    tt = lambda a: torch.tensor(np.asarray(a), device=DEV)
    kw = dict(obs=tt(obs), noise=tt(noise), tie_idx=tt(tie), action_u=tt(u), minmax_in=tt(mm))
    eng = mzh.Engine(n, S, B, 33)
    eng.load_weights(flats[1])
    before = _host(eng.search(S, **kw))

    def raw(net_index, n_networks=M, status=None, edit=None, **over):
        """mzh_search_multi called directly: (status code, the outputs prefilled with the sentinel)"""
        k2 = dict(kw, **over)
        B2 = int(k2["tie_idx"].shape[0])
        out = _sentinel_outputs(eng, B2, S)
        a, out = eng._search_args(S, replay=None, temperature=1.0, deterministic=False, discount=0.8, eps=0.25,
                                  out=out, flags=0, **k2)
        m = _lib.MultiArgs()
        m.n_networks = n_networks
        m.net_index = _lib.ptr(net_index)
        m.status = _lib.ptr(status)
        if edit:
            edit(a)
        st = L.mzh_search_multi(eng._h, ctypes.byref(a), ctypes.byref(m), eng._stream())
        torch.cuda.synchronize()
        return st, out

    good = tt(np.repeat(np.arange(M), [10, 14, 16]).astype(np.int32))
    # no set loaded yet
    st, out = raw(good)
    assert st == _lib.MZH_ERR_STATE and _untouched(out)
    with pytest.raises(RuntimeError):
        eng.search_multi(S, net_index=good, **kw)
    for bad_m in (0, 257):
        with pytest.raises(ValueError):
            eng.load_weight_set(flats[:1] * bad_m)
    with pytest.raises(ValueError):
        eng.load_weight_set([flats[0][:-1]])
    eng.load_weight_set(flats)

    # refused on the host, before anything is launched
    def flag(f):
        def edit(a):
            a.flags = f
        return edit

    def replay_in(a):
        a.rp_sim = 0x1000

    def root_pi_in(a):
        a.rp_root_pi = 0x1000

    def hot(a):
        a.temperature = 1.5

    big = _inputs(B + 1, n, 32)
    kbig = dict(obs=tt(big[0]), noise=tt(big[1]), tie_idx=tt(big[2]), action_u=tt(big[3]), minmax_in=tt(big[4]))

    def more_sims(a):
        a.n_sims = S + 1

    for code, args in ((_lib.MZH_ERR_ARG, dict(n_networks=M + 1)), (_lib.MZH_ERR_ARG, dict(n_networks=0)),
                       (_lib.MZH_ERR_ARG, dict(net_index=None)),
                       (_lib.MZH_ERR_ARG, dict(edit=replay_in)), (_lib.MZH_ERR_ARG, dict(edit=root_pi_in)),
                       (_lib.MZH_ERR_ARG, dict(edit=flag(_lib.MZH_FLAG_KERNEL_WAVE))),
                       (_lib.MZH_ERR_ARG, dict(edit=flag(_lib.MZH_FLAG_KERNEL_WAVE16))),
                       (_lib.MZH_ERR_ARG, dict(edit=flag(_lib.MZH_FLAG_KERNEL_ONE))),
                       (_lib.MZH_ERR_ARG, dict(edit=flag(_lib.MZH_FLAG_KERNEL_COOP | _lib.MZH_FLAG_COOP_OCC2))),
                       (_lib.MZH_ERR_CAPACITY, dict(**kbig)), (_lib.MZH_ERR_CAPACITY, dict(edit=more_sims)),
                       (_lib.MZH_ERR_TEMPERATURE, dict(edit=hot))):
        args = dict(args)
        ni = args.pop("net_index", good)
        if "tie_idx" in args:
            ni = tt(np.zeros(B + 1, np.int32))
        status = torch.full((2,), SENTINEL, dtype=torch.int32, device=DEV)
        st, out = raw(ni, status=status, **args)
        assert st == code, (st, code, _lib.last_error())
        assert _untouched(out) and status.tolist() == [SENTINEL, SENTINEL]

    # refused on the device: a decreasing net_index, an index equal to M, a negative one
    for bad in (np.repeat([0, 2, 1], [10, 14, 16]), np.repeat([0, 1, 3], [10, 14, 16]), np.repeat([-1, 1, 2], [10, 14, 16]),
                np.r_[np.zeros(B - 1), 2 ** 30]):
        status = torch.full((2,), SENTINEL, dtype=torch.int32, device=DEV)
        st, out = raw(tt(bad.astype(np.int32)), status=status)
        assert st == _lib.MZH_OK and status.tolist() == [1, 0], bad
        assert _untouched(out), bad
    # n_networks below the set's M narrows the accepted range
    status = torch.full((2,), SENTINEL, dtype=torch.int32, device=DEV)
    st, out = raw(good, n_networks=2, status=status)
    assert st == _lib.MZH_OK and status.tolist() == [1, 0] and _untouched(out)
    # and a good one is searched (status nullable)
    st, out = raw(good)
    assert st == _lib.MZH_OK and not _untouched(out)

    # the engine's own network is untouched by the set
    after = _host(eng.search(S, **kw))
    for k in before:
        if k != "latent":
            assert np.array_equal(before[k], after[k]), k
    ref = oracle.search(n, S, obs, flat=flats[1], support=33, noise=noise, tie_idx=tie, action_u=u, minmax_in=mm)
    _assert_equals_oracle(after, ref, slice(0, B), "single-network search after a set was loaded")


# ------------------------------------------------------------------------------------------ self-play
def _module(w):
    from muzero_hanoi_amd.networks import MuZeroNet

    in_dim, sup = w["representation_net.0.weight"].shape[1], w["value_net.2.bias"].shape[0]
    net = MuZeroNet(in_dim, 6, 0.002, "cpu", TD_return=sup == 33)
    net.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    return net


def _oracle_play(oracle, flats, net_index, starts, n, S, max_steps, seed, T=1.0, det=False, alpha=0.25, minmax=None):
    """BatchedSelfPlay.play simulated move by move with the oracle: the same synthetic draws (one seed per move
    from default_rng(seed), rows = the active envs in env order), the oracle search called per network segment
    of the active envs.  -> actions [T][B] (-1: not playing), steps, illegal counts, final MinMaxStats"""
    B = len(starts)
    gen = np.random.default_rng(seed)
    st = np.stack([(starts // 3 ** (n - 1 - d)) % 3 for d in range(n)], 1).astype(np.uint8)
    ctr, alive = np.zeros(B, int), np.ones(B, bool)
    steps, illegal = np.zeros(B, int), np.zeros(B, int)
    mm = np.tile([-np.inf, np.inf], (B, 1)) if minmax is None else np.array(minmax, np.float64)
    obs = np.zeros((B, 3 * n), np.float32)
    obs[np.arange(B)[:, None], np.arange(n) * 3 + st] = 1
    acts = []
    while alive.any():
        idx = np.nonzero(alive)[0]
        noise, tie, u = mrng.synthetic_draws(len(idx), deterministic=det, alpha=alpha, seed=int(gen.integers(2**31)))
        row = np.full(B, -1, np.int64)
        for m in np.unique(net_index[idx]):
            sel = np.nonzero(net_index[idx] == m)[0]
            o = oracle.search(n, S, obs[idx[sel]], flat=flats[m], support=33, noise=None if noise is None else noise[sel],
                              tie_idx=tie[sel], action_u=None if u is None else u[sel], temperature=T,
                              deterministic=det, minmax_in=mm[idx[sel]])
            row[idx[sel]] = o["action"]
            mm[idx[sel]] = np.stack([o["mm_max"], o["mm_min"]], 1)
        for b in idx:
            code, s2, moved, c2, a2, d, ill = oracle.env_step(st[b], int(row[b]), int(ctr[b]), 1, max_steps)
            st[b], ctr[b] = s2, c2
            steps[b] += 1
            illegal[b] += ill
            obs[b] = 0
            obs[b, np.arange(n) * 3 + moved] = 1
            if d:
                alive[b] = False
        acts.append(row)
    return np.stack(acts), steps, illegal, mm


def test_selfplay_network_set_vs_oracle(oracle, dicts_n3):
    from muzero_hanoi_amd.networks import NetworkSet
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay

    n, S, per, max_steps, seed = 3, 12, 11, 15, 5
    flats = [oracle.flat_weights(w) for w in dicts_n3]
    nets = [_module(w) for w in dicts_n3]
    B = 3 * per
    net_index = np.repeat(np.arange(3), per)
    starts = np.random.RandomState(1).randint(0, 3 ** n - 1, B)
    mm0 = np.stack([np.linspace(-2.0, 0.0, B), np.linspace(0.5, 3.0, B)], 1)  # agents with history
    mm0[::3] = (-np.inf, np.inf)  # and fresh ones
    sp = BatchedSelfPlay(NetworkSet(nets), n, max_steps, S)
    res = sp.play(starts, temperature=1.0, deterministic=False, seed=seed, minmax=mm0, net_index=net_index)
    acts, steps, illegal, mm = _oracle_play(oracle, flats, net_index, starts, n, S, max_steps, seed, minmax=mm0)
    got = res["action"].cpu().numpy()
    assert got.shape == acts.shape
    for t in range(len(acts)):
        assert np.array_equal(got[t], acts[t]), f"step {t}"
    assert np.array_equal(res["steps"].cpu().numpy(), steps)
    assert np.array_equal(res["illegal"].cpu().numpy(), illegal)
    assert np.array_equal(res["minmax"].cpu().numpy(), mm)
    # the three networks do not play alike (else the segments would prove nothing)
    assert len({_oracle_play(oracle, [f] * 3, net_index, starts, n, S, max_steps, seed, minmax=mm0)[0].tobytes()
                for f in flats}) == 3

    with pytest.raises(ValueError):
        sp.play(starts, seed=seed)  # a set needs net_index
    with pytest.raises(ValueError):
        sp.play(starts, seed=seed, net_index=net_index[::-1].copy())
    with pytest.raises(ValueError):
        BatchedSelfPlay(nets[0], n, max_steps, S).play(starts, seed=seed, net_index=net_index)

    # one network three times == single-network play of the same batch
    same = BatchedSelfPlay(NetworkSet([nets[2]] * 3), n, max_steps, S).play(
        starts, temperature=1.0, deterministic=False, seed=seed, minmax=mm0, net_index=net_index, record_obs=True)
    single = BatchedSelfPlay(nets[2], n, max_steps, S).play(starts, temperature=1.0, deterministic=False, seed=seed,
                                                            minmax=mm0, record_obs=True)
    assert set(same) == set(single)
    for k in single:
        assert torch.equal(same[k], single[k]), k


def test_evaluate_networks_vs_oracle(oracle, dicts_n3):
    """evaluate_networks == evaluate's scores of the oracle's episodes (the draws of a batch of len(networks) x
    episodes envs are not those of evaluate's per-network batches, so the episodes are reconstructed with the
    oracle as in the self-play test), also where max_roots splits a budget into several launches"""
    from muzero_hanoi_amd.selfplay import evaluate_networks

    n, max_steps, seed, budgets = 3, 25, 3, [5, 10]
    ws = [dicts_n3[2], dicts_n3[0]]
    flats = [oracle.flat_weights(w) for w in ws]
    nets = [_module(w) for w in ws]
    starts = np.array([5, 0, 17, 25, 12, 5])
    E, M = len(starts), 2
    net_index, all_starts = np.repeat(np.arange(M), E), np.tile(starts, M)
    opt = np.array([oracle.hanoi_solver([(s // 3 ** (n - 1 - d)) % 3 for d in range(n)]) for s in starts])
    for max_roots in (65536, 7):
        res = evaluate_networks(nets, n, budgets, start_idx=starts, max_steps=max_steps, seed=seed, max_roots=max_roots)
        assert len(res) == M and all(r["minmax"] is None for r in res)
        for i, S in enumerate(budgets):
            steps, ill = [], []
            for k, lo in enumerate(range(0, M * E, max_roots)):
                sl = slice(lo, min(M * E, lo + max_roots))
                _, s, il, _ = _oracle_play(oracle, flats, net_index[sl], all_starts[sl], n, S, max_steps, seed + k)
                steps.append(s)
                ill.append(il)
            steps, ill = np.concatenate(steps), np.concatenate(ill)
            for m in range(M):
                s, il = steps[m * E:(m + 1) * E], ill[m * E:(m + 1) * E]
                r = res[m]
                assert np.array_equal(r["steps"][i], s) and np.array_equal(r["errors"][i], s - opt)
                rates = il / np.maximum(s, 1)
                assert np.array_equal(r["illegal_rates"][i], rates)
                assert r["data"][i] == [S, float(sum(int(e) for e in s - opt) / E)]
                assert r["illegal"][i] == [S, float(np.mean(rates)), float(np.std(rates, ddof=1) / np.sqrt(E))]
