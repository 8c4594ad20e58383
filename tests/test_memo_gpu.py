"""The wave kernel's expansion memo (include/mzh.h) on the GPU.

The table's rows equal the inference kernels chained along the row's action path; a search with the memo equals
the search without it and the oracle bit for bit, whichever of the three M-phase forms (no chain, the packed
16-column tile, the wave's own tiles) a simulation takes; and how often each form runs is exactly what the
oracle's selection depths predict (tests/test_memo_cpu.py holds that prediction and checks, without a GPU,
that the inputs used here reach all three).
"""
import numpy as np
import pytest
import torch

from test_memo_cpu import (CASE_MODES, MIXED, N, S, case_inputs, invalidation_weights, mixed_inputs, onehot_rows,
                           predict_paths, scramble_inputs, weights)

DEV = "cuda"
OUTPUTS = (("visits", "visits"), ("root_q", "rootQ"), ("action", "action"), ("pi", "pi"), ("sel_steps", "sel_steps"),
           ("extra_ties", "extra_ties"), ("latent", "latent"), ("latent_len", "latent_len"))
RPW = {"wave": 32, "wave16": 16}


def _tt(a):
    return None if a is None else torch.tensor(np.asarray(a), device=DEV)


@pytest.fixture(scope="module")
def eng64(oracle):
    """one engine for every search case of this file (64 roots, S simulations, the golden N = 4 weights)"""
    from muzero_hanoi_amd import engine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    flat, sup = weights(oracle)
    eng = engine.Engine(N, S, 64, sup)
    eng.load_weights(flat)
    yield eng
    eng.close()


def _search(eng, kernel, inp, deterministic):
    obs, noise, tie, u, mm = inp
    o = eng.search(S, obs=_tt(obs), tie_idx=_tt(tie), noise=_tt(noise), action_u=_tt(u), minmax_in=_tt(mm),
                   temperature=1.0, deterministic=deterministic, kernel=kernel)
    want_nt = 2 if kernel == "wave" else 1
    assert o["_plan"]["kernel"] == f"mzh_wave_kernel<{want_nt}, false, true>", o["_plan"]
    return {k: v.cpu().numpy() for k, v in o.items() if not k.startswith("_")}


def _paths(eng, fn):
    """fn()'s result and the (skipped, packed, full) pairs its searches added to the engine's counters"""
    a = eng.memo_stats()
    out = fn()
    b = eng.memo_stats()
    return out, tuple(int(b[k] - a[k]) for k in ("pairs_skipped", "pairs_packed", "pairs_full"))


def _scramble(eng, kernel):
    """a search of other roots with other draws, memo off: the engine's tree and latent workspace (never cleared
    between searches, no output) then holds other trees' nodes at every slot, so a memo search that gathered a
    parent latent from the workspace where it should read the table cannot find the right one left there"""
    inp = scramble_inputs()
    eng.set_memo_depth(0)
    eng.search(S, obs=_tt(inp[0]), tie_idx=_tt(inp[2]), noise=_tt(inp[1]), action_u=_tt(inp[3]), temperature=1.0,
               deterministic=False, kernel=kernel)


def _on_off_oracle(oracle, eng, kernel, D, inp, deterministic, flat=None, sup=33):
    """the search without the memo, with it at depth D, and the oracle's: all equal; returns the counted paths
    of the memo leg and the oracle's prediction of them.  Between the two legs the workspace is scrambled."""
    if flat is None:
        flat, sup = weights(oracle)
    obs, noise, tie, u, mm = inp
    eng.set_memo_depth(0)
    off, took_off = _paths(eng, lambda: _search(eng, kernel, inp, deterministic))
    assert took_off == (0, 0, 0) and eng.memo_stats()["depth"] == 0
    _scramble(eng, kernel)
    eng.set_memo_depth(D)
    on, took = _paths(eng, lambda: _search(eng, kernel, inp, deterministic))
    st = eng.memo_stats()
    assert st["depth"] == D and st["built"] == 1 and st["table_bytes"] == 288 * 81 * (6 ** (D + 1) - 1) // 5
    assert set(on) == set(off)
    for k in on:
        assert on[k].tobytes() == off[k].tobytes(), k  # every output array, the carried MinMaxStats included
    ref = oracle.search(N, S, obs, flat=flat, support=sup, noise=noise, tie_idx=tie, action_u=u, temperature=1.0,
                        deterministic=deterministic, minmax_in=mm, depths=True)
    for k, rk in OUTPUTS:
        assert np.array_equal(on[k], ref[rk]), k
    assert np.array_equal(on["minmax"][:, 0], ref["mm_max"]) and np.array_equal(on["minmax"][:, 1], ref["mm_min"])
    return took, predict_paths(ref["depths"], obs, D, RPW[kernel])


def _assert_paths(kernel, took, want):
    print("paths (skipped, packed, full):", took, "predicted:", want)
    assert took == want
    if kernel == "wave":
        assert min(took) >= 1, took  # all three forms ran
    else:
        assert took[0] >= 1 and took[1] == 0 and took[2] >= 1, took  # 16-root waves: the skip and the full form


@pytest.mark.gpu
@pytest.mark.parametrize("B", [40, 64])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("mode", CASE_MODES)
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_memo_search_equals_no_memo_and_oracle(oracle, eng64, kernel, mode, D, B):
    inp, deterministic = case_inputs(mode, B)
    took, want = _on_off_oracle(oracle, eng64, kernel, D, inp, deterministic)
    _assert_paths(kernel, took, want)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_memo_mixed_rows(oracle, eng64, kernel):
    """rows that are no state's observation (always missing) beside the goal state and duplicated roots"""
    inp = mixed_inputs()
    obs = inp[0]
    onehot = onehot_rows(obs)
    assert not onehot[list(MIXED["perturbed"])].any() and onehot.sum() == len(obs) - len(MIXED["perturbed"])
    took, want = _on_off_oracle(oracle, eng64, kernel, 2, inp, False)
    _assert_paths(kernel, took, want)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,D", [("noise", 2), ("deterministic", 3)])
def test_memo_first_search_of_a_fresh_engine(oracle, mode, D):
    """the memo search is the engine's first: no earlier search left a latent in the workspace, so every parent
    of a table node's child comes from the table or the result is wrong (32-root waves, all three forms)"""
    from muzero_hanoi_amd import engine

    flat, sup = weights(oracle)
    inp, deterministic = case_inputs(mode, 64)
    obs, noise, tie, u, mm = inp
    eng = engine.Engine(N, S, 64, sup)
    try:
        eng.load_weights(flat)
        eng.set_memo_depth(D)
        on, took = _paths(eng, lambda: _search(eng, "wave", inp, deterministic))
    finally:
        eng.close()
    ref = oracle.search(N, S, obs, flat=flat, support=sup, noise=noise, tie_idx=tie, action_u=u, temperature=1.0,
                        deterministic=deterministic, minmax_in=mm, depths=True)
    for k, rk in OUTPUTS:
        assert np.array_equal(on[k], ref[rk]), k
    assert np.array_equal(on["minmax"][:, 0], ref["mm_max"]) and np.array_equal(on["minmax"][:, 1], ref["mm_min"])
    _assert_paths("wave", took, predict_paths(ref["depths"], obs, D, 32))


@pytest.mark.gpu
def test_memo_depth_environment_variable(monkeypatch):
    """MZH_MEMO_DEPTH is a new engine's initial request; a value that is no depth refuses the engine"""
    from muzero_hanoi_amd import engine

    monkeypatch.setenv("MZH_MEMO_DEPTH", "3")
    eng = engine.Engine(N, S, 64, 33)
    assert eng.memo_stats()["depth"] == 3
    eng.close()
    for bad in ("x", "4x", "", "-2", "13"):
        monkeypatch.setenv("MZH_MEMO_DEPTH", bad)
        with pytest.raises(ValueError, match="MZH_MEMO_DEPTH"):
            engine.Engine(N, S, 64, 33)


@pytest.mark.gpu
def test_memo_invalidated_by_load_weights(oracle):
    """other weights through load_weights: the next search rebuilds the table and equals the oracle's for them"""
    from muzero_hanoi_amd import engine

    flat, sup = weights(oracle)
    eng = engine.Engine(N, S, 64, sup)
    try:
        eng.load_weights(flat)
        inp, deterministic = case_inputs("noise", 64)
        eng.set_memo_depth(2)
        _search(eng, "wave", inp, deterministic)
        assert eng.memo_stats()["built"] == 1
        flat2 = invalidation_weights(oracle)
        eng.load_weights(flat2)
        assert eng.memo_stats()["built"] == 0
        took, want = _on_off_oracle(oracle, eng, "wave", 2, inp, deterministic, flat=flat2, sup=sup)
        assert took == want and took[0] + took[1] >= 1
    finally:
        eng.close()


@pytest.mark.gpu
def test_memo_off_is_the_plain_search(oracle, eng64):
    """set_memo_depth(0): no table, no counted pair, the oracle's outputs"""
    inp, deterministic = case_inputs("noise", 64)
    obs, noise, tie, u, mm = inp
    eng64.set_memo_depth(0)
    o, took = _paths(eng64, lambda: _search(eng64, "wave", inp, deterministic))
    st = eng64.memo_stats()
    assert took == (0, 0, 0) and (st["depth"], st["built"], st["table_bytes"]) == (0, 0, 0)
    assert eng64.memo_table() is None
    flat, sup = weights(oracle)
    ref = oracle.search(N, S, obs, flat=flat, support=sup, noise=noise, tie_idx=tie, action_u=u, temperature=1.0,
                        deterministic=deterministic, minmax_in=mm)
    for k, rk in OUTPUTS:
        assert np.array_equal(o[k], ref[rk]), k
    eng64.set_memo_depth(-1)
    assert eng64.memo_stats()["depth"] == 5  # the automatic depth at four discs


@pytest.mark.gpu
@pytest.mark.parametrize("n_disks,D", [(3, 3), (4, 2)])
def test_memo_table_rows_equal_chained_inference(oracle, n_disks, D):
    """random (state, path) rows: the latent and the record equal initial_inference, then recurrent_inference
    along the path, bit for bit"""
    from muzero_hanoi_amd import engine
    from muzero_hanoi_amd.networks import MuZeroNet

    torch.manual_seed(n_disks)
    net = MuZeroNet(3 * n_disks, 6, 0.002, "cpu", TD_return=True)
    flat = engine.flat_weights(net.state_dict())
    eng = engine.Engine(n_disks, 2, 32, 33)
    try:
        eng.load_weights(flat)
        eng.set_memo_depth(D)
        obs1 = np.zeros((1, 3 * n_disks), np.float32)
        obs1[0, ::3] = 1
        eng.search(2, obs=_tt(obs1), tie_idx=_tt(np.zeros(1, np.int32)), deterministic=True, kernel="wave")
        h, rec, depth = eng.memo_table()
        K = engine.memo_nodes(D)
        assert depth == D and tuple(h.shape) == (3 ** n_disks * K, 64) and tuple(rec.shape) == (3 ** n_disks * K, 8)
        rs = np.random.RandomState(7)
        R = 96
        pegs = rs.randint(0, 3, (R, n_disks))
        lens = np.arange(R) % (D + 1)  # every depth 0..D
        paths = rs.randint(0, 6, (R, D))
        obs = np.zeros((R, 3 * n_disks), np.float32)
        obs[np.arange(R)[:, None], np.arange(n_disks) * 3 + pegs] = 1
        rows = np.array([engine.memo_state_index(pegs[i]) * K + engine.memo_node_id(paths[i, :lens[i]])
                         for i in range(R)])
        cur = eng.initial_inference(_tt(obs))
        want_h, want_pi, want_v = cur["h"].clone(), cur["pi"].clone(), cur["value"].clone()
        want_r = torch.zeros(R, device=DEV)
        for d in range(D):
            cur = eng.recurrent_inference(cur["h"], _tt(paths[:, d].astype(np.int32)))
            m = _tt(lens > d)
            want_h[m], want_pi[m], want_v[m], want_r[m] = cur["h"][m], cur["pi"][m], cur["value"][m], cur["reward"][m]
        want_rec = torch.cat([want_pi, want_r[:, None], want_v[:, None]], 1)
        idx = _tt(rows)
        assert h[idx].cpu().numpy().tobytes() == want_h.cpu().numpy().tobytes()
        assert rec[idx].cpu().numpy().tobytes() == want_rec.cpu().numpy().tobytes()
        # and the oracle's inference for the depth-0 rows
        oh = oracle.initial_inference(flat, 3 * n_disks, 33, obs)["h"]
        z = lens == 0
        assert np.array_equal(h[idx].cpu().numpy()[z], oh[z])
    finally:
        eng.close()
