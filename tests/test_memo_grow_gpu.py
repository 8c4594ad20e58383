"""The expansion memo's grown extension (include/mzh.h mzh_set_memo_grow) on the GPU.

Three discs (27 states), 72-200 roots, S = 20 and the dense depth forced to 1 or 2, so that most new nodes lie
below the dense table and miss until the harvest after a search has inserted them.  Whatever the extension holds,
every output array of a search equals, byte for byte, the search of an engine without a memo.
"""
import itertools

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_memo_paths_gpu import N3, _tt, inputs3, weights3

S = 20
KEYS = ("pairs_skipped", "pairs_packed", "pairs_full")
PAIRS = np.array([[-np.inf, np.inf], [0.4, -0.2], [0.05, 0.05], [1.5, 0.0], [0.0, -1.0]], np.float64)


def _engine(oracle, B, D, flat=None, grow=None, log=None):
    from muzero_hanoi_amd import engine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    if flat is None:
        flat = weights3(oracle)[0]
    eng = engine.Engine(N3, S, B, 33)
    eng.load_weights(flat)
    eng.set_memo_depth(D)
    if grow is not None or log is not None:
        eng.set_memo_grow(-1 if grow is None else grow, -1 if log is None else log)
    return eng


def _inputs(B, form, seed=0, perturbed=()):
    """B three-disc roots: "plain" stochastic with root noise, "minmax" deterministic with caller-given bounds"""
    obs, noise, tie, u, _ = inputs3(B, perturbed, deterministic=form == "minmax", seed=seed)
    mm = PAIRS[np.arange(B) % len(PAIRS)] if form == "minmax" else None
    return (obs, noise, tie, u, mm), form == "minmax"


def _search(eng, kernel, inp, deterministic):
    obs, noise, tie, u, mm = inp
    o = eng.search(S, obs=_tt(obs), tie_idx=_tt(tie), noise=_tt(noise), action_u=_tt(u), minmax_in=_tt(mm),
                   temperature=1.0, deterministic=deterministic, kernel=kernel)
    want_nt = 2 if kernel == "wave" else 1
    assert o["_plan"]["kernel"] == f"mzh_wave_kernel<{want_nt}, false, true>", o["_plan"]
    return {k: v.cpu().numpy() for k, v in o.items() if not k.startswith("_")}


def _counted(eng, fn):
    a = eng.memo_stats()
    out = fn()
    b = eng.memo_stats()
    return out, tuple(int(b[k] - a[k]) for k in KEYS), b


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k  # every output array, latents and carried MinMaxStats included


@pytest.fixture(scope="module")
def off(oracle):
    """the engine without a memo: the reference of every case"""
    eng = _engine(oracle, 200, 0)
    yield eng
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["plain", "minmax"])
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_repeated_searches_equal_memo_off_and_converge(oracle, off, kernel, form):
    """the same search again and again: equal to memo-off each time, rows inserted after the first, the no-MLP
    share of (wave, simulation) pairs never falls and reaches 1.0 (every root is a state's observation)"""
    B, D = 72, 1  # 72 roots: a last 32-root wave of 8, a last 16-root wave of 8
    inp, det = _inputs(B, form)
    want = _search(off, kernel, inp, det)
    eng = _engine(oracle, B, D)
    try:
        st = eng.memo_stats()
        assert st["grow_rows"] == 0 and st["grow_capacity"] == 0  # nothing is built before the first search
        shares, rows = [], []
        for launch in range(8):
            got, took, st = _counted(eng, lambda: _search(eng, kernel, inp, det))
            _same(got, want)
            assert sum(took) == S * -(-B // (32 if kernel == "wave" else 16))
            shares.append(took[0] / sum(took))
            rows.append(st["grow_rows"])
            assert st["grow_capacity"] == st["grow_budget_bytes"] // 288 and st["grow_rows_last"] == rows[-1] - (
                rows[-2] if launch else 0)
        print("no-MLP share per launch:", shares, "rows:", rows)
        assert rows[0] > 0 and shares[0] < 1.0
        assert all(b >= a for a, b in zip(shares, shares[1:])) and all(b >= a for a, b in zip(rows, rows[1:]))
        assert shares[2] > shares[0]
        assert shares[-1] == 1.0 and rows[-1] == rows[-2]  # converged: nothing misses, nothing is inserted
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,D", [("wave", 2), ("wave16", 1)])
def test_fresh_draws_each_launch(oracle, off, kernel, D):
    """noise, tie and action draws redrawn for every launch over a growing table: each equals memo-off"""
    B = 200
    eng = _engine(oracle, B, D)
    try:
        rows = []
        for launch in range(4):
            inp, det = _inputs(B, "plain", seed=10 + launch)
            _same(_search(eng, kernel, inp, det), _search(off, kernel, inp, det))
            rows.append(eng.memo_stats()["grow_rows"])
        assert rows[0] > 0 and rows[-1] > rows[0], rows
    finally:
        eng.close()


@pytest.mark.gpu
def test_extension_rows_equal_chained_inference(oracle):
    """every extension row, found through the trie from the depth-D rows: its latent and record equal
    initial_inference then recurrent_inference along the (state, path), bit for bit"""
    from muzero_hanoi_amd import engine

    B, D = 96, 1
    eng = _engine(oracle, B, D)
    try:
        for launch in range(3):
            inp, det = _inputs(B, "plain", seed=20 + launch)
            _search(eng, "wave", inp, det)
        h, rec, link, base = eng.memo_grow_table()
        link = link.cpu().numpy()
        used = len(h)
        K = engine.memo_nodes(D)
        assert base == 27 * K and used == eng.memo_stats()["grow_rows"] > 0
        # walk the trie: table row -> (state, path)
        where = {}
        todo = [(s * K + engine.memo_node_id(p), s, p) for s in range(27) for d in range(D + 1)
                for p in itertools.product(range(6), repeat=d)]
        dense = {r for r, _, _ in todo}
        while todo:
            row, s, p = todo.pop()
            for a in range(6):
                c = int(link[row, a])
                if len(p) < D:
                    assert c == 0  # links hang off the depth-D rows and the extension's only
                elif c:
                    assert base <= c < base + used and c not in where and c not in dense
                    where[c] = (s, p + (a,))
                    todo.append((c, s, p + (a,)))
        assert sorted(where) == list(range(base, base + used))  # every row in use is reachable, exactly once
        assert (link[base + used:] == 0).all()
        rows = sorted(where)
        R, L = len(rows), max(len(where[r][1]) for r in rows)
        assert L > D + 1  # chains of extension rows, not only children of dense ones
        pegs = np.array([[(where[r][0] // 3 ** i) % 3 for i in range(N3)] for r in rows])
        lens = np.array([len(where[r][1]) for r in rows])
        paths = np.array([list(where[r][1]) + [0] * (L - len(where[r][1])) for r in rows], np.int32)
        obs = np.zeros((R, 3 * N3), np.float32)
        obs[np.arange(R)[:, None], np.arange(N3) * 3 + pegs] = 1
        cur = eng.initial_inference(_tt(obs))
        want_h, want_pi, want_v = cur["h"].clone(), cur["pi"].clone(), cur["value"].clone()
        want_r = torch.zeros(R, device="cuda")
        for d in range(L):
            cur = eng.recurrent_inference(cur["h"], _tt(paths[:, d]))
            m = _tt(lens > d)
            want_h[m], want_pi[m], want_v[m], want_r[m] = cur["h"][m], cur["pi"][m], cur["value"][m], cur["reward"][m]
        want_rec = torch.cat([want_pi, want_r[:, None], want_v[:, None]], 1)
        idx = _tt(np.array(rows) - base)
        assert h[idx].cpu().numpy().tobytes() == want_h.cpu().numpy().tobytes()
        assert rec[idx].cpu().numpy().tobytes() == want_rec.cpu().numpy().tobytes()
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_tiny_capacity_fills_and_stops(oracle, off, kernel):
    """room for five rows: outputs identical, exactly five rows used, nothing written past the arrays"""
    B, D, cap = 72, 1, 5
    inp, det = _inputs(B, "plain", seed=30)
    want = _search(off, kernel, inp, det)
    eng = _engine(oracle, B, D, grow=cap * 288 + 100)
    try:
        for launch in range(3):
            _same(_search(eng, kernel, inp, det), want)
            st = eng.memo_stats()
            assert st["grow_capacity"] == cap and st["grow_rows"] == cap, st
            assert st["grow_rows_last"] == (cap if launch == 0 else 0)
        h, rec, link, base = eng.memo_grow_table()
        link = link.cpu().numpy()
        assert len(h) == cap and link.shape == (base + cap, 6)
        assert sorted(link[link != 0].tolist()) == list(range(base, base + cap))  # five links, no claim left behind
        # the dense table's last rows, next to the extension, are what a table without one holds
        ref = _engine(oracle, B, D, grow=0)
        try:
            _search(ref, kernel, inp, det)
            (dh, drec, _), (rh, rrec, _) = eng.memo_table(), ref.memo_table()
            assert dh.cpu().numpy().tobytes() == rh.cpu().numpy().tobytes()
            assert drec.cpu().numpy().tobytes() == rrec.cpu().numpy().tobytes()
        finally:
            ref.close()
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_capacity_zero_is_the_parent_behaviour(oracle, off, kernel):
    """growth off: no extension, no harvest, the same forms at every launch, outputs identical"""
    B, D = 72, 1
    inp, det = _inputs(B, "plain", seed=31)
    want = _search(off, kernel, inp, det)
    eng = _engine(oracle, B, D, grow=0)
    try:
        first = None
        for launch in range(3):
            got, took, st = _counted(eng, lambda: _search(eng, kernel, inp, det))
            _same(got, want)
            first = first or took
            assert took == first and took[0] < sum(took)
            assert (st["grow_capacity"], st["grow_rows"], st["grow_rows_last"], st["grow_budget_bytes"]) == (0, 0, 0, 0)
        assert eng.memo_grow_table() is None
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_mixed_waves(oracle, off, kernel):
    """roots that are no state's observation beside roots that are: they never touch the table, and their waves
    keep running an M phase at every simulation"""
    B, D = 72, 1
    perturbed = (1, 9, 17, 30, 71)  # the first wave and the ragged one; roots 32-63 are all states' observations
    inp, det = _inputs(B, "plain", seed=32, perturbed=perturbed)
    want = _search(off, kernel, inp, det)
    eng = _engine(oracle, B, D)
    try:
        skipped = []
        for launch in range(8):
            got, took, st = _counted(eng, lambda: _search(eng, kernel, inp, det))
            _same(got, want)
            skipped.append(took[0])
        rpw = 32 if kernel == "wave" else 16
        clean = sum(1 for w0 in range(0, B, rpw) if not any(w0 <= r < w0 + rpw for r in perturbed))
        print("skipped per launch:", skipped, "waves without a perturbed root:", clean)
        assert skipped[-1] == S * clean and skipped[0] < skipped[-1]
        assert st["grow_rows"] > 0
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("log", [1, 2])
def test_log_overflow_only_delays_insertion(oracle, off, log):
    """a miss log of one or two entries per root: outputs identical, fewer rows per launch than the default log"""
    B, D = 72, 1
    inp, det = _inputs(B, "plain", seed=33)
    want = _search(off, "wave", inp, det)
    eng, full = _engine(oracle, B, D, log=log), _engine(oracle, B, D)
    try:
        rows = []
        for launch in range(4):
            _same(_search(eng, "wave", inp, det), want)
            st = eng.memo_stats()
            assert st["grow_log_entries"] == log and st["grow_rows_last"] <= log * B
            rows.append(st["grow_rows"])
        _search(full, "wave", inp, det)
        assert 0 < rows[0] < full.memo_stats()["grow_rows"] and rows[-1] > rows[0], rows
    finally:
        eng.close()
        full.close()


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["host", "device"])
def test_weight_reload_drops_the_extension(oracle, how):
    """other weights through load_weights / load_weights_from: the extension goes with the table, and the searches
    that follow equal a fresh engine's under the new weights"""
    from muzero_hanoi_amd import engine

    B, D = 72, 1
    w2, _, _ = oracle.load_weights_npz(f"{GOLDEN}/weights_N3_s0.npz")  # weights3(other=True), as parameters
    w2 = {k: np.ascontiguousarray(v, np.float32).copy() for k, v in w2.items()}
    w2["policy_net.2.weight"] *= np.float32(-3.0)
    w2["value_net.2.weight"] *= np.float32(1.5)
    w2["dynamic_net.2.bias"] += np.float32(0.125)
    flat2 = oracle.flat_weights(w2)
    assert np.array_equal(flat2, weights3(oracle, other=True)[0])
    inp, det = _inputs(B, "plain", seed=34)
    eng = _engine(oracle, B, D)
    fresh = _engine(oracle, B, 0, flat=flat2)
    try:
        for launch in range(2):
            _search(eng, "wave", inp, det)
        assert eng.memo_stats()["grow_rows"] > 0
        if how == "host":
            eng.load_weights(flat2)
        else:
            eng.load_weights_from([torch.tensor(w2[k], device="cuda") for k in engine.WEIGHT_KEYS])
        st = eng.memo_stats()
        assert (st["built"], st["grow_rows"], st["grow_capacity"]) == (0, 0, 0)
        want = _search(fresh, "wave", inp, det)
        for launch in range(3):
            _same(_search(eng, "wave", inp, det), want)
        assert eng.memo_stats()["grow_rows"] > 0
    finally:
        eng.close()
        fresh.close()
