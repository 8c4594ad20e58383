"""The wave kernels' record form of a new node (csrc/mzh_wave.hip phase_head): the 128-byte tree block is written
by the root's lane pair, four 16-byte chunks each, and the expansion and backup stores by one lane of the pair.

A search must not see what an earlier search left in the engine's tree buffer: every new block is written whole
before anything reads it.  So a search that follows a different one on the same engine equals, byte for byte, the
same search on an engine that has searched nothing else -- in the replay form, and in the no-MLP form that every
(wave, simulation) pair takes once the expansion memo holds all of a search's nodes.  Three discs, S = 20, 72 roots
(a last 32-root wave and a last 16-root wave of 8).
"""
import numpy as np
import pytest
import torch

from test_memo_grow_gpu import KEYS, S, _counted, _engine, _inputs, _same, _search
from test_memo_paths_gpu import N3, _tt

B = 72


def _replay_inputs(seed):
    """synthetic records: softmax priors, small rewards and values; deterministic search, distinct tie draws"""
    r = np.random.RandomState(seed)

    def softmax(x):
        e = np.exp(x - x.max(-1, keepdims=True))
        return (e / e.sum(-1, keepdims=True)).astype(np.float32)

    obs = np.zeros((B, 3 * N3), np.float32)
    obs[:, ::3] = 1.0
    return dict(obs=obs, root_pi=softmax(r.randn(B, 6)), pi=softmax(r.randn(B, S, 6)),
                reward=(0.1 * r.randn(B, S)).astype(np.float32), value=r.randn(B, S).astype(np.float32),
                tie=r.randint(0, 6, B).astype(np.int32))  # the child a root's first six-way tie takes: 0..5


def _replay(eng, kernel, x):
    o = eng.search(S, obs=_tt(x["obs"]), replay={k: _tt(x[k]) for k in ("root_pi", "pi", "reward", "value")},
                   tie_idx=_tt(x["tie"]), temperature=1.0, deterministic=True, kernel=kernel)
    nt = 2 if kernel == "wave" else 1
    assert o["_plan"]["kernel"].startswith(f"mzh_wave_kernel<{nt}, true,"), o["_plan"]
    return {k: v.cpu().numpy() for k, v in o.items() if not k.startswith("_")}


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_replay_form_over_a_used_tree(oracle, kernel):
    x, y = _replay_inputs(1), _replay_inputs(2)
    fresh = _engine(oracle, B, 0)
    used = _engine(oracle, B, 0)
    try:
        want = _replay(fresh, kernel, x)
        other = _replay(used, kernel, y)
        assert other["visits"].tobytes() != want["visits"].tobytes()  # the two searches do differ
        _same(_replay(used, kernel, x), want)
        assert int(want["visits"].sum()) == B * S
    finally:
        fresh.close()
        used.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_no_mlp_form_over_a_used_tree(oracle, kernel):
    """search x until the memo holds its nodes, then y, then x again: x runs no MLP and equals the memo-off engine"""
    ix, det = _inputs(B, "plain", seed=0)
    iy, _ = _inputs(B, "plain", seed=5)
    off = _engine(oracle, B, 0)
    eng = _engine(oracle, B, 1)
    try:
        want = _search(off, kernel, ix, det)
        for _ in range(8):  # (test_memo_grow_gpu: converged by the eighth identical launch)
            _search(eng, kernel, ix, det)
        _same(_search(eng, kernel, iy, det), _search(off, kernel, iy, det))
        got, took, _ = _counted(eng, lambda: _search(eng, kernel, ix, det))
        pairs = S * -(-B // (32 if kernel == "wave" else 16))
        assert dict(zip(KEYS, took)) == {"pairs_skipped": pairs, "pairs_packed": 0, "pairs_full": 0}
        _same(got, want)
    finally:
        off.close()
        eng.close()
