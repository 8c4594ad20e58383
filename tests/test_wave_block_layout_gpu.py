"""The wave kernels' tree block, keyed by child and split by lane half (csrc/mzh_wave.hip MzwBlock, DESIGN.md
section 2): four aligned 16-byte loads per selection level, one 16-byte store {W | N X | R} per backed-up node,
the node's memo row + 1 in the priors' chunk of both halves.

Three discs, the kernel forced to `wave` (32 roots per wave) and `wave16`:

- replayed searches with peaked priors, so that the paths run deeper than the LDS path cache (MZW_DC = 16): the
  statistics of the nodes below it come back from the block (one load of the unit) and go out in the merged store,
  with the child index and reward the unit already holds;
- 300 simulations, so that a child's expanded index and visit count need all sixteen bits of their fields;
- one engine from a cold memo to a warm one: both block writers' row words, the harvest's publication into both
  halves and the lookup from the word selection's last load brought.
"""
import numpy as np
import pytest
import torch

from test_memo_grow_gpu import KEYS, _counted, _engine, _inputs, _same, _search
from test_memo_paths_gpu import N3, OUTPUTS, _tt

MZW_DC = 16  # csrc/mzh_wave.hip: selection-path depths cached in LDS


def _peaked_replay(B, S, peak, vmean):
    """records whose priors favour one random action each (softmax of 0.3 randn, + peak on it): long, narrow trees"""
    r = np.random.RandomState(3)

    def priors(*shape):
        x = 0.3 * r.randn(*shape, 6)
        hot = r.randint(0, 6, shape)
        x += peak * (np.arange(6) == hot[..., None])
        e = np.exp(x - x.max(-1, keepdims=True))
        return (e / e.sum(-1, keepdims=True)).astype(np.float32)

    obs = np.zeros((B, 3 * N3), np.float32)
    obs[:, ::3] = 1.0
    return dict(obs=obs, root_pi=priors(B), pi=priors(B, S), rwd=(0.05 * r.randn(B, S)).astype(np.float32),
                value=(vmean + 0.1 * r.randn(B, S)).astype(np.float32), tie=r.randint(0, 6, B).astype(np.int32))


_REF = {}


def _reference(oracle, name, B, S, peak, vmean):
    """the inputs and the oracle's search of them, computed once per case and shared by both kernels"""
    if name not in _REF:
        x = _peaked_replay(B, S, peak, vmean)
        ref = oracle.search(N3, S, x["obs"], replay={k: x[k] for k in ("root_pi", "pi", "rwd", "value")},
                            tie_idx=x["tie"], temperature=1.0, deterministic=True, depths=True)
        _REF[name] = (x, ref)
    return _REF[name]


def _replay_equals_oracle(kernel, B, S, x, ref):
    from muzero_hanoi_amd import engine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    eng = engine.Engine(N3, S, B, 33)
    try:
        o = eng.search(S, obs=_tt(x["obs"]), replay=dict(root_pi=_tt(x["root_pi"]), pi=_tt(x["pi"]), reward=_tt(x["rwd"]),
                                                         value=_tt(x["value"])),
                       tie_idx=_tt(x["tie"]), temperature=1.0, deterministic=True, kernel=kernel)
        nt = 2 if kernel == "wave" else 1
        assert o["_plan"]["kernel"].startswith(f"mzh_wave_kernel<{nt}, true,"), o["_plan"]
        got = {k: v.cpu().numpy() for k, v in o.items() if not k.startswith("_")}
    finally:
        eng.close()
    for k, rk in OUTPUTS:
        assert np.array_equal(got[k], ref[rk]), k
    assert np.array_equal(got["minmax"][:, 0], ref["mm_max"]) and np.array_equal(got["minmax"][:, 1], ref["mm_min"])


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_paths_below_the_lds_path_cache(oracle, kernel):
    """B = 40 (a full 32-root wave and 8, or two 16-root waves and 8), S = 24: most roots walk below depth 16"""
    B, S = 40, 24
    x, ref = _reference(oracle, "deep", B, S, 6.0, 0.5)
    deepest = ref["depths"].max(1)
    print("deepest path per root:", sorted(deepest.tolist()))
    assert (deepest > MZW_DC).sum() >= B // 2
    _replay_equals_oracle(kernel, B, S, x, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_sixteen_bit_fields(oracle, kernel):
    """B = 33, S = 300: expanded indices run to 300 and a child's visit count past 255 -- neither field may be
    narrower than sixteen bits, nor clobber its neighbour in the unit's shared word"""
    B, S = 33, 300
    x, ref = _reference(oracle, "wide", B, S, 3.0, 0.2)
    print("largest child visit count:", int(ref["visits"].max()), "deepest path per root:",
          sorted(ref["depths"].max(1).tolist()))
    assert ref["visits"].max() > 255 and (ref["depths"].max(1) > MZW_DC).all()
    _replay_equals_oracle(kernel, B, S, x, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_cold_to_warm_on_one_engine(oracle, kernel):
    """B = 72, S = 20, the dense depth forced to 1, eight identical launches over a growing memo: each equals the
    memo-off engine byte for byte, every M-phase form occurs, the last launch runs no MLP at all, and another
    search in between (a used tree buffer) does not change the next one's bytes"""
    B = 72
    inp, det = _inputs(B, "plain", seed=40)
    other, _ = _inputs(B, "plain", seed=41)
    off = _engine(oracle, B, 0)
    eng = _engine(oracle, B, 1)
    try:
        want = _search(off, kernel, inp, det)
        want_other = _search(off, kernel, other, det)
        seen = np.zeros(3, np.int64)
        for launch in range(8):
            got, took, _ = _counted(eng, lambda: _search(eng, kernel, inp, det))
            _same(got, want)
            seen += took
            if launch == 3:
                _same(_search(eng, kernel, other, det), want_other)
        pairs = 20 * -(-B // (32 if kernel == "wave" else 16))
        print("pairs (skipped, packed, full) over the eight launches:", seen.tolist(), "last launch:", took)
        assert seen[0] > 0 and seen[2] > 0 and (kernel != "wave" or seen[1] > 0)
        assert dict(zip(KEYS, took)) == {"pairs_skipped": pairs, "pairs_packed": 0, "pairs_full": 0}
    finally:
        off.close()
        eng.close()
