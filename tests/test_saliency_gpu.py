"""Input saliency on the GPU (mzh_saliency: mzh_saliency_kernel / mzh_saliency_multi_kernel, Engine.saliency), the
drop-in acting.compute_saliency and the batched selfplay.evaluate_saliency.

Numbers are compared with this repository's MuZeroNet torch path in float64 on the CPU by the rule of
tests/saliency_ref.py (test_train_grad.py's): per case and head e = max|x - x64| / max|x64| must stay within
max(4 x the fp32 torch path's error on that tensor, FLOOR).  The forward's outputs, the position, tile and set
independence and the per-disc sums are compared bit for bit.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import saliency_ref as sr
from conftest import golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
NROWS = 37
VEC = ("policy", "value", "picked", "disc_policy", "disc_value", "h0", "pi0", "value0")


@pytest.fixture(scope="module")
def mzh():
    from muzero_hanoi_amd import _lib, engine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return engine


def tt(a):
    return torch.tensor(np.asarray(a), device=DEV)


def _flat(mzh, net):
    return mzh.flat_weights(net.state_dict())


def _prefilled(B, n_disks):
    """every output NaN (picked: -7), so a write outside the call shows"""
    shapes = dict(policy=(B, 3 * n_disks), value=(B, 3 * n_disks), disc_policy=(B, n_disks), disc_value=(B, n_disks),
                  h0=(B, 64), pi0=(B, 6), value0=(B,))
    out = {k: torch.full(s, float("nan"), dtype=torch.float32, device=DEV) for k, s in shapes.items()}
    out["picked"] = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    return out


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(a, b):
    """bit for bit (NaN patterns included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _untouched(got, rows):
    return all(np.isnan(got[k][rows]).all() for k in VEC if k != "picked") and (got["picked"][rows] == -7).all()


@pytest.fixture(scope="module", params=sr.WEIGHTS, ids=[w[0] for w in sr.WEIGHTS])
def case(request, mzh):
    """per weight fixture, computed once: the engine, the float64 reference of its 37 rows and the dense call"""
    name, n, sup = request.param
    net = sr.npz_net(name)
    ref = sr.weights_reference(name)
    eng = mzh.Engine(n, 1, 64, sup)
    eng.load_weights(_flat(mzh, net))
    dense = _np(eng.saliency(tt(ref.obs), full=True, tile=16))
    return name, n, eng, ref, dense


# ------------------------------------------------------------------------------------ single network
def test_saliency_agrees_with_float64(case):
    """37 rows (two 16-row tiles and a ragged third), 5 of them arbitrary floats: both heads within the bound of
    float64, no row excluded, and the logit differentiated is float64's argmax"""
    name, n, eng, ref, dense = case
    errs = ref.errors(dense["policy"], dense["value"])
    ref.report(name, errs)
    assert ref.bad.size == 0 and len(ref.obs) == NROWS
    assert np.array_equal(dense["picked"], ref.r64["picked"])
    for h in ("policy", "value"):
        assert np.isfinite(dense[h]).all() and errs[h] <= ref.bound[h], (name, h, errs[h], ref.bound[h])


def test_forward_outputs_are_initial_inference_bit_for_bit(case):
    """h0 / pi0 / value0 equal mzh_initial_inference on the row; picked is the lowest index of the largest logit"""
    name, n, eng, ref, dense = case
    ii = _np(eng.initial_inference(tt(ref.obs)))
    assert _same(dense["h0"], ii["h"]) and _same(dense["pi0"], ii["pi"]) and _same(dense["value0"], ii["value"])
    assert np.array_equal(dense["picked"], ii["policy_logits"].argmax(axis=1).astype(np.int32))


def test_explicit_logit_index_is_honoured(case):
    """logit_index = (row % 7) - 1: -1 keeps the argmax, 0..5 name the logit; the policy saliency follows float64 of
    that logit, the value saliency does not move"""
    name, n, eng, ref, dense = case
    li = (np.arange(NROWS) % 7 - 1).astype(np.int32)
    got = _np(eng.saliency(tt(ref.obs), logit_index=tt(li), full=True))
    want = np.where(li >= 0, li, dense["picked"])
    assert np.array_equal(got["picked"], want) and (want != dense["picked"]).any()
    r2 = sr.Reference(sr.npz_net(name), ref.obs, logit_index=li)
    errs = r2.errors(got["policy"], got["value"])
    r2.report(name + " logit_index", errs)
    assert r2.bad.size == 0 and np.array_equal(r2.r64["picked"], want)
    assert errs["policy"] <= r2.bound["policy"] and _same(got["value"], dense["value"])
    same = want == dense["picked"]
    assert _same(got["policy"][same], dense["policy"][same])


def test_rows_do_not_depend_on_tile_position_or_env_index(case):
    """tile 16 vs 32, a permuted env_index sub-batch of a larger batch and a row repeated in another position give
    the same bits; rows outside the call keep their prefill"""
    name, n, eng, ref, dense = case
    t32 = _np(eng.saliency(tt(ref.obs), full=True, tile=32))
    for k in VEC:
        assert _same(t32[k], dense[k]), f"{name}: {k} differs between the tiles"
    B = 45
    rs = np.random.RandomState(5)
    full = rs.uniform(-1, 1, (B, 3 * n)).astype(np.float32)
    envs = rs.permutation(B)[:NROWS + 1].astype(np.int32)
    full[envs[:NROWS]] = ref.obs
    full[envs[NROWS]] = ref.obs[3]  # row 3 once more, as the call's last row (the third tile at 16)
    for tile in (16, 32):
        out = _prefilled(B, n)
        eng.saliency(tt(full), env_index=tt(envs), out=out, tile=tile)
        got = _np(out)
        for k in VEC:
            assert _same(got[k][envs[:NROWS]], dense[k]), f"{name} tile {tile}: {k} moved with the row's position"
            assert _same(got[k][envs[NROWS]], dense[k][3]), f"{name} tile {tile}: {k} of the repeated row"
        assert _untouched(got, np.setdiff1d(np.arange(B), envs))


def test_bad_env_index_and_logit_index_are_counted_and_skipped(case):
    name, n, eng, ref, dense = case
    B = NROWS
    envs = np.arange(20, dtype=np.int32)
    envs[4], envs[17] = B, -1  # outside [0, B)
    li = np.full(B, -1, np.int32)
    li[2], li[9], li[19] = 6, -2, 5  # 6 and -2 are outside [-1, 6)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = _prefilled(B, n)
    eng.saliency(tt(ref.obs), env_index=tt(envs), logit_index=tt(li), out=out, err=err)
    got = _np(out)
    assert int(err.item()) == 4
    ok = np.setdiff1d(np.arange(20), [2, 4, 9, 17, 19])
    for k in VEC:
        assert _same(got[k][ok], dense[k][ok]), k
    assert got["picked"][19] == 5 and _same(got["value"][19], dense["value"][19])
    assert _untouched(got, np.array([2, 4, 9, 17] + list(range(20, B))))


def test_per_disc_outputs_are_the_fp32_formula(case):
    name, n, eng, ref, dense = case
    for h in ("policy", "value"):
        a = np.abs(dense[h]).reshape(NROWS, n, 3)
        assert _same(dense["disc_" + h], (a[:, :, 0] + a[:, :, 1]) + a[:, :, 2]), h


# ------------------------------------------------------------------------------------ several networks
@pytest.fixture(scope="module")
def set_case(mzh):
    """the fixture's three networks as a set on one engine and alone on one engine each"""
    nets = sr.fixture_nets()
    flats = [_flat(mzh, net) for net in nets]
    eng = mzh.Engine(3, 1, 128, 33)
    eng.load_weight_set(flats)
    singles = []
    for f in flats:
        e1 = mzh.Engine(3, 1, 64, 33)
        e1.load_weights(f)
        singles.append(e1)
    obs = np.concatenate([sr.state_obs(sr.all_states(3)), sr.case_obs(3, seed=1)[27:]])  # 27 states + 10 more rows
    return eng, singles, obs


@pytest.mark.parametrize("tile", [16, 32])
@pytest.mark.parametrize("counts", [(5, 0, 20), (17, 16, 1)], ids=lambda c: "-".join(map(str, c)))
def test_set_equals_single_network_calls(set_case, counts, tile):
    """uneven row counts per network: every output equals the single-network call's, bit for bit"""
    eng, singles, obs = set_case
    n = sum(counts)
    net_index = np.repeat(np.arange(3), counts).astype(np.int32)
    out = _prefilled(NROWS, 3)
    res = eng.saliency(tt(obs), env_index=torch.arange(n, dtype=torch.int32, device=DEV), net_index=tt(net_index),
                       out=out, tile=tile)
    assert res["_status"].tolist() == [0, sum(-(-c // tile) for c in counts)]
    got = _np(out)
    lo = 0
    for m, c in enumerate(counts):
        if c:
            one = _np(singles[m].saliency(tt(obs[lo:lo + c]), full=True, tile=tile))
            for k in VEC:
                assert _same(got[k][lo:lo + c], one[k]), f"counts {counts} tile {tile} network {m}: {k}"
            if m:  # a kernel that ignored net_index would not pass
                other = _np(singles[0].saliency(tt(obs[lo:lo + c]), full=True, tile=tile))
                assert not _same(got["policy" if m == 1 else "value"][lo:lo + c], other["policy" if m == 1 else "value"])
        lo += c
    assert _untouched(got, np.arange(n, NROWS))


@pytest.mark.parametrize("tile", [16, 32])
def test_set_refuses_a_decreasing_net_index_on_the_device(set_case, tile):
    """a decreasing net_index and an entry equal to M: nothing is written, status[0] == 1"""
    eng, _, obs = set_case
    for bad in ([0] * 10 + [2] * 5 + [1] * 6, [0] * 20 + [3]):
        ni = np.array(bad, np.int32)
        out = _prefilled(len(ni), 3)
        res = eng.saliency(tt(obs[:len(ni)]), net_index=tt(ni), out=out, tile=tile)
        assert res["_status"].tolist()[0] == 1
        assert _untouched(_np(out), np.arange(len(ni)))


# ------------------------------------------------------------------------------------ the drop-in and the atlas
def test_evaluate_saliency_and_drop_in_on_the_fixture_networks():
    """selfplay.evaluate_saliency (27 states x 3 networks, one call on a set) and acting.compute_saliency (one
    state, one network per call): within the bound of float64, the fixture's picked indices, and the reference's
    own fp32 vectors within the sum of the kernel's bound and the fixture's fp32 error"""
    from muzero_hanoi_amd import acting, selfplay

    g = golden("saliency_n3.npz")
    nets, refs = sr.fixture_nets(), sr.fixture_reference()
    got = selfplay.evaluate_saliency(list(nets), 3)
    assert got["policy"].shape == got["value"].shape == (3, 27, 9) and got["picked"].shape == (3, 27)
    assert got["disc_policy"].shape == got["disc_value"].shape == (3, 27, 3)
    assert np.array_equal(got["states"], np.arange(27)) and np.array_equal(got["picked"], g["picked"])
    for m, ref in enumerate(refs):
        errs = ref.errors(got["policy"][m], got["value"][m])
        ref.report(f"evaluate_saliency network {m}", errs)
        assert ref.bad.size == 0
        for h in ("policy", "value"):
            assert errs[h] <= ref.bound[h], (m, h, errs[h], ref.bound[h])
            fix = sr.rel_err(g[h][m], ref.r64[h])  # the fixture's own fp32 error
            vs_ref = float(np.abs(got[h][m].astype(np.float64) - g[h][m]).max() / np.abs(ref.r64[h]).max())
            print(f"  {h}: against the reference's vectors {vs_ref:.2e} (fixture's fp32 error {fix:.2e})")
            assert vs_ref <= ref.bound[h] + fix
            a = np.abs(got[h][m]).reshape(27, 3, 3)
            assert _same(got["disc_" + h][m], (a[:, :, 0] + a[:, :, 1]) + a[:, :, 2])
    # a subset of states through state tuples, one network
    sub = selfplay.evaluate_saliency(nets[1], 3, states=[(2, 2, 0), (0, 0, 2), (1, 2, 2)])
    idx = [selfplay.state_index(s) for s in ((2, 2, 0), (0, 0, 2), (1, 2, 2))]
    assert np.array_equal(sub["states"], idx) and _same(sub["policy"][0], got["policy"][1][idx])
    assert _same(sub["value"][0], got["value"][1][idx])
    # the sequential drop-in: the same bits as the batch's rows
    for m, s in ((0, 0), (1, 13), (2, 26), (1, 21)):
        state = tuple(int(x) for x in sr.all_states(3)[s])
        d = acting.compute_saliency(state, 3, nets[m], 0)
        assert set(d) == {"policy", "value"} and d["policy"].dtype == d["value"].dtype == np.float32
        assert d["policy"].shape == d["value"].shape == (9,)
        assert _same(d["policy"], got["policy"][m, s]) and _same(d["value"], got["value"][m, s])
        per_disc = acting.aggregate_saliency_per_disk(d["policy"])
        assert np.allclose(per_disc, got["disc_policy"][m, s], rtol=1e-6)
    with pytest.raises(ValueError):
        acting.compute_saliency((0, 1), 2, nets[0], 0)
