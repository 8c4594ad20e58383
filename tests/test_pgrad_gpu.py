"""Parameter gradients of the five sub-networks on the GPU (mzh_param_grads: mzh_pgrad_kernel /
mzh_pgrad_multi_kernel / mzh_pgrad_expand_kernel, Engine.param_grads), the drop-in acting.gradient_get_results and
the batched selfplay.evaluate_gradients.

Numbers are compared with this repository's MuZeroNet torch path in float64 on the CPU by the rule of
tests/pgrad_ref.py: per case and tensor kind e = max|x - x64| / max|x64| must stay within max(4 x the fp32 torch
path's error on that tensor, FLOOR); the policy net's deltas under the reference's (constant) objective are held to
absolute bounds.  The forward's outputs, the position, tile and set independence and the dense expansion are
compared bit for bit.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import pgrad_ref as pr
from conftest import golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
NROWS = pr.NROWS
SHAPES = dict(delta1=(5, 256), delta2=(5, 64), act=(5, 256), h0=(64,), z1=(64,), h1=(64,), pi0=(6,), value0=(),
              reward=(), objective=(5,))
VEC = tuple(SHAPES)
NF3 = pr.dense_slices(9, 33)[-1][2]  # floats of an N = 3, 33-bin network


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


def _prefilled(B):
    """every output NaN, so a write outside the call shows"""
    return {k: torch.full((B,) + s, float("nan"), dtype=torch.float32, device=DEV) for k, s in SHAPES.items()}


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(a, b):
    """bit for bit (NaN patterns included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _untouched(got, rows):
    return all(np.isnan(got[k][rows]).all() for k in VEC)


def _check_factors(title, ref, got):
    """the rule: every kind and net within its bound, the policy net's constant-objective rows within the absolute
    bounds, every output finite; prints before it asserts"""
    errs = ref.errors(got)
    ref.report(title, errs)
    d2, d1, nabs = ref.policy_abs(got)
    print(f"  policy net, {nabs} rows of the reference's objective: max |delta2| {d2:.3e}, max |delta1| / sum|W2| {d1:.3e} "
          f"(bound {pr.ABS_POLICY:.3e})")
    assert int(ref.forced.sum()) + nabs == len(ref.obs)  # every row is compared, one way or the other
    for k in VEC:
        assert np.isfinite(got[k]).all(), k
    for key, e in errs.items():
        assert e <= ref.bound[key], (title, key, e, ref.bound[key])
    assert d2 <= pr.ABS_POLICY and d1 <= pr.ABS_POLICY


@pytest.fixture(scope="module", params=pr.WEIGHTS, ids=[w[0] for w in pr.WEIGHTS])
def case(request, mzh):
    """per weight fixture, computed once: the engine, the float64 reference of its 37 rows and the dense call"""
    name, n, sup = request.param
    net = pr.npz_net(name)
    ref = pr.weights_reference(name)
    eng = mzh.Engine(n, 1, 64, sup)
    eng.load_weights(_flat(mzh, net))
    args = (tt(ref.obs), tt(ref.action))
    dense = _np(eng.param_grads(*args, policy_logit=tt(ref.policy_logit), full=True, dense=True, tile=16))
    return name, n, sup, eng, ref, dense


# ------------------------------------------------------------------------------------ single network
def test_factors_and_objectives_agree_with_float64(case):
    """37 rows (two 16-row tiles and a ragged third), 5 of them arbitrary floats, both policy objectives: every
    factor and the five scalars within the bound of float64, no row excluded"""
    name, n, sup, eng, ref, dense = case
    assert ref.bad.size == 0 and ref.near0_rows.size == 0 and len(ref.obs) == NROWS
    _check_factors(name, ref, dense)
    outs = (64, 64, sup, 6, sup)
    for i in range(5):  # delta2 beyond the net's outputs is +0
        assert not dense["delta2"][:, i, outs[i]:].view(np.uint32).any()


def test_forward_outputs_are_the_inference_calls_bit_for_bit(case):
    """h0 / pi0 / value0 equal mzh_initial_inference, h1 / reward mzh_recurrent_inference(h0, action); z1 normalised
    by normalize_h_state's formula in fp32 gives h1"""
    name, n, sup, eng, ref, dense = case
    ii = _np(eng.initial_inference(tt(ref.obs)))
    assert _same(dense["h0"], ii["h"]) and _same(dense["pi0"], ii["pi"]) and _same(dense["value0"], ii["value"])
    ri = _np(eng.recurrent_inference(tt(ii["h"]), tt(ref.action)))
    assert _same(dense["h1"], ri["h"]) and _same(dense["reward"], ri["reward"])
    z = dense["z1"]
    mn, mx = z.min(axis=1, keepdims=True), z.max(axis=1, keepdims=True)
    assert _same((z - mn) / (mx - mn + np.float32(1e-8)), dense["h1"])


def test_rows_do_not_depend_on_tile_position_or_env_index(case):
    """tile 16 vs 32, a permuted env_index sub-batch of B = 45 and a row repeated as the call's last give the same
    bits; rows outside the call keep their NaN prefill"""
    name, n, sup, eng, ref, dense = case
    t32 = _np(eng.param_grads(tt(ref.obs), tt(ref.action), policy_logit=tt(ref.policy_logit), full=True, tile=32))
    for k in VEC:
        assert _same(t32[k], dense[k]), f"{name}: {k} differs between the tiles"
    B = 45
    rs = np.random.RandomState(5)
    full = rs.uniform(-1, 1, (B, 3 * n)).astype(np.float32)
    act = rs.randint(0, 6, B).astype(np.int32)
    pl = rs.randint(-1, 6, B).astype(np.int32)
    envs = rs.permutation(B)[:NROWS + 1].astype(np.int32)
    full[envs[:NROWS]], act[envs[:NROWS]], pl[envs[:NROWS]] = ref.obs, ref.action, ref.policy_logit
    full[envs[NROWS]], act[envs[NROWS]], pl[envs[NROWS]] = ref.obs[3], ref.action[3], ref.policy_logit[3]
    for tile in (16, 32):
        out = _prefilled(B)
        eng.param_grads(tt(full), tt(act), env_index=tt(envs), policy_logit=tt(pl), out=out, tile=tile)
        got = _np(out)
        for k in VEC:
            assert _same(got[k][envs[:NROWS]], dense[k]), f"{name} tile {tile}: {k} moved with the row's position"
            assert _same(got[k][envs[NROWS]], dense[k][3]), f"{name} tile {tile}: {k} of the repeated row"
        assert _untouched(got, np.setdiff1d(np.arange(B), envs))


def test_bad_env_index_action_and_policy_logit_are_counted_and_skipped(case):
    name, n, sup, eng, ref, dense = case
    B = NROWS
    envs = np.arange(20, dtype=np.int32)
    envs[4], envs[17] = B, -1  # outside [0, B)
    act = ref.action.copy()
    act[7], act[11] = 6, -1  # outside 0..5
    pl = ref.policy_logit.copy()
    pl[2], pl[9] = 6, -2  # outside [-1, 6)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = _prefilled(B)
    nf = dense["grad"].shape[1]
    out["grad"] = torch.full((20, nf), float("nan"), dtype=torch.float32, device=DEV)
    eng.param_grads(tt(ref.obs), tt(act), env_index=tt(envs), policy_logit=tt(pl), out=out, err=err)
    got = _np(out)
    assert int(err.item()) == 6
    skipped = [2, 4, 7, 9, 11, 17]
    ok = np.setdiff1d(np.arange(20), skipped)
    for k in VEC:
        assert _same(got[k][ok], dense[k][ok]), k
    assert _untouched(got, np.array([2, 7, 9, 11] + list(range(20, B))))
    assert _same(got["grad"][ok], dense["grad"][ok]) and np.isnan(got["grad"][skipped]).all()


def test_dense_gradients_are_the_factors_products_and_agree_with_float64(case):
    """grad equals dense_gradients of the call's own factors bit for bit, agrees with float64 by the rule, and the
    factor outputs are the same bits with grad NULL"""
    from muzero_hanoi_amd import selfplay

    name, n, sup, eng, ref, dense = case
    fac = {k: tt(dense[k]) for k in ("delta1", "delta2", "act", "h0", "z1")}
    want = selfplay.dense_gradients(fac, tt(ref.obs), tt(ref.action), sup).cpu().numpy()
    assert dense["grad"].shape == want.shape == (NROWS, sum(hi - lo for _, lo, hi in pr.dense_slices(3 * n, sup)))
    assert _same(dense["grad"], want)
    for key, (e, bound) in ref.dense_errors(dense["grad"]).items():
        print(f"{name} {key}: e {e:.2e} bound {bound:.2e}")
        assert e <= bound, (name, key, e, bound)
    plain = _np(eng.param_grads(tt(ref.obs), tt(ref.action), policy_logit=tt(ref.policy_logit), full=True, tile=16))
    assert "grad" not in plain
    for k in VEC:
        assert _same(plain[k], dense[k]), k


def test_a_weight_refresh_of_either_kind_reaches_the_extra_buffer(mzh):
    """load_weights, then load_weights_from, each followed by param_grads: the new network's result (the buffer of
    dynamic_net.2 / rwd_net.2 transposed is made again after every load)"""
    import copy

    a, b = pr.npz_net("weights_N3_s0"), pr.fixture_nets()[0]
    ref = pr.weights_reference("weights_N3_s0")
    args = dict(policy_logit=tt(ref.policy_logit), full=True)
    fresh = []
    for net in (a, b):
        e1 = mzh.Engine(3, 1, 64, 33)
        e1.load_weights(_flat(mzh, net))
        fresh.append(_np(e1.param_grads(tt(ref.obs), tt(ref.action), **args)))
    assert not _same(fresh[0]["delta1"][:, 1], fresh[1]["delta1"][:, 1]) and not _same(fresh[0]["delta1"][:, 2], fresh[1]["delta1"][:, 2])
    eng = mzh.Engine(3, 1, 64, 33)
    eng.load_weights(_flat(mzh, a))
    first = _np(eng.param_grads(tt(ref.obs), tt(ref.action), **args))
    eng.load_weights(_flat(mzh, b))
    second = _np(eng.param_grads(tt(ref.obs), tt(ref.action), **args))
    live = copy.deepcopy(a).to(DEV)
    eng.load_weights_from(live.state_dict())
    third = _np(eng.param_grads(tt(ref.obs), tt(ref.action), **args))
    for k in VEC:
        assert _same(first[k], fresh[0][k]) and _same(second[k], fresh[1][k]) and _same(third[k], fresh[0][k]), k


# ------------------------------------------------------------------------------------ several networks
@pytest.fixture(scope="module")
def set_case(mzh):
    """the fixture's three networks as a set on one engine and alone on one engine each; 37 rows"""
    nets = pr.fixture_nets()
    flats = [_flat(mzh, net) for net in nets]
    eng = mzh.Engine(3, 1, 128, 33)
    eng.load_weight_set(flats)
    singles = []
    for f in flats:
        e1 = mzh.Engine(3, 1, 64, 33)
        e1.load_weights(f)
        singles.append(e1)
    ref = pr.weights_reference("weights_N3_s0")  # its rows, under these networks
    return eng, singles, ref.obs, ref.action, ref.policy_logit


@pytest.mark.parametrize("tile", [16, 32])
@pytest.mark.parametrize("counts", [(5, 0, 20), (17, 16, 1)], ids=lambda c: "-".join(map(str, c)))
def test_set_equals_single_network_calls(set_case, counts, tile):
    """uneven row counts per network: every output equals the single-network call's, bit for bit"""
    eng, singles, obs, act, pl = set_case
    n = sum(counts)
    net_index = np.repeat(np.arange(3), counts).astype(np.int32)
    out = _prefilled(NROWS)
    res = eng.param_grads(tt(obs), tt(act), env_index=torch.arange(n, dtype=torch.int32, device=DEV), net_index=tt(net_index),
                          policy_logit=tt(pl), out=out, tile=tile, dense=True)
    assert res["_status"].tolist() == [0, sum(-(-c // tile) for c in counts)]
    got = _np(out)
    grad = res["grad"].cpu().numpy()
    lo = 0
    for m, c in enumerate(counts):
        if c:
            sl = slice(lo, lo + c)
            one = _np(singles[m].param_grads(tt(obs[sl]), tt(act[sl]), policy_logit=tt(pl[sl]), full=True, tile=tile, dense=True))
            for k in VEC:
                assert _same(got[k][sl], one[k]), f"counts {counts} tile {tile} network {m}: {k}"
            assert _same(grad[sl], one["grad"])
            if m:  # a kernel that ignored net_index would not pass: the ablated head's own gradients differ
                other = _np(singles[0].param_grads(tt(obs[sl]), tt(act[sl]), policy_logit=tt(pl[sl]), full=True, tile=tile))
                ni = 3 if m == 1 else 4
                assert not _same(got["act"][sl, ni], other["act"][:, ni])
        lo += c
    assert _untouched(got, np.arange(n, NROWS))


@pytest.mark.parametrize("tile", [16, 32])
def test_set_refuses_a_decreasing_net_index_on_the_device(set_case, tile):
    """a decreasing net_index and an entry equal to M: nothing is written (grad included), status[0] == 1"""
    eng, _, obs, act, pl = set_case
    for bad in ([0] * 10 + [2] * 5 + [1] * 6, [0] * 20 + [3]):
        ni = np.array(bad, np.int32)
        out = _prefilled(len(ni))
        out["grad"] = torch.full((len(ni), NF3), float("nan"), dtype=torch.float32, device=DEV)
        res = eng.param_grads(tt(obs[:len(ni)]), tt(act[:len(ni)]), net_index=tt(ni), out=out, tile=tile)
        assert res["_status"].tolist()[0] == 1
        assert _untouched(_np(out), np.arange(len(ni))) and bool(torch.isnan(out["grad"]).all())


# ------------------------------------------------------------------------------------ the drop-in and the atlas
def test_evaluate_gradients_and_drop_in_on_the_fixture_networks():
    """selfplay.evaluate_gradients (3 networks x 27 states x 6 actions, one call on a set) within the bound of
    float64 and of the reference's own recorded numbers (the kernel's bound plus the fixture's fp32 error); the
    default pair's dense gradients against the fixture's 20 tensors; acting.gradient_get_results gives the atlas
    rows' bits in the reference's tuple shapes"""
    from muzero_hanoi_amd import acting, selfplay

    g = golden("pgrad_n3.npz")
    nets, refs = pr.fixture_nets(), pr.fixture_reference()
    got = selfplay.evaluate_gradients(list(nets), 3)
    assert got["delta1"].shape == got["act"].shape == (3, 27, 6, 5, 256) and got["delta2"].shape == (3, 27, 6, 5, 64)
    assert got["objective"].shape == (3, 27, 6, 5) and got["reward"].shape == (3, 27, 6)
    assert np.array_equal(got["states"], np.arange(27)) and np.array_equal(got["actions"], np.arange(6))
    rows = np.arange(27) * 6 + np.arange(27) % 6
    for m, ref in enumerate(refs):
        flat = {k: got[k][m].reshape((162,) + got[k].shape[3:]) for k in VEC}
        assert ref.bad.size == 0 and ref.near0_rows.size <= pr.NEAR0_ROWS_CAP
        _check_factors(f"evaluate_gradients network {m}", ref, flat)
        for kind in ("delta1", "delta2"):
            for i in (0, 1, 2, 4):
                scale = np.abs(ref.r64[kind][:, i]).max()
                x64 = ref.r64[kind][rows, i].astype(np.float64)
                dfix = np.abs(g[kind][m, :, i] - x64)
                dgot = np.abs(flat[kind][rows, i].astype(np.float64) - g[kind][m, :, i])
                if kind == "delta1":  # a unit at the kink: either side may have taken either mask
                    near = ref.near0[rows, i]
                    open64 = ref.r64["d1_open"][rows, i]
                    dfix = np.where(near, np.minimum(dfix, np.minimum(np.abs(g[kind][m, :, i]), np.abs(g[kind][m, :, i] - open64))), dfix)
                    dgot = np.where(near, np.minimum(dgot, np.abs(dgot - np.abs(open64))), dgot)  # or they differ by it
                fix, vs_ref = dfix.max() / scale, dgot.max() / scale
                print(f"  network {m} {kind} {pr.NETS[i]}: against the reference's numbers {vs_ref:.2e} (fixture's fp32 error {fix:.2e})")
                assert vs_ref <= ref.bound[kind, i] + fix
    # the default pair (state 0_0_0, action 0) under the base network: the dense gradients
    one = selfplay.evaluate_gradients(nets[0], 3, states=[(0, 0, 0)], actions=[0], dense=True)
    assert one["grad"].shape == (1, 1, 1, NF3)
    for k in VEC:
        assert _same(one[k][0, 0, 0], got[k][0, 0, 0])
    want = refs[0].dense64()[0]
    d = acting.gradient_get_results(nets[0], (0, 0, 0), 0)
    assert tuple(d) == pr.NETS
    for i, (name, module) in enumerate(zip(pr.NETS, pr.MODULES)):
        params = list(getattr(nets[0], module).parameters())
        assert isinstance(d[name], tuple) and len(d[name]) == 4
        for (key, lo, hi), t, prm in zip(pr.dense_slices(9, 33)[4 * i: 4 * i + 4], d[name], params):
            assert t.dtype == torch.float32 and t.shape == prm.shape and t.device.type == "cpu"
            assert _same(t.numpy().reshape(-1), one["grad"][0, 0, 0, lo:hi]), key
            fx = g["grad." + key].reshape(-1)
            if i == 3:
                assert np.abs(t.numpy()).max() <= pr.ABS_POLICY * max(1.0, refs[0].w2abs[3].max(), refs[0].r64["act"][0, 3].max())
                continue
            fix = pr.rel(fx, want[lo:hi])
            vs_ref = float(np.abs(t.numpy().reshape(-1).astype(np.float64) - fx).max() / np.abs(want[lo:hi]).max())
            bound = max(refs[0].bound["delta1" if ".0." in key else "delta2", i], refs[0].bound["act", i] if ".2.weight" in key else 0.0)
            print(f"  default pair {key}: against the fixture's tensor {vs_ref:.2e} (fixture's fp32 error {fix:.2e}, bound {bound:.2e})")
            assert vs_ref <= 2 * bound + fix  # a product of two factors, each within its bound
    # the sequential drop-in elsewhere in the atlas, and its refusals
    for m, s, a in ((1, 13, 1), (2, 26, 5)):
        state = tuple(int(x) for x in pr.all_states(3)[s])
        d = acting.gradient_get_results(nets[m], state, a)
        assert _same(d["value"][1].numpy(), got["delta1"][m, s, a, 4]) and _same(d["dynamic"][3].numpy(), got["delta2"][m, s, a, 1])
        assert _same(d["reward"][3].numpy(), got["delta2"][m, s, a, 2, :33])
    with pytest.raises(ValueError):
        acting.gradient_get_results(nets[0], (0, 1), 0)
    with pytest.raises(ValueError):
        acting.gradient_get_results(nets[0], (0, 1, 2), 6)
