"""Every kernel that runs a network, over the engine's whole observation-width range.

The other GPU tests run a network at n_disks 3, 4 and 7 (in_dim 9, 12, 21: one or two 16-column k-blocks of the
first representation layer).  Here every such kernel runs at widths.WIDTHS -- in_dim 3, 6, 15, 18, 33 and 48, which
is one, one, one, two, three and three k-blocks, with 13 padding columns at one end of the range and none at the
other -- on seeded networks of this repository's MuZeroNet:

  a. initial / recurrent inference               bit for bit against the C oracle; within the project's bars of float64
  b. every search kernel                         bit for bit against the oracle's search
  c. the wave kernels' expansion memo            on, on again (the grown extension), off: the same bits, the oracle's
  d. probe, saliency, parameter gradients        against the inference calls and the oracle bit for bit, against
     and their set forms; search_multi           float64 by the rules of saliency_ref / pgrad_ref
  f. whole episodes in one launch                against the lockstep pieces and the lone engines, bit for bit

(e, the training update, is tests/test_train_grad.py's and tests/test_train_set_gpu.py's cases at in_dim 3 to 30;
g, the row copies, tests/test_replay.py's and tests/test_ingest.py's at d_state 3 and 48.)

Every observation goes in as a view inside a larger buffer whose neighbouring 64 words are NaN canaries, so a read
past a row's end poisons a compared output; outputs a wrapper lets the caller give are placed the same way and
their canaries checked.  tests/test_widths_cpu.py shows that zeroing any single input column -- every k-block's
first and last among them -- changes the bits these tests compare.

Measured on an MI355X.  Every bit comparison holds at every width, so the kernels' distance from float64 in (a)
is the oracle's, the table of tests/test_widths_cpu.py (latents <= 4.6e-7, logits <= 2.7e-7, transformed value and
reward <= 2.1e-4).  The memo legs count 40 pairs skipped or packed per search at one disc (every expansion of the
state roots is in the depth-6 table), 4 to 32 in the first and 37 to 40 in the second search at 2, 5 and 6 discs
(the extension grew to 282 to 585 rows), and none from 11 discs on.  Against float64 (e = max|x - x64| / max|x64|,
worst head / worst factor of the five nets; bounds max(4 x fp32-torch, floor) as in saliency_ref / pgrad_ref):

    width     saliency e policy / value   (bound)                pgrad factors   objectives (bound 1.82e-03)   dense, worst e / bound
    n1_s33    5.21e-07 / 7.87e-07         (4.62e-05 / 8.78e-05)  8.08e-07        1.10e-03                       6.21e-07 / 6.48e-05
    n2_s1     3.79e-07 / 4.11e-07         (4.62e-05 / 4.62e-05)  4.89e-07        5.65e-07                       5.29e-07 / 6.48e-05
    n5_s33    3.87e-07 / 6.02e-07         (4.62e-05 / 1.96e-04)  9.30e-07        3.71e-04                       5.58e-07 / 6.48e-05
    n6_s1     4.16e-07 / 4.54e-07         (4.62e-05 / 4.62e-05)  4.88e-07        9.06e-07                       6.80e-07 / 6.48e-05
    n11_s33   4.61e-07 / 8.97e-07         (4.62e-05 / 1.32e-04)  7.55e-07        9.27e-04                       7.02e-07 / 6.48e-05
    n16_s33   4.70e-07 / 4.72e-07         (4.62e-05 / 2.18e-04)  8.76e-07        7.00e-04                       5.49e-07 / 6.48e-05
    n16_s1    5.10e-07 / 3.67e-07         (4.62e-05 / 4.62e-05)  5.32e-07        5.29e-07                       5.49e-07 / 6.48e-05

The objectives' error with 33 bins is the signed parabolic transform's cancellation, the same in the fp32 torch
path (1.10e-03 at n1_s33).  The policy net's deltas under the reference's constant objective stay below 3.3e-9
(bound 2^-21).  The whole module runs in 7 s.
"""
import numpy as np
import pytest
import torch

import pgrad_ref as pr
import widths as wd
from test_legality_cpu import oracle_probe
from test_legality_gpu import _composition

pytestmark = pytest.mark.gpu

DEV = "cuda"
S, B_SEARCH = 20, 40
FORMS = [("coop", 16), ("coop", 32), ("occ2", None), ("wave", None), ("wave16", None), ("one", None)]
SEARCH_KEYS = (("visits", "visits"), ("root_q", "rootQ"), ("pi", "pi"), ("action", "action"), ("sel_steps", "sel_steps"),
               ("extra_ties", "extra_ties"), ("latent", "latent"), ("latent_len", "latent_len"))
MEMO_DEPTH = {1: -1, 2: 2, 5: 2, 6: 2, 11: -1, 16: -1}  # -1: automatic (6 at one disc, 0 from 11 discs on)


def tt(a):
    return torch.tensor(np.asarray(a), device=DEV)


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


def _same(a, b):
    """bit for bit (NaN patterns included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def mzh():
    from muzero_hanoi_amd import _lib, engine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return engine


@pytest.fixture(scope="module", params=wd.WIDTHS, ids=wd.IDS)
def width(request, mzh):
    """per width, made once: the seeded network, its canonical vector and an engine holding it"""
    n, support = request.param
    net = wd.net(n, support)
    flat = wd.flat(net)
    eng = mzh.Engine(n, S, 64, support)
    eng.load_weights(flat)
    yield n, support, net, flat, eng
    eng.close()


def _guarded_outputs(shapes):
    """{key: (whole allocation, view)} of canary-filled output tensors; shapes: key -> (shape, dtype)"""
    out = {}
    for k, (shape, dt) in shapes.items():
        out[k] = wd.canaried_like(torch.empty(shape, dtype=dt, device=DEV))
    return out


def _assert_intact(guards, *inputs):
    for k, (big, _) in guards.items():
        assert wd.intact(big), f"write outside {k}"
    for big in inputs:
        assert wd.intact(big), "an input's canaries moved"


# ------------------------------------------------------------------------------------ a. inference
def test_inference_equals_the_oracle_and_float64(width, oracle):
    """37 observations (two 16-row tiles and a ragged third; 5 rows of arbitrary floats) and 37 random latents and
    actions: every output of both calls equals the oracle's bit for bit and stays within the bars of float64"""
    n, support, net, flat, eng = width
    x = wd.rows(n, 100 + n, 32, 5)
    h_in, a_in = wd.recurrent_case(n)
    bx, xd = wd.canaried(x)
    bh, hd = wd.canaried(h_in)
    ba, ad = wd.canaried(a_in)
    ii = _np(eng.initial_inference(xd))
    ri = _np(eng.recurrent_inference(hd, ad))
    torch.cuda.synchronize()
    assert wd.intact(bx) and wd.intact(bh) and wd.intact(ba)
    ei, er = wd.float64_errors(ii, wd.initial64(net, x)), wd.float64_errors(ri, wd.recurrent64(net, h_in, a_in))
    print(f"\nn{n}_s{support} initial   " + " ".join(f"{k} {e:.2e}" for k, e in ei.items() if k != "reward"))
    print(f"n{n}_s{support} recurrent " + " ".join(f"{k} {e:.2e}" for k, e in er.items()))
    oi = oracle.initial_inference(flat, 3 * n, support, x)
    orr = oracle.recurrent_inference(flat, 3 * n, support, h_in, a_in)
    for k in ("h", "pi", "value", "policy_logits", "value_logits"):
        assert _same(ii[k], oi[k]), f"initial {k}: max |d| = {np.abs(ii[k] - oi[k]).max()}"
    for k in ("h", "pi", "value", "reward", "policy_logits", "value_logits", "reward_logits"):
        assert _same(ri[k], orr[k]), f"recurrent {k}: max |d| = {np.abs(ri[k] - orr[k]).max()}"
    for what, errs in (("initial", ei), ("recurrent", er)):
        for k, e in errs.items():
            if not (what == "initial" and k == "reward"):
                assert e <= wd.BARS[k], (what, k, e)


# ------------------------------------------------------------------------------------ b. every search kernel
_SEARCH_REF = {}


def _search_ref(oracle, n, support, flat, B=B_SEARCH):
    """the width's search case and the oracle's result, computed once"""
    key = (n, support, B)
    if key not in _SEARCH_REF:
        obs, noise, tie, u = wd.search_case(n, B)
        ref = oracle.search(n, S, obs, flat=flat, support=support, noise=noise, tie_idx=tie, action_u=u, temperature=1.0)
        _SEARCH_REF[key] = (obs, noise, tie, u, ref)
    return _SEARCH_REF[key]


def _kernel_name(kernel, tile):
    return {"coop": f"mzh_search_kernel<{tile}, ", "occ2": "mzh_search_occ2_kernel<", "one": "mzh_search_one_kernel<",
            "wave": "mzh_wave_kernel<2, ", "wave16": "mzh_wave_kernel<1, "}[kernel]


def _search(eng, case, kernel, tile):
    obs, noise, tie, u, _ = case
    bo, od = wd.canaried(obs)
    o = eng.search(S, obs=od, tie_idx=tt(tie), noise=tt(noise), action_u=tt(u), temperature=1.0, kernel=kernel, tile=tile)
    assert o["_plan"]["kernel"].startswith(_kernel_name(kernel, tile)), o["_plan"]
    got = _np(o)
    assert wd.intact(bo)
    return got


def _assert_search_equals_oracle(got, ref, what):
    for k, rk in SEARCH_KEYS:
        assert np.array_equal(got[k], ref[rk]), f"{what}: {k}"
    assert np.array_equal(got["minmax"], np.stack([ref["mm_max"], ref["mm_min"]], 1)), f"{what}: minmax"


@pytest.mark.parametrize("kernel,tile", FORMS, ids=[k + (str(t) if t else "") for k, t in FORMS])
def test_search_equals_the_oracle(width, oracle, mzh, kernel, tile):
    """40 roots (37 states, 3 rows of arbitrary floats; 16- and 32-root tiles and waves with a ragged last), 20
    simulations, Dirichlet noise, temperature 1, through each forced kernel: every output equals the oracle's"""
    from muzero_hanoi_amd import _lib

    n, support, net, flat, eng = width
    _lib.search_plan(support, B_SEARCH, S, mzh.search_flags(kernel, tile))  # a forced kernel that does not fit raises
    case = _search_ref(oracle, n, support, flat)
    got = _search(eng, case, kernel, tile)
    _assert_search_equals_oracle(got, case[4], f"n{n}_s{support} {kernel} {tile}")
    assert (got["visits"].sum(1) == S).all()


# ------------------------------------------------------------------------------------ c. the expansion memo
@pytest.mark.parametrize("kernel", ["wave", "wave16"])
def test_memo_on_twice_and_off_equal_the_oracle(width, oracle, mzh, kernel):
    """the wave kernels with the memo at the width's depth (automatic at 1, 11 and 16 discs: 6, 0 and 0; forced to
    2 at 2, 5 and 6 discs), searched twice so that the second search meets the grown extension, then with the memo
    off: the same bits three times, and the oracle's"""
    from muzero_hanoi_amd import _lib

    n, support, net, flat, _ = width
    case = _search_ref(oracle, n, support, flat)
    plan = _lib.memo_plan(n)
    assert (plan["depth"] > 0) == (n < 11) and (n != 1 or plan["depth"] == 6), plan
    depth = plan["depth"] if MEMO_DEPTH[n] < 0 else MEMO_DEPTH[n]
    eng = mzh.Engine(n, S, B_SEARCH, support)
    try:
        eng.load_weights(flat)
        eng.set_memo_depth(MEMO_DEPTH[n])
        assert eng.memo_stats()["depth"] == depth
        runs = []
        for leg in range(2):
            before = eng.memo_stats()
            runs.append(_search(eng, case, kernel, None))
            st = eng.memo_stats()
            took = st["pairs_skipped"] + st["pairs_packed"] - before["pairs_skipped"] - before["pairs_packed"]
            print(f"\nn{n}_s{support} {kernel} memo leg {leg}: depth {st['depth']} built {st['built']} rows {st['rows']} "
                  f"grown rows {st['grow_rows']}; pairs skipped + packed {took}")
            assert st["depth"] == depth and st["built"] == (1 if depth else 0)
            if depth:
                assert st["rows"] >= _lib.memo_plan(n, MEMO_DEPTH[n])["rows"] and took > 0
            else:
                assert st["table_bytes"] == 0 and took == 0
        eng.set_memo_depth(0)
        before = eng.memo_stats()
        runs.append(_search(eng, case, kernel, None))
        st = eng.memo_stats()
        assert st["depth"] == 0 and st["pairs_skipped"] + st["pairs_packed"] == before["pairs_skipped"] + before["pairs_packed"]
    finally:
        eng.close()
    for leg, got in enumerate(runs):
        assert set(got) == set(runs[0])
        for k in got:
            assert _same(got[k], runs[0][k]), f"leg {leg}: {k} differs from the first search"
        _assert_search_equals_oracle(got, case[4], f"n{n}_s{support} {kernel} leg {leg}")


# ------------------------------------------------------------------------------------ d. the row-tile kernels
PROBE_OUT = ("reward", "value", "h0", "pi0", "value0", "h1", "pi1")
SAL_OUT = ("policy", "value", "picked", "disc_policy", "disc_value", "h0", "pi0", "value0")


def _probe_shapes(B):
    f = torch.float32
    return dict(reward=((B, 6), f), value=((B, 6), f), h0=((B, 64), f), pi0=((B, 6), f), value0=((B,), f),
                h1=((B, 6, 64), f), pi1=((B, 6, 6), f))


def _sal_shapes(B, n):
    f = torch.float32
    return dict(policy=((B, 3 * n), f), value=((B, 3 * n), f), disc_policy=((B, n), f), disc_value=((B, n), f),
                h0=((B, 64), f), pi0=((B, 6), f), value0=((B,), f), picked=((B,), torch.int32))


def _pgrad_shapes(B, n_rows, n_floats):
    f = torch.float32
    shapes = {k: ((B,) + s, f) for k, s in dict(delta1=(5, 256), delta2=(5, 64), act=(5, 256), h0=(64,), z1=(64,), h1=(64,),
                                                 pi0=(6,), value0=(), reward=(), objective=(5,)).items()}
    if n_floats:
        shapes["grad"] = ((n_rows, n_floats), f)
    return shapes


def _probe(eng, obs, tile, **kw):
    bo, od = wd.canaried(obs)
    guards = _guarded_outputs(_probe_shapes(len(obs)))
    res = eng.probe_actions(od, out={k: v for k, (_, v) in guards.items()}, tile=tile, **kw)
    got = _np(res)
    _assert_intact(guards, bo)
    return got, res


def _saliency(eng, obs, n, tile, **kw):
    bo, od = wd.canaried(obs)
    guards = _guarded_outputs(_sal_shapes(len(obs), n))
    res = eng.saliency(od, out={k: v for k, (_, v) in guards.items()}, tile=tile, **kw)
    got = _np(res)
    _assert_intact(guards, bo)
    return got, res


def _pgrads(eng, obs, action, pl, n_floats, tile, n_rows=None, **kw):
    bo, od = wd.canaried(obs)
    ba, ad = wd.canaried(np.asarray(action, np.int32))
    bp, pd = wd.canaried(np.asarray(pl, np.int32))
    guards = _guarded_outputs(_pgrad_shapes(len(obs), len(obs) if n_rows is None else n_rows, n_floats))
    res = eng.param_grads(od, ad, policy_logit=pd, out={k: v for k, (_, v) in guards.items()}, tile=tile, **kw)
    got = _np(res)
    _assert_intact(guards, bo, ba, bp)
    return got, res


@pytest.mark.parametrize("tile", [16, 32])
def test_probe_equals_composition_and_oracle(width, oracle, tile):
    """37 rows: every output of every row equals the seven-call composition on the engine and on the oracle"""
    n, support, net, flat, eng = width
    obs = wd.rows(n, 100 + n, 32, 5)
    comp = _composition(eng, obs)
    orc = oracle_probe(oracle, flat, n, support, obs)
    got, _ = _probe(eng, obs, tile)
    assert not _same(comp["reward"][:, 0], comp["reward"][:, 1])  # the action matters
    for k in PROBE_OUT:
        assert _same(got[k], comp[k]), f"tile {tile}: {k} vs the composition"
        assert _same(got[k], orc[k]), f"tile {tile}: {k} vs the oracle"


def test_saliency_agrees_with_float64_and_the_inference_call(width):
    """the width's 37 rows: both heads within the rule's bound of float64 with no row excluded, the forward's
    outputs initial_inference's bits, the per-disc sums the fp32 formula, and the rows independent of tile, position
    and env_index"""
    n, support, net, flat, eng = width
    ref = wd.saliency_reference(n, support)
    dense, _ = _saliency(eng, ref.obs, n, 16)
    errs = ref.errors(dense["policy"], dense["value"])
    ref.report(f"n{n}_s{support}", errs)
    assert ref.bad.size == 0 and len(ref.obs) == wd.NROWS
    assert np.array_equal(dense["picked"], ref.r64["picked"])
    for h in ("policy", "value"):
        assert np.isfinite(dense[h]).all() and errs[h] <= ref.bound[h], (h, errs[h], ref.bound[h])
    ii = _np(eng.initial_inference(tt(ref.obs)))
    assert _same(dense["h0"], ii["h"]) and _same(dense["pi0"], ii["pi"]) and _same(dense["value0"], ii["value"])
    assert np.array_equal(dense["picked"], ii["policy_logits"].argmax(axis=1).astype(np.int32))
    for h in ("policy", "value"):
        a = np.abs(dense[h]).reshape(wd.NROWS, n, 3)
        assert _same(dense["disc_" + h], (a[:, :, 0] + a[:, :, 1]) + a[:, :, 2]), h
    t32, _ = _saliency(eng, ref.obs, n, 32)
    for k in SAL_OUT:
        assert _same(t32[k], dense[k]), f"{k} differs between the tiles"
    B = 45
    rs = np.random.RandomState(5)
    full = rs.uniform(-1, 1, (B, 3 * n)).astype(np.float32)
    envs = rs.permutation(B)[:wd.NROWS + 1].astype(np.int32)
    full[envs[:wd.NROWS]] = ref.obs
    full[envs[wd.NROWS]] = ref.obs[3]  # row 3 once more, as the call's last row
    for tile in (16, 32):
        got, _ = _saliency(eng, full, n, tile, env_index=tt(envs))
        for k in SAL_OUT:
            assert _same(got[k][envs[:wd.NROWS]], dense[k]), f"tile {tile}: {k} moved with the row's position"
            assert _same(got[k][envs[wd.NROWS]], dense[k][3]), f"tile {tile}: {k} of the repeated row"
        rest = np.setdiff1d(np.arange(B), envs)
        assert all(np.isnan(got[k][rest]).all() for k in SAL_OUT if k != "picked")  # the canary's NaN is still there


def test_param_grads_agree_with_float64_and_the_inference_calls(width):
    """the width's 37 rows, both policy objectives: every factor, scalar and dense tensor within the rule's bound of
    float64, the forward's outputs the inference calls' bits, the dense gradients the factors' products, and the
    two tiles the same bits"""
    from muzero_hanoi_amd import selfplay
    from test_pgrad_gpu import _check_factors

    n, support, net, flat, eng = width
    ref = wd.pgrad_reference(n, support)
    assert ref.bad.size == 0 and ref.near0_rows.size == 0 and len(ref.obs) == wd.NROWS
    n_floats = pr.dense_slices(3 * n, support)[-1][2]
    assert n_floats == flat.size
    dense, _ = _pgrads(eng, ref.obs, ref.action, ref.policy_logit, n_floats, 16)
    _check_factors(f"n{n}_s{support}", ref, {k: v for k, v in dense.items() if k != "grad"})
    outs = (64, 64, support, 6, support)
    for i in range(5):  # delta2 beyond the net's outputs is +0
        assert not dense["delta2"][:, i, outs[i]:].view(np.uint32).any()
    ii = _np(eng.initial_inference(tt(ref.obs)))
    assert _same(dense["h0"], ii["h"]) and _same(dense["pi0"], ii["pi"]) and _same(dense["value0"], ii["value"])
    ri = _np(eng.recurrent_inference(tt(ii["h"]), tt(ref.action)))
    assert _same(dense["h1"], ri["h"]) and _same(dense["reward"], ri["reward"])
    fac = {k: tt(dense[k]) for k in ("delta1", "delta2", "act", "h0", "z1")}
    want = selfplay.dense_gradients(fac, tt(ref.obs), tt(ref.action), support).cpu().numpy()
    assert dense["grad"].shape == (wd.NROWS, n_floats) and _same(dense["grad"], want)
    worst = max(ref.dense_errors(dense["grad"]).items(), key=lambda kv: kv[1][0] / kv[1][1])
    print(f"n{n}_s{support} dense: largest e / bound at {worst[0]}: e {worst[1][0]:.2e} bound {worst[1][1]:.2e}")
    for key, (e, bound) in ref.dense_errors(dense["grad"]).items():
        assert e <= bound, (key, e, bound)
    t32, _ = _pgrads(eng, ref.obs, ref.action, ref.policy_logit, 0, 32)
    for k in t32:
        assert _same(t32[k], dense[k]), f"{k} differs between the tiles"


@pytest.fixture(scope="module")
def set16(mzh):
    """three seeded 16-disc, 33-bin networks as a set on one engine and alone on one engine each"""
    nets = [wd.net(16, 33, seed) for seed in (0, 1, 2)]
    flats = [wd.flat(net) for net in nets]
    eng = mzh.Engine(16, S, 64, 33)
    eng.load_weight_set(flats)
    singles = []
    for f in flats:
        e1 = mzh.Engine(16, S, 64, 33)
        e1.load_weights(f)
        singles.append(e1)
    yield eng, singles, flats
    for e in [eng] + singles:
        e.close()


@pytest.mark.parametrize("tile", [16, 32])
def test_set_forms_equal_the_single_network_calls_at_48_columns(set16, tile):
    """16 discs, three networks with 17, 16 and 1 rows: probe, saliency and parameter gradients under net_index
    equal the single-network calls bit for bit"""
    eng, singles, flats = set16
    counts, n = (17, 16, 1), 16
    B = sum(counts)
    ref = wd.pgrad_reference(16, 33)  # its rows, under these networks
    obs, act, pl = ref.obs[:B], ref.action[:B], ref.policy_logit[:B]
    ni = tt(np.repeat(np.arange(3), counts).astype(np.int32))
    tiles = sum(-(-c // tile) for c in counts)
    probe, res = _probe(eng, obs, tile, net_index=ni)
    assert res["_status"].tolist() == [0, tiles]
    sal, res = _saliency(eng, obs, n, tile, net_index=ni)
    assert res["_status"].tolist() == [0, tiles]
    pg, res = _pgrads(eng, obs, act, pl, flats[0].size, tile, net_index=ni)
    assert res["_status"].tolist() == [0, tiles]
    lo = 0
    for m, c in enumerate(counts):
        sl = slice(lo, lo + c)
        one, _ = _probe(singles[m], obs[sl], tile)
        for k in PROBE_OUT:
            assert _same(probe[k][sl], one[k]), f"probe, network {m}: {k}"
        one, _ = _saliency(singles[m], obs[sl], n, tile)
        for k in SAL_OUT:
            assert _same(sal[k][sl], one[k]), f"saliency, network {m}: {k}"
        one, _ = _pgrads(singles[m], obs[sl], act[sl], pl[sl], flats[0].size, tile)
        for k in one:
            assert _same(pg[k][sl], one[k]), f"param_grads, network {m}: {k}"
        if m:  # a kernel that ignored net_index would not pass
            other, _ = _probe(singles[0], obs[sl], tile)
            assert not _same(probe["h0"][sl], other["h0"])
        lo += c


@pytest.mark.parametrize("n", [11, 16])
def test_search_multi_equals_the_single_network_searches(mzh, n):
    """three seeded networks with 1, 17 and 16 roots at three k-blocks: search_multi on both tiles equals
    Engine.search on an engine holding the root's network, every output bit for bit"""
    counts = (1, 17, 16)
    B = sum(counts)
    flats = [wd.flat(wd.net(n, 33, seed)) for seed in (0, 1, 2)]
    obs, noise, tie, u = wd.search_case(n, B)
    ni = np.repeat(np.arange(3), counts).astype(np.int32)
    eng = mzh.Engine(n, S, B, 33)
    eng.load_weight_set(flats)
    want, lo = [], 0
    for m, c in enumerate(counts):
        sl = slice(lo, lo + c)
        e1 = mzh.Engine(n, S, B, 33)
        e1.load_weights(flats[m])
        bo, od = wd.canaried(obs[sl])
        want.append(_np(e1.search(S, obs=od, tie_idx=tt(tie[sl]), noise=tt(noise[sl]), action_u=tt(u[sl]), temperature=1.0)))
        assert wd.intact(bo)
        if m == 0:  # a kernel that ignored net_index (network 0 for every root) would not pass
            under0 = _np(e1.search(S, obs=tt(obs), tie_idx=tt(tie), noise=tt(noise), action_u=tt(u), temperature=1.0))
        else:
            assert not np.array_equal(under0["visits"][sl], want[m]["visits"]), "choose other seeds"
        e1.close()
        lo += c
    for tile in (16, 32):
        bo, od = wd.canaried(obs)
        o = eng.search_multi(S, net_index=tt(ni), obs=od, tie_idx=tt(tie), noise=tt(noise), action_u=tt(u),
                             temperature=1.0, tile=tile)
        assert o["_plan"]["kernel"].startswith(f"mzh_search_multi_kernel<{tile}, ")
        assert o["_status"].tolist() == [0, sum(-(-c // tile) for c in counts)]
        got = _np(o)
        assert wd.intact(bo)
        lo = 0
        for m, c in enumerate(counts):
            for k in want[m]:
                assert _same(got[k][lo:lo + c], want[m][k]), f"tile {tile} network {m}: {k}"
            lo += c
    eng.close()


# ------------------------------------------------------------------------------------ f. episodes
def test_episodes_at_one_disc():
    """N = 1: the goal is one move away.  8 simulations, at most 4 moves, starts 0, 1, 0"""
    from test_episode_gpu import check_case

    got, _, _, _ = check_case(1, 33, 8, 4, [0, 1, 0], seed=11)
    steps, solved, illegal = (got[k].cpu().numpy() for k in ("steps", "solved", "illegal"))
    print(f"\nsteps {steps.tolist()} solved {solved.tolist()} illegal {illegal.tolist()}")
    assert (solved == 1).any(), "no env reached the goal: choose another seed"
    assert (illegal > 0).any(), "no env played an illegal move: choose another seed"


def test_episodes_at_sixteen_discs():
    """N = 16: the observation built from the start state fills all 48 columns"""
    from test_episode_gpu import check_case

    got, want, _, _ = check_case(16, 33, 8, 6, [0, 3 ** 16 - 2, 21523360, 7], seed=12)
    steps = got["steps"].cpu().numpy()
    print(f"\nsteps {steps.tolist()} solved {got['solved'].cpu().numpy().tolist()}")
    assert (steps >= 1).all() and (steps <= 6).all()
    obs = got["obs"][0].cpu().numpy()  # the first move's observations: one peg per disc over all 48 columns
    assert obs.shape == (4, 48) and (obs.reshape(4, 16, 3).sum(2) == 1).all() and obs[:, 45:].any()


def test_episode_set_at_sixteen_discs():
    from test_episode_set_gpu import check_set

    check_set(16, 33, 8, 5, [0, 3 ** 16 - 2, 21523360, 7, 14348907], [0, 0, 1, 2, 2], 3, seed=13)
