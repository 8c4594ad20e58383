"""Legal-versus-illegal predictions (legal_illegal_preds.py evaluate_network), the checks that need no GPU: the
boundary of mzh_probe_actions (export, struct layout; its argument errors: tests/rows_refusals.py),
acting.legality_summary against the reference's returned numbers, the oracle composition
(oracle.initial_inference + six oracle.recurrent_inference + oracle.legal_mask) against every recorded probe, and
the reference's run replayed on the oracle search and env (tests/golden/legality_n3.npz,
tests/golden/gen_legality_golden.py).
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import rows_refusals as rr
from conftest import GOLDEN, ROOT, golden
from muzero_hanoi_amd import rng as mrng

HEADER = os.path.join(ROOT, "include", "mzh.h")
KEYS = ("reward_diff_mean", "reward_diff_std", "value_diff_mean", "value_diff_std")


@pytest.fixture(scope="module")
def lib():
    from muzero_hanoi_amd import build

    build.build()
    from muzero_hanoi_amd import _lib

    return _lib


def fixture_flats(oracle, g):
    """the fixture's two networks as canonical flat vectors: the checkpoint, and the checkpoint with the recorded
    re-initialised policy_net tensors (legal_illegal_preds.ablate_network(net, ablate_policy=True))"""
    ck = torch.load(os.path.join(GOLDEN, "muzero_model_N3.pt"), map_location="cpu", weights_only=True)["Muzero_net"]
    base = {k: ck[k].numpy().astype(np.float32) for k in oracle.WEIGHT_KEYS}
    abl = {k: (g["ablated." + k] if "ablated." + k in g.files else v) for k, v in base.items()}
    assert sum("ablated." + k in g.files for k in base) == 4
    return [oracle.flat_weights(base), oracle.flat_weights(abl)]


def network_rows(g):
    """per network: (its decisions' slice of the per-decision arrays, its episodes' slice of the per-episode ones)"""
    E = int(g["episodes"])
    d = np.concatenate([[0], np.cumsum(g["net_decisions"])])
    return [(slice(int(d[m]), int(d[m + 1])), slice(m * E, (m + 1) * E)) for m in range(len(g["net_decisions"]))]


def probe_record(g, dec, eps):
    """a network's recorded probes as legality_summary's arrays: [T][E][6], [T][E], steps [E]"""
    steps = g["ep_steps"][eps]
    T, E = int(steps.max()), len(steps)
    reward, value = np.zeros((T, E, 6), np.float32), np.zeros((T, E, 6), np.float32)
    legal = np.zeros((T, E), np.uint8)
    p = dec.start
    for b, k in enumerate(steps):
        reward[:k, b], value[:k, b], legal[:k, b] = (g[f"probe_{x}"][p:p + k] for x in ("reward", "value", "legal"))
        p += int(k)
    assert p == dec.stop
    return reward, value, legal, steps


# ------------------------------------------------------------------------------------ the C boundary
def test_symbol_declared_exported_and_abi_version_unchanged(lib):
    L = lib.lib()
    assert hasattr(L, "mzh_probe_actions") and "mzh_probe_actions" in lib.SIGNATURES
    hdr = open(HEADER).read()
    assert "int mzh_probe_actions(mzh_engine* eng, const mzh_probe_args* args, const mzh_multi_args* multi" in hdr
    assert "#define MZH_ABI_VERSION 6" in hdr and L.mzh_abi_version() == lib.ABI_VERSION == 6
    assert "legal_illegal_preds.py" in hdr  # the entry cites the reference script it replaces


def test_probe_args_layout_matches_header(lib, tmp_path):
    """ctypes ProbeArgs == struct mzh_probe_args as the C compiler lays out include/mzh.h"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [f[0] for f in lib.ProbeArgs._fields_]
    src = tmp_path / "probe_args.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mzh.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof(mzh_probe_args, {f}));\n' for f in fields)
                   + 'printf("%zu\\n", sizeof(mzh_probe_args)); return 0; }\n')
    exe = tmp_path / "probe_args"
    subprocess.run([cc, "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [getattr(lib.ProbeArgs, f).offset for f in fields] + [ctypes.sizeof(lib.ProbeArgs)]
    assert fields == ["B", "n", "flags", "env_index", "obs", "state", "reward", "value", "legal", "h0", "pi0", "value0",
                      "h1", "pi1", "err_count"]


# the argument errors: the cases and checks shared by the three row calls (tests/rows_refusals.py)
@pytest.mark.parametrize("field,value,msg", rr.argument_errors("mzh_probe_actions"))
def test_argument_errors_without_device_or_engine(lib, field, value, msg):
    rr.check_argument_error(lib, "mzh_probe_actions", field, value, msg)


def test_rows_beyond_the_batch_null_args_and_the_tile_flags(lib):
    rr.check_rows_beyond_the_batch_null_args_optional_outputs_and_the_tile_flags(lib, "mzh_probe_actions")


@pytest.mark.parametrize("field,value,msg", rr.MULTI_ERRORS)
def test_multi_argument_errors_without_device_or_engine(lib, field, value, msg):
    rr.check_multi_argument_error(lib, "mzh_probe_actions", field, value, msg)


# ------------------------------------------------------------------------------------ the fixture
def test_fixture_records_are_consistent():
    g = golden("legality_n3.npz")
    n, E, D = int(g["n"]), int(g["episodes"]), len(g["actions"])
    assert (n, int(g["n_sims"]), int(g["max_steps"]), E) == (3, 25, 12, 4) and g["dicts"].shape == (2, 4)
    assert int(g["net_decisions"].sum()) == int(g["ep_steps"].sum()) == D == len(g["run_S"]) == len(g["env_done"])
    assert g["ep_start"].shape == (2 * E, n) and g["probe_reward"].shape == g["probe_value"].shape == (D, 6)
    assert g["probe_reward"].dtype == g["probe_value"].dtype == g["run_obs"].dtype == np.float32
    assert set(g["run_S"].tolist()) == {25} and len(g["post_rng"]) == 3
    assert len(set(g["ep_steps"].tolist())) > 1  # episodes of different lengths
    ends = np.cumsum(g["ep_steps"]) - 1
    assert g["env_done"][ends].all() and g["env_done"].sum() == 2 * E
    for (dec, eps), nd in zip(network_rows(g), g["net_decisions"]):
        assert int(g["ep_steps"][eps].sum()) == int(nd) == dec.stop - dec.start
    # the observation of an episode's first decision is its start's one-hot; both legality classes occur
    for s, p in zip(g["ep_start"], ends - g["ep_steps"] + 1):
        onehot = np.zeros(3 * n, np.float32)
        onehot[np.arange(n) * 3 + s] = 1
        assert np.array_equal(g["run_obs"][p], onehot)
    assert ((g["probe_legal"] > 0) & (g["probe_legal"] < 63)).all()


# ------------------------------------------------------------------------------------ the statistics
def test_legality_summary_reproduces_the_reference_bit_for_bit():
    """from the fixture's own recorded probe values, legality and step counts: the reference's four numbers"""
    from muzero_hanoi_amd.acting import legality_summary

    g = golden("legality_n3.npz")
    for m, (dec, eps) in enumerate(network_rows(g)):
        d = legality_summary(*probe_record(g, dec, eps))
        assert list(d) == list(KEYS)
        for k, want in zip(KEYS, g["dicts"][m]):
            assert isinstance(d[k], float) and d[k] == float(want), (m, k, d[k], float(want))


def test_legality_summary_guards_and_padding():
    """the reference's `else 0.0` guards, and rows beyond an episode's steps are not read"""
    from muzero_hanoi_amd.acting import legality_summary

    assert legality_summary(np.zeros((0, 0, 6)), np.zeros((0, 0, 6)), np.zeros((0, 0)), []) == dict.fromkeys(KEYS, 0.0)
    r = np.arange(24, dtype=np.float32).reshape(2, 2, 6)
    v = -r
    legal = np.array([[63, 0], [5, 9]], np.uint8)  # episode 0, decision 0: no illegal move; episode 1: no legal one
    a = legality_summary(r, v, legal, [1, 1])
    assert a["reward_diff_mean"] == float(np.mean([np.mean(r[0, 0]) - 0.0, 0.0 - np.mean(r[0, 1])]))
    r2, v2, l2 = r.copy(), v.copy(), legal.copy()
    r2[1], v2[1], l2[1] = 1e9, 1e9, 63
    assert legality_summary(r2, v2, l2, [1, 1]) == a
    b = legality_summary(r, v, legal, [2, 1])  # decision 1 of episode 0: moves 0 and 2 legal
    lg = np.concatenate([r[0, 0], r[1, 0, [0, 2]]]).astype(np.float64)
    il = r[1, 0, [1, 3, 4, 5]].astype(np.float64)
    assert b["reward_diff_mean"] == float(np.mean([np.mean(lg) - np.mean(il), 0.0 - np.mean(r[0, 1])]))
    one = legality_summary(r[:, :1], v[:, :1], legal[:, :1], [2])
    assert np.isnan(one["reward_diff_std"])  # one episode: np.std(ddof=1) of one value, as the reference gives


# ------------------------------------------------------------------------------------ the oracle composition
def oracle_probe(oracle, flat, n, support, obs, states=None):
    """the probe composed on the oracle: represent / initial_inference, then recurrent_inference(h, a), a = 0..5"""
    obs = np.ascontiguousarray(obs, np.float32)
    B = obs.shape[0]
    ii = oracle.initial_inference(flat, 3 * n, support, obs)
    out = dict(h0=ii["h"], pi0=ii["pi"], value0=ii["value"], reward=np.zeros((B, 6), np.float32),
               value=np.zeros((B, 6), np.float32), h1=np.zeros((B, 6, 64), np.float32),
               pi1=np.zeros((B, 6, 6), np.float32))
    for a in range(6):
        ri = oracle.recurrent_inference(flat, 3 * n, support, ii["h"], np.full(B, a, np.int32))
        out["reward"][:, a], out["value"][:, a], out["h1"][:, a], out["pi1"][:, a] = (ri[k] for k in
                                                                                     ("reward", "value", "h", "pi"))
    if states is not None:
        out["legal"] = np.array([oracle.legal_mask(s) for s in states], np.uint8)
    return out


def test_oracle_composition_agrees_with_every_recorded_probe(oracle):
    """every recorded element, none skipped, within 2e-3 of the reference's torch values (DESIGN.md section 4
    item 8: transformed scalars against torch); the legal mask exactly"""
    g = golden("legality_n3.npz")
    n = int(g["n"])
    states = g["run_obs"].reshape(-1, n, 3).argmax(2).astype(np.uint8)
    assert np.array_equal(np.eye(3, dtype=np.float32)[states].reshape(-1, 3 * n), g["run_obs"])
    worst = 0.0
    for (dec, _), flat in zip(network_rows(g), fixture_flats(oracle, g)):
        o = oracle_probe(oracle, flat, n, 33, g["run_obs"][dec], states[dec])
        assert np.array_equal(o["legal"], g["probe_legal"][dec])
        for k in ("reward", "value"):
            err = np.abs(o[k].astype(np.float64) - g[f"probe_{k}"][dec].astype(np.float64))
            assert err.shape == (dec.stop - dec.start, 6) and np.isfinite(err).all()
            worst = max(worst, float(err.max()))
            bad = np.argwhere(err > 2e-3)
            assert bad.size == 0, [(k, tuple(i), float(err[tuple(i)])) for i in bad]
    print(f"largest |oracle - torch| over every recorded probe element: {worst:.3e}")


# ------------------------------------------------------------------------------------ the run on the oracle
def test_reference_run_replayed_on_the_oracle(oracle):
    """the drop-in's loop (acting.legality_evaluate_network) with every device call replaced by its oracle
    counterpart and the network by the recording: random_reset's draws, the search's draws, the recorded search
    outputs through the oracle search, the recorded probes, the oracle env -- the reference's starts, actions,
    MinMaxStats chain, step counts, dicts and the stream position after the run, exactly"""
    from muzero_hanoi_amd.acting import legality_summary
    from muzero_hanoi_amd.selfplay import index_state

    g = golden("legality_n3.npz")
    n, S, max_steps, E = int(g["n"]), int(g["n_sims"]), int(g["max_steps"]), int(g["episodes"])
    np.random.seed(int(g["seed"]))
    mm = np.array([[-np.inf, np.inf]])
    k, off, ep = 0, 0, 0
    for m in range(2):
        rec_r, rec_v, rec_l, steps = [], [], [], []
        for _ in range(E):
            while True:  # env/hanoi.py:103-109 on the global stream
                idx = np.random.randint(3 ** n)
                if idx != 3 ** n - 1:
                    break
            st = np.array(index_state(idx, n), np.uint8)
            assert np.array_equal(st, g["ep_start"][ep])
            ctr, active, done, t0 = 0, 1, 0, k
            while not done:
                obs = np.zeros(3 * n)
                obs[np.arange(n) * 3 + st] = 1
                assert np.array_equal(obs.astype(np.float32), g["run_obs"][k])
                noise, tie, u = mrng.predraw(1, deterministic=False, alpha=0.25)
                rp = dict(root_pi=g["run_root_pi"][k][None], pi=g["run_pi"][off:off + S][None],
                          rwd=g["run_reward"][off:off + S][None], value=g["run_value"][off:off + S][None])
                o = oracle.search(n, S, obs[None], replay=rp, noise=noise, tie_idx=tie, action_u=u, temperature=0.0,
                                  minmax_in=mm)
                mm = np.stack([o["mm_max"], o["mm_min"]], 1)
                a = int(o["action"][0])
                assert a == int(g["actions"][k]) and np.array_equal(mm[0], g["mm"][k])
                assert oracle.legal_mask(st) == int(g["probe_legal"][k])
                _, st, _, ctr, active, done, _ = oracle.env_step(st, a, ctr, active, max_steps)
                k, off = k + 1, off + S
            assert k - t0 == int(g["ep_steps"][ep])
            rec_r.append(g["probe_reward"][t0:k])
            rec_v.append(g["probe_value"][t0:k])
            rec_l.append(g["probe_legal"][t0:k])
            steps.append(k - t0)
            ep += 1
        T = max(steps)
        reward, value = np.zeros((T, E, 6), np.float32), np.zeros((T, E, 6), np.float32)
        legal = np.zeros((T, E), np.uint8)
        for b in range(E):
            reward[:steps[b], b], value[:steps[b], b], legal[:steps[b], b] = rec_r[b], rec_v[b], rec_l[b]
        d = legality_summary(reward, value, legal, steps)
        assert [d[key] for key in KEYS] == g["dicts"][m].tolist()
    assert k == len(g["actions"])
    assert np.array_equal(np.random.random_sample(3), g["post_rng"]), "RNG stream position differs"
