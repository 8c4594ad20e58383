"""Parameter gradients of the five sub-networks (gradient_analysis.py get_results), the checks that need no GPU:
the boundary of mzh_param_grads (export, struct layout; its argument errors: tests/rows_refusals.py),
the gather map of the extra transposed buffer against a direct transposed pack (tests/pgrad_map_check.cpp under
the host sanitizers, as its own program), the conditioning of every case, the reference's recorded gradients
(tests/golden/pgrad_n3.npz, tests/golden/gen_pgrad_golden.py) against this repository's float64 torch path, and
the rank-one expansion of the reference module against autograd on the parameters themselves.
"""
import copy
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import pgrad_ref as pr
import rows_refusals as rr
from conftest import ROOT, golden

HEADER = os.path.join(ROOT, "include", "mzh.h")
FIELDS = ["B", "n", "flags", "env_index", "obs", "action", "policy_logit", "delta1", "delta2", "act", "h0", "z1", "h1",
          "pi0", "value0", "reward", "objective", "grad", "err_count"]


@pytest.fixture(scope="module")
def lib():
    from muzero_hanoi_amd import build

    build.build()
    from muzero_hanoi_amd import _lib

    return _lib


# ------------------------------------------------------------------------------------ the C boundary
def test_symbol_declared_exported_and_abi_version_unchanged(lib):
    L = lib.lib()
    assert hasattr(L, "mzh_param_grads") and "mzh_param_grads" in lib.SIGNATURES
    hdr = open(HEADER).read()
    assert "int mzh_param_grads(mzh_engine* eng, const mzh_pgrad_args* args, const mzh_multi_args* multi" in hdr
    assert "#define MZH_ABI_VERSION 6" in hdr and L.mzh_abi_version() == lib.ABI_VERSION == 6
    assert "gradient_analysis.py get_results, lines\n * 274-338" in hdr  # the entry cites what it replaces


def test_pgrad_args_layout_matches_header(lib, tmp_path):
    """ctypes PgradArgs == struct mzh_pgrad_args as the C compiler lays out include/mzh.h"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "the build needs a C compiler too"
    fields = [f[0] for f in lib.PgradArgs._fields_]
    src = tmp_path / "pgrad_args.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mzh.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof(mzh_pgrad_args, {f}));\n' for f in fields)
                   + 'printf("%zu\\n", sizeof(mzh_pgrad_args)); return 0; }\n')
    exe = tmp_path / "pgrad_args"
    subprocess.run([cc, "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [getattr(lib.PgradArgs, f).offset for f in fields] + [ctypes.sizeof(lib.PgradArgs)]
    assert fields == FIELDS


# the argument errors: the cases and checks shared by the three row calls (tests/rows_refusals.py)
@pytest.mark.parametrize("field,value,msg", rr.argument_errors("mzh_param_grads"))
def test_argument_errors_without_device_or_engine(lib, field, value, msg):
    rr.check_argument_error(lib, "mzh_param_grads", field, value, msg)


def test_rows_beyond_the_batch_null_args_optional_outputs_and_the_tile_flags(lib):
    rr.check_rows_beyond_the_batch_null_args_optional_outputs_and_the_tile_flags(lib, "mzh_param_grads")


@pytest.mark.parametrize("field,value,msg", rr.MULTI_ERRORS)
def test_multi_argument_errors_without_device_or_engine(lib, field, value, msg):
    rr.check_multi_argument_error(lib, "mzh_param_grads", field, value, msg)


# ------------------------------------------------------------------------------------ the extra buffer's gather map
@pytest.fixture(scope="module")
def map_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "the build needs a C++ compiler too"
    exe = tmp_path_factory.mktemp("pgrad_map_check") / "pgrad_map_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "pgrad_map_check.cpp"),
                    os.path.join(ROOT, "muzero-hanoi_amd", "csrc", "mzh_pack.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("n_disks", [3, 4, 7])
@pytest.mark.parametrize("support", [33, 1])
def test_gather_map_reproduces_the_direct_transposed_pack(map_check, n_disks, support):
    """the main blob gathered through mzh_pgrad_map equals mzh_pack_pgrad float for float, and that pack holds
    dynamic_net.2 and rwd_net.2 where MzhPackedT's formula puts them"""
    r = subprocess.run([map_check, str(n_disks), str(support)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith(f"ok n_disks={n_disks} support={support}")


# ------------------------------------------------------------------------------------ conditioning, fixture, expansion
def _references():
    return [(name, pr.weights_reference(name)) for name, _, _ in pr.WEIGHTS] + \
        [(f"fixture network {m}", r) for m, r in enumerate(pr.fixture_reference())]


def test_conditioning_report():
    """the conditions the bound rests on: no row of any case is ill-conditioned; no row of a weight case holds a
    hidden unit within NEAR0 of the ReLU's kink, the atlas at most NEAR0_ROWS_CAP rows per network; each weight case
    draws both kinds of policy objective; the floors are the measured fp32 errors"""
    worst = worst_obj = 0.0
    for name, ref in _references():
        ref.report(name)
        assert ref.bad.size == 0, (name, ref.bad)
        worst = max(worst, max(v for (k, _), v in ref.base.items() if k != "objective"))
        worst_obj = max(worst_obj, max(v for (k, _), v in ref.base.items() if k == "objective"))
        if name.startswith("weights"):
            assert len(ref.obs) == pr.NROWS and ref.near0_rows.size == 0
            assert 0 < ref.forced.sum() < pr.NROWS and set(ref.action.tolist()) == set(range(6))
            assert (ref.obs[:32].sum(axis=1) == ref.obs.shape[1] // 3).all() and not np.isin(ref.obs[32:], (0.0, 1.0)).all()
            print(f"  {name}: {ref.rejected} candidates rejected before the 37 rows were found")
        else:
            assert len(ref.obs) == 162 and ref.near0_rows.size <= pr.NEAR0_ROWS_CAP
            assert np.abs(ref.r64["pre"]).min() > 1e-6 and min(ref.gaps["z0"].min(), ref.gaps["z1"].min()) >= 2.7e-4 - 1e-6
    print(f"\nlargest fp32-torch e: factors {worst:.3e} (FLOOR {pr.FLOOR:.3e}), objective {worst_obj:.3e} "
          f"(FLOOR_OBJECTIVE {pr.FLOOR_OBJECTIVE:.3e})")
    # the floors are what was measured (the baseline moves a little with the host's torch build)
    assert 0.5 * pr.FLOOR <= worst <= 2 * pr.FLOOR and 0.5 * pr.FLOOR_OBJECTIVE <= worst_obj <= 2 * pr.FLOOR_OBJECTIVE


def test_fixture_agrees_with_the_float64_path():
    """the reference's own get_results (fp32 torch autograd on the parameters) against this repository's float64
    path: its bias gradients are the deltas of all 27 states (action s % 6) x 3 networks within the fp32 floor, the
    policy net's within the absolute bounds; the 20 tensors of the default pair are the rank-one expansion"""
    g = golden("pgrad_n3.npz")
    assert (int(g["n"]), g["delta1"].shape, g["delta2"].shape) == (3, (3, 27, 5, 256), (3, 27, 5, 64))
    assert g["delta1"].dtype == g["delta2"].dtype == np.float32
    assert np.array_equal(g["states"], pr.all_states(3)) and np.array_equal(g["actions"], np.arange(27) % 6)
    rows = np.arange(27) * 6 + np.arange(27) % 6  # the atlas rows of (s, s % 6)
    for m, ref in enumerate(pr.fixture_reference()):
        for kind in ("delta1", "delta2"):
            for i in range(5):
                x64 = ref.r64[kind][rows, i].astype(np.float64)
                x = g[kind][m, :, i].astype(np.float64)
                if i == 3:  # true value 0
                    scale = pr.ABS_POLICY * (1.0 if kind == "delta2" else ref.w2abs[3][None, :])
                    assert (np.abs(x) <= scale).all(), (m, kind)
                    continue
                d = np.abs(x - x64)
                if kind == "delta1":  # a unit at the kink may take either mask
                    near = ref.near0[rows, i]
                    d = np.where(near, np.minimum(d, np.minimum(np.abs(x), np.abs(x - ref.r64["d1_open"][rows, i]))), d)
                e = d.max() / np.abs(ref.r64[kind][:, i]).max()
                print(f"fixture network {m} {kind} {pr.NETS[i]}: e {e:.2e}")
                assert e <= pr.FLOOR, (m, kind, i, e)
    # an ablated head changes its own gradients and leaves the other nets' as they were
    assert not np.array_equal(g["delta1"][0, :, 4], g["delta1"][2, :, 4]) and np.array_equal(g["delta1"][0, :, :3], g["delta1"][2, :, :3])
    assert np.array_equal(g["delta1"][0, :, 4], g["delta1"][1, :, 4])
    # the default pair's 20 tensors
    ref = pr.fixture_reference()[0]
    want = ref.dense64()[0]
    keys = pr.dense_slices(9, 33)
    assert len(keys) == 20 and keys[-1][2] == want.shape[0]
    for key, lo, hi in keys:
        t = g["grad." + key]
        assert t.dtype == np.float32 and t.size == hi - lo
        if key.startswith("policy_net"):
            assert np.abs(t).max() <= pr.ABS_POLICY * max(1.0, ref.w2abs[3].max(), ref.r64["act"][0, 3].max())
            continue
        e = pr.rel(t.reshape(-1), want[lo:hi])
        print(f"default pair {key}: e {e:.2e}")
        assert e <= pr.FLOOR, (key, e)
    assert np.array_equal(g["grad.value_net.0.bias"], g["delta1"][0, 0, 4])


def test_rank_one_expansion_is_autograd_on_the_parameters():
    """dense_from_factors of the float64 factors equals autograd.grad of each objective with respect to the net's
    own parameters, row by row (what get_results returns), to float64 rounding; both policy objectives"""
    name, n, sup = pr.WEIGHTS[0]
    ref = pr.weights_reference(name)
    net = copy.deepcopy(pr.npz_net(name)).to(torch.float64)
    dense = ref.dense64()
    slices = pr.dense_slices(3 * n, sup)
    for r in (0, 5, 33, 36):
        x = torch.as_tensor(ref.obs[r:r + 1], dtype=torch.float64)
        a = torch.zeros(1, 6, dtype=torch.float64)
        a[0, int(ref.action[r])] = 1.0
        h0 = net.represent(x)
        lp, v = net.prediction(h0)
        h1, rwd = net.dynamics(h0, a)
        k = int(ref.policy_logit[r])
        objs = (h0.mean(), h1.mean(), rwd.mean(), torch.softmax(lp, dim=-1).mean() if k < 0 else lp[0, k], v.mean())
        for i, obj in enumerate(objs):
            grads = torch.autograd.grad(obj, list(getattr(net, pr.MODULES[i]).parameters()), retain_graph=True)
            for (key, lo, hi), gt in zip(slices[4 * i: 4 * i + 4], grads):
                want = gt.numpy().reshape(-1)
                tol = 1e-12 * max(1.0, np.abs(want).max()) if not (i == 3 and k < 0) else 1e-15
                assert np.abs(dense[r, lo:hi] - want).max() <= tol, (r, key)


def test_dense_gradients_is_the_reference_modules_expansion():
    """selfplay.dense_gradients (torch) and pgrad_ref.dense_from_factors (numpy) are the same fp32 products"""
    from muzero_hanoi_amd import selfplay

    ref = pr.weights_reference("weights_N3_s0")
    g = ref.r32
    want = pr.dense_from_factors(g["delta1"], g["delta2"], g["act"], g["ins"], 33)
    got = selfplay.dense_gradients(dict(delta1=g["delta1"], delta2=g["delta2"], act=g["act"], h0=g["h0"], z1=g["z1"]),
                                   ref.obs, ref.action, 33).numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
