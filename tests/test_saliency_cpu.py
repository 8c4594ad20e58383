"""Input saliency (gradient_analysis.py compute_saliency), the checks that need no GPU: the boundary of
mzh_saliency (export, struct layout; its argument errors: tests/rows_refusals.py), the transposed
weight blob element by element (tests/saliency_pack_check.cpp under the host sanitizers, as its own program),
the reference's recorded vectors (tests/golden/saliency_n3.npz, tests/golden/gen_saliency_golden.py) against
this repository's float64 torch path, the conditioning of every case's inputs, and that the bound the GPU tests
apply tells a wrong backward from a right one.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import rows_refusals as rr
import saliency_ref as sr
from conftest import ROOT, golden

HEADER = os.path.join(ROOT, "include", "mzh.h")
FIELDS = ["B", "n", "flags", "env_index", "obs", "logit_index", "sal_policy", "sal_value", "picked", "disc_policy",
          "disc_value", "h0", "pi0", "value0", "err_count"]


@pytest.fixture(scope="module")
def lib():
    from muzero_hanoi_amd import build

    build.build()
    from muzero_hanoi_amd import _lib

    return _lib


# ------------------------------------------------------------------------------------ the C boundary
def test_symbol_declared_exported_and_abi_version_unchanged(lib):
    L = lib.lib()
    assert hasattr(L, "mzh_saliency") and "mzh_saliency" in lib.SIGNATURES
    hdr = open(HEADER).read()
    assert "int mzh_saliency(mzh_engine* eng, const mzh_saliency_args* args, const mzh_multi_args* multi" in hdr
    assert "#define MZH_ABI_VERSION 6" in hdr and L.mzh_abi_version() == lib.ABI_VERSION == 6
    assert "gradient_analysis.py" in hdr  # the entry cites the reference script it replaces


def test_saliency_args_layout_matches_header(lib, tmp_path):
    """ctypes SaliencyArgs == struct mzh_saliency_args as the C compiler lays out include/mzh.h"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [f[0] for f in lib.SaliencyArgs._fields_]
    src = tmp_path / "saliency_args.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mzh.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof(mzh_saliency_args, {f}));\n' for f in fields)
                   + 'printf("%zu\\n", sizeof(mzh_saliency_args)); return 0; }\n')
    exe = tmp_path / "saliency_args"
    subprocess.run([cc, "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [getattr(lib.SaliencyArgs, f).offset for f in fields] + [ctypes.sizeof(lib.SaliencyArgs)]
    assert fields == FIELDS


# the argument errors: the cases and checks shared by the three row calls (tests/rows_refusals.py)
@pytest.mark.parametrize("field,value,msg", rr.argument_errors("mzh_saliency"))
def test_argument_errors_without_device_or_engine(lib, field, value, msg):
    rr.check_argument_error(lib, "mzh_saliency", field, value, msg)


def test_rows_beyond_the_batch_null_args_optional_outputs_and_the_tile_flags(lib):
    rr.check_rows_beyond_the_batch_null_args_optional_outputs_and_the_tile_flags(lib, "mzh_saliency")


@pytest.mark.parametrize("field,value,msg", rr.MULTI_ERRORS)
def test_multi_argument_errors_without_device_or_engine(lib, field, value, msg):
    rr.check_multi_argument_error(lib, "mzh_saliency", field, value, msg)


# ------------------------------------------------------------------------------------ the transposed blob
@pytest.fixture(scope="module")
def pack_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("saliency_pack_check") / "saliency_pack_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "saliency_pack_check.cpp"),
                    os.path.join(ROOT, "muzero-hanoi_amd", "csrc", "mzh_pack.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("n_disks", [3, 4, 7])
@pytest.mark.parametrize("support", [33, 1])
def test_transposed_blob_element_by_element(pack_check, n_disks, support):
    """every weight of the six layers at the position MzhPackedT's comment gives it, zero padding elsewhere"""
    r = subprocess.run([pack_check, str(n_disks), str(support)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith(f"ok n_disks={n_disks} support={support}")


# ------------------------------------------------------------------------------------ the fixture and the bound
def test_fixture_agrees_with_the_float64_path():
    """the reference's own compute_saliency (fp32 torch) on all 27 states x 3 networks against this repository's
    torch path in float64: within the fp32 floor, the same logit picked"""
    g = golden("saliency_n3.npz")
    assert (int(g["n"]), g["policy"].shape, g["value"].shape, g["picked"].shape) == (3, (3, 27, 9), (3, 27, 9), (3, 27))
    assert g["policy"].dtype == g["value"].dtype == np.float32
    assert np.array_equal(g["states"], sr.all_states(3))
    assert sum(k.startswith("policy_ablated.") for k in g.files) == sum(k.startswith("value_ablated.") for k in g.files) == 4
    for m, ref in enumerate(sr.fixture_reference()):
        errs = ref.errors(g["policy"][m], g["value"][m])
        ref.report(f"fixture network {m}", errs)
        assert np.array_equal(g["picked"][m], ref.r64["picked"])
        assert errs["policy"] <= sr.FLOOR and errs["value"] <= sr.FLOOR, errs
    # an ablated head changes its own saliency and leaves the other head's as it was
    assert not np.array_equal(g["policy"][0], g["policy"][1]) and np.array_equal(g["policy"][0], g["policy"][2])
    assert not np.array_equal(g["value"][0], g["value"][2]) and np.array_equal(g["value"][0], g["value"][1])


def _references():
    return [(name, sr.weights_reference(name)) for name, _, _ in sr.WEIGHTS] + \
        [(f"fixture network {m}", r) for m, r in enumerate(sr.fixture_reference())]


def test_inputs_are_well_conditioned():
    """the condition the bound rests on: no row of any case is a bad input (a near-tie of the top two logits or
    of the latent's extremes in float64, or the fp32 torch path off by more than 1e-2)"""
    for name, ref in _references():
        ref.report(name)
        assert len(ref.obs) in (27, 37) and ref.bad.size == 0, (name, ref.bad)
        assert max(ref.base.values()) < sr.BAD_INPUT
    n3 = sr.weights_reference("weights_N3_s0")
    assert (n3.obs[:32].sum(axis=1) == 3).all() and not np.isin(n3.obs[32:], (0.0, 1.0)).all()


def test_bound_discriminates():
    """the float64 path with the normalisation's min and max detached -- a backward that forgets the arg-min and
    arg-max terms -- lands far outside the bound: at least 1000 x, for every case and head"""
    for name, ref in _references():
        net = sr.npz_net(name) if name.startswith("weights") else sr.fixture_nets()[int(name[-1])]
        d = sr.torch_saliency(net, ref.obs, torch.float64, detach_minmax=True)
        errs = ref.errors(d["policy"], d["value"])
        print(f"\n{name}: detached min / max deviates by policy {errs['policy']:.3g} value {errs['value']:.3g}")
        for h in ("policy", "value"):
            assert errs[h] >= 1000 * ref.bound[h], (name, h, errs[h], ref.bound[h])


def test_aggregate_saliency_per_disk_is_the_references():
    from muzero_hanoi_amd import acting

    v = np.array([1, -2, 3, -4, 5, -6, 0.5, 0.25, -0.125], np.float32)
    got = acting.aggregate_saliency_per_disk(v)
    assert got == [np.float32(6), np.float32(15), np.float32(0.875)] and got[0].dtype == np.float32
    assert acting.aggregate_saliency_per_disk(np.arange(8.0), num_disks=4, num_rods=2) == [1, 5, 9, 13]
    with pytest.raises(ValueError, match="does not match num_disks"):
        acting.aggregate_saliency_per_disk(v, num_disks=4)
