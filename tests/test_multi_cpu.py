"""Search over a set of networks (mzh_load_weight_set / mzh_search_multi), the checks that need no GPU: the
boundary (struct layout, exports, ABI version), the host-side set packer against the single-network packer
(tests/pack_set_check.cpp, a stand-alone program under the host sanitizers), networks.NetworkSet's shape
check and checkpoint.ablation_variants against ablate_networks applied by hand."""
import copy
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import GOLDEN, ROOT

HEADER = os.path.join(ROOT, "include", "mzh.h")


@pytest.fixture(scope="module")
def lib():
    from muzero_hanoi_amd import build

    build.build()
    from muzero_hanoi_amd import _lib

    return _lib


def test_multi_args_layout_matches_header(lib, tmp_path):
    """ctypes MultiArgs == struct mzh_multi_args as the C compiler lays out include/mzh.h"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [f[0] for f in lib.MultiArgs._fields_]
    assert fields == ["n_networks", "net_index", "status"]
    src = tmp_path / "multi_args.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mzh.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof(mzh_multi_args, {f}));\n' for f in fields)
                   + 'printf("%zu\\n", sizeof(mzh_multi_args)); return 0; }\n')
    exe = tmp_path / "multi_args"
    subprocess.run([cc, "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [getattr(lib.MultiArgs, f).offset for f in fields] + [ctypes.sizeof(lib.MultiArgs)]
    hdr = open(HEADER).read()
    block = hdr[hdr.index("typedef struct mzh_multi_args"):]
    block = block[:block.index("} mzh_multi_args;")]
    assert re.sub(r"/\*.*?\*/", "", block, flags=re.S).count(";") == len(fields)  # one declaration per field


def test_symbols_exported_and_abi_version_unchanged(lib):
    L = lib.lib()
    for name in ("mzh_load_weight_set", "mzh_search_multi"):
        assert hasattr(L, name) and name in lib.SIGNATURES
    assert L.mzh_abi_version() == lib.ABI_VERSION == 6
    # the argument checks that come before any device call
    assert L.mzh_load_weight_set(None, None, 0, 1) == lib.MZH_ERR_ARG
    assert L.mzh_search_multi(None, None, None, None) == lib.MZH_ERR_ARG


@pytest.fixture(scope="module")
def pack_set_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("pack_set_check") / "pack_set_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "pack_set_check.cpp"),
                    os.path.join(ROOT, "muzero-hanoi_amd", "csrc", "mzh_pack.cpp"), "-o", str(exe)], check=True)
    return str(exe)


# in_dim 9 / 12 / 48 (1, 1, 3 first-layer k-blocks), both head kinds
@pytest.mark.parametrize("n_disks,support", [(3, 33), (3, 1), (4, 33), (16, 1)])
def test_set_blobs_equal_single_network_blobs(pack_set_check, n_disks, support):
    r = subprocess.run([pack_set_check, str(n_disks), str(support)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def _net(n, td=True, seed=0):
    from muzero_hanoi_amd.networks import MuZeroNet

    torch.manual_seed(seed)
    return MuZeroNet(3 * n, 6, 0.002, "cpu", TD_return=td)


def test_network_set_refuses_mixed_shapes():
    from muzero_hanoi_amd.networks import NetworkSet

    a, b = _net(3), _net(3, seed=1)
    s = NetworkSet([a, b])
    assert len(s) == 2 and s[1] is b and (s.in_dim, s.support) == (9, 33)
    with pytest.raises(TypeError):
        NetworkSet([a, _net(4)])  # mixed N
    with pytest.raises(TypeError):
        NetworkSet([a, _net(3, td=False)])  # mixed support
    with pytest.raises(TypeError):
        NetworkSet([])
    with pytest.raises(TypeError):
        NetworkSet([a, torch.nn.Linear(9, 6)])  # not MuZeroNet's state-dict keys
    with pytest.raises(TypeError):
        NetworkSet([a, a.state_dict()])


REF_LABELS = ["Muzero_", "ResetLatentRwd_", "ResetLatentVal_", "ResetLatentVal_ResetLatentRwd_", "ResetLatentPol_",
              "ResetLatentPol_ResetLatentRwd_", "ResetLatentPol_ResetLatentVal_",
              "ResetLatentPol_ResetLatentVal_ResetLatentRwd_"]


def test_ablation_variants_labels_and_weights():
    """the 8 switch combinations under the reference's labels (acting_ablations.py:149-162), each network equal
    to ablate_networks applied by hand to a copy, drawing from the same torch seed in the documented order"""
    from muzero_hanoi_amd.checkpoint import ablate_networks, ablation_variants, load_model

    net = load_model(os.path.join(GOLDEN, "muzero_model_N3.pt"))
    before = copy.deepcopy(net.state_dict())
    torch.manual_seed(77)
    variants = ablation_variants(net)
    assert [l for l, _ in variants] == REF_LABELS
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), f"ablation_variants changed its argument: {k}"
    torch.manual_seed(77)
    heads = {"Pol": "policy_net", "Val": "value_net", "Rwd": "rwd_net"}
    for label, got in variants:
        sw = [f"ResetLatent{h}_" in label for h in ("Pol", "Val", "Rwd")]
        want = ablate_networks(*sw, copy.deepcopy(net))
        for k, v in want.state_dict().items():
            assert torch.equal(got.state_dict()[k], v), (label, k)
            reset = any(on and k.startswith(heads[h]) for on, h in zip(sw, ("Pol", "Val", "Rwd")))
            assert torch.equal(v, before[k]) != reset, (label, k)  # exactly the switched heads were re-drawn
    assert got is not net and all(a is not b for (_, a), (_, b) in zip(variants, variants[1:]))
