"""A simulation budget per root (mzh_search_multi_budget, Engine.search_multi(sims=...), BatchedSelfPlay.play(sims=...),
evaluate_networks(budgets="fused")): the checks that need no GPU -- the boundary (struct layout, export, ABI
version), the host refusals that need neither an engine nor a device, and the Python refusals that come before
any device work."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mzh.h")


@pytest.fixture(scope="module")
def lib():
    from muzero_hanoi_amd import build

    build.build()
    from muzero_hanoi_amd import _lib

    return _lib


def test_abi_version_unchanged_and_symbol_exported(lib):
    L = lib.lib()
    assert hasattr(L, "mzh_search_multi_budget") and "mzh_search_multi_budget" in lib.SIGNATURES
    hdr = open(HEADER).read()
    assert "#define MZH_ABI_VERSION 6" in hdr and L.mzh_abi_version() == lib.ABI_VERSION == 6
    assert ("int mzh_search_multi_budget(mzh_engine* eng, const mzh_search_args* args, const mzh_multi_args* multi,"
            in hdr)


def test_budget_args_layout_matches_header(lib, tmp_path):
    """ctypes BudgetArgs == struct mzh_budget_args as the C compiler lays out include/mzh.h"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [f[0] for f in lib.BudgetArgs._fields_]
    assert fields == ["n_sims", "max_runs"]
    want = [getattr(lib.BudgetArgs, f).offset for f in fields] + [ctypes.sizeof(lib.BudgetArgs)]
    src = tmp_path / "budget_args.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mzh.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof(mzh_budget_args, {f}));\n' for f in fields)
                   + 'printf("%zu\\n", sizeof(mzh_budget_args)); return 0; }\n')
    exe = tmp_path / "budget_args"
    subprocess.run([cc, "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    hdr = open(HEADER).read()
    block = hdr[hdr.index("typedef struct mzh_budget_args"):]
    block = block[:block.index("} mzh_budget_args;")]
    assert re.sub(r"/\*.*?\*/", "", block, flags=re.S).count(";") == len(fields)  # one declaration per field


def test_host_refusals_without_engine_or_device(lib):
    """what the budget block alone decides is refused first, with its own message; then the NULL engine"""
    L = lib.lib()
    a, m = lib.SearchArgs(), lib.MultiArgs()
    a.B, a.n_sims = 4, 5
    m.n_networks, m.net_index = 1, 0x1000  # never dereferenced
    ref = ctypes.byref

    def budget(n_sims, max_runs):
        b = lib.BudgetArgs()
        b.n_sims, b.max_runs = n_sims, max_runs
        return b

    assert L.mzh_search_multi_budget(None, None, None, None, None) == lib.MZH_ERR_ARG
    assert "NULL" in lib.last_error()
    assert L.mzh_search_multi_budget(None, ref(a), ref(m), None, None) == lib.MZH_ERR_ARG
    assert "budget NULL" in lib.last_error()
    assert L.mzh_search_multi_budget(None, ref(a), ref(m), ref(budget(None, 3)), None) == lib.MZH_ERR_ARG
    assert "n_sims is NULL" in lib.last_error()
    for bad in (0, -1):
        assert L.mzh_search_multi_budget(None, ref(a), ref(m), ref(budget(0x1000, bad)), None) == lib.MZH_ERR_ARG
        assert f"max_runs={bad} < 1" in lib.last_error()
    # a complete budget block reaches the checks mzh_search_multi makes: first the engine
    assert L.mzh_search_multi_budget(None, ref(a), ref(m), ref(budget(0x1000, 3)), None) == lib.MZH_ERR_ARG
    assert "engine or args NULL" in lib.last_error()


def _nets(n=3, count=2):
    from muzero_hanoi_amd.networks import MuZeroNet, NetworkSet

    nets = []
    for s in range(count):
        torch.manual_seed(s)
        nets.append(MuZeroNet(3 * n, 6, 0.002, "cpu", TD_return=True))
    return NetworkSet(nets)


def test_evaluate_networks_budget_refusals_before_device_work(monkeypatch):
    from muzero_hanoi_amd import selfplay

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(selfplay, "engine_for_set", no_device)
    monkeypatch.setattr(selfplay, "engine_for", no_device)
    nset = _nets()
    with pytest.raises(ValueError, match="budgets must be 'each' or 'fused'"):
        selfplay.evaluate_networks(nset, 3, [5, 10], start_idx=[0, 1], budgets="x")
    with pytest.raises(ValueError, match="lockstep form"):
        selfplay.evaluate_networks(nset, 3, [5, 10], start_idx=[0, 1], budgets="fused", launch="episodes")
    with pytest.raises(ValueError, match="budgets >= 0"):
        selfplay.evaluate_networks(nset, 3, [5, -1], start_idx=[0, 1], budgets="fused")


def test_sims_of_wrong_length_or_dtype_refused_before_device_work(monkeypatch):
    from muzero_hanoi_amd import engine, selfplay

    # Engine.search_multi: sims is an int32 tensor [B]; the check precedes every use of the device
    eng = engine.Engine.__new__(engine.Engine)
    eng.set_size = 2

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(engine.Engine, "_search_args", no_device)
    B = 4
    kw = dict(net_index=torch.zeros(B, dtype=torch.int32), obs=torch.zeros(B, 9), tie_idx=torch.zeros(B, dtype=torch.int32))
    for bad in (torch.zeros(B - 1, dtype=torch.int32), torch.zeros(B + 1, dtype=torch.int32),
                torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.float32),
                torch.zeros((B, 1), dtype=torch.int32), np.zeros(B, np.int32), [5] * B):
        with pytest.raises(ValueError, match="sims must be an int32 tensor"):
            eng.search_multi(5, sims=bad, **kw)
    with pytest.raises(ValueError, match="max_runs"):
        eng.search_multi(5, sims=torch.zeros(B, dtype=torch.int32), max_runs=0, **kw)
    with pytest.raises(ValueError, match="max_runs goes with sims"):
        eng.search_multi(5, max_runs=2, **kw)

    # BatchedSelfPlay.play / play_plans: sims [B] integers in [0, n_simulations], a NetworkSet only
    monkeypatch.setattr(selfplay, "engine_for_set", no_device)
    monkeypatch.setattr(selfplay, "engine_for", no_device)
    nset = _nets()
    sp = selfplay.BatchedSelfPlay(nset, 3, 10, 12)
    starts, ni = [0, 1, 2], [0, 0, 1]
    for bad in ([5, 5], [5, 5, 5, 5], [5.0, 5.0, 5.0], [5, 13, 5], [5, -1, 5], [[5, 5, 5]]):
        with pytest.raises(ValueError, match="sims must be 3 integer budgets"):
            sp.play(starts, net_index=ni, sims=bad)
    with pytest.raises(ValueError, match="budget >= 1"):
        sp.play_plans(starts, 2, net_index=ni, sims=[5, 0, 5])
    with pytest.raises(ValueError, match="needs a NetworkSet"):
        selfplay.BatchedSelfPlay(nset[0], 3, 10, 12).play(starts, sims=[5, 5, 5])
