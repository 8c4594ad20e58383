"""Acting on perturbed observations (noise_injection_comparison.py, permutation_importance.py), the checks that
need no GPU: the boundary of mzh_env_step_observe (struct layout, export, argument errors before any device
call), evaluate_perturbed's host-only row layout and scoring, its argument errors, the perturbation draws'
prefix property and their stream apart from the search draws, and the shape of the reference fixtures
tests/golden/perturb_*.npz (tests/golden/gen_perturb_golden.py).
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden
from muzero_hanoi_amd import rng as mrng

HEADER = os.path.join(ROOT, "include", "mzh.h")
PERTURB = sorted(f[len("perturb_"):-4] for f in os.listdir(GOLDEN) if f.startswith("perturb_") and f.endswith(".npz"))


@pytest.fixture(scope="module")
def lib():
    from muzero_hanoi_amd import build

    build.build()
    from muzero_hanoi_amd import _lib

    return _lib


# ------------------------------------------------------------------------------------ the C boundary
def test_observe_args_layout_matches_header(lib, tmp_path):
    """ctypes ObserveArgs == struct mzh_observe_args as the C compiler lays out include/mzh.h"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [f[0] for f in lib.ObserveArgs._fields_]
    src = tmp_path / "observe_args.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mzh.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof(mzh_observe_args, {f}));\n' for f in fields)
                   + 'printf("%zu\\n", sizeof(mzh_observe_args)); return 0; }\n')
    exe = tmp_path / "observe_args"
    subprocess.run([cc, "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [getattr(lib.ObserveArgs, f).offset for f in fields] + [ctypes.sizeof(lib.ObserveArgs)]
    hdr = open(HEADER).read()
    block = hdr[hdr.index("typedef struct mzh_observe_args"):]
    block = block[:block.index("} mzh_observe_args;")]
    decls = [ln for ln in block.splitlines()[1:] if re.match(r"  (const )?\w+\*? [\w, ]+;", ln)]
    assert len(decls) == len(fields) - 2  # "int32_t n_disks, goal_peg, max_steps;" declares three
    assert set(fields) == {"n_disks", "goal_peg", "max_steps", "B", "n", "env_index", "action", "state", "step_ctr",
                           "active", "steps_total", "illegal_total", "solved", "perm_disc", "perm_peg", "noise", "obs",
                           "reward", "done", "err_count"}


def test_symbol_exported_and_abi_version_unchanged(lib):
    L = lib.lib()
    assert hasattr(L, "mzh_env_step_observe") and "mzh_env_step_observe" in lib.SIGNATURES
    assert L.mzh_abi_version() == lib.ABI_VERSION == 6
    hdr = open(HEADER).read()
    assert "#define MZH_ABI_VERSION 6" in hdr and "int mzh_env_step_observe(const mzh_observe_args*" in hdr


REQUIRED = ("state", "step_ctr", "active", "steps_total", "illegal_total", "solved", "obs")
OPTIONAL = ("env_index", "action", "perm_disc", "perm_peg", "noise", "reward", "done", "err_count")


def _valid_args(lib):
    """arguments that pass every check (the pointers are never dereferenced by the checks)"""
    a = lib.ObserveArgs()
    a.n_disks, a.goal_peg, a.max_steps, a.B, a.n = 3, 2, 50, 8, 4
    for f in REQUIRED + OPTIONAL:
        setattr(a, f, 0x1000)
    return a


@pytest.mark.parametrize("field,value,msg", [
    ("n", 0, "bad n=0"), ("n", -3, "bad n=-3"), ("B", 0, "B=0"), ("B", -1, "B=-1"), ("n_disks", 0, "bad n_disks=0"),
    ("n_disks", 33, "bad n_disks=33"), ("goal_peg", 3, "goal_peg=3"), ("goal_peg", -1, "goal_peg=-1")]
    + [(f, None, "required buffer is NULL") for f in REQUIRED + ("perm_peg",)])
def test_argument_errors_without_device(lib, field, value, msg):
    """refused before any launch (no device is touched: the valid pointers are not addresses of anything);
    perm_peg is required here because perm_disc is given"""
    L = lib.lib()
    a = _valid_args(lib)
    setattr(a, field, value)
    assert L.mzh_env_step_observe(ctypes.byref(a), None) == lib.MZH_ERR_ARG
    assert msg in lib.last_error()
    with pytest.raises(ValueError):
        lib.check(lib.MZH_ERR_ARG, "mzh_env_step_observe")


def test_null_args_and_rows_beyond_the_batch(lib):
    L = lib.lib()
    assert L.mzh_env_step_observe(None, None) == lib.MZH_ERR_ARG
    a = _valid_args(lib)
    a.env_index, a.n, a.B = None, 9, 8  # without env_index row j is env j: n <= B
    assert L.mzh_env_step_observe(ctypes.byref(a), None) == lib.MZH_ERR_ARG and "bad n=9" in lib.last_error()


# ------------------------------------------------------------------------------------ the row layout
CONDITIONS = [("baseline",), ("noise", 0.05), ("noise", 0.3), ("permute", 0), ("permute", 2), ("baseline",)]


def test_layout_shapes_order_and_shared_starts():
    from muzero_hanoi_amd.selfplay import perturbed_layout

    starts = np.array([0, 13, 5, 21, 8], np.int64)
    M, C, E = 3, len(CONDITIONS), len(starts)
    lay = perturbed_layout(M, CONDITIONS, starts, 3)
    assert set(lay) == {"net_index", "cond_index", "start_idx", "noise_std", "permute_disc"}
    assert all(v.shape == (M * C * E,) for v in lay.values())
    assert lay["permute_disc"].dtype == np.int32 and lay["noise_std"].dtype == np.float64
    assert np.all(np.diff(lay["net_index"]) >= 0) and np.array_equal(np.unique(lay["net_index"]), np.arange(M))
    for m in range(M):
        for c in range(C):
            rows = (lay["net_index"] == m) & (lay["cond_index"] == c)
            assert rows.sum() == E and np.array_equal(lay["start_idx"][rows], starts)  # the same starts, in order
            std = CONDITIONS[c][1] if CONDITIONS[c][0] == "noise" else 0.0
            disc = CONDITIONS[c][1] if CONDITIONS[c][0] == "permute" else -1
            assert np.all(lay["noise_std"][rows] == std) and np.all(lay["permute_disc"][rows] == disc)
    r = np.arange(M * C * E)  # network-major, then condition, then start
    assert np.array_equal(lay["net_index"], r // (C * E)) and np.array_equal(lay["cond_index"], (r // E) % C)


def test_scores_from_per_row_solved():
    from muzero_hanoi_amd.selfplay import perturbed_scores

    M, C, E = 2, len(CONDITIONS), 4
    solved = np.random.RandomState(3).randint(0, 2, M * C * E).astype(np.uint8)
    rate, imp = perturbed_scores(solved, M, CONDITIONS)
    s = solved.reshape(M, C, E)
    assert rate.shape == imp.shape == (M, C)
    for m in range(M):
        for c, cond in enumerate(CONDITIONS):
            assert rate[m, c] == s[m, c].sum() / E
            if cond[0] == "permute":  # the first baseline, not the second
                assert imp[m, c] == s[m, 0].sum() / E - s[m, c].sum() / E
            else:
                assert np.isnan(imp[m, c])
    _, imp = perturbed_scores(solved[:2 * E], 1, [("permute", 1), ("noise", 0.1)])
    assert np.isnan(imp).all()  # no baseline


@pytest.mark.parametrize("conditions,start_idx,msg", [
    ([("blur", 1.0)], [0], "unknown condition"), ([("baseline", 1)], [0], "unknown condition"),
    ([("noise",)], [0], "unknown condition"), (["noise"], [0], "unknown condition"),
    ([("noise", -0.1)], [0], "std must be >= 0"), ([("noise", float("nan"))], [0], "std must be >= 0"),
    ([("permute", 3)], [0], "disc must be in"), ([("permute", -1)], [0], "disc must be in"),
    ([("permute", 0.5)], [0], "disc must be in"), ([("baseline",)], [], "starts"), ([], [0], "conditions"),
    ([("baseline",)], [27], "start indices")])
def test_layout_value_errors(conditions, start_idx, msg):
    from muzero_hanoi_amd.selfplay import perturbed_layout

    with pytest.raises(ValueError, match=msg):
        perturbed_layout(2, conditions, start_idx, 3)


def _Net(n=3):
    """a network on the host: every refusal below comes before any device use"""
    from muzero_hanoi_amd.networks import MuZeroNet

    return MuZeroNet(3 * n, 6, 0.002, "cpu", TD_return=True)


def test_evaluate_perturbed_value_errors():
    from muzero_hanoi_amd import selfplay

    ev = selfplay.evaluate_perturbed
    with pytest.raises(ValueError, match="unknown condition"):
        ev(_Net(), 3, conditions=[("shuffle", 0)], start_idx=[0])
    with pytest.raises(ValueError, match="std must be >= 0"):
        ev([_Net(), _Net()], 3, conditions=[("baseline",), ("noise", -1.0)], starts=[(0, 0, 0)])
    with pytest.raises(ValueError, match="disc must be in"):
        ev(_Net(), 3, conditions=[("permute", 3)], starts=[(0, 0, 0)])
    with pytest.raises(ValueError, match="disc must be in"):
        ev(_Net(4), 4, conditions=[("permute", 4)], episodes=2)
    with pytest.raises(ValueError, match="n_disks"):
        ev(_Net(4), 3, conditions=[("baseline",)], episodes=2)
    with pytest.raises(ValueError, match="no starts"):
        ev(_Net(), 3, conditions=[("baseline",)])
    with pytest.raises(ValueError, match="no starts"):
        ev(_Net(), 3, conditions=[("baseline",)], episodes=0)
    with pytest.raises(ValueError, match="starts"):
        ev(_Net(), 3, conditions=[("baseline",)], starts=[])
    with pytest.raises(ValueError, match="max_roots"):
        ev(_Net(), 3, conditions=[("baseline",)], start_idx=[0], max_roots=0)


def test_play_perturbed_condition_arrays():
    from muzero_hanoi_amd.selfplay import perturbation_arrays

    assert perturbation_arrays(4, 3, None, None) == (None, None)
    assert perturbation_arrays(4, 3, 0.0, -1) == (None, None)  # nothing perturbed: play's path
    std, disc = perturbation_arrays(4, 3, 0.3, [None, 0, -1, 2])
    assert std.tolist() == [0.3] * 4 and disc.tolist() == [-1, 0, -1, 2] and disc.dtype == np.int32
    std, disc = perturbation_arrays(3, 3, [0.0, 0.1, 0.0], 1)
    assert std.tolist() == [0.0, 0.1, 0.0] and disc.tolist() == [1, 1, 1]
    for kw in (dict(noise_std=-0.5, permute_disc=None), dict(noise_std=[0.1, float("nan")], permute_disc=None),
               dict(noise_std=None, permute_disc=3), dict(noise_std=None, permute_disc=[0, -2]),
               dict(noise_std=[0.1] * 3, permute_disc=None), dict(noise_std=None, permute_disc=0.5)):
        with pytest.raises(ValueError):
            perturbation_arrays(2, 3, **kw)


# ------------------------------------------------------------------------------------ the draws
@pytest.mark.parametrize("seed", [0, 7, 2**31 - 1])
def test_perturbation_draws_prefix_property(seed):
    peg, z = mrng.perturbation_draws(1000, 9, seed)
    assert peg.shape == (1000,) and peg.dtype == np.int32 and z.shape == (1000, 9) and z.dtype == np.float64
    assert set(np.unique(peg)) == {0, 1, 2}
    for n in (1, 2, 37, 999):
        p2, z2 = mrng.perturbation_draws(n, 9, seed)
        assert np.array_equal(p2, peg[:n]) and np.array_equal(z2.view(np.uint64), z[:n].view(np.uint64))
    p3, z3 = mrng.perturbation_draws(1000, 9, seed + 1)
    assert not np.array_equal(p3, peg) and not np.array_equal(z3, z)
    assert abs(z.mean()) < 0.05 and abs(z.std() - 1) < 0.05  # 9000 standard normals


def test_perturbation_seeds_are_a_stream_apart_from_the_search_seeds():
    """the search draws' seeds are default_rng(seed).integers(2**31) (selfplay._Lockstep._draw); the perturbation
    draws' come from a child of seed's sequence, and taking them does not move the search seeds"""
    for seed in (0, 5):
        search = np.random.default_rng(seed).integers(2**31, size=8)
        pert = mrng.perturbation_seeds(seed).integers(2**31, size=8)
        assert not np.intersect1d(search, pert).size
        assert np.array_equal(mrng.perturbation_seeds(seed).integers(2**31, size=8), pert)
    assert not np.array_equal(mrng.perturbation_seeds(0).integers(2**31, size=8),
                              mrng.perturbation_seeds(1).integers(2**31, size=8))


# ------------------------------------------------------------------------------------ the fixtures
def test_fixture_set():
    assert PERTURB == ["noise", "permute"]


@pytest.mark.parametrize("name", ["noise", "permute"])
def test_fixture_records_are_consistent(name):
    """per game: its decisions add up, solved == a reward of 100 on its last step, the observation of its first
    decision under no perturbation is the start's one-hot; float32 observations; noise only where std > 0; a
    permuted observation differs from the true state on the permuted disc at most"""
    g = golden(f"perturb_{name}.npz")
    n = int(g["n"])
    assert g["run_obs"].dtype == np.float32 and g["run_obs"].shape == (len(g["actions"]), 3 * n)
    assert int(g["decisions"].sum()) == len(g["actions"]) == len(g["env_rwd"]) == len(g["run_S"])
    assert set(g["run_S"].tolist()) == {int(g["n_sims"])} and len(g["post_rng"]) == 3
    assert {0, 1} == set(g["solved"].tolist())  # both outcomes occur
    p = 0
    for cond, start, solved, k in zip(g["cond"], g["start"], g["solved"], g["decisions"]):
        k = int(k)
        assert 1 <= k <= int(g["max_game_steps"])
        assert bool(solved) == (g["env_rwd"][p + k - 1] == 100.0) and not (g["env_rwd"][p:p + k - 1] == 100.0).any()
        assert bool(g["env_done"][p + k - 1]) and not g["env_done"][p:p + k - 1].any()
        onehot = np.zeros(3 * n, np.float32)
        onehot[np.arange(n) * 3 + start] = 1
        obs = g["run_obs"][p:p + k]
        if name == "noise":
            exact = np.isin(obs, (0.0, 1.0)).all()
            assert exact == (cond == 0.0) and (cond > 0 or np.array_equal(obs[0], onehot))
        else:
            assert np.isin(obs, (0.0, 1.0)).all() and (obs.reshape(k, n, 3).sum(2) == 1).all()
            keep = np.arange(n) != int(cond)
            assert np.array_equal(obs[0].reshape(n, 3)[keep], onehot.reshape(n, 3)[keep])
        p += k
