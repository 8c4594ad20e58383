"""Plan-ahead acting (acting_experiments/planning_multiple_actions.py:111-183), the checks that need no GPU:
the boundary of mzh_env_run_plan (struct layout, export, argument errors before any device call) and the
fixtures tests/golden/plan_*.npz (runs of the reference's own MCTS / TowersOfHanoi / MuZeroNet under the
restated loop, tests/golden/gen_plan_golden.py) replayed with the oracle search and the oracle env step:
executed actions, plan lengths, steps, errors, the MinMaxStats chain and the RNG position.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden
from muzero_hanoi_amd import rng as mrng

HEADER = os.path.join(ROOT, "include", "mzh.h")
PLAN = sorted(f[len("plan_"):-4] for f in os.listdir(GOLDEN) if f.startswith("plan_") and f.endswith(".npz"))


@pytest.fixture(scope="module")
def lib():
    from muzero_hanoi_amd import build

    build.build()
    from muzero_hanoi_amd import _lib

    return _lib


def test_fixture_set():
    assert PLAN == ["es_l7", "rand_l3"]


def test_plan_args_layout_matches_header(lib, tmp_path):
    """ctypes PlanArgs == struct mzh_plan_args as the C compiler lays out include/mzh.h"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [f[0] for f in lib.PlanArgs._fields_]
    src = tmp_path / "plan_args.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mzh.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof(mzh_plan_args, {f}));\n' for f in fields)
                   + 'printf("%zu\\n", sizeof(mzh_plan_args)); return 0; }\n')
    exe = tmp_path / "plan_args"
    subprocess.run([cc, "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [getattr(lib.PlanArgs, f).offset for f in fields] + [ctypes.sizeof(lib.PlanArgs)]
    hdr = open(HEADER).read()
    block = hdr[hdr.index("typedef struct mzh_plan_args"):]
    block = block[:block.index("} mzh_plan_args;")]
    assert block.count(";") == len(fields) - 2  # "int32_t n_disks, goal_peg, max_steps;" declares three


def test_symbol_exported_and_abi_version_unchanged(lib):
    L = lib.lib()
    assert hasattr(L, "mzh_env_run_plan") and "mzh_env_run_plan" in lib.SIGNATURES
    assert L.mzh_abi_version() == lib.ABI_VERSION == 6


REQUIRED = ("plan", "plan_len", "state", "step_ctr", "active", "obs", "executed", "steps_total", "illegal_total")


def _valid_args(lib):
    """arguments that pass every check (the pointers are never dereferenced by the checks)"""
    a = lib.PlanArgs()
    a.n_disks, a.goal_peg, a.max_steps, a.B, a.n, a.max_plan_len, a.plan_stride = 3, 2, 30, 8, 4, 7, 26
    for f in REQUIRED + ("env_index",):
        setattr(a, f, 0x1000)
    return a


@pytest.mark.parametrize("field,value,msg", [
    ("n", 0, "bad n=0"), ("n", -3, "bad n=-3"), ("B", 0, "B=0"), ("max_plan_len", 0, "bad max_plan_len=0"),
    ("plan_stride", 6, "plan_stride=6"), ("n_disks", 0, "bad n_disks=0"), ("n_disks", 33, "bad n_disks=33"),
    ("goal_peg", 3, "goal_peg=3")] + [(f, None, "required buffer is NULL") for f in REQUIRED])
def test_argument_errors_without_device(lib, field, value, msg):
    L = lib.lib()
    a = _valid_args(lib)
    setattr(a, field, value)
    assert L.mzh_env_run_plan(ctypes.byref(a), None) == lib.MZH_ERR_ARG
    assert msg in lib.last_error()
    with pytest.raises(ValueError):
        lib.check(lib.MZH_ERR_ARG, "mzh_env_run_plan")


def test_null_args_and_rows_beyond_the_batch(lib):
    L = lib.lib()
    assert L.mzh_env_run_plan(None, None) == lib.MZH_ERR_ARG
    a = _valid_args(lib)
    a.env_index, a.n, a.B = None, 9, 8  # without env_index row j is env j: n <= B
    assert L.mzh_env_run_plan(ctypes.byref(a), None) == lib.MZH_ERR_ARG and "bad n=9" in lib.last_error()


# ------------------------------------------------------------------------------------ fixtures on the oracle
def recorded_calls(g):
    """per run_mcts call: the recorded root policy and per-simulation outputs (RecordedNetwork format)"""
    calls, off = [], 0
    for k, S in enumerate(g["run_S"]):
        S = int(S)
        calls.append(dict(root_pi=g["run_root_pi"][k], pi=g["run_pi"][off:off + S],
                          reward=g["run_reward"][off:off + S], value=g["run_value"][off:off + S]))
        off += S
    return calls


def oracle_plan_episodes(oracle, g):
    """the plan-ahead loop on oracle.search (replay mode, carried bounds) + oracle.env_step, draws from the
    global NumPy stream; returns dict(data, actions, plan_lens, steps, errors, nplans, starts, mm, search_action)"""
    from muzero_hanoi_amd.hanoi_utils import hanoi_solver
    from muzero_hanoi_amd.selfplay import index_state

    n, max_steps, L = int(g["n"]), int(g["max_steps"]), int(g["max_plan_len"])
    alpha, T = float(g["alpha"]), float(g["temperature"])
    calls = recorded_calls(g)
    out = dict(data=[], actions=[], plan_lens=[], steps=[], errors=[], nplans=[], starts=[], mm=[], search_action=[])
    state = dict(k=0, mm=np.array([[-np.inf, np.inf]]))

    def plan(st, S):
        obs = np.zeros(3 * n)
        obs[np.arange(n) * 3 + st] = 1
        noise, tie, u = mrng.predraw(1, deterministic=False, alpha=alpha)
        c = calls[state["k"]]
        state["k"] += 1
        assert np.array_equal(obs, g["run_obs"][state["k"] - 1]), "the search starts from another observation"
        o = oracle.search(n, S, obs[None], replay=dict(root_pi=c["root_pi"][None], pi=c["pi"][None],
                                                       rwd=c["reward"][None], value=c["value"][None]),
                          noise=noise, tie_idx=tie, action_u=u, temperature=T, minmax_in=state["mm"])
        state["mm"] = np.stack([o["mm_max"], o["mm_min"]], 1)
        out["mm"].append(state["mm"][0].copy())
        out["search_action"].append(int(o["action"][0]))
        seq = [int(a) for a in o["latent"][0, :int(o["latent_len"][0])][:L]]
        out["plan_lens"].append(len(seq))
        return seq

    for S in (int(b) for b in g["budgets"]):
        errors = []
        for _ in range(int(g["episodes"])):
            if int(g["start"]) >= 0:
                idx = int(g["init_state_idx"])
            else:  # env/hanoi.py:103-109 on the global stream
                while True:
                    idx = np.random.randint(3 ** n)
                    if idx != 3 ** n - 1:
                        break
            st = np.array(index_state(idx, n), np.uint8)
            s0 = tuple(int(x) for x in st)
            ctr, active, done, steps, t, nplans = 0, 1, 0, 0, 0, 1
            seq = plan(st, S)
            while not done:
                _, st, moved, ctr, active, done, _ = oracle.env_step(st, seq[t], ctr, active, max_steps)
                out["actions"].append(seq[t])
                steps += 1
                t += 1
                if t >= len(seq) and not done:
                    seq = plan(moved, S)
                    nplans += 1
                    t = 0
            errors.append(steps - hanoi_solver(s0))
            out["starts"].append(s0)
            out["steps"].append(steps)
            out["nplans"].append(nplans)
        out["errors"] += errors
        out["data"].append([S, sum(errors) / len(errors)])
    assert state["k"] == len(calls)
    return out


@pytest.mark.parametrize("name", PLAN)
def test_plan_fixture_oracle(oracle, lib, name):
    g = golden(f"plan_{name}.npz")
    np.random.seed(int(g["seed"]))
    o = oracle_plan_episodes(oracle, g)
    assert o["data"] == g["data"].tolist()
    assert np.array_equal(o["actions"], g["actions"])
    assert np.array_equal(o["plan_lens"], g["plan_lens"])
    assert np.array_equal(o["steps"], g["ep_steps"]) and np.array_equal(o["errors"], g["ep_error"])
    assert np.array_equal(o["nplans"], g["ep_nplans"]) and np.array_equal(o["starts"], g["ep_start"])
    assert np.array_equal(o["search_action"], g["search_action"])
    assert np.array_equal(np.array(o["mm"]), g["mm"])
    assert np.array_equal(np.random.random_sample(3), g["post_rng"]), "RNG stream position differs"


def test_fixtures_cover_the_terminations():
    """the cases the fixtures were chosen for: an episode that ends on max_steps inside a plan (the rest of the
    plan dropped), one that ends on the goal inside a plan, and re-planning after a plan ran out"""
    seen = set()
    for name in PLAN:
        g = golden(f"plan_{name}.npz")
        lens, p = g["plan_lens"], 0
        for steps, nplans in zip(g["ep_steps"], g["ep_nplans"]):
            planned = int(lens[p:p + nplans].sum())
            p += nplans
            assert planned >= steps and int(lens[p - nplans:p - 1].sum()) < steps
            if planned > steps:
                seen.add("max_steps mid-plan" if steps == int(g["max_steps"]) else "goal mid-plan")
            if nplans > 1:
                seen.add("re-plan")
        assert p == len(lens) and int(g["ep_steps"].sum()) == len(g["actions"])
    assert seen == {"max_steps mid-plan", "goal mid-plan", "re-plan"}
