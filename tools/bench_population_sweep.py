"""Agents of different configurations trained abreast (MuzeroPopulation(overrides=...), mzh_play_episodes_sweep)
against the same agents as lone runs one after another.

Workload: tools/bench_population.py's -- N = 3, max_steps = 200, the reference's TrainingConfig (batch 256, unroll 5,
buffer 50,000, one episode and one update per loop), fused update, device ingest, selfplay="device" -- with agent m
searching BUDGETS[m % 4] simulations per move (n_mcts_simulations in {5, 10, 25, 50}) and everything else shared.

Legs (--legs, default all):
  loops    whole training loops.  For M = --sizes agents: a MuzeroPopulation with those overrides against the same M
           lone Muzero(selfplay="device") agents, each with its own budget, run one after another.  Both sides are
           built from the same seeds and run the same blocks, and a population's agent ends bit for bit as its lone
           run, so every block pair is the same work; blocks alternate (population first on even blocks).  Per M:
           agent-loops/s of each side as median with p10..p90 over the blocks, their ratio, whether the population's
           p10 clears the lone sequence's p90, and whether the agents equal their twins afterwards.
  kernel   the kernel alone, device time from events around the calls: one sweep launch of M networks of one env
           each with those budgets, against one mzh_play_episodes_multi launch of the same envs with every env at the
           maximum budget.  Untrained networks: the episodes run to max_steps or near it.
  --existing name=file.json[,name=file.json...] folds records of other tools' runs (tools/bench_population.py's
           loops leg, tools/one_probe.py, on this build and on the parent's) into the profile as they are.

  python tools/bench_population_sweep.py [--out profiles/population_sweep_bench.json] [--legs loops,kernel]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_population import BATCH, DEV, MAX_STEPS, N, muzero_kwargs, spread  # noqa: E402

BUDGETS = (5, 10, 25, 50)


def overrides_for(M):
    return [{"n_mcts_simulations": BUDGETS[m % len(BUDGETS)]} for m in range(M)]


def loops_leg(sizes, loops, blocks, warmup):
    from muzero_hanoi_amd.muzero import Muzero, MuzeroPopulation

    out = []
    for M in sizes:
        seeds, over = list(range(100, 100 + M)), overrides_for(M)
        pop = MuzeroPopulation(seeds, overrides=over, **muzero_kwargs())
        lone, streams = [], []
        for s, o in zip(seeds, over):
            torch.manual_seed(s)
            lone.append(Muzero(selfplay="device", **{**muzero_kwargs(), **o}))
            streams.append(np.random.RandomState(s).get_state())

        def run_pop(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pop.training_loop(n_loops=n + 1, min_replay_size=BATCH, print_acc=10 ** 9)
            torch.cuda.synchronize()
            return M * n / (time.perf_counter() - t0)

        def run_lone(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i, mz in enumerate(lone):
                np.random.set_state(streams[i])
                mz.training_loop(n_loops=n + 1, min_replay_size=BATCH, print_acc=10 ** 9)
                streams[i] = np.random.get_state()
            torch.cuda.synchronize()
            return M * n / (time.perf_counter() - t0)

        for _ in range(20):  # fill every buffer past the batch, build every workspace
            run_pop(warmup)
            run_lone(warmup)
            if min(len(a.buffer) for a in pop.agents) > 2 * BATCH:
                break
        else:
            raise SystemExit(f"M={M}: a buffer stayed at {min(len(a.buffer) for a in pop.agents)} rows")
        rates = {"population": [], "lone": []}
        for b in range(blocks):
            for side in (("population", "lone") if b % 2 == 0 else ("lone", "population")):
                rates[side].append((run_pop if side == "population" else run_lone)(loops))
        same = all(len(a.buffer) == len(b.buffer) and a.buffer.ptr == b.buffer.ptr and all(
            torch.equal(p, q) for p, q in zip(a.networks.parameters(), b.networks.parameters()))
            for a, b in zip(pop.agents, lone))
        p, l = spread(rates["population"]), spread(rates["lone"])
        rec = {"M": M, "n_mcts_simulations": [o["n_mcts_simulations"] for o in over],
               "agent_loops_per_sec": {"population": p, "lone_sequence": l},
               "ratio_of_medians": p["median"] / l["median"],
               "population_p10_above_lone_p90": p["p10"] > l["p90"],
               "agents_equal_their_lone_runs_afterwards": bool(same),
               "buffer_rows_min": min(len(a.buffer) for a in pop.agents)}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del pop, lone
        torch.cuda.empty_cache()
    return {"workload": f"hanoi{N}_s{'-'.join(map(str, BUDGETS))}_maxsteps{MAX_STEPS}_batch{BATCH}_unroll5_1ep_1update_"
                        "per_loop_fused_device_ingest",
            "loops_per_block": loops, "blocks": blocks, "sizes": out}


def kernel_leg(sizes, reps):
    from muzero_hanoi_amd import rng
    from muzero_hanoi_amd.engine import Engine, flat_weights
    from muzero_hanoi_amd.networks import MuZeroNet

    out, Mmax, S = [], max(sizes), max(BUDGETS)
    nets = []
    for m in range(Mmax):
        torch.manual_seed(500 + m)
        nets.append(flat_weights(MuZeroNet(3 * N, 6, 0.002, "cpu", TD_return=True).state_dict()))
    eng = Engine(N, S, Mmax, 33)
    eng.load_weight_set(nets)
    fl = rng.synthetic_draws(MAX_STEPS * Mmax, deterministic=False, alpha=0.25, seed=1)
    table = tuple(torch.from_numpy(x).reshape((MAX_STEPS, Mmax) + x.shape[1:]).to(DEV) for x in fl)
    state = torch.zeros((Mmax, N), dtype=torch.uint8, device=DEV)

    def timed(fn):
        ms = []
        for i in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            steps = fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms.append(e0.elapsed_time(e1))
        return spread(ms), steps

    for M in sizes:
        draws = dict(tie_idx=table[1][:, :M].contiguous(), noise=table[0][:, :M].contiguous(),
                     action_u=table[2][:, :M].contiguous())
        ni = torch.arange(M, dtype=torch.int32, device=DEV)
        sims = torch.tensor([BUDGETS[m % len(BUDGETS)] for m in range(M)], dtype=torch.int32, device=DEV)
        forms = (("sweep_form_own_budgets", dict(sims=sims)), ("set_form_every_env_at_the_maximum", {}))
        rec = {"M": M, "budgets": sims.tolist(), "maximum": S}
        for name, kw in forms:
            sp, steps = timed(lambda: eng.play_episodes(S, state[:M], MAX_STEPS, net_index=ni, **draws, **kw)["steps"])
            rec[name] = {"device_ms": sp, "moves": int(steps.sum()), "longest_episode": int(steps.max()),
                         "simulations": int((steps * (sims if kw else S)).sum())}
        a, b = (rec[k]["device_ms"] for k, _ in forms)
        rec["set_form_over_sweep_form"] = b["median"] / a["median"]
        rec["sweep_p90_below_set_p10"] = a["p90"] < b["p10"]
        print(json.dumps(rec), flush=True)
        out.append(rec)
    eng.close()
    return {"workload": f"hanoi{N}_maxsteps{MAX_STEPS}_untrained_one_env_per_network", "reps": reps, "sizes": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="loops,kernel")
    ap.add_argument("--sizes", default="4,8,16")
    ap.add_argument("--loops", type=int, default=10, help="loops of every agent per block")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--existing", default="", help="name=file.json,...: records of other tools' runs, folded in")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from muzero_hanoi_amd import _lib

    sizes = [int(x) for x in a.sizes.split(",")]
    rec = {"build_id": _lib.build_id(), "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None}
    if a.out and os.path.exists(a.out):  # legs run one by one add to the record of the same build
        with open(a.out) as f:
            old = json.load(f)
        if old.get("build_id") == rec["build_id"]:
            rec = old
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for leg in [x for x in a.legs.split(",") if x]:
            if leg == "loops":
                rec["training_loops"] = loops_leg(sizes, a.loops, a.blocks, a.warmup)
            elif leg == "kernel":
                rec["kernel_alone"] = kernel_leg(sizes, a.reps)
            else:
                raise SystemExit(f"unknown leg {leg!r}")
            if a.out:  # after every leg: a later leg's failure keeps the earlier ones
                with open(a.out, "w") as f:
                    json.dump(rec, f, indent=1)
    for item in [x for x in a.existing.split(",") if x]:
        name, path = item.split("=", 1)
        with open(path) as f:
            rec.setdefault("existing_paths", {})[name] = json.load(f)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
