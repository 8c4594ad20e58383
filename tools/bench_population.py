"""Several seeds trained abreast (muzero.MuzeroPopulation, mzh_play_episodes_multi) against what exists without them.

Workload of the training legs: tools/bench_reload.py's -- N = 3, S = 25, max_steps = 200, the reference's
TrainingConfig (batch 256, unroll 5, buffer 50,000, one episode and one update per loop), fused update, device
ingest, selfplay="device".

Legs (--legs, default all):
  loops    (a) whole training loops.  For M = --sizes agents: a MuzeroPopulation of M seeds against the same M lone
           Muzero(selfplay="device") agents run one after another.  Both sides are built from the same seeds and
           run the same blocks, and a population's agent ends bit for bit as its lone run, so every block pair is
           the same work; blocks alternate (population first on even blocks).  Per M: agent-loops/s of each side as
           median with p10..p90 over the blocks, their ratio, whether the population's gain exceeds both sides'
           spread, and the population's wall time per loop split into the launch (to its one host read) and the
           per-agent host work after it.
  kernel   (b) the kernel alone, device time from events around the calls: mzh_play_episodes_multi on M networks of
           one env each, against M mzh_play_episodes launches of one env, and against one single-network launch of
           B = M envs (the difference to that one is what the set form costs).  Untrained networks: the episodes
           run to max_steps or near it (a launch takes as long as its longest episode).  A fourth row runs the set
           form with every env on network 0: the set form's code without the other networks' weights.
  sweep    (c) tools/bench_ablation.py's set form (8 variants x 3 starts x --episodes episodes per budget) with
           evaluate_networks(launch="episodes") against launch="lockstep", whole sweeps alternated.

  python tools/bench_population.py [--out profiles/population_bench.json] [--legs loops,kernel,sweep]
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

DEV = "cuda"
N, S, MAX_STEPS, BATCH = 3, 25, 200, 256


def spread(xs):
    xs = [float(x) for x in xs]
    return {"median": float(np.median(xs)), "p10": float(np.percentile(xs, 10)), "p90": float(np.percentile(xs, 90)),
            "min": min(xs), "max": max(xs), "samples": xs}


def muzero_kwargs():
    from muzero_hanoi_amd.env import TowersOfHanoi

    return dict(env=TowersOfHanoi(N=N, max_steps=MAX_STEPS), s_space_size=3 * N, n_action=6, discount=0.8,
                dirichlet_alpha=0.25, n_mcts_simulations=S, unroll_n_steps=5, batch_s=BATCH, TD_return=True,
                n_TD_step=10, lr=0.002, buffer_size=50000, priority_replay=True, device=DEV, n_ep_x_loop=1,
                update_impl="fused", ingest="device")


def loops_leg(sizes, loops, blocks, warmup):
    from muzero_hanoi_amd.muzero import Muzero, MuzeroPopulation

    out = []
    for M in sizes:
        seeds = list(range(100, 100 + M))
        pop = MuzeroPopulation(seeds, **muzero_kwargs())
        lone, streams = [], []
        for s in seeds:
            torch.manual_seed(s)
            lone.append(Muzero(selfplay="device", **muzero_kwargs()))
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
        # where a population loop's wall time goes: the launch up to its host read, and the agents' work after it
        split = population_split(pop, loops)
        p, l = spread(rates["population"]), spread(rates["lone"])
        rec = {"M": M, "agent_loops_per_sec": {"population": p, "lone_sequence": l},
               "ratio_of_medians": p["median"] / l["median"],
               "gain_exceeds_both_spreads": p["median"] - l["median"] > max(p["p90"] - p["p10"], l["p90"] - l["p10"]),
               "population_p10_above_lone_p90": p["p10"] > l["p90"],
               "agents_equal_their_lone_runs_afterwards": bool(same),
               "buffer_rows_min": min(len(a.buffer) for a in pop.agents), "population_loop_ms": split}
        print(json.dumps({k: v for k, v in rec.items()}), flush=True)
        out.append(rec)
        del pop, lone
        torch.cuda.empty_cache()
    return {"workload": f"hanoi{N}_s{S}_maxsteps{MAX_STEPS}_batch{BATCH}_unroll5_1ep_1update_per_loop_fused_device_ingest",
            "loops_per_block": loops, "blocks": blocks, "sizes": out}


def population_split(pop, loops):
    """mean wall ms per loop of `loops` more population loops, split at the launch's host read (measured by wrapping
    the two calls; the agents move on, so this runs after the compared blocks)"""
    from muzero_hanoi_amd import selfplay

    acc = {"launch_and_read": 0.0}
    launch = selfplay.BatchedSelfPlay._launch_episodes

    def timed(self, *a, **k):
        t0 = time.perf_counter()
        out = launch(self, *a, **k)
        out["steps"].cpu()  # the wait the loop's own read would take
        acc["launch_and_read"] += time.perf_counter() - t0
        return out

    selfplay.BatchedSelfPlay._launch_episodes = timed
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pop.training_loop(n_loops=loops + 1, min_replay_size=BATCH, print_acc=10 ** 9)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    finally:
        selfplay.BatchedSelfPlay._launch_episodes = launch
    lr = 1e3 * acc["launch_and_read"] / loops
    return {"total": 1e3 * total / loops, "launch_and_read": lr, "per_agent_host_and_updates": 1e3 * total / loops - lr}


def kernel_leg(sizes, reps):
    from muzero_hanoi_amd.engine import Engine, flat_weights
    from muzero_hanoi_amd.networks import MuZeroNet
    from muzero_hanoi_amd import rng

    out = []
    Mmax = max(sizes)
    nets = []
    for m in range(Mmax):
        torch.manual_seed(500 + m)
        nets.append(flat_weights(MuZeroNet(3 * N, 6, 0.002, "cpu", TD_return=True).state_dict()))
    eng = Engine(N, S, Mmax, 33)
    eng.load_weights(nets[0])
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
            moves = fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms.append(e0.elapsed_time(e1))
        return spread(ms), int(moves)

    for M in sizes:
        cols = lambda sl: dict(tie_idx=table[1][:, sl].contiguous(), noise=table[0][:, sl].contiguous(),
                               action_u=table[2][:, sl].contiguous())
        whole, ni = cols(slice(0, M)), torch.arange(M, dtype=torch.int32, device=DEV)
        singles = [cols(slice(m, m + 1)) for m in range(M)]

        last = {}

        def set_form():
            last["steps"] = eng.play_episodes(S, state[:M], MAX_STEPS, net_index=ni, **whole)["steps"]
            return last["steps"].sum()

        def set_form_one_network():  # the set form's code on network 0's weights alone
            last["steps"] = eng.play_episodes(S, state[:M], MAX_STEPS, net_index=torch.zeros_like(ni), **whole)["steps"]
            return last["steps"].sum()

        def one_network():
            last["steps"] = eng.play_episodes(S, state[:M], MAX_STEPS, **whole)["steps"]
            return last["steps"].sum()

        def m_launches():
            each = [eng.play_episodes(S, state[m:m + 1], MAX_STEPS, **singles[m])["steps"] for m in range(M)]
            last["steps"] = torch.cat(each)
            return last["steps"].sum()

        rec = {"M": M}
        for name, fn in (("set_form_M_networks_one_env_each", set_form), ("one_network_B_equals_M", one_network),
                         ("set_form_all_envs_on_network_0", set_form_one_network), ("M_single_env_launches", m_launches)):
            sp, moves = timed(fn)
            rec[name] = {"device_ms": sp, "moves": moves, "longest_episode": int(last["steps"].max())}
        a, b, c = (rec[k]["device_ms"]["median"] for k in ("set_form_M_networks_one_env_each", "one_network_B_equals_M",
                                                             "M_single_env_launches"))
        rec["set_form_minus_one_network_ms"] = a - b
        rec["M_launches_over_set_form"] = c / a
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return {"workload": f"hanoi{N}_s{S}_maxsteps{MAX_STEPS}_untrained", "reps": reps, "sizes": out}


def sweep_leg(episodes, runs):
    import bench_ablation as ba
    from muzero_hanoi_amd.checkpoint import ablation_variants, load_model
    from muzero_hanoi_amd.networks import NetworkSet
    from muzero_hanoi_amd.selfplay import START_STATES, evaluate_networks, state_index

    torch.manual_seed(1)
    nset = NetworkSet([v[1] for v in ablation_variants(load_model(ba.CHECKPOINT))])
    start_idx = np.repeat([state_index(START_STATES[s]) for s in ba.STARTS], episodes)
    kw = dict(start_idx=start_idx, max_steps=ba.MAX_STEPS, temperature=ba.T, dirichlet_alpha=ba.ALPHA)
    from muzero_hanoi_amd import _lib

    def fits(b):  # launch="episodes" runs the latency kernel, whose LDS holds the whole tree
        return _lib.lib().mzh_search_plan_query(33, 2, b, _lib.MZH_FLAG_KERNEL_ONE, 0, 1, _lib.SearchPlan()) == 0

    budgets = [b for b in ba.BUDGETS if fits(b)]
    forms = ("lockstep", "episodes")
    times, errors = {f: [] for f in forms}, {}
    for f in forms:
        evaluate_networks(nset, ba.N, [max(budgets)], launch=f, **kw)  # warm-up
    for r in range(runs):
        for f in (forms if r % 2 == 0 else forms[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = evaluate_networks(nset, ba.N, budgets, launch=f, **kw)
            torch.cuda.synchronize()
            times[f].append(time.perf_counter() - t0)
            errors[f] = [[float(np.mean(e)) for e in r_["errors"]] for r_ in res]
    rec = {"config": {"variants": len(nset), "starts": list(ba.STARTS), "budgets": budgets,
                      "budgets_beyond_the_latency_kernels_lds": [b for b in ba.BUDGETS if not fits(b)], "episodes": episodes,
                      "envs_per_budget": len(nset) * len(start_idx), "temperature": ba.T, "dirichlet_alpha": ba.ALPHA},
           "seconds": {f: spread(times[f]) for f in forms},
           "mean_steps_over_optimal_per_variant_and_budget": errors,
           "note": "temperature 0 without root noise: the two forms differ only in which tie draw an env takes"}
    rec["lockstep_over_episodes"] = rec["seconds"]["lockstep"]["median"] / rec["seconds"]["episodes"]["median"]
    print(json.dumps({k: v for k, v in rec.items() if not k.startswith("mean_steps")}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="loops,kernel,sweep")
    ap.add_argument("--sizes", default="1,2,4,8,16,32")
    ap.add_argument("--loops", type=int, default=10, help="loops of every agent per block")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--episodes", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from muzero_hanoi_amd import _lib

    sizes = [int(x) for x in a.sizes.split(",")]
    rec = {"build_id": _lib.build_id(), "device": torch.cuda.get_device_name(0)}
    if a.out and os.path.exists(a.out):  # legs run one by one add to the record of the same build
        with open(a.out) as f:
            old = json.load(f)
        if old.get("build_id") == rec["build_id"]:
            rec = old
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for leg in a.legs.split(","):
            if leg == "loops":
                rec["training_loops"] = loops_leg(sizes, a.loops, a.blocks, a.warmup)
            elif leg == "kernel":
                rec["kernel_alone"] = kernel_leg(sizes, a.reps)
            elif leg == "sweep":
                rec["ablation_sweep"] = sweep_leg(a.episodes, a.runs)
            else:
                raise SystemExit(f"unknown leg {leg!r}")
            if a.out:  # after every leg: a later leg's failure keeps the earlier ones
                with open(a.out, "w") as f:
                    json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
