"""MuzeroPopulation(update="set") -- the agents' update rounds as one launch sequence (mzh_train_set_update) --
against update="each", the per-agent draws, updates and write-backs that existed.

Workload: tools/bench_population.py's -- N = 3, S = 25, max_steps = 200, the reference's
TrainingConfig (batch 256, unroll 5, buffer 50,000, one episode and one update per loop), fused update, device
ingest, selfplay="device".

Legs (--legs, default all):
  loops     (a) whole training loops.  For M = --sizes: a population with update="set" against one with
            update="each", built from the same seeds and run in alternated blocks of the same loops, so every
            block pair is the same work (a "set" agent ends bit for bit as its "each" twin, checked afterwards).
            Agent-loops/s of each side as median with p10..p90 over the blocks, and whether "set"'s p10 lies above
            "each"'s p90 (the rule for the default).
  baseline  (b) "each" is the code path tools/bench_population.py measures as its population side, and that tool
            is unchanged: one run of its loops leg at M = 8, and whether its median lies inside "each"'s p10..p90.
  device    (c) device time from events: the four launches of one mzh_train_set_update over M networks against M
            times mzh_replay_sample + mzh_train_update + mzh_replay_set_priorities (four launches each) issued
            back to back without a synchronisation, on the same buffers.
  split     (d) where the host time of a "set" loop goes, per agent: the ingest with its read, staging (uniforms and
            Adam scalars), the stream bookkeeping and the rest; per loop: the episode launch to its read and the
            set's rounds with their one synchronisation.

  python tools/bench_population_update.py [--out profiles/population_update_bench.json] [--legs ...] [--sizes ...]
"""
import argparse
import ctypes
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

from bench_population import BATCH, muzero_kwargs, spread  # noqa: E402  (the same workload and statistics)


def build(M, update):
    from muzero_hanoi_amd.muzero import MuzeroPopulation

    return MuzeroPopulation(list(range(100, 100 + M)), update=update, **muzero_kwargs())


def run(pop, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pop.training_loop(n_loops=n + 1, min_replay_size=BATCH, print_acc=10 ** 9)
    torch.cuda.synchronize()
    return len(pop.agents) * n / (time.perf_counter() - t0)


def warm(pops, warmup):
    for _ in range(20):  # fill every buffer past the batch, build every workspace
        for p in pops:
            run(p, warmup)
        if min(len(a.buffer) for p in pops for a in p.agents) > 2 * BATCH:
            return
    raise SystemExit("a buffer stayed below two batches")


def twins_equal(x, y):
    return all(len(a.buffer) == len(b.buffer) and a.buffer.ptr == b.buffer.ptr
               and all(torch.equal(p, q) for p, q in zip(a.networks.parameters(), b.networks.parameters()))
               and bool(torch.equal(a.buffer._prio, b.buffer._prio))
               for a, b in zip(x.agents, y.agents))


def device_leg(pop, reps):
    """(c) on a warmed "set" population's own handle and buffers (the agents move on: run after the comparison)"""
    from muzero_hanoi_amd import _lib

    su, L = pop._set_update, _lib.lib()
    M, B = su.M, su.B
    stream = _lib.stream_handle(su.dev)
    su.begin_loop()
    for m, a in enumerate(pop.agents):
        su.step_np[0, m] = (1, len(a.buffer), 0.002, 1.0)
        su.u_np[0, m] = np.random.default_rng(m).random(B)

    def set_form():
        _lib.check(L.mzh_train_set_update(su.handle, su.step_dev, su.u_dev, su.status_dev, stream), "set")

    def singles():
        for m, a in enumerate(pop.agents):
            d, t = su._draw[m], su._train[m]
            d.n, d.u, d.status = len(a.buffer), su.u_dev + m * B * 8, su.status_dev + m * 16
            t.step_size, t.bc2_sqrt = 0.002, 1.0
            _lib.check(L.mzh_replay_sample(ctypes.byref(d), stream), "draw")
            _lib.check(L.mzh_train_update(ctypes.byref(t), stream), "update")
            _lib.check(L.mzh_replay_set_priorities(d.prio, a.buffer.size, d.indx, t.new_prio, B,
                                                   su.status_dev + m * 16 + 8, stream), "write-back")

    def timed(fn):
        ms = []
        for i in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms.append(e0.elapsed_time(e1))
        return spread(ms)

    a, b = timed(set_form), timed(singles)
    return {"set_four_launches_ms": a, "M_times_four_single_launches_ms": b, "singles_over_set": b["median"] / a["median"]}


def split_leg(pop, loops):
    """(d) wall time of `loops` more "set" loops, by wrapping the calls (the agents move on: run last)"""
    from muzero_hanoi_amd import muzero, selfplay

    acc = {"launch_and_read": 0.0, "ingest_with_read": 0.0, "stage": 0.0, "rounds_and_sync": 0.0}
    orig = (selfplay.BatchedSelfPlay._launch_episodes, muzero.Muzero._games_played, muzero.SetUpdate.stage,
            muzero.SetUpdate.run)

    def wrap(fn, key, after=None):
        def timed(*a, **k):
            t0 = time.perf_counter()
            out = fn(*a, **k)
            if after:
                after(out)
            acc[key] += time.perf_counter() - t0
            return out
        return timed

    selfplay.BatchedSelfPlay._launch_episodes = wrap(orig[0], "launch_and_read", lambda out: out["steps"].cpu())
    muzero.Muzero._games_played = wrap(orig[1], "ingest_with_read")
    muzero.SetUpdate.stage = wrap(orig[2], "stage")
    muzero.SetUpdate.run = wrap(orig[3], "rounds_and_sync")
    try:
        t0 = time.perf_counter()
        run(pop, loops)
        total = time.perf_counter() - t0
    finally:
        (selfplay.BatchedSelfPlay._launch_episodes, muzero.Muzero._games_played, muzero.SetUpdate.stage,
         muzero.SetUpdate.run) = orig
    M = len(pop.agents)
    per_loop = {k: 1e3 * v / loops for k, v in acc.items()}
    rest = 1e3 * total / loops - sum(per_loop.values())
    return {"loop_ms": 1e3 * total / loops, "episode_launch_to_its_read_ms": per_loop["launch_and_read"],
            "set_rounds_and_the_one_sync_ms": per_loop["rounds_and_sync"],
            "per_agent_ms": {"ingest_with_its_read": per_loop["ingest_with_read"] / M, "stage": per_loop["stage"] / M,
                             "stream_bookkeeping_and_rest": rest / M}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="loops,baseline,device,split")
    ap.add_argument("--sizes", default="1,2,4,8,16,32")
    ap.add_argument("--loops", type=int, default=10, help="loops of every agent per block")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from muzero_hanoi_amd import _lib

    legs = a.legs.split(",")
    rec = {"build_id": _lib.build_id(), "device": torch.cuda.get_device_name(0),
           "workload": f"bench_population.py's: batch {BATCH}, one episode and one update per loop, fused, device ingest",
           "loops_per_block": a.loops, "blocks": a.blocks, "sizes": []}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for M in (int(x) for x in a.sizes.split(",")):
            pops = {"set": build(M, "set"), "each": build(M, "each")}
            warm(pops.values(), a.warmup)
            r = {"M": M}
            if "loops" in legs:
                rates = {"set": [], "each": []}
                for b in range(a.blocks):
                    for side in (("set", "each") if b % 2 == 0 else ("each", "set")):
                        rates[side].append(run(pops[side], a.loops))
                s, e = spread(rates["set"]), spread(rates["each"])
                r.update(agent_loops_per_sec={"set": s, "each": e}, ratio_of_medians=s["median"] / e["median"],
                         set_p10_above_each_p90=s["p10"] > e["p90"],
                         agents_equal_their_twins_afterwards=bool(twins_equal(pops["set"], pops["each"])))
            if "baseline" in legs and M == 8 and "agent_loops_per_sec" in r:
                import bench_population as bp

                base = bp.loops_leg([8], a.loops, a.blocks, a.warmup)["sizes"][0]["agent_loops_per_sec"]["population"]
                e = r["agent_loops_per_sec"]["each"]
                r["bench_population_py_M8"] = {"population_agent_loops_per_sec": base,
                                               "median_inside_each_p10_p90": e["p10"] <= base["median"] <= e["p90"]}
            if "device" in legs:
                r["device_time"] = device_leg(pops["set"], a.reps)
            if "split" in legs:
                r["set_loop_host_split"] = split_leg(pops["set"], a.loops)
            print(json.dumps(r), flush=True)
            rec["sizes"].append(r)
            del pops
            torch.cuda.empty_cache()
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(rec, f, indent=1)
    if "loops" in legs:
        big = [r for r in rec["sizes"] if r["M"] >= 2]
        rec["set_p10_above_each_p90_at_every_M_from_2"] = bool(big) and all(r["set_p10_above_each_p90"] for r in big)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
