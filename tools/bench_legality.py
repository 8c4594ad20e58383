"""legal_illegal_preds.py's workload in its own default shape, and the time of the kernel behind it.

  workload  N = 3, 25 simulations, at most 200 steps, 3 networks (the checkpoint, its policy-ablated and its
            value-ablated copy) x 100 episodes from random non-goal starts = 300 episodes

Legs:
  batched   selfplay.evaluate_legality: the 300 episodes as one batch, per move one mzh_search_multi over the
            unfinished rows + one mzh_probe_actions on the same rows + one env step + one host read (episodes/s)
  dropin    acting.legality_evaluate_network on the drop-in MCTS / TowersOfHanoi, network after network: the
            reference's schedule, per decision one search, one probe of one row and one env.step (episodes/s;
            the whole workload once, after a one-episode warm-up)
  kernel    mzh_probe_actions alone against what it fuses -- one mzh_initial_inference + six
            mzh_recurrent_inference on the same rows, the only path before the probe existed -- at n = 300 and
            n = 65,536 rows of 4 discs, interleaved A B B A per round (A = the seven calls, B = the probe) as
            tools/abba.py interleaves two builds: per leg the median of 20 calls, device events around each call;
            and, at the workload's own shape (300 rows of 3 discs, the set of 3 networks), the probe next to the
            mzh_search_multi launch it accompanies in a move

The network is the reference-written checkpoint tests/golden/muzero_model_N3.pt (the 4-disc kernel legs: a
MuZeroNet of torch seed 0).  Every leg runs in a child process of its own under a time limit; the first leg that
fails or runs out of time ends the run.  One record (with the library's build id) is printed and written to --out.

  python tools/bench_legality.py [--out profiles/legality_bench.json] [--legs batched,kernel]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("batched", "dropin", "kernel")
N, S, MAX_STEPS, EPISODES = 3, 25, 200, 100
KERNEL_ROWS, KERNEL_DISKS, ROUNDS, CALLS = (300, 65536), 4, 4, 20


def _networks():
    import torch

    from muzero_hanoi_amd import acting
    from muzero_hanoi_amd.checkpoint import load_model

    net = load_model(os.path.join(ROOT, "tests", "golden", "muzero_model_N3.pt"), load_optimiser=False)
    torch.manual_seed(1)
    return [net, acting.ablate_network(net, ablate_policy=True), acting.ablate_network(net, ablate_value=True)]


def run_batched():
    import numpy as np
    import torch

    from muzero_hanoi_amd.selfplay import evaluate_legality

    nets = _networks()
    run = lambda: evaluate_legality(nets, N, episodes=EPISODES, n_sims=S, max_steps=MAX_STEPS, seed=1)
    run()  # warm-up: engine, weight set, code objects
    torch.cuda.synchronize()
    times, out = [], None
    while len(times) < 3 or (sum(times) < 2.0 and len(times) < 50):
        t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    dt = float(np.median(times))
    games = len(nets) * EPISODES
    return {"leg": "batched", "episodes": games, "seconds": dt, "episodes_per_sec": games / dt, "runs": len(times),
            "seconds_min": min(times), "seconds_max": max(times), "moves": int(max(d["steps"].max() for d in out)),
            "decisions": int(sum(d["steps"].sum() for d in out)),
            "seconds_what": "median over `runs` repetitions of the whole leg, host clock ending in a synchronise",
            "results": [{k: v for k, v in d.items() if k != "steps"} for d in out]}


def run_dropin():
    import numpy as np
    import torch

    from muzero_hanoi_amd import acting
    from muzero_hanoi_amd.env import TowersOfHanoi
    from muzero_hanoi_amd.mcts import MCTS

    nets = _networks()
    env = TowersOfHanoi(N=N, max_steps=MAX_STEPS)
    mcts = MCTS(discount=0.8, root_dirichlet_alpha=0.25, n_simulations=S, batch_s=1, device="cpu")
    np.random.seed(1)
    for net in nets:  # warm-up: engines, weights, staging buffers
        acting.legality_evaluate_network(env, mcts, net, 1, "cuda")
    torch.cuda.synchronize()
    trace = []
    t0 = time.perf_counter()
    out = [acting.legality_evaluate_network(env, mcts, net, EPISODES, "cuda", trace=trace) for net in nets]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    games = len(nets) * EPISODES
    return {"leg": "dropin", "episodes": games, "seconds": dt, "episodes_per_sec": games / dt, "runs": 1,
            "decisions": len(trace), "seconds_per_decision": dt / len(trace),
            "seconds_what": "the whole workload once, host clock ending in a synchronise", "results": out}


def _median_ms(call):
    import numpy as np
    import torch

    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
    for s, e in ev:
        s.record()
        call()
        e.record()
    torch.cuda.synchronize()
    return float(np.median([s.elapsed_time(e) for s, e in ev]))


def _stats(x):
    import numpy as np

    x = np.asarray(x)
    return {"ms": [float(v) for v in x], "median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()),
            "spread": float(x.max() - x.min())}


def run_kernel():
    import numpy as np
    import torch

    from muzero_hanoi_amd import engine
    from muzero_hanoi_amd.networks import MuZeroNet

    dev = "cuda"
    torch.manual_seed(0)
    flat = engine.flat_weights(MuZeroNet(3 * KERNEL_DISKS, 6, 0.002, "cpu", TD_return=True).state_dict())
    sizes = []
    for n in KERNEL_ROWS:
        eng = engine.Engine(KERNEL_DISKS, 1, n, 33)
        eng.load_weights(flat)
        st = torch.randint(0, 3, (n, KERNEL_DISKS), dtype=torch.uint8, device=dev)
        obs = engine.encode_obs(KERNEL_DISKS, st)
        acts = [torch.full((n,), a, dtype=torch.int32, device=dev) for a in range(6)]

        def seven():
            h = eng.initial_inference(obs)["h"]
            return [eng.recurrent_inference(h, a) for a in acts]

        probe = lambda: eng.probe_actions(obs, state=st)
        full = lambda: eng.probe_actions(obs, state=st, full=True)
        want = seven()
        got = full()
        same = all(torch.equal(got["reward"][:, a], want[a]["reward"]) and torch.equal(got["value"][:, a], want[a]["value"])
                   and torch.equal(got["h1"][:, a], want[a]["h"]) for a in range(6))
        for f in (seven, probe, full):  # warm-up of every timed shape
            f()
        torch.cuda.synchronize()
        ms = {"seven_calls": [], "probe": [], "probe_full": []}
        for _ in range(ROUNDS):
            for name, f in (("seven_calls", seven), ("probe", probe), ("probe_full", full), ("probe_full", full),
                            ("probe", probe), ("seven_calls", seven)):
                ms[name].append(_median_ms(f))
        a, b, c = (_stats(ms[k]) for k in ("seven_calls", "probe", "probe_full"))
        sizes.append({"rows": n, "disks": KERNEL_DISKS, "outputs_bit_identical": bool(same), "seven_calls": a, "probe": b,
                      "probe_full": c, "probe_over_seven_calls": b["median"] / a["median"],
                      "probe_full_over_seven_calls": c["median"] / a["median"],
                      "probe_slower_beyond_spread": b["median"] - a["median"] > max(a["spread"], b["spread"]),
                      "probe_full_slower_beyond_spread": c["median"] - a["median"] > max(a["spread"], c["spread"])})
        eng.close()
    # the probe next to the search of the same move, at the workload's shape
    from muzero_hanoi_amd import rng as mrng
    from muzero_hanoi_amd.networks import NetworkSet, engine_for_set

    B = 3 * EPISODES
    eng = engine_for_set(NetworkSet(_networks()), S, B)
    st = torch.randint(0, 3, (B, N), dtype=torch.uint8, device=dev)
    st[st.sum(1) == 2 * N] = 0
    obs = engine.encode_obs(N, st)
    ni = torch.arange(B, dtype=torch.int32, device=dev) // EPISODES
    noise, tie, u = (torch.as_tensor(x).to(dev) for x in mrng.synthetic_draws(B, deterministic=False, alpha=0.25, seed=1))
    search = lambda: eng.search_multi(S, net_index=ni, obs=obs, tie_idx=tie, noise=noise, action_u=u, temperature=0.0)
    probe = lambda: eng.probe_actions(obs, state=st, net_index=ni)
    for f in (search, probe):
        f()
    torch.cuda.synchronize()
    ms = {"search": [], "probe": []}
    for _ in range(ROUNDS):
        for name, f in (("search", search), ("probe", probe), ("probe", probe), ("search", search)):
            ms[name].append(_median_ms(f))
    s_, p_ = _stats(ms["search"]), _stats(ms["probe"])
    move = {"rows": B, "disks": N, "n_sims": S, "networks": 3, "search_multi": s_, "probe_multi": p_,
            "probe_share_of_search_plus_probe": p_["median"] / (p_["median"] + s_["median"])}
    return {"leg": "kernel", "rounds": ROUNDS, "calls_per_leg": CALLS,
            "order": "A B B A per round; a leg = the median of `calls_per_leg` calls, device events around each call "
                     "(host launch gaps between the seven calls included: they are part of that path)",
            "sizes": sizes, "move": move}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--leg-seconds", type=float, default=300.0, help="time limit of one leg's child process")
    ap.add_argument("--leg", choices=LEGS, help="(child) run one leg and print its record")
    a = ap.parse_args()
    if a.leg:
        print("LEG " + json.dumps({"batched": run_batched, "dropin": run_dropin, "kernel": run_kernel}[a.leg]()), flush=True)
        return 0
    from muzero_hanoi_amd import _lib

    rec = {"build_id": _lib.build_id(), "legs": [],
           "config": {"workload": f"hanoi{N}_sims{S}_maxsteps{MAX_STEPS}", "networks": 3, "episodes_per_network": EPISODES,
                      "temperature": 0.0, "deterministic": False, "dirichlet_alpha": 0.25,
                      "network": "tests/golden/muzero_model_N3.pt (reference-written checkpoint)"}}
    status = 0
    for leg in a.legs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_seconds)
        except subprocess.TimeoutExpired:
            print(f"leg {leg} ran out of time: stopping", file=sys.stderr)
            status = 124
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
        if r.returncode != 0 or not line:
            print(f"leg {leg} failed ({r.returncode}): stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            status = r.returncode or 1
            break
        rec["legs"].append(json.loads(line[-1][4:]))
        print(json.dumps(rec["legs"][-1]), flush=True)
    rec["complete"] = status == 0 and a.legs == ",".join(LEGS)
    by = {r["leg"]: r["episodes_per_sec"] for r in rec["legs"] if "episodes_per_sec" in r}
    if "batched" in by and "dropin" in by:
        rec["batched_over_dropin"] = by["batched"] / by["dropin"]
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
