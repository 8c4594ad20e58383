"""Plan-ahead acting throughput (acting_experiments/planning_multiple_actions.py) in the script's own
configuration: N = 3, max_steps 30, the ES start, 100 episodes, max_plan_len 7, temperature 0, no root
noise, at the budgets 25 and 1,000 simulations.

Legs, each in episodes/s per budget:
  dropin       acting.plan_multiple_actions on the drop-in MCTS / TowersOfHanoi: the reference's schedule,
               one search and one env.step call at a time
  plan         selfplay.evaluate(max_plan_len=7): the episodes as one batch, per round one search over the
               unfinished envs + one mzh_env_run_plan launch + one host read
  closed_loop  selfplay.evaluate without max_plan_len (a search per step), for context

Every leg runs in a child process of its own under a time limit; the first leg that fails or runs out of
time ends the run.  One record (with the library's build id) is printed and written to --out.

  python tools/bench_plan.py [--out profiles/plan_bench.json] [--budgets 25,1000] [--episodes 100]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("dropin", "plan", "closed_loop")
N, MAX_STEPS, START, L, T, ALPHA = 3, 30, "ES", 7, 0.0, 0.0


def run_leg(leg, n_sims, episodes):
    import numpy as np
    import torch

    from muzero_hanoi_amd import acting
    from muzero_hanoi_amd.env import TowersOfHanoi
    from muzero_hanoi_amd.mcts import MCTS
    from muzero_hanoi_amd.networks import MuZeroNet
    from muzero_hanoi_amd.selfplay import evaluate

    torch.manual_seed(1)
    net = MuZeroNet(3 * N, 6, 0.002, "cuda", TD_return=True).to("cuda")
    np.random.seed(1)
    if leg == "dropin":
        env = TowersOfHanoi(N=N, max_steps=MAX_STEPS)
        acting.get_starting_state(env, 0)
        mcts = MCTS(discount=0.8, root_dirichlet_alpha=ALPHA, n_simulations=n_sims, batch_s=1, device="cpu")
        run = lambda eps: acting.plan_multiple_actions(env, 0, net, mcts, eps, [n_sims], T, max_plan_len=L)
        warm = 2
    else:
        kw = dict(max_plan_len=L) if leg == "plan" else {}
        run = lambda eps: evaluate(net, N, [n_sims], episodes=eps, start=START, max_steps=MAX_STEPS, temperature=T,
                                   dirichlet_alpha=ALPHA, **kw)["data"]
        warm = episodes
    run(warm)  # warm-up: engine, weights, staging buffers
    torch.cuda.synchronize()
    # the run of `episodes` episodes repeated (each ending in a synchronise) until 2 s of timed work, 3 to 50 times
    times = []
    while len(times) < 3 or (sum(times) < 2.0 and len(times) < 50):
        t0 = time.perf_counter()
        data = run(episodes)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    dt = float(np.median(times))
    return {"leg": leg, "n_sims": n_sims, "episodes": episodes, "seconds": dt, "episodes_per_sec": episodes / dt,
            "runs": len(times), "seconds_min": min(times), "seconds_max": max(times),
            "seconds_what": "median over `runs` repetitions of the whole leg, host clock ending in a synchronise",
            "mean_steps_over_optimal": data[0][1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--budgets", default="25,1000")
    ap.add_argument("--episodes", type=int, default=100)
    ap.add_argument("--leg-seconds", type=float, default=240.0, help="time limit of one leg's child process")
    ap.add_argument("--leg", choices=LEGS, help="(child) run one leg and print its record")
    ap.add_argument("--n-sims", type=int)
    a = ap.parse_args()
    if a.leg:
        print("LEG " + json.dumps(run_leg(a.leg, a.n_sims, a.episodes)), flush=True)
        return 0
    from muzero_hanoi_amd import _lib

    rec = {"build_id": _lib.build_id(), "legs": [],
           "config": {"workload": f"hanoi{N}_maxsteps{MAX_STEPS}_start{START}", "episodes": a.episodes,
                      "max_plan_len": L, "temperature": T, "dirichlet_alpha": ALPHA, "deterministic": False,
                      "network": "random-init MuZeroNet(TD_return=True), torch seed 1"}}
    status = 0
    for n_sims in (int(x) for x in a.budgets.split(",")):
        for leg in LEGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--n-sims", str(n_sims), "--episodes",
                   str(a.episodes)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_seconds)
            except subprocess.TimeoutExpired:
                print(f"leg {leg} at {n_sims} simulations ran out of time: stopping", file=sys.stderr)
                status = 124
                break
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
            if r.returncode != 0 or not line:
                print(f"leg {leg} at {n_sims} simulations failed ({r.returncode}): stopping\n{r.stderr[-2000:]}",
                      file=sys.stderr)
                status = r.returncode or 1
                break
            rec["legs"].append(json.loads(line[-1][4:]))
            print(json.dumps(rec["legs"][-1]), flush=True)
        if status:
            break
    rec["complete"] = status == 0
    by = {(r["leg"], r["n_sims"]): r["episodes_per_sec"] for r in rec["legs"]}
    rec["plan_over_dropin"] = {str(n): by[("plan", n)] / by[("dropin", n)]
                               for (leg, n) in by if leg == "plan" and ("dropin", n) in by}
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return status


if __name__ == "__main__":
    sys.exit(main())
