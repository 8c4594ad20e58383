"""Perturbed-observation acting throughput in the two scripts' own default workloads, and the time of the
kernel behind them.

  noise     noise_injection_comparison.py: N = 3, 25 simulations, at most 50 steps, 8 noise levels
            (0, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6) x 100 random non-goal starts = 800 games
  permute   permutation_importance.py: the same search, 3 networks (base, policy head re-initialised, value
            head re-initialised) x (baseline + 3 permuted discs) x its 12 test states = 144 games

Legs, each in games/s:
  <workload>_batched  selfplay.evaluate_perturbed: every game of the workload in one batch, per move one search
                      over the unfinished envs + one mzh_env_step_observe launch + one host read
  <workload>_dropin   acting.noise_run_evaluation / permutation_run_evaluation on the drop-in MCTS /
                      TowersOfHanoi: the reference's schedule, one search and one env.step call at a time
  kernel              mzh_env_step_observe alone at 2^20 envs of 4 discs (tools/bench_env.py's shape) with a
                      permuted disc and noise on every env, without either, and mzh_env_step next to them:
                      device events around each launch, median of 50

The network is the reference-written checkpoint tests/golden/muzero_model_N3.pt.  Every leg runs in a child
process of its own under a time limit; the first leg that fails or runs out of time ends the run.  One record
(with the library's build id) is printed and written to --out.

  python tools/bench_perturb.py [--out profiles/perturb_bench.json] [--legs noise_batched,kernel]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("noise_batched", "noise_dropin", "permute_batched", "permute_dropin", "kernel")
N, S, MAX_STEPS = 3, 25, 50
NOISE_STDS = [0.0, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6]  # noise_injection_comparison.py:64
NUM_STATES = 100  # noise_injection_comparison.py:70
TEST_STATES = [(0, 0, 0), (1, 1, 1), (0, 1, 2), (2, 1, 0), (0, 0, 1), (1, 0, 0), (2, 2, 0), (1, 2, 1), (0, 2, 2),
               (2, 0, 1), (1, 1, 0), (0, 2, 1)]  # permutation_importance.py:143-156
KERNEL_ENVS, KERNEL_DISKS = 1 << 20, 4


def _timed(run):
    """the whole leg repeated (each run ending in a synchronise) until 2 s of timed work, 3 to 50 times"""
    import torch

    run()  # warm-up: engine, weights, staging buffers
    torch.cuda.synchronize()
    times, out = [], None
    while len(times) < 3 or (sum(times) < 2.0 and len(times) < 50):
        t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times, out


def _networks(workload):
    import torch

    from muzero_hanoi_amd import acting
    from muzero_hanoi_amd.checkpoint import load_model

    net = load_model(os.path.join(ROOT, "tests", "golden", "muzero_model_N3.pt"), load_optimiser=False)
    if workload == "noise":
        return [net]
    torch.manual_seed(1)
    return [net, acting.get_ablated_network(net, ablate_policy=True), acting.get_ablated_network(net, ablate_value=True)]


def run_games(leg):
    import numpy as np

    from muzero_hanoi_amd import acting
    from muzero_hanoi_amd.env import TowersOfHanoi
    from muzero_hanoi_amd.mcts import MCTS
    from muzero_hanoi_amd.selfplay import _batch_starts, evaluate_perturbed, index_state

    workload, form = leg.split("_")
    nets = _networks(workload)
    if workload == "noise":
        conditions = [("noise", s) for s in NOISE_STDS]
        starts = [index_state(int(i), N) for i in _batch_starts(N, NUM_STATES, None, None, 1, 2)]
    else:
        conditions = [("baseline",)] + [("permute", d) for d in range(N)]
        starts = TEST_STATES
    games = len(nets) * len(conditions) * len(starts)
    if form == "batched":
        run = lambda: evaluate_perturbed(nets, N, conditions=conditions, starts=starts, n_sims=S, max_steps=MAX_STEPS,
                                         seed=1)["solve_rate"]
    else:
        env = TowersOfHanoi(N=N, max_steps=MAX_STEPS)
        mcts = MCTS(discount=0.8, root_dirichlet_alpha=0.25, n_simulations=S, batch_s=1, device="cpu")

        def run():
            np.random.seed(1)
            rates = np.zeros((len(nets), len(conditions)))
            for m, net in enumerate(nets):
                for c, cond in enumerate(conditions):
                    if workload == "noise":
                        rates[m, c] = acting.noise_run_evaluation(net, env, starts, MAX_STEPS, mcts, noise_std=cond[1])
                    else:
                        rates[m, c] = acting.permutation_run_evaluation(
                            net, env, starts, MAX_STEPS, mcts, permute_feature=cond[1] if len(cond) > 1 else None)
            return rates

    times, rates = _timed(run)
    dt = float(np.median(times))
    return {"leg": leg, "games": games, "networks": len(nets), "conditions": [list(c) for c in conditions],
            "starts": len(starts), "seconds": dt, "games_per_sec": games / dt, "runs": len(times),
            "seconds_min": min(times), "seconds_max": max(times),
            "seconds_what": "median over `runs` repetitions of the whole leg, host clock ending in a synchronise",
            "solve_rate": np.asarray(rates).tolist()}


def run_kernel():
    import numpy as np
    import torch

    from muzero_hanoi_amd.env import HanoiBatch

    B, n, reps = KERNEL_ENVS, KERNEL_DISKS, 50
    env = HanoiBatch(n, 200, B)
    dev = env.device
    acts = torch.randint(0, 6, (reps, B), dtype=torch.int32, device=dev)
    idx = torch.arange(B, dtype=torch.int32, device=dev)
    peg = torch.randint(0, 3, (B,), dtype=torch.int32, device=dev)
    noise = 0.3 * torch.randn((B, 3 * n), dtype=torch.float64, device=dev)

    def median_launch(step):
        env.reset(torch.zeros(B, dtype=torch.int64))
        step(0)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for k in range(reps):
            ev[k][0].record()
            step(k)
            ev[k][1].record()
            env.active.fill_(1)  # finished episodes continue (a reset without a host round trip)
        torch.cuda.synchronize()
        return float(np.median([s.elapsed_time(e) for s, e in ev])) * 1e-3

    def perturbed(k):
        if env.perm_disc is None:
            env.set_perturbation(torch.randint(0, n, (B,), dtype=torch.int32, device=dev))
        env.step_observe(acts[k], idx, perm_peg=peg, noise=noise)

    # bytes a row moves: state read + write, action, env index, counter and the two sums read + write, active read +
    # write, solved, reward, done, the observation; with the perturbation its disc, peg and 3n float64 of noise
    plain_bytes = 2 * n + 4 + 4 + 3 * 8 + 2 + 1 + 2 + 12 * n
    rows = []
    for name, step, nbytes in (
            ("step_observe_perturbed", perturbed, plain_bytes + 8 + 24 * n),
            ("step_observe_plain", lambda k: env.step_observe(acts[k], idx), plain_bytes),
            ("env_step", lambda k: env.step(acts[k]), 2 * n + 4 + 3 + 4 + 12 * n)):
        t = median_launch(step)
        rows.append({"kernel": name, "s_per_launch": t, "steps_per_s": B / t, "gbps": B * nbytes / t / 1e9,
                     "bytes_per_row": nbytes})
    return {"leg": "kernel", "envs": B, "disks": n, "launches": reps,
            "seconds_what": "median of device events around one launch", "kernels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--leg-seconds", type=float, default=240.0, help="time limit of one leg's child process")
    ap.add_argument("--leg", choices=LEGS, help="(child) run one leg and print its record")
    a = ap.parse_args()
    if a.leg:
        print("LEG " + json.dumps(run_kernel() if a.leg == "kernel" else run_games(a.leg)), flush=True)
        return 0
    from muzero_hanoi_amd import _lib

    rec = {"build_id": _lib.build_id(), "legs": [],
           "config": {"workload": f"hanoi{N}_sims{S}_maxsteps{MAX_STEPS}", "temperature": 0.0, "deterministic": True,
                      "dirichlet_alpha": 0.25, "network": "tests/golden/muzero_model_N3.pt (reference-written checkpoint)"}}
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
    by = {r["leg"]: r["games_per_sec"] for r in rec["legs"] if "games_per_sec" in r}
    rec["batched_over_dropin"] = {w: by[f"{w}_batched"] / by[f"{w}_dropin"] for w in ("noise", "permute")
                                  if f"{w}_batched" in by and f"{w}_dropin" in by}
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return status


if __name__ == "__main__":
    sys.exit(main())
