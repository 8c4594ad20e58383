"""The reference's ablation sweep (acting_experiments/acting_ablations.py run once per variant by the
run_*_ablations*.sh family) on its checkpoint tests/golden/muzero_model_N3.pt: the 8 head re-initialisations
(checkpoint.ablation_variants, torch seed 1) x the ES / MS / LS starts x the budgets 5, 10, 30, 50, 80, 110, 150
x 100 episodes, temperature 0, no root noise, max_steps 200 -- 16,800 episodes.

Forms, each timed in a child process of its own (host clock ending in a synchronise, median of --runs sweeps):
  loop   what exists without network sets: selfplay.evaluate per variant and start (24 calls), each budget a
         batch of 100 envs of one network
  set    selfplay.evaluate_networks: per budget ONE batch of 8 networks x 300 envs (the three starts, 100
         episodes each), searched by one mzh_search_multi launch per move

  fused  selfplay.evaluate_networks(budgets="fused"): ONE batch of 8 networks x 7 budgets x 300 envs, every env
         searching with its own budget in one mzh_search_multi_budget launch per move

The forms give their envs different synthetic tie draws, so their scores agree statistically, not bit
for bit (tests/test_multi_gpu.py checks evaluate_networks against the oracle, tests/test_budget_gpu.py the fused
search against the per-budget one).  One record (with the library's build id and the kernel each form's first
move launches per budget) is printed and written to --out.

  python tools/bench_ablation.py [--out profiles/ablation_sweep_bench.json] [--episodes 100] [--runs 5]
                                 [--forms loop,set]   (default; fused is run when named)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("loop", "set", "fused")
DEFAULT_FORMS = "loop,set"
N, MAX_STEPS, T, ALPHA = 3, 200, 0.0, 0.0
STARTS = ("ES", "MS", "LS")
BUDGETS = (5, 10, 30, 50, 80, 110, 150)
CHECKPOINT = os.path.join(ROOT, "tests", "golden", "muzero_model_N3.pt")


def run_form(form, episodes, runs, budgets):
    import numpy as np
    import torch

    from muzero_hanoi_amd import _lib
    from muzero_hanoi_amd.checkpoint import ablation_variants, load_model
    from muzero_hanoi_amd.networks import NetworkSet, engine_for_set
    from muzero_hanoi_amd.selfplay import START_STATES, evaluate, evaluate_networks, state_index

    torch.manual_seed(1)
    variants = ablation_variants(load_model(CHECKPOINT))
    labels, nets = [v[0] for v in variants], [v[1] for v in variants]
    kw = dict(max_steps=MAX_STEPS, temperature=T, dirichlet_alpha=ALPHA)
    if form == "loop":
        def sweep(bs):
            return {lb: {s: evaluate(net, N, bs, episodes=episodes, start=s, **kw)["data"] for s in STARTS}
                    for lb, net in zip(labels, nets)}

        plans = {str(b): _lib.search_plan(33, episodes, b, minmax_in=True)["kernel"] for b in budgets}
    else:
        nset = NetworkSet(nets)
        start_idx = np.repeat([state_index(START_STATES[s]) for s in STARTS], episodes)

        def sweep(bs):
            res = evaluate_networks(nset, N, bs, start_idx=start_idx, budgets="fused" if form == "fused" else "each", **kw)
            # evaluate's "data" per start: the mean error over that start's episodes
            return {lb: {s: [[int(b), float(np.mean(r["errors"][i][j * episodes:(j + 1) * episodes]))]
                             for i, b in enumerate(bs)] for j, s in enumerate(STARTS)}
                    for lb, r in zip(labels, res)}

        B = len(nets) * len(start_idx) * (len(budgets) if form == "fused" else 1)
        eng = engine_for_set(nset, max(budgets), B)
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=eng.device)
        ni = torch.arange(len(nets), device=eng.device).repeat_interleave(B // len(nets))
        if form == "fused":  # the one launch of the first move: every budget abreast
            sims = torch.tensor(budgets, dtype=torch.int32, device=eng.device).repeat_interleave(len(start_idx)).repeat(len(nets))
            o = eng.search_multi(max(budgets), net_index=ni, sims=sims, max_runs=len(nets) * len(budgets),
                                 obs=z(B, 3 * N), tie_idx=z(B, dt=torch.int32), deterministic=True)
            plans = {"all": o["_plan"]["kernel"], "workgroups": o["_plan"]["workgroups"], "tiles": int(o["_status"][1])}
        else:
            plans = {str(b): eng.search_multi(b, net_index=ni, obs=z(B, 3 * N), tie_idx=z(B, dt=torch.int32),
                                              deterministic=True)["_plan"]["kernel"] for b in budgets}
    # warm-up: every engine at its final capacity, weights, staging buffers
    sweep(list(budgets) if form == "fused" else [max(budgets)])
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        data = sweep(list(budgets))
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    n_ep = len(nets) * len(STARTS) * len(budgets) * episodes
    dt = float(np.median(times))
    return {"form": form, "seconds": dt, "seconds_min": min(times), "seconds_max": max(times), "runs": runs,
            "seconds_what": "median over `runs` whole sweeps, host clock ending in a synchronise",
            "episodes": n_ep, "episodes_per_sec": n_ep / dt, "kernels_first_move": plans,
            "mean_steps_over_optimal": data}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--episodes", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--budgets", default=",".join(map(str, BUDGETS)))
    ap.add_argument("--form-seconds", type=float, default=540.0, help="time limit of one form's child process")
    ap.add_argument("--forms", default=DEFAULT_FORMS, help="the forms to time, in order (of loop, set, fused)")
    ap.add_argument("--form", choices=FORMS, help="(child) run one form and print its record")
    a = ap.parse_args()
    budgets = tuple(int(x) for x in a.budgets.split(","))
    if a.form:
        print("FORM " + json.dumps(run_form(a.form, a.episodes, a.runs, budgets)), flush=True)
        return 0
    from muzero_hanoi_amd import _lib

    rec = {"build_id": _lib.build_id(), "forms": [],
           "config": {"workload": f"hanoi{N}_maxsteps{MAX_STEPS}", "checkpoint": os.path.relpath(CHECKPOINT, ROOT),
                      "variants": 8, "variant_seed": 1, "starts": list(STARTS), "budgets": list(budgets),
                      "episodes": a.episodes, "temperature": T, "dirichlet_alpha": ALPHA, "deterministic": False}}
    status = 0
    forms = [f for f in a.forms.split(",") if f]
    if any(f not in FORMS for f in forms):
        ap.error(f"--forms takes a comma-separated list of {FORMS}")
    for form in forms:
        cmd = [sys.executable, os.path.abspath(__file__), "--form", form, "--episodes", str(a.episodes), "--runs",
               str(a.runs), "--budgets", a.budgets]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.form_seconds)
        except subprocess.TimeoutExpired:
            print(f"form {form} ran out of time: stopping", file=sys.stderr)
            status = 124
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("FORM ")]
        if r.returncode != 0 or not line:
            print(f"form {form} failed ({r.returncode}): stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            status = r.returncode or 1
            break
        rec["forms"].append(json.loads(line[-1][5:]))
        print(json.dumps({k: v for k, v in rec["forms"][-1].items() if k != "mean_steps_over_optimal"}), flush=True)
    rec["complete"] = status == 0
    by = {r["form"]: r["seconds"] for r in rec["forms"]}
    if "loop" in by and "set" in by:
        rec["loop_over_set"] = by["loop"] / by["set"]
    if "set" in by and "fused" in by:
        rec["set_over_fused"] = by["set"] / by["fused"]
    print(json.dumps({k: v for k, v in rec.items() if k != "forms"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return status


if __name__ == "__main__":
    sys.exit(main())
