"""Depth A/B of the wave kernel's expansion memo on bench.py: for each depth one fresh `python bench.py` child per
round with MZH_MEMO_DEPTH naming it (0 = no memo), the depths taken in turn within a round, each child under its
own time limit; the first child that fails ends the run.  Then, in this process, one search of the same roots per
depth for the table's bytes and build time and the share of (wave, simulation) pairs that ran no MLP, the packed
tile and the full MLP (Engine.memo_stats).  Prints and optionally writes one JSON record.

    python tools/memo_depth_ab.py --depths 0,3,4,5 [--rounds 2] [--out profiles/x.json] -- [bench.py arguments]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench(depth, args, limit):
    env = dict(os.environ, MZH_MEMO_DEPTH=str(depth))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True, text=True,
                       timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"bench.py failed ({r.returncode}) at depth {depth}:\n{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def stats(depths, n_disks, roots, sims, seed):
    import torch

    import bench as b
    from muzero_hanoi_amd import engine, rng
    from muzero_hanoi_amd.networks import MuZeroNet

    torch.manual_seed(seed)
    flat = engine.flat_weights(MuZeroNet(3 * n_disks, 6, 0.002, "cpu", TD_return=True).state_dict())
    obs = torch.from_numpy(b.random_roots(n_disks, roots, seed)).cuda()
    noise, tie, u = (torch.from_numpy(x).cuda() for x in rng.synthetic_draws(roots, deterministic=False, alpha=0.25,
                                                                            seed=seed))
    eng = engine.Engine(n_disks, sims, roots, 33)
    eng.load_weights(flat)
    out = {}
    for d in depths:
        if d == 0:
            continue
        eng.set_memo_depth(d)
        s0 = eng.memo_stats()
        o = eng.search(sims, obs=obs, tie_idx=tie, noise=noise, action_u=u, temperature=1.0, deterministic=False)
        s1 = eng.memo_stats()
        took = np.array([s1[k] - s0[k] for k in ("pairs_skipped", "pairs_packed", "pairs_full")], np.float64)
        share = took / took.sum()
        out[str(d)] = {"table_bytes": s1["table_bytes"], "rows": s1["rows"], "build_ms": s1["build_ms"],
                       "kernel": o["_plan"]["kernel"], "pairs_skipped_packed_full": [int(t) for t in took],
                       "share_skipped_packed_full": [float(x) for x in share],
                       "mlp_work_model": float(0.5 * share[1] + share[2])}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", required=True, help="comma-separated memo depths (0 = off)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds per bench.py child")
    ap.add_argument("--out", default=None)
    ap.add_argument("bench_args", nargs="*")
    a = ap.parse_args()
    depths = [int(d) for d in a.depths.split(",")]
    ms, line = {d: [] for d in depths}, None
    for rnd in range(a.rounds):
        for d in (depths if rnd % 2 == 0 else depths[::-1]):
            line = bench(d, a.bench_args, a.limit)
            ms[d].append(line["roofline"]["kernel_ms"])
            print(f"round {rnd} depth {d} {ms[d][-1]:.4f} ms", file=sys.stderr, flush=True)
    cfg = line["config"]
    rec = {"bench_args": a.bench_args, "rounds": a.rounds, "kernel": line["roofline"]["kernel"], "build_id": line["build_id"],
           "n_disks": cfg["n_disks"], "roots": cfg["roots_per_gpu"], "sims": cfg["sims_per_move"],
           "order": "one bench.py child per depth and round, depths ascending in even rounds, descending in odd ones",
           "kernel_ms": {str(d): {"runs": ms[d], "median": float(np.median(ms[d])), "min": min(ms[d]), "max": max(ms[d])}
                         for d in depths},
           "memo": stats(depths, cfg["n_disks"], cfg["roots_per_gpu"], cfg["sims_per_move"], 0)}
    print(json.dumps(rec, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
