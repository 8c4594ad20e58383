"""The wave search with fresh draws at every launch: what the expansion memo's grown extension gives in real use.

bench.py replays identical inputs every step, so after its warm-up every new node below the dense table has been
inserted and the hit rate is 100 %.  This tool redraws the Dirichlet noise, the tie choices and the action uniforms
(and, with --fresh-roots, the root states) for every launch after one weight load, and reports per launch index:
the launch's time on HIP events (the search kernel and, where the library has one, the harvest behind it -- the
harvest's own time is in the kernel trace, `rocprofv3 --kernel-trace --stats -- python tools/bench_memo_grow.py`),
the share of (wave, simulation) pairs that ran no MLP / the packed tile / the full tiles, and the extension's rows.

    python tools/bench_memo_grow.py [--config 2] [--launches 12] [--grow-bytes -1] [--out profiles/x.json]

Run it once per library (MZH_LIB, or from a checkout of the parent with PYTHONPATH naming that tree): it uses only
what both bindings have.  `steady` is the median of the last third of the launches.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("PYTHONPATH", "").split(os.pathsep)[0] or ROOT)
sys.path.insert(1, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, help="bench.py's BASELINE configs[K]")
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--grow-bytes", type=int, default=None, help="Engine.set_memo_grow (libraries that have it)")
    ap.add_argument("--fresh-roots", action="store_true", help="redraw the root states too")
    ap.add_argument("--same-draws", action="store_true", help="bench.py's replay: the same inputs at every launch")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from muzero_hanoi_amd import _lib, engine, rng
    from muzero_hanoi_amd.networks import MuZeroNet

    N, B, S, what = bench.CONFIGS[a.config]
    dev = torch.device("cuda", 0)
    torch.manual_seed(a.seed)
    net = MuZeroNet(3 * N, 6, 0.002, "cpu", TD_return=True)
    eng = engine.Engine(N, S, B, 33)
    eng.load_weights(engine.flat_weights(net.state_dict()))
    if a.grow_bytes is not None:
        eng.set_memo_grow(a.grow_bytes)
    out = eng.alloc_search_outputs(B, S)
    stream = torch.cuda.current_stream(dev)

    def inputs(k):
        k = 0 if a.same_draws else k
        obs = bench.random_roots(N, B, a.seed + (k if a.fresh_roots else 0))
        noise, tie, u = rng.predraw(B, deterministic=False, alpha=0.25, rng=np.random.RandomState(a.seed + 1000 * k))
        return [torch.from_numpy(x).to(dev) for x in (obs, noise, tie, u)]

    # the dense table is built by the first wave search: one of 32 roots and a single simulation, whose new nodes
    # all lie at depth 1 (no miss, nothing to harvest), so that launch 0 below is the cold launch on its own
    obs, noise, tie, u = inputs(0)
    eng.search(1, obs=obs[:32].contiguous(), tie_idx=tie[:32].contiguous(), noise=noise[:32].contiguous(),
               action_u=u[:32].contiguous(), temperature=1.0, deterministic=False, discount=0.8, eps=0.25, kernel="wave")
    rows = []
    prev = eng.memo_stats()
    for k in range(a.launches):
        obs, noise, tie, u = inputs(k)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        eng.search(S, obs=obs, tie_idx=tie, noise=noise, action_u=u, temperature=1.0, deterministic=False,
                   discount=0.8, eps=0.25, out=out)
        e1.record(stream)
        torch.cuda.synchronize(dev)
        st = eng.memo_stats()
        took = [int(st[f] - prev[f]) for f in ("pairs_skipped", "pairs_packed", "pairs_full")]
        prev = st
        n = max(1, sum(took))
        rows.append({"launch": k, "launch_ms": e0.elapsed_time(e1),
                     "share_none": took[0] / n, "share_packed": took[1] / n, "share_full": took[2] / n,
                     "grow_rows": st.get("grow_rows"), "grow_rows_last": st.get("grow_rows_last")})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    tail = rows[-max(1, a.launches // 3):]
    rec = {"config": what, "n_disks": N, "roots": B, "sims": S, "kernel": out["_plan"]["kernel"],
           "build_id": _lib.build_id() if hasattr(_lib, "build_id") else None, "draws": "same" if a.same_draws else "fresh",
           "fresh_roots": a.fresh_roots, "memo": {k: v for k, v in prev.items() if not k.startswith("pairs_")},
           "launches": rows,
           "cold_ms": rows[0]["launch_ms"],
           "steady": {"launch_ms": float(np.median([r["launch_ms"] for r in tail])),
                      "share_none": float(np.median([r["share_none"] for r in tail])),
                      "share_packed": float(np.median([r["share_packed"] for r in tail])),
                      "share_full": float(np.median([r["share_full"] for r in tail]))}}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()
