"""Weight refresh after a parameter change: the host path (flat_weights: 20 copies to the host, mzh_load_weights:
pack on the host, free, allocate, two uploads) against the device repack (mzh_load_weights_device: one gather
launch from the live parameter tensors, csrc/mzh_repack.hip).

Legs:
  refresh  one refresh after an in-place parameter change, host path against device path, alternated in one
           process after warm-up, each timed on the host clock from the call to the end of a synchronise;
           N = 3 and N = 4, a single network (Engine.load_weights / load_weights_from) and a set of 8
           (load_weight_set / load_weight_set_from).
  loop     Muzero(update_impl="fused", selfplay="batched", ingest="device") training loops per second at
           N = 3, S = 25, batch 256, with engine_for on "host" against "device" (networks.AUTO_DEVICE_RELOAD),
           alternated in blocks on two agents that replay the same draws (the same episodes and updates).
  kernel   --kernel-run CASE only issues device refreshes (N3_single, N4_single, N3_set8), for a separate
           `rocprofv3 --kernel-trace --stats` run; --kernel-stats CASE=<csv> then adds mzh_repack_kernel's time
           beside its algorithmic bytes (map read, sources read, blob written) to the output.

  python tools/bench_reload.py [--legs refresh,loop] [--reps 30] [--loops 40] [--out profiles/reload_bench.json]
  rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_reload.py --kernel-run N3_single
  python tools/bench_reload.py --legs '' --kernel-stats N3_single=DIR/.../*_kernel_stats.csv --out profiles/reload_bench.json

The output file is a JSON object of legs; a run that measures some legs keeps the others it finds in --out.
"""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda"


def make_nets(n_disks, count, seed=0):
    from muzero_hanoi_amd.networks import MuZeroNet

    nets = []
    for i in range(count):
        torch.manual_seed(seed + i)
        nets.append(MuZeroNet(rpr_input_s=3 * n_disks, action_s=6, lr=0.002, device=DEV, TD_return=True).to(DEV))
    return nets


def summary(ms):
    ms = sorted(ms)
    q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
    return {"median_ms": statistics.median(ms), "p10_ms": q(0.1), "p90_ms": q(0.9), "min_ms": ms[0], "max_ms": ms[-1],
            "n": len(ms)}


def refresh_case(n_disks, set_size, reps, warmup):
    """one refresh per timed sample, host and device alternated; the parameters change in place before each"""
    from muzero_hanoi_amd import engine

    nets = make_nets(n_disks, max(1, set_size))
    eng = engine.Engine(n_disks, 25, 256, 33)
    params = [[n.state_dict()[k] for k in engine.WEIGHT_KEYS] for n in nets]

    def host():
        if set_size:
            eng.load_weight_set([engine.flat_weights(n.state_dict()) for n in nets])
        else:
            eng.load_weights(engine.flat_weights(nets[0].state_dict()))

    def device():
        if set_size:
            eng.load_weight_set_from(params)
        else:
            eng.load_weights_from(params[0])

    def sample(fn):
        with torch.no_grad():
            for ps in params:
                torch._foreach_mul_(ps, 1.0001)  # the update's stand-in: the parameters change where they lie
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for _ in range(warmup):
        sample(host), sample(device)
    t = {"host": [], "device": []}
    for _ in range(reps):
        t["host"].append(sample(host))
        t["device"].append(sample(device))
    h, d = summary(t["host"]), summary(t["device"])
    rec = {"n_disks": n_disks, "networks": set_size or 1, "form": "set" if set_size else "single", "host": h, "device": d,
           "speedup_median": h["median_ms"] / d["median_ms"],
           # faster by more than the host path's own run-to-run spread (p90 - p10)
           "device_faster_beyond_host_spread": h["median_ms"] - d["median_ms"] > h["p90_ms"] - h["p10_ms"]}
    eng.close()
    return rec


def loop_leg(loops, blocks, warmup):
    """training loops per second, engine_for on the host path against the device path"""
    from muzero_hanoi_amd import networks
    from muzero_hanoi_amd.env import TowersOfHanoi
    from muzero_hanoi_amd.muzero import Muzero

    def agent():
        torch.manual_seed(3)
        np.random.seed(3)
        env = TowersOfHanoi(N=3, max_steps=200)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return Muzero(env=env, s_space_size=9, n_action=6, discount=0.8, dirichlet_alpha=0.25, n_mcts_simulations=25,
                          unroll_n_steps=5, batch_s=256, TD_return=True, n_TD_step=10, lr=0.002, buffer_size=50000,
                          priority_replay=True, device=DEV, n_ep_x_loop=1, selfplay="batched", update_impl="fused",
                          ingest="device")

    agents = {"host": agent(), "device": agent()}
    rates = {"host": [], "device": []}

    def block(mode, n, seed):
        # both agents replay the same draws block by block: the two paths give the same weight bytes, so the
        # agents play the same episodes and make the same updates, and a block pair differs in the reload alone
        networks.AUTO_DEVICE_RELOAD = mode == "device"
        mz = agents[mode]
        np.random.seed(seed)
        torch.manual_seed(seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mz.training_loop(n_loops=n + 1, min_replay_size=256, print_acc=10 ** 9)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    default = networks.AUTO_DEVICE_RELOAD
    try:
        for mode, mz in agents.items():  # fill the buffers past min_replay_size, build every workspace
            for i in range(20):
                block(mode, warmup, i)
                if len(mz.buffer) > 2 * 256:
                    break
            else:
                raise SystemExit(f"the {mode} agent's buffer stayed at {len(mz.buffer)} rows: no updates would run")
        for b in range(blocks):
            for mode in (("host", "device") if b % 2 == 0 else ("device", "host")):
                rates[mode].append(block(mode, loops, 1000 + b))
    finally:
        networks.AUTO_DEVICE_RELOAD = default
    out = {"workload": "hanoi3_s25_batch256_unroll5_1ep_1update_per_loop_fused_batched_device_ingest", "loops_per_block": loops,
           "blocks": blocks, "buffer_rows": {m: len(a.buffer) for m, a in agents.items()}}
    for m, r in rates.items():
        out[m] = {"loops_per_sec_median": statistics.median(r), "loops_per_sec_min": min(r), "loops_per_sec_max": max(r),
                  "blocks": r}
    out["speedup_median"] = out["device"]["loops_per_sec_median"] / out["host"]["loops_per_sec_median"]
    out["device_faster_beyond_host_spread"] = (out["device"]["loops_per_sec_median"] - out["host"]["loops_per_sec_median"]
                                               > max(rates["host"]) - min(rates["host"]))
    return out


def algorithmic_bytes(n_disks, support, networks=1):
    """what one gather moves: its map, the source floats it reads, the blob floats it writes"""
    from muzero_hanoi_amd import _lib

    n, total = ctypes.c_size_t(), ctypes.c_size_t()
    L = _lib.lib()
    _lib.check(L.mzh_weights_size(n_disks, support, ctypes.byref(total)), "mzh_weights_size")
    out = {"map_read": 0, "sources_read": 0, "blob_written": 0}
    for which in (0, 1):
        _lib.check(L.mzh_pack_map(n_disks, support, which, None, ctypes.byref(n), None), "mzh_pack_map")
        m = np.empty(n.value, np.int32)
        _lib.check(L.mzh_pack_map(n_disks, support, which, m.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n), None),
                   "mzh_pack_map")
        out["map_read"] += 4 * m.size
        out["sources_read"] += 4 * int((m >= 0).sum()) * networks
        out["blob_written"] += 4 * m.size * networks
    out["canonical_bytes"] = 4 * total.value * networks
    return out


KERNEL_CASES = {"N3_single": (3, 1), "N4_single": (4, 1), "N3_set8": (3, 8)}


def kernel_run(case, reps):
    """device refreshes only, for a profiler run of one case"""
    from muzero_hanoi_amd import engine

    n_disks, count = KERNEL_CASES[case]
    nets = make_nets(n_disks, count)
    eng = engine.Engine(n_disks, 25, 256, 33)
    params = [[n.state_dict()[k] for k in engine.WEIGHT_KEYS] for n in nets]
    for _ in range(reps):
        if count > 1:
            eng.load_weight_set_from(params)
        else:
            eng.load_weights_from(params[0])
    torch.cuda.synchronize()
    eng.close()


def kernel_stats(specs):
    """mzh_repack_kernel's row of each case's rocprofv3 kernel stats csv (case=path) beside the case's bytes"""
    out = {"source": "rocprofv3 --kernel-trace --stats -- python tools/bench_reload.py --kernel-run CASE", "cases": {}}
    for spec in specs:
        case, path = spec.split("=", 1)
        row = None
        with open(path) as f:
            for r in csv.DictReader(f):
                if "mzh_repack_kernel" in r.get("Name", ""):
                    row = r
        if row is None:
            raise SystemExit(f"no mzh_repack_kernel row in {path}")
        n_disks, count = KERNEL_CASES[case]
        nbytes = algorithmic_bytes(n_disks, 33, count)
        moved = nbytes["map_read"] + nbytes["sources_read"] + nbytes["blob_written"]
        out["cases"][case] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                              "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3,
                              "algorithmic_bytes": nbytes,
                              "algorithmic_GBps_at_average": moved / float(row["AverageNs"])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="refresh,loop")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--loops", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--kernel-run", default=None, choices=sorted(KERNEL_CASES))
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="CASE=CSV")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernel_run:
        kernel_run(args.kernel_run, args.kernel_reps)
        return
    out = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    legs = [x for x in args.legs.split(",") if x]
    if legs:
        from muzero_hanoi_amd import _lib

        out["device"] = torch.cuda.get_device_name(0)
        out["build_id"] = _lib.build_id()
    if "refresh" in legs:
        out["refresh"] = [refresh_case(n, m, args.reps, args.warmup) for n in (3, 4) for m in (0, 8)]
        for r in out["refresh"]:
            print(json.dumps({"leg": "refresh", **r}), flush=True)
    if "loop" in legs:
        out["loop"] = loop_leg(args.loops, args.blocks, warmup=6)
        print(json.dumps({"leg": "loop", **out["loop"]}), flush=True)
    if args.kernel_stats:
        out["kernel"] = kernel_stats(args.kernel_stats)
        print(json.dumps({"leg": "kernel", **out["kernel"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
