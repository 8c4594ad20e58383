"""gradient_analysis.py's saliency workload in its own shape, and the time of the kernel behind it.

  workload  N = 3, every one of the 27 states under 3 networks (the checkpoint, its policy-ablated and its
            value-ablated copy) = 81 (network, state) pairs, each d(policy logit at its argmax)/d(obs) and
            d(value)/d(obs)

Legs:
  batched   selfplay.evaluate_saliency: the 81 pairs as one mzh_saliency call on the network set (pairs/s; host
            clock around the whole call, observations built and results read back included)
  dropin    acting.compute_saliency, pair after pair: the reference's schedule, one launch and one read-back per
            pair (pairs/s; the whole workload once, after a warm-up pair per network)
  kernel    mzh_saliency alone at n = 300 and n = 65,536 rows of 4 discs, beside batched torch autograd on the
            device (the network as float32 torch modules on the same device, one backward per head over the whole
            batch -- the only path to an input gradient before the kernel existed), interleaved A B B A per round
            (A = torch, B = the kernel): per leg the median of 20 calls, device events around each call; and the
            kernel's largest deviation from that torch path relative to the torch tensor's largest magnitude

The network is the reference-written checkpoint tests/golden/muzero_model_N3.pt (the 4-disc kernel legs: a
MuZeroNet of torch seed 0).  Every leg runs in a child process of its own under a time limit; the first leg that
fails or runs out of time ends the run.  One record (with the library's build id) is printed and written to --out.

  python tools/bench_saliency.py [--out profiles/saliency_bench.json] [--legs batched,kernel]
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
N = 3
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

    from muzero_hanoi_amd.selfplay import evaluate_saliency

    nets = _networks()
    run = lambda: evaluate_saliency(nets, N)
    run()  # warm-up: engine, weight set, code objects
    torch.cuda.synchronize()
    times = []
    while len(times) < 3 or (sum(times) < 2.0 and len(times) < 200):
        t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    dt = float(np.median(times))
    pairs = int(out["picked"].size)
    return {"leg": "batched", "pairs": pairs, "seconds": dt, "pairs_per_sec": pairs / dt, "runs": len(times),
            "seconds_min": min(times), "seconds_max": max(times),
            "seconds_what": "median over `runs` repetitions of the whole leg, host clock ending in a synchronise"}


def run_dropin():
    import torch

    from muzero_hanoi_amd import acting
    from muzero_hanoi_amd.selfplay import index_state

    nets = _networks()
    states = [index_state(i, N) for i in range(3 ** N)]
    for net in nets:  # warm-up: engines, weights
        acting.compute_saliency(states[0], N, net, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = [acting.compute_saliency(s, N, net, 0) for net in nets for s in states]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"leg": "dropin", "pairs": len(out), "seconds": dt, "pairs_per_sec": len(out) / dt, "runs": 1,
            "seconds_per_pair": dt / len(out),
            "seconds_what": "the whole workload once, host clock ending in a synchronise"}


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
    import copy

    import torch

    from muzero_hanoi_amd import engine
    from muzero_hanoi_amd.networks import MuZeroNet

    dev = "cuda"
    torch.manual_seed(0)
    net = MuZeroNet(3 * KERNEL_DISKS, 6, 0.002, "cpu", TD_return=True)
    flat = engine.flat_weights(net.state_dict())
    tnet = copy.deepcopy(net).to(dev)
    sizes = []
    for n in KERNEL_ROWS:
        eng = engine.Engine(KERNEL_DISKS, 1, n, 33)
        eng.load_weights(flat)
        st = torch.randint(0, 3, (n, KERNEL_DISKS), dtype=torch.uint8, device=dev)
        obs = engine.encode_obs(KERNEL_DISKS, st)
        out = {k: torch.empty((n, 3 * KERNEL_DISKS), dtype=torch.float32, device=dev) for k in ("policy", "value")}

        def autograd():
            x = obs.clone().requires_grad_()
            logits = tnet.prediction(tnet.represent(x))[0]
            gp, = torch.autograd.grad(logits.gather(1, logits.argmax(dim=1, keepdim=True)).sum(), x)
            x = obs.clone().requires_grad_()
            gv, = torch.autograd.grad(tnet.prediction(tnet.represent(x))[1].sum(), x)
            return gp, gv

        kernel = lambda: eng.saliency(obs, out=out)
        gp, gv = autograd()
        got = kernel()
        dev_p = float((got["policy"] - gp).abs().max() / gp.abs().max())
        dev_v = float((got["value"] - gv).abs().max() / gv.abs().max())
        for f in (autograd, kernel):  # warm-up of every timed shape
            f()
        torch.cuda.synchronize()
        ms = {"torch_autograd": [], "kernel": []}
        for _ in range(ROUNDS):
            for name, f in (("torch_autograd", autograd), ("kernel", kernel), ("kernel", kernel), ("torch_autograd", autograd)):
                ms[name].append(_median_ms(f))
        a, b = _stats(ms["torch_autograd"]), _stats(ms["kernel"])
        sizes.append({"rows": n, "disks": KERNEL_DISKS, "torch_autograd": a, "kernel": b,
                      "kernel_over_torch_autograd": b["median"] / a["median"],
                      "kernel_vs_torch_fp32_rel_dev": {"policy": dev_p, "value": dev_v}})
        eng.close()
    return {"leg": "kernel", "rounds": ROUNDS, "calls_per_leg": CALLS,
            "order": "A B B A per round; a leg = the median of `calls_per_leg` calls, device events around each call "
                     "(host launch gaps between torch's kernels included: they are part of that path)",
            "sizes": sizes}


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
           "config": {"workload": f"hanoi{N}_all_states_x_3_networks", "networks": 3, "states": 3 ** N,
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
    by = {r["leg"]: r["pairs_per_sec"] for r in rec["legs"] if "pairs_per_sec" in r}
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
