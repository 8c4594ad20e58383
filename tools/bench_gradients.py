"""gradient_analysis.py's parameter-gradient workload (get_results) in its own shape, and the time of the kernels
behind it.

  workload  N = 3, every one of the 27 states x 6 actions under 3 networks (the checkpoint, its policy-ablated and
            its value-ablated copy) = 486 (network, state, action) pairs, each the gradients of the five
            sub-networks' objectives with respect to their own parameters (20 tensors, 122,056 floats a pair)

Legs:
  batched   selfplay.evaluate_gradients: the 486 pairs as one mzh_param_grads call on the network set, factors
            only and with dense=True (pairs/s; host clock around the whole call, observations built and results
            read back included)
  dropin    acting.gradient_get_results, pair after pair: the reference's schedule, one call (factor kernel and
            expansion) and one read-back per pair (pairs/s; the whole workload once, after a warm-up pair per network)
  cputorch  the same 486 pairs as the reference computes them: this repository's MuZeroNet on the CPU, five
            torch.autograd.grad calls per pair (pairs/s; the whole workload once)
  kernel    the factor kernel alone at n = 300 and n = 65,536 rows of 4 discs, beside batched torch autograd on the
            device (the network as float32 torch modules on the same device; one backward per sub-network over the
            whole batch to the Linear outputs, which yields the same factors), interleaved A B B A per round
            (A = torch, B = the kernel): per leg the median of 20 calls, device events around each call; and the
            kernel's largest deviation from that torch path per factor, relative to the torch tensor's largest magnitude
  expand    mzh_pgrad_expand_kernel alone at 4,096 rows of 3 discs (the time of a dense call minus the time of the
            factor call on the same rows, and the bytes it stores per second), beside a device fill and a
            device-to-device copy of the same number of bytes measured in the same process (a copy reads as many
            bytes as it writes; the fill is the store-only stream)

The network is the reference-written checkpoint tests/golden/muzero_model_N3.pt (the 4-disc kernel legs: a
MuZeroNet of torch seed 0).  Every leg runs in a child process of its own under a time limit; the first leg that
fails or runs out of time ends the run.  One record (with the library's build id) is printed and written to --out.

  python tools/bench_gradients.py [--out profiles/gradients_bench.json] [--legs batched,kernel]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("batched", "dropin", "cputorch", "kernel", "expand")
N = 3
KERNEL_ROWS, KERNEL_DISKS, ROUNDS, CALLS = (300, 65536), 4, 4, 20
EXPAND_ROWS = 4096
MODULES = ("representation_net", "dynamic_net", "rwd_net", "policy_net", "value_net")


def _networks():
    import torch

    from muzero_hanoi_amd import acting
    from muzero_hanoi_amd.checkpoint import load_model

    net = load_model(os.path.join(ROOT, "tests", "golden", "muzero_model_N3.pt"), load_optimiser=False)
    torch.manual_seed(1)
    return [net, acting.ablate_network(net, ablate_policy=True), acting.ablate_network(net, ablate_value=True)]


def _repeat(run):
    import numpy as np
    import torch

    run()  # warm-up: engine, weight set, code objects
    torch.cuda.synchronize()
    times = []
    while len(times) < 3 or (sum(times) < 2.0 and len(times) < 200):
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), times


def run_batched():
    from muzero_hanoi_amd.selfplay import evaluate_gradients

    nets = _networks()
    pairs = 3 * 27 * 6
    rec = {"leg": "batched", "pairs": pairs,
           "seconds_what": "median over `runs` repetitions of the whole leg, host clock ending in a synchronise"}
    for name, dense in (("factors", False), ("dense", True)):
        dt, times = _repeat(lambda: evaluate_gradients(nets, N, dense=dense))
        rec[name] = {"seconds": dt, "pairs_per_sec": pairs / dt, "runs": len(times), "seconds_min": min(times),
                     "seconds_max": max(times)}
    rec["pairs_per_sec"] = rec["dense"]["pairs_per_sec"]
    return rec


def run_dropin():
    import torch

    from muzero_hanoi_amd import acting
    from muzero_hanoi_amd.selfplay import index_state

    nets = _networks()
    states = [index_state(i, N) for i in range(3 ** N)]
    for net in nets:  # warm-up: engines, weights
        acting.gradient_get_results(net, states[0], 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = [acting.gradient_get_results(net, s, a) for net in nets for s in states for a in range(6)]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"leg": "dropin", "pairs": len(out), "seconds": dt, "pairs_per_sec": len(out) / dt, "runs": 1,
            "seconds_per_pair": dt / len(out),
            "seconds_what": "the whole workload once, host clock ending in a synchronise"}


def run_cputorch():
    import copy

    import torch
    import torch.nn.functional as F

    from muzero_hanoi_amd.selfplay import index_state
    from muzero_hanoi_amd.utils import oneHot_encoding

    nets = [copy.deepcopy(n).to("cpu") for n in _networks()]
    states = [index_state(i, N) for i in range(3 ** N)]

    def get_results(net, state, action):  # gradient_analysis.py:274-338 on this repository's torch path
        x = torch.tensor(oneHot_encoding(state, n_integers=3), dtype=torch.float32).unsqueeze(0)
        h = net.represent(x)
        pi_logits, value = net.prediction(h)
        probs = F.softmax(pi_logits, dim=-1)
        a = torch.zeros(1, 6)
        a[0, action] = 1.0
        h1, rwd = net.dynamics(h, a)
        objs = (h.mean(), h1.mean(), rwd.mean(), probs.mean(), value.mean())
        return [torch.autograd.grad(o, getattr(net, m).parameters(), retain_graph=True, create_graph=True)
                for o, m in zip(objs, MODULES)]

    get_results(nets[0], states[0], 0)
    t0 = time.perf_counter()
    out = [get_results(net, s, a) for net in nets for s in states for a in range(6)]
    dt = time.perf_counter() - t0
    return {"leg": "cputorch", "pairs": len(out), "seconds": dt, "pairs_per_sec": len(out) / dt, "runs": 1,
            "threads": torch.get_num_threads(), "seconds_what": "the whole workload once, host clock"}


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


def _abba(a, b):
    ms = {"a": [], "b": []}
    for _ in range(ROUNDS):
        for name, f in (("a", a), ("b", b), ("b", b), ("a", a)):
            ms[name].append(_median_ms(f))
    return _stats(ms["a"]), _stats(ms["b"])


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
        action = torch.randint(0, 6, (n,), dtype=torch.int32, device=dev)
        onehot = torch.nn.functional.one_hot(action.long(), 6).float()
        out = eng.param_grads(obs, action, full=True)
        out.pop("_status", None)

        def autograd():
            res = []

            def run(i, inp, objective):
                seq = getattr(tnet, MODULES[i])
                pre = seq[0](inp.detach())
                act = torch.relu(pre)
                o2 = seq[2](act)
                d1, d2 = torch.autograd.grad(objective(o2).sum(), [pre, o2])
                res.append((d1, d2, act.detach()))
                return o2.detach()

            norm = lambda z: tnet.normalize_h_state(z).mean(dim=1)
            scal = lambda l: tnet.logits_to_transformed_expected_value(l)[:, 0]
            z0 = run(0, obs, norm)
            h0 = tnet.normalize_h_state(z0)
            z1 = run(1, torch.cat([h0, onehot], dim=1), norm)
            run(2, z1, scal)
            run(3, h0, lambda lp: torch.softmax(lp, dim=-1).mean(dim=1))
            run(4, h0, scal)
            return res

        kernel = lambda: eng.param_grads(obs, action, out=out)
        ref = autograd()
        got = kernel()
        devs = {}
        for i, m in enumerate(MODULES):
            if i == 3:
                continue  # the constant objective: both are rounding noise around 0
            d1, d2, act = ref[i]
            devs[m] = {"delta1": float((got["delta1"][:, i] - d1).abs().max() / d1.abs().max()),
                       "delta2": float((got["delta2"][:, i, :d2.shape[1]] - d2).abs().max() / d2.abs().max()),
                       "act": float((got["act"][:, i] - act).abs().max() / act.abs().max())}
        for f in (autograd, kernel):  # warm-up of every timed shape
            f()
        torch.cuda.synchronize()
        a, b = _abba(autograd, kernel)
        sizes.append({"rows": n, "disks": KERNEL_DISKS, "torch_autograd": a, "kernel": b,
                      "kernel_over_torch_autograd": b["median"] / a["median"], "kernel_vs_torch_fp32_rel_dev": devs})
        eng.close()
    return {"leg": "kernel", "rounds": ROUNDS, "calls_per_leg": CALLS,
            "order": "A B B A per round; a leg = the median of `calls_per_leg` calls, device events around each call "
                     "(host launch gaps between torch's kernels included: they are part of that path)",
            "sizes": sizes}


def run_expand():
    import torch

    from muzero_hanoi_amd import engine
    from muzero_hanoi_amd.checkpoint import load_model

    dev = "cuda"
    net = load_model(os.path.join(ROOT, "tests", "golden", "muzero_model_N3.pt"), load_optimiser=False)
    n = EXPAND_ROWS
    eng = engine.Engine(N, 1, n, 33)
    eng.load_weights(engine.flat_weights(net.state_dict()))
    st = torch.randint(0, 3, (n, N), dtype=torch.uint8, device=dev)
    obs = engine.encode_obs(N, st)
    action = torch.randint(0, 6, (n,), dtype=torch.int32, device=dev)
    out = eng.param_grads(obs, action, full=True, dense=True)
    out.pop("_status", None)
    fac = {k: v for k, v in out.items() if k != "grad"}
    grad = out["grad"]
    other = torch.empty_like(grad)
    nbytes = grad.numel() * 4
    dense = lambda: eng.param_grads(obs, action, out=out)
    factors = lambda: eng.param_grads(obs, action, out=fac)
    fill = lambda: other.fill_(1.0)
    copy = lambda: other.copy_(grad)
    for f in (dense, factors, fill, copy):
        f()
    torch.cuda.synchronize()
    a, b = _abba(factors, dense)
    c, d = _abba(fill, copy)
    ms = b["median"] - a["median"]
    eng.close()
    return {"leg": "expand", "rows": n, "disks": N, "floats_per_row": grad.shape[1], "bytes": nbytes, "rounds": ROUNDS,
            "calls_per_leg": CALLS, "factor_call": a, "dense_call": b, "expand_ms": ms,
            "expand_bytes_per_sec": nbytes / (ms * 1e-3), "fill": c, "copy": d,
            "fill_bytes_per_sec": nbytes / (c["median"] * 1e-3), "copy_written_bytes_per_sec": nbytes / (d["median"] * 1e-3),
            "what": "expand_ms = median dense call - median factor call (A B B A rounds, device events); the fill and "
                    "the copy are torch's on a tensor of the same bytes in this process"}


RUN = {"batched": run_batched, "dropin": run_dropin, "cputorch": run_cputorch, "kernel": run_kernel, "expand": run_expand}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--leg-seconds", type=float, default=300.0, help="time limit of one leg's child process")
    ap.add_argument("--leg", choices=LEGS, help="(child) run one leg and print its record")
    a = ap.parse_args()
    if a.leg:
        print("LEG " + json.dumps(RUN[a.leg]()), flush=True)
        return 0
    from muzero_hanoi_amd import _lib

    rec = {"build_id": _lib.build_id(), "legs": [],
           "config": {"workload": f"hanoi{N}_all_states_x_6_actions_x_3_networks", "networks": 3, "states": 3 ** N,
                      "actions": 6, "network": "tests/golden/muzero_model_N3.pt (reference-written checkpoint)"}}
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
    for other in ("dropin", "cputorch"):
        if "batched" in by and other in by:
            rec[f"batched_over_{other}"] = by["batched"] / by[other]
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
