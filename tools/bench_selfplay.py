"""Self-play / acting throughput: decisions per second, one decision = one
MCTS search of S simulations from the current state + one TowersOfHanoi step, episodes from
uniform random non-goal starts until the goal or max_steps (Muzero._play_game, Muzero.py:153-207;
acting_ablations.get_results, acting_experiments/acting_ablations.py:72-128).  Reference training
config: N=3, max_steps=200, S=25, T=1 stochastic, random-init MuZeroNet(TD_return=True).

Legs:
  batched   B episodes in lockstep on one GPU (selfplay.BatchedSelfPlay: one search launch and one
            env-kernel launch per move over every unfinished episode)
  batched-legacy  the same with every draw from NumPy's global legacy stream in the reference's
            order (legacy_rng=True; rng.predraw, the bit-exact mode)
  drop-in   the reference's sequential loop through the drop-ins (selfplay.play_game: one
            MCTS.run_mcts launch and one env.step per decision, as Muzero._play_game runs it)
  ingest    the step between self-play and training on one batched play's record (B episodes, record_obs):
            the host path (selfplay.episode_records, the success filter, Buffer.add per episode) against
            the device path (selfplay.ingest_records -> Buffer.add_episodes, csrc/mzh_ingest.hip) into equal
            buffers, which must come out bit-identical; wall clock (ending in a synchronise) around both,
            device events around the device path; written to --ingest-out
  cpu       the reference algorithm on one host core (bench.cpu_baseline_selfplay: oracle/py_port.py's
            object-tree MCTS with a batch-1 torch-CPU MLP + the C env restatement), bounded to
            --cpu-seconds

  python tools/bench_selfplay.py [--legs batched,batched-legacy,drop-in,ingest,cpu] [--episodes 4096] [--sims 25]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def start_states(n_disks, B, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, 3 ** n_disks - 1, size=B)  # every state index but the goal's


def leg_batched(args, net):
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay

    sp = BatchedSelfPlay(net, args.disks, args.max_steps, args.sims)
    sp.play(start_states(args.disks, min(args.episodes, 256), 1), seed=1)  # warm-up (engine, kernels)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = sp.play(start_states(args.disks, args.episodes, 2), seed=2)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    moves = int(res["steps"].sum())
    return dict(decisions=moves, episodes=args.episodes, seconds=dt,
                solved=int((res["steps"] < args.max_steps).sum()))


def leg_batched_legacy(args, net):
    """the batched leg with every draw from NumPy's global legacy stream in the reference's order
    (legacy_rng=True: rng.predraw per move over the unfinished episodes) -- the bit-exact mode"""
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay

    sp = BatchedSelfPlay(net, args.disks, args.max_steps, args.sims)
    np.random.seed(1)
    sp.play(start_states(args.disks, min(args.episodes, 256), 1), legacy_rng=True)  # warm-up
    torch.cuda.synchronize()
    np.random.seed(2)
    t0 = time.perf_counter()
    res = sp.play(start_states(args.disks, args.episodes, 2), legacy_rng=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    moves = int(res["steps"].sum())
    return dict(decisions=moves, episodes=args.episodes, seconds=dt,
                solved=int((res["steps"] < args.max_steps).sum()))


def leg_dropin(args, net):
    from muzero_hanoi_amd.env import TowersOfHanoi
    from muzero_hanoi_amd.mcts import MCTS
    from muzero_hanoi_amd.selfplay import play_game

    env = TowersOfHanoi(N=args.disks, max_steps=args.max_steps)
    mcts = MCTS(discount=0.8, root_dirichlet_alpha=0.25, n_simulations=args.sims, batch_s=256, device="cuda")
    np.random.seed(3)
    play_game(env, mcts, net, 1, temperature=1.0)  # warm-up
    moves, eps_done = 0, 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.dropin_seconds:
        env.init_state_idx = int(start_states(args.disks, 1, 100 + eps_done)[0])
        steps = play_game(env, mcts, net, 1, temperature=1.0)[0]
        moves += steps
        eps_done += 1
    dt = time.perf_counter() - t0
    return dict(decisions=moves, episodes=eps_done, seconds=dt)


def leg_ingest(args, net):
    from muzero_hanoi_amd.buffer import Buffer
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay, episode_records, ingest_records

    U, n_step, A, D, discount = 5, 10, 6, 3 * args.disks, 0.8
    sp = BatchedSelfPlay(net, args.disks, args.max_steps, args.sims)
    res = sp.play(start_states(args.disks, args.episodes, 2), seed=2, record_obs=True)
    torch.cuda.synchronize()
    T, B = res["action"].shape
    size = 1 << 20  # above B * max_steps rows: nothing is overwritten
    new_buffer = lambda: Buffer(size, U, D, A, "cuda", device_sampling=True)
    kw = dict(discount=discount, n_step=n_step, unroll_n_steps=U, n_action=A)

    def device_path(buf):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev0.record()
        ingest_records(res, buf, **kw)
        ev1.record()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, ev0.elapsed_time(ev1) * 1e-3

    device_path(new_buffer())  # warm-up: code objects, allocator
    dev_buf, dev_runs = None, []
    for _ in range(args.ingest_reps):
        dev_buf = new_buffer()
        np.random.seed(5)
        dev_runs.append(device_path(dev_buf))
    rows = dev_buf.ptr
    # what the writer kernel moves for `rows` transitions: the ring rows and priorities it stores, and the
    # record elements it loads (observation and root value once per row, reward / action and the n-step
    # window's rewards per row, U policy rows per row; repeated loads mostly hit in cache)
    stored = rows * (4 * D + 4 * U + 8 * U + 4 * U * A + 4 * U + 4)
    loaded = rows * (4 * D + 8 + 8 + 4 + 8 * U * A)
    out = dict(episodes=int(B), recorded_steps=int(T), rows=int(rows), solved=int((res["steps"] < args.max_steps).sum()),
               device_wall_s=[w for w, _ in dev_runs], device_event_s=[e for _, e in dev_runs],
               writer_bytes_stored=int(stored), writer_bytes_loaded=int(loaded))
    if not args.ingest_device_only:
        host_buf = new_buffer()
        np.random.seed(5)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _, states, rwds, actions, pi_probs, returns, prio in episode_records(res, TD_return=True, **kw):
            if returns[-1, 0] > 0:
                host_buf.add(states, rwds, actions, pi_probs, returns, prio)
        torch.cuda.synchronize()
        out["host_wall_s"] = time.perf_counter() - t0
        same = host_buf.ptr == dev_buf.ptr and all(
            torch.equal(getattr(host_buf, k), getattr(dev_buf, k))
            for k in ("states", "rwds", "actions", "pi_probs", "mc_returns", "_prio"))
        if not same:
            raise RuntimeError("ingest leg: the device path's buffer differs from the host path's")
        out["buffers_identical"] = True
        out["host_over_device_wall"] = out["host_wall_s"] / float(np.median(out["device_wall_s"]))
    if args.ingest_out:
        with open(args.ingest_out, "w") as f:
            json.dump(dict(out, config={"workload": f"hanoi{args.disks}_s{args.sims}_maxsteps{args.max_steps}",
                                        "U": U, "n_step": n_step, "ring_rows": size}), f, indent=1)
    dt = float(np.median(out["device_wall_s"]))
    return dict(out, decisions=int(res["steps"].sum()), seconds=dt)


def leg_cpu(args, net):
    from bench import cpu_baseline_selfplay

    moves, eps_done, dt = cpu_baseline_selfplay(args.disks, args.sims, args.max_steps, args.cpu_seconds,
                                                net.state_dict(),
                                                lambda k: start_states(args.disks, 1, 200 + k)[0])
    return dict(decisions=moves, episodes=eps_done, seconds=dt, cores=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="batched,drop-in,cpu")
    ap.add_argument("--episodes", type=int, default=4096)
    ap.add_argument("--disks", type=int, default=3)
    ap.add_argument("--max-steps", type=int, default=200)
    ap.add_argument("--sims", type=int, default=25)
    ap.add_argument("--dropin-seconds", type=float, default=10.0)
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--ingest-out", default=os.path.join(ROOT, "profiles", "ingest_bench.json"))
    ap.add_argument("--ingest-reps", type=int, default=5)
    ap.add_argument("--ingest-device-only", action="store_true", help="skip the host path (profiler runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from muzero_hanoi_amd.networks import MuZeroNet

    torch.manual_seed(1)
    recs = []
    for leg in args.legs.split(","):
        dev = "cpu" if leg == "cpu" else "cuda"
        torch.manual_seed(1)
        net = MuZeroNet(3 * args.disks, 6, 0.002, dev, TD_return=True).to(dev)
        r = {"batched": leg_batched, "batched-legacy": leg_batched_legacy, "drop-in": leg_dropin,
             "ingest": leg_ingest, "cpu": leg_cpu}[leg](args, net)
        if leg == "ingest":
            r.update(leg=leg, metric="ingest_rows_per_sec", value=r["rows"] / r["seconds"], unit="rows/s")
            print(json.dumps(r), flush=True)
            recs.append(r)
            continue
        r.update(leg=leg, metric="selfplay_decisions_per_sec", value=r["decisions"] / r["seconds"],
                 unit="decisions/s", sims_per_sec=r["decisions"] * args.sims / r["seconds"],
                 config={"workload": f"hanoi{args.disks}_s{args.sims}_maxsteps{args.max_steps}",
                         "episodes": r["episodes"], "T": 1.0, "stochastic": True})
        print(json.dumps(r), flush=True)
        recs.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
