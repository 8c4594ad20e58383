"""Whole episodes in one launch (BatchedSelfPlay.play_episodes, mzh_play_episodes) against the lockstep move loop
(BatchedSelfPlay.play: one search launch, one env launch and one host read per move) and the sequential drop-in.

Workload: N = 3, S = 25, max_steps = 200, an untrained network (episodes run long), temperature 1, root noise.

Legs:
  rate    decisions per second, end to end (host clock, call to the end of a synchronise; a decision is one
          searched and executed move, summed over the envs), of play_episodes and of play(record_obs=True) at
          B = 1, 16, 100, 256, 512, alternated in one process after warm-up; medians with p10 / p90 / min / max.
          The two draw different tables (play_episodes' schedule), so their episodes differ in length: the rate
          is per decision.
  seq     decisions per second of the sequential drop-in selfplay.play_game (one env, MCTS.run_mcts per move).
  device  device time of the kernels alone (HIP events around the C calls mzh_play_episodes and mzh_search, every
          input and output allocated beforehand, so no fill or allocation lies between the events) at every B:
          one episode launch per move of its longest episode, beside one search launch of the same B on the
          latency kernel, in the same run.  The difference is what the in-kernel env step, record and per-move
          set-up cost.
  loop    Muzero training loops per second with selfplay="device" beside "batched" (tools/bench_reload.py's
          workload: fused update, device ingest, one episode and one update per loop), alternated in blocks on
          two agents that replay the same draws.

  python tools/bench_episode.py [--legs rate,seq,device,loop] [--reps 9] [--out profiles/episode_bench.json]

The output file is a JSON object of legs; a run that measures some legs keeps the others it finds in --out.
"""
import argparse
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
N, S, MAX_STEPS = 3, 25, 200
BATCHES = (1, 16, 100, 256, 512)


def make_net(seed=0):
    from muzero_hanoi_amd.networks import MuZeroNet

    torch.manual_seed(seed)
    return MuZeroNet(rpr_input_s=3 * N, action_s=6, lr=0.002, device=DEV, TD_return=True).to(DEV)


def summary(xs):
    xs = sorted(xs)
    q = lambda f: xs[min(len(xs) - 1, int(f * len(xs)))]
    return {"median": statistics.median(xs), "p10": q(0.1), "p90": q(0.9), "min": xs[0], "max": xs[-1], "n": len(xs)}


def starts(B, seed=0):
    g = np.random.default_rng(seed)
    s = g.integers(0, 3 ** N - 1, size=B)
    return s + (s >= 3 ** N - 1)  # uniform over the non-goal states


def rate_leg(reps, warmup):
    from muzero_hanoi_amd.selfplay import BatchedSelfPlay

    sp = BatchedSelfPlay(make_net(), N, MAX_STEPS, S)
    out = []
    for B in BATCHES:
        st = starts(B)

        def sample(fn, seed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn(st, temperature=1.0, seed=seed)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            return int(res["steps"].sum()) / dt, int(res["steps"].sum()), int(res["steps"].max())

        forms = {"play_episodes": sp.play_episodes, "play": lambda s, **kw: sp.play(s, record_obs=True, **kw)}
        for i in range(warmup):
            for fn in forms.values():
                sample(fn, 100 + i)
        got = {k: [] for k in forms}
        for i in range(reps):
            for k in (list(forms) if i % 2 == 0 else list(forms)[::-1]):
                got[k].append(sample(forms[k], i))
        rec = {"B": B}
        for k, v in got.items():
            rec[k] = {"decisions_per_sec": summary([x[0] for x in v]),
                      "decisions_per_run_median": statistics.median(x[1] for x in v),
                      "longest_episode_median": statistics.median(x[2] for x in v)}
        e, p = rec["play_episodes"]["decisions_per_sec"], rec["play"]["decisions_per_sec"]
        rec["ratio_median"] = e["median"] / p["median"]
        # faster by more than both forms' own run-to-run spread (p10 of one above p90 of the other)
        rec["episodes_faster_beyond_spread"] = e["p10"] > p["p90"]
        out.append(rec)
        print(json.dumps({"leg": "rate", **rec}), flush=True)
    return out


def seq_leg(reps, warmup):
    from muzero_hanoi_amd.env import TowersOfHanoi
    from muzero_hanoi_amd.mcts import MCTS
    from muzero_hanoi_amd.selfplay import play_game

    net = make_net()
    env = TowersOfHanoi(N=N, max_steps=MAX_STEPS)
    mcts = MCTS(discount=0.8, root_dirichlet_alpha=0.25, n_simulations=S, batch_s=256, device=DEV)
    rates = []
    np.random.seed(0)
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = play_game(env, mcts, net, episode=1)[0]
        torch.cuda.synchronize()
        if i >= warmup:
            rates.append(steps / (time.perf_counter() - t0))
    rec = {"decisions_per_sec": summary(rates)}
    print(json.dumps({"leg": "seq", **rec}), flush=True)
    return rec


def device_leg(reps, warmup):
    """HIP-event time of the launches alone, inputs resident on the device"""
    from muzero_hanoi_amd import rng
    from muzero_hanoi_amd.networks import engine_for

    import ctypes

    from muzero_hanoi_amd import _lib
    from muzero_hanoi_amd.engine import ptr, search_flags

    net = make_net()
    out = []
    for B in BATCHES:
        eng = engine_for(net, S, B)
        T = MAX_STEPS
        flat = rng.synthetic_draws(T * B, deterministic=False, alpha=0.25, seed=1)
        noise, tie, u = (torch.from_numpy(x).reshape((T, B) + x.shape[1:]).to(DEV) for x in flat)
        st = torch.from_numpy(starts(B))
        state = ((st[:, None] // (3 ** torch.arange(N - 1, -1, -1))) % 3).to(torch.uint8).to(DEV)
        obs = torch.zeros((B, 3 * N), dtype=torch.float32, device=DEV)
        obs[:, ::3] = 1.0
        # fresh bounds, given explicitly: the search then runs the MMIN instantiation, as the episode form does
        mm = torch.tensor([[-float("inf"), float("inf")]] * B, dtype=torch.float64, device=DEV)
        ev = lambda: torch.cuda.Event(enable_timing=True)
        # the argument blocks of both calls, built once by the bindings' own code on outputs that stay allocated
        res = eng.play_episodes(S, state, T, tie_idx=tie, noise=noise, action_u=u, record_obs=True)
        ea = _lib.EpisodeArgs(B=B, T=T, n_sims=S, goal_peg=2, max_steps=T, deterministic=0, flags=search_flags(),
                              discount=0.8, eps=0.25, temperature=1.0)
        for k, t in (("state", state), ("noise", noise), ("tie_idx", tie), ("action_u", u), ("pi", res["pi"]),
                     ("root_q", res["root_q"]), ("action", res["action"]), ("reward", res["reward"]),
                     ("obs", res["obs"]), ("steps", res["steps"]), ("illegal", res["illegal"]),
                     ("solved", res["solved"]), ("final_state", res["final_state"]), ("minmax_out", res["minmax"]),
                     ("err_count", res["err"])):
            setattr(ea, k, ptr(t))
        sa, sout = eng._search_args(S, obs=obs, replay=None, tie_idx=tie[0], noise=noise[0], action_u=u[0],
                                    minmax_in=mm, temperature=1.0, deterministic=False, discount=0.8, eps=0.25,
                                    out=None, flags=search_flags("one"))
        L, stream = _lib.lib(), eng._stream()
        per_move, per_search = [], []
        for i in range(warmup + reps):
            a, b, c, d = ev(), ev(), ev(), ev()
            a.record()
            _lib.check(L.mzh_play_episodes(eng._h, ctypes.byref(ea), stream), "mzh_play_episodes")
            b.record()
            c.record()
            _lib.check(L.mzh_search(eng._h, ctypes.byref(sa), stream), "mzh_search")
            d.record()
            torch.cuda.synchronize()
            if i >= warmup:
                per_move.append(a.elapsed_time(b) / int(res["steps"].max()))
                per_search.append(c.elapsed_time(d))
        assert "mzh_search_one_kernel" in sout["_plan_struct"].as_dict()["kernel"]
        rec = {"B": B, "episode_ms_per_move": summary(per_move), "search_ms_per_launch": summary(per_search),
               "longest_episode": int(res["steps"].max())}
        rec["step_and_record_ms_per_move"] = rec["episode_ms_per_move"]["median"] - rec["search_ms_per_launch"]["median"]
        out.append(rec)
        print(json.dumps({"leg": "device", **rec}), flush=True)
    return out


def loop_leg(loops, blocks, warmup):
    """training loops per second, selfplay="device" beside "batched" (bench_reload.py's loop workload)"""
    from muzero_hanoi_amd.env import TowersOfHanoi
    from muzero_hanoi_amd.muzero import Muzero

    def agent(mode):
        torch.manual_seed(3)
        np.random.seed(3)
        env = TowersOfHanoi(N=N, max_steps=MAX_STEPS)
        return Muzero(env=env, s_space_size=9, n_action=6, discount=0.8, dirichlet_alpha=0.25, n_mcts_simulations=S,
                      unroll_n_steps=5, batch_s=256, TD_return=True, n_TD_step=10, lr=0.002, buffer_size=50000,
                      priority_replay=True, device=DEV, n_ep_x_loop=1, selfplay=mode, update_impl="fused",
                      ingest="device")

    agents = {m: agent(m) for m in ("batched", "device")}
    rates = {m: [] for m in agents}

    def block(mode, n, seed):
        # both agents replay the same draws block by block and, with one episode per loop, play the same episodes
        np.random.seed(seed)
        torch.manual_seed(seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        agents[mode].training_loop(n_loops=n + 1, min_replay_size=256, print_acc=10 ** 9)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    for mode, mz in agents.items():  # fill the buffers past min_replay_size, build every workspace
        for i in range(20):
            block(mode, warmup, i)
            if len(mz.buffer) > 2 * 256:
                break
        else:
            raise SystemExit(f"the {mode} agent's buffer stayed at {len(mz.buffer)} rows: no updates would run")
    for b in range(blocks):
        for mode in (("batched", "device") if b % 2 == 0 else ("device", "batched")):
            rates[mode].append(block(mode, loops, 1000 + b))
    out = {"workload": "hanoi3_s25_batch256_unroll5_1ep_1update_per_loop_fused_device_ingest", "loops_per_block": loops,
           "blocks": blocks, "buffer_rows": {m: len(a.buffer) for m, a in agents.items()}}
    for m, r in rates.items():
        out[m] = {"loops_per_sec_median": statistics.median(r), "loops_per_sec_min": min(r), "loops_per_sec_max": max(r),
                  "blocks": r}
    out["ratio_median"] = out["device"]["loops_per_sec_median"] / out["batched"]["loops_per_sec_median"]
    out["device_faster_beyond_batched_spread"] = (out["device"]["loops_per_sec_median"]
                                                  - out["batched"]["loops_per_sec_median"]
                                                  > max(rates["batched"]) - min(rates["batched"]))
    print(json.dumps({"leg": "loop", **out}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="rate,seq,device,loop")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loops", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    legs = [x for x in args.legs.split(",") if x]
    from muzero_hanoi_amd import _lib

    out["device"] = torch.cuda.get_device_name(0)
    out["build_id"] = _lib.build_id()
    out["workload"] = {"n_disks": N, "n_sims": S, "max_steps": MAX_STEPS, "network": "untrained, seed 0"}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        if "rate" in legs:
            out["rate"] = rate_leg(args.reps, args.warmup)
        if "seq" in legs:
            out["seq"] = seq_leg(args.reps, args.warmup)
        if "device" in legs:
            out["device_time"] = device_leg(args.reps, args.warmup)
        if "loop" in legs:
            out["loop"] = loop_leg(args.loops, args.blocks, warmup=6)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
