"""In-kernel phase stamps of the wave search kernels (mzh_wave_kernel), diagnostic build only
(libmzh_diag.so: python -m muzero_hanoi_amd.build --diag).  s_memtime ticks per simulation of the four
waves of workgroup 0, averaged over the launches: where one simulation of the bench workload's search goes.
A stamp closes the phase it names: the ticks since the previous stamp.  The latent gather's stamp closes
when its loads are issued, so the wait for them falls into the dynamics chain.  In a simulation that runs no MLP
the stamps between the lookup's and the new block's are empty, so it splits into select / lookup / record + new
block / backup; "record + new block" closes when the block's stores are issued.  --warm: launches before the
stamped ones (the grown memo fills over the first few; a warm table is what bench.py times).

    MZH_DIAG_LIB=muzero-hanoi_amd/libmzh_diag.so python tools/wave_stamps.py [--config 2] [--launches 5] [--warm 1]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["MZH_LIB"] = os.environ.get("MZH_DIAG_LIB", os.path.join(ROOT, "muzero-hanoi_amd", "libmzh_diag.so"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

# stamp index -> phase, in the order a simulation runs them (mzh_wave.hip)
PHASES = [(4, "loop top"), (0, "select"), (3, "memo lookup + mode ballot"), (10, "gather issue"), (5, "dyn chain + bias"), (6, "rwd chain + bias"),
          (11, "rwd head"), (7, "normalise + latent store"), (8, "pol chain + softmax"), (9, "val chain + bias"),
          (1, "val head"), (12, "record + new block"), (2, "backup")]
MLP = (10, 5, 6, 11, 7, 8, 9, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, help="bench.py's BASELINE config (2: the default workload)")
    ap.add_argument("--kernel", choices=["auto", "wave", "wave16"], default="auto")
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1, help="launches before the stamped ones")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import bench
    from muzero_hanoi_amd import _lib, engine, rng
    from muzero_hanoi_amd.networks import MuZeroNet

    n, B, S, _ = bench.CONFIGS[a.config]
    torch.manual_seed(a.seed)
    net = MuZeroNet(3 * n, 6, 0.002, "cpu", TD_return=True)
    eng = engine.Engine(n, S, B, 33)
    eng.load_weights(engine.flat_weights(net.state_dict()))
    obs = torch.from_numpy(bench.random_roots(n, B, a.seed)).cuda()
    noise, tie, u = (torch.from_numpy(x).cuda()
                     for x in rng.predraw(B, deterministic=False, alpha=0.25, rng=np.random.RandomState(a.seed)))
    out = eng.alloc_search_outputs(B, S)
    L = _lib.lib()
    L.mzh_diag_wave_stamps.argtypes = [ctypes.c_void_p]
    buf = np.zeros((8, 32), np.uint64)
    kern = None if a.kernel == "auto" else a.kernel

    def run():
        return eng.search(S, obs=obs, tie_idx=tie, noise=noise, action_u=u, temperature=1.0, deterministic=False,
                          discount=0.8, eps=0.25, out=out, kernel=kern)

    for _ in range(max(1, a.warm)):
        o = run()
    torch.cuda.synchronize()
    assert "mzh_wave_kernel" in o["_plan"]["kernel"], f"{o['_plan']['kernel']}: not a wave kernel"
    assert L.mzh_diag_wave_stamps(buf.ctypes.data_as(ctypes.c_void_p)) == 0  # clears the warm-up launch's
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
    for s_, e_ in ev:
        s_.record()
        run()
        e_.record()
    torch.cuda.synchronize()
    assert L.mzh_diag_wave_stamps(buf.ctypes.data_as(ctypes.c_void_p)) == 0
    per = buf.astype(np.float64) / (a.launches * S)
    waves = range(4)
    mean = per[:4].mean(0)
    total = float(sum(mean[k] for k, _ in PHASES))
    res = {"config": a.config, "disks": n, "roots": B, "sims": S, "kernel": o["_plan"]["kernel"],
           "launches": a.launches, "warm_launches": max(1, a.warm), "build_id": _lib.build_id(),
           "kernel_ms_diag_build": float(np.median([s_.elapsed_time(e_) for s_, e_ in ev])),
           "sel_steps_per_sim": float(out["sel_steps"].double().sum()) / (B * S),
           "what": "s_memtime ticks per simulation, workgroup 0, lane 0 of each wave; a phase = the ticks since "
                   "the previous stamp; mean4 = mean over the workgroup's four waves, share = mean4 / their sum",
           "ticks_per_sim": {name: {**{f"wave{w}": round(float(per[w, k]), 1) for w in waves},
                                    "mean4": round(float(mean[k]), 1), "share": round(float(mean[k]) / total, 4)}
                             for k, name in PHASES},
           "mean4_total": round(total, 1),
           "mean4_mlp_phase": round(float(sum(mean[k] for k in MLP)), 1)}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
