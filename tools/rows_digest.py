"""sha256 of every byte Engine.probe_actions, Engine.saliency and Engine.param_grads write, for comparing two builds.

The three calls share one row frame (csrc/mzh_rows.h); a change to it must leave every output bit where it was.  This
tool uses the public Engine API only, so the same file runs in a checkout of another commit: run it there and here on
one machine and compare the records (`--compare a.json b.json` exits 1 on any difference).

Cases, per (n_disks, support) in (3, 33), (7, 33), (3, 1) -- seven discs: two observation tiles in rep0's transposed
product -- with MuZeroNets of fixed torch seeds:
  batch     B = 40 envs, n = 37 rows through a permuted env_index: three tiles at R = 16, two at R = 32, both ragged
  skipped   one env index out of range, and where the call takes them one bad logit_index / policy_logit and one bad
            action, each on an env of the call
  outputs   every optional output (legal, the per-disc sums, the dense grad ...), all prefilled, so a row the call
            must leave alone is part of the digest; the err count
  tiles     both tile flags
  set       the first 34 of the same rows under a set of three networks with row counts (17, 16, 1); and a decreasing
            net_index, where _status must be nonzero and every output buffer untouched

  python tools/rows_digest.py --out record.json
  python tools/rows_digest.py --compare profiles/rows_digest_parent.json profiles/rows_digest_new.json
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((3, 33), (7, 33), (3, 1))
B, ROWS, SET_COUNTS = 40, 37, (17, 16, 1)
FILL = {"float32": -777.0, "int32": -7, "uint8": 0xAB}


def _digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _inputs(n_disks, seed):
    import numpy as np

    rng = np.random.RandomState(seed)
    state = rng.randint(0, 3, (B, n_disks)).astype(np.uint8)
    obs = np.eye(3, dtype=np.float32)[state].reshape(B, 3 * n_disks)
    obs[-5:] = rng.standard_normal((5, 3 * n_disks)).astype(np.float32)  # and a few rows of arbitrary floats
    env_index = rng.permutation(B)[:ROWS].astype(np.int32)
    logit = rng.randint(-1, 6, B).astype(np.int32)
    action = rng.randint(0, 6, B).astype(np.int32)
    logit[env_index[3]] = 6    # the three skipped rows, all among the first 34
    action[env_index[20]] = 7
    env_index[9] = B
    return state, obs, env_index, logit, action


def _outputs(call, n_disks, support, n, dev):
    import numpy as np
    import torch

    from muzero_hanoi_amd import engine

    N, f32, i32, u8 = n_disks, torch.float32, torch.int32, torch.uint8
    n_floats = sum(int(np.prod(s)) for s in engine.weight_shapes(N, support))
    spec = {
        "probe_actions": dict(reward=((B, 6), f32), value=((B, 6), f32), legal=((B,), u8), h0=((B, 64), f32),
                              pi0=((B, 6), f32), value0=((B,), f32), h1=((B, 6, 64), f32), pi1=((B, 6, 6), f32)),
        "saliency": dict(policy=((B, 3 * N), f32), value=((B, 3 * N), f32), picked=((B,), i32),
                         disc_policy=((B, N), f32), disc_value=((B, N), f32), h0=((B, 64), f32), pi0=((B, 6), f32),
                         value0=((B,), f32)),
        "param_grads": dict(delta1=((B, 5, 256), f32), delta2=((B, 5, 64), f32), act=((B, 5, 256), f32),
                            h0=((B, 64), f32), z1=((B, 64), f32), h1=((B, 64), f32), pi0=((B, 6), f32),
                            value0=((B,), f32), reward=((B,), f32), objective=((B, 5), f32), grad=((n, n_floats), f32)),
    }[call]
    return {k: torch.full(shp, FILL[str(dt).split(".")[1]], dtype=dt, device=dev) for k, (shp, dt) in spec.items()}


def run():
    import numpy as np
    import torch

    from muzero_hanoi_amd import _lib, engine
    from muzero_hanoi_amd.networks import MuZeroNet

    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.as_tensor(a, device=dev)
    cases = {}
    for n_disks, support in SHAPES:
        flats = []
        for m in range(3):
            torch.manual_seed(1000 * n_disks + 10 * support + m)
            flats.append(engine.flat_weights(MuZeroNet(3 * n_disks, 6, 0.002, "cpu", TD_return=support == 33).state_dict()))
        eng = engine.Engine(n_disks, 1, 64, support)
        eng.load_weights(flats[0])
        eng.load_weight_set(flats)
        state, obs, env_index, logit, action = _inputs(n_disks, 7 * n_disks + support)
        state, obs, logit, action = up(state), up(obs), up(logit), up(action)
        n_set = sum(SET_COUNTS)
        net_index = np.repeat(np.arange(3), SET_COUNTS).astype(np.int32)
        forms = {"single": (up(env_index), None), "set": (up(env_index[:n_set]), up(net_index)),
                 "decreasing": (up(env_index[:n_set]), up(net_index[::-1].copy()))}
        calls = {"probe_actions": lambda **kw: eng.probe_actions(obs, state=state, **kw),
                 "saliency": lambda **kw: eng.saliency(obs, logit_index=logit, **kw),
                 "param_grads": lambda **kw: eng.param_grads(obs, action, policy_logit=logit, **kw)}
        for call, fn in calls.items():
            for tile in (16, 32):
                for form, (idx, nets) in forms.items():
                    out = _outputs(call, n_disks, support, int(idx.shape[0]), dev)
                    err = torch.zeros(1, dtype=torch.int32, device=dev)
                    got = fn(env_index=idx, net_index=nets, out=out, tile=tile, err=err)
                    torch.cuda.synchronize()
                    rec = {k: _digest(got[k]) for k in out}
                    rec["err_count"] = int(err.item())
                    if nets is not None:
                        rec["_status"] = [int(v) for v in got["_status"].cpu()]
                    if form == "decreasing":  # refused on the device: nothing written, nothing counted
                        fresh = _outputs(call, n_disks, support, int(idx.shape[0]), dev)
                        assert rec["_status"][0] != 0 and rec["err_count"] == 0, rec
                        assert all(torch.equal(got[k], fresh[k]) for k in out), (call, tile, "buffers touched")
                    else:
                        assert rec["err_count"] == (1 if call == "probe_actions" else 2 if call == "saliency" else 3), rec
                    cases[f"N{n_disks}_s{support}/{call}/tile{tile}/{form}"] = rec
        eng.close()
    return {"build_id": _lib.build_id(), "cases": cases}


def compare(a, b):
    ra, rb = (json.load(open(p))["cases"] for p in (a, b))
    bad = [f"{c}/{k}" for c in sorted(set(ra) | set(rb)) for k in sorted(set(ra.get(c, {})) | set(rb.get(c, {})))
           if ra.get(c, {}).get(k) != rb.get(c, {}).get(k)]
    n = sum(len(v) for v in ra.values())
    print(f"{len(ra)} cases, {n} records compared, {len(bad)} differ" + "".join("\n  " + x for x in bad))
    return 1 if bad or not ra else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    rec = run()
    print(json.dumps({"build_id": rec["build_id"], "cases": len(rec["cases"])}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
