"""Same-box A/B of two library builds on bench.py, interleaved A B B A per round (as tools/gpu/ab.sh
interleaves its rounds): every leg is one fresh `python bench.py` child with MZH_LIB naming the build,
under its own time limit; the first child that fails ends the run.  Prints and optionally writes one
JSON record: each leg's roofline.kernel_ms per round, its median and min-to-max spread, the ratio of
the medians, and whether B's median is below A's by more than `--bar` times A's own spread.

    python tools/abba.py --a muzero-hanoi_amd/libmzh_parent.so --b muzero-hanoi_amd/libmzh.so \
        [--rounds 4] [--out profiles/x.json] [--dump-dir DIR] -- [bench.py arguments]

--dump-dir: the first run of each leg also writes its outputs (bench.py --dump-outputs) to DIR/a, DIR/b;
the record then says whether every array is byte-identical, and the dumps are removed.
--a-root DIR: leg A runs DIR/bench.py on DIR's own package and built library (a checkout of the parent commit),
for a parent whose library this tree's binding no longer loads (new entry points); --a is then only named.
--env-b K=V: an environment variable of leg B's children alone (repeatable).
--memo: after the legs, one search of the config's roots in this process on this tree's library and the record of
its expansion memo beside leg B (tools/memo_depth_ab.py stats: automatic depth, table bytes, the build's time on
the host's clock, the share of each M-phase form).
"""
import argparse
import filecmp
import json
import os
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench(lib, args, limit, dump=None, root=None, extra_env=()):
    env = dict(os.environ, MZH_LIB=os.path.abspath(lib))
    if root is not None:  # that tree's bench.py, package and library
        root = os.path.abspath(root)
        env.pop("MZH_LIB")
        env["PYTHONPATH"] = root
    env.update(kv.split("=", 1) for kv in extra_env)
    cmd = [sys.executable, os.path.join(root or ROOT, "bench.py"), *args] + (["--dump-outputs", dump] if dump else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit, cwd=root or ROOT)
    if r.returncode != 0:
        raise SystemExit(f"bench.py failed ({r.returncode}) with {lib}:\n{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", required=True, help="library A (the parent build)")
    ap.add_argument("--b", required=True, help="library B (the new build)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--bar", type=float, default=3.0, help="B wins if A's median - B's median > bar x A's spread")
    ap.add_argument("--limit", type=float, default=300.0, help="seconds per bench.py child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dump-dir", default=None)
    ap.add_argument("--a-root", default=None, help="a checkout whose own bench.py, package and library are leg A")
    ap.add_argument("--memo", action="store_true", help="record this tree's expansion memo beside leg B")
    ap.add_argument("--env-b", action="append", default=[], metavar="K=V", help="environment of leg B only")
    ap.add_argument("bench_args", nargs="*")
    a = ap.parse_args()
    libs = (a.a, a.b)
    ms, lines = ([], []), [None, None]
    for rnd in range(a.rounds):
        for leg in (0, 1, 1, 0):
            dump = None
            if a.dump_dir and lines[leg] is None:
                dump = os.path.abspath(os.path.join(a.dump_dir, "ab"[leg]))
            d = bench(libs[leg], a.bench_args, a.limit, dump, a.a_root if leg == 0 else None, a.env_b if leg == 1 else ())
            lines[leg] = lines[leg] or d
            ms[leg].append(d["roofline"]["kernel_ms"])
            print(f"round {rnd} {'AB'[leg]} {ms[leg][-1]:.4f} ms", file=sys.stderr, flush=True)

    def leg_stats(x):
        x = np.asarray(x)
        return {"kernel_ms": [float(v) for v in x], "median": float(np.median(x)), "min": float(x.min()),
                "max": float(x.max()), "spread": float(x.max() - x.min())}

    sa, sb = leg_stats(ms[0]), leg_stats(ms[1])
    rec = {"bench_args": a.bench_args, "rounds": a.rounds, "order": "A B B A per round, one bench.py child per leg",
           "kernel": lines[0]["roofline"]["kernel"],
           "a": dict(sa, lib=os.path.basename(a.a), build_id=lines[0]["build_id"], frac=lines[0]["roofline"]["frac"]),
           "b": dict(sb, lib=os.path.basename(a.b), build_id=lines[1]["build_id"], frac=lines[1]["roofline"]["frac"]),
           "ratio_median": sb["median"] / sa["median"], "gain_ms": sa["median"] - sb["median"],
           "bar_ms": a.bar * sa["spread"], "b_faster_beyond_bar": sa["median"] - sb["median"] > a.bar * sa["spread"],
           "b_slower_beyond_a_spread": sb["median"] - sa["median"] > sa["spread"]}
    if a.env_b:
        rec["b"]["env"] = a.env_b
    if a.memo:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import memo_depth_ab
        from muzero_hanoi_amd import _lib

        cfg = lines[1]["config"]
        d = _lib.memo_plan(cfg["n_disks"], -1)["depth"]
        rec["b"]["memo"] = dict(memo_depth_ab.stats([d], cfg["n_disks"], cfg["roots_per_gpu"], cfg["sims_per_move"], 0)
                                .get(str(d), {}), depth=d)
    if a.dump_dir:
        da, db = os.path.join(a.dump_dir, "a"), os.path.join(a.dump_dir, "b")
        names = sorted(os.listdir(da))
        same = {n: os.path.exists(os.path.join(db, n)) and filecmp.cmp(os.path.join(da, n), os.path.join(db, n), shallow=False)
                for n in names}
        rec["outputs"] = {"arrays": names, "byte_identical": bool(names) and all(same.values()) and names == sorted(os.listdir(db)),
                          "different": [n for n, s in same.items() if not s]}
        shutil.rmtree(a.dump_dir)
    print(json.dumps(rec, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
