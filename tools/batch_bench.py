#!/usr/bin/env python3
"""Batched solves against the same solves one after another.

One N^2 config-3 map (bench.py's workload: splitmix64 U(1,5) speed, 2 % obstacles) shared
by B goals, for N in --ns and B in --bs:

  batch       dymu_stack_speed_device once, then dymu_solve_batch_device on the B planes;
  sequential  B dymu_solve_device calls on the same map and the same goals, back to back.

Times are device times from HIP events (dymu_stats.ms), the median over --reps after one
untimed solve; passes and tile visits are the engine's counters (sequential: summed over
the B solves).  Each leg runs in a child process of its own.  The sequential leg is code a
change to the batch path must not alter, so --seq-libdir may name the lib directory of
another build (the parent commit's) to run it from, side by side in the same session.
DYMU_BATCH_TARGET_PER_CU in the environment reaches the batch leg (the per-pass target
override of dymu_solve_batch_device); --tag names the setting in the output.
Prints one JSON object (kept as profiles/batch_solve.json).

    python tools/batch_bench.py [--ns 512,1024,2048] [--bs 1,4,16,64] [--reps 5]
                                [--seq-libdir DIR] [--tag default]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "planning-path_planning_amd"))


def spread(v):
    return {"min": round(min(v), 4), "median": round(float(np.median(v)), 4),
            "max": round(max(v), 4)}


def goals_for(F, B):
    """B distinct free interior cells, the centre first, then uniformly random (seed 11)."""
    ny, nx = F.shape
    rng = np.random.default_rng(11)
    out = {(nx // 2, ny // 2): None}
    while len(out) < B:
        i, j = int(rng.integers(2, nx - 2)), int(rng.integers(2, ny - 2))
        if np.isfinite(F[j - 1:j + 2, i - 1:i + 2]).all():
            out[(i, j)] = None
    return list(out)[:B]


def leg(args):
    """One leg in this process: a JSON list of rows on stdout."""
    import dymu

    eng = dymu.Engine(device=int(os.environ.get("LOCAL_RANK", "0")))
    rows = []
    for N in args.ns:
        src, dT1 = eng.alloc(8 * N * N), eng.alloc(8 * N * N)
        eng.synth_speed(src, N, N, N, 0, 1, args.obst, 3, N // 2, N // 2)
        F = np.empty((N, N))
        eng.d2h(F, src)
        for B in args.bs:
            goals = goals_for(F, B)
            if args.leg == "seq":
                def run():
                    st = [eng.solve_device(src, dT1, N, N, N, gi, gj) for gi, gj in goals]
                    return {k: sum(s[k] for s in st) for k in ("ms", "passes", "tile_visits")}
            else:
                P = dymu.batch_plane_rows(N)
                dF, dT = eng.alloc(8 * B * P * N), eng.alloc(8 * B * P * N)
                eng.stack_speed(src, N, 0, N, N, B, dF, N)
                seeds = [(b, gi, gj) for b, (gi, gj) in enumerate(goals)]

                def run():
                    return eng.solve_batch_device(dF, dT, N, N, B, N, seeds)
            run()  # first launches: code object load, workspace growth
            st = [run() for _ in range(args.reps)]
            rows.append({"n": N, "B": B, "ms": spread([s["ms"] for s in st]),
                         "passes": int(np.median([s["passes"] for s in st])),
                         "tile_visits": int(np.median([s["tile_visits"] for s in st]))})
            print(f"[batch_bench] {args.leg} {rows[-1]}", file=sys.stderr, flush=True)
            if args.leg != "seq":
                eng.free(dF)
                eng.free(dT)
        eng.free(src)
        eng.free(dT1)
    eng.close()
    print(json.dumps(rows))


def child(args, which, libdir):
    env = dict(os.environ)
    if libdir:
        env["DYMU_LIBDIR"] = os.path.abspath(libdir)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", which, "--reps", str(args.reps),
           "--ns", ",".join(map(str, args.ns)), "--bs", ",".join(map(str, args.bs)),
           "--obst", str(args.obst)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, check=True, timeout=args.timeout)
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="512,1024,2048")
    ap.add_argument("--bs", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--obst", type=float, default=0.02)
    ap.add_argument("--seq-libdir", default="")
    ap.add_argument("--tag", default="default")
    ap.add_argument("--timeout", type=float, default=500.0)
    ap.add_argument("--leg", choices=["seq", "batch"], default="")
    args = ap.parse_args()
    args.ns = [int(s) for s in str(args.ns).split(",")]
    args.bs = [int(s) for s in str(args.bs).split(",")]
    if args.leg:
        return leg(args)
    seq = child(args, "seq", args.seq_libdir)
    bat = child(args, "batch", "")
    rows = []
    for s, b in zip(seq, bat):
        assert (s["n"], s["B"]) == (b["n"], b["B"])
        rows.append({"n": s["n"], "B": s["B"],
                     "batch_ms": b["ms"], "batch_passes": b["passes"],
                     "batch_tile_visits": b["tile_visits"],
                     "sequential_ms": s["ms"], "sequential_passes": s["passes"],
                     "sequential_tile_visits": s["tile_visits"],
                     "sequential_over_batch": round(s["ms"]["median"] / b["ms"]["median"], 3)})
    print(json.dumps({
        "tool": "batch_bench",
        "workload": f"config 3: N^2, U(1,5) speed, {args.obst:.0%} obstacles, one map shared by "
                    "B goals (the centre, then uniformly random free interior cells, seed 11)",
        "reps": args.reps,
        "batch_target": {"tag": args.tag,
                         "DYMU_BATCH_TARGET_PER_CU": os.environ.get("DYMU_BATCH_TARGET_PER_CU")},
        "sequential_leg": ("another build: " + args.seq_libdir) if args.seq_libdir
                          else "this build",
        "rows": rows,
    }))


if __name__ == "__main__":
    main()
