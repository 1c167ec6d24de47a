#!/usr/bin/env python3
"""The obstacle clearance field and the inflated speed, measured.

Maps: N^2 config 3 (bench.py's workload: splitmix64 U(1,5) speed, 2 % obstacles) for N in
--ns; risk distances of --rds cells (c = 1 / rd).

Per (N, rd), from this build: dymu_clearance_device (device ms from HIP events -- the fill,
the seeding and the passes -- as the median over --reps after one untimed run; passes, tile
visits; the host's wall time around the call) and dymu_inflate_speed_device (HIP events
around --inflate-reps launches).

Alongside, the same field by the means of a build without the entry (--base-libdir: the
parent commit's, run in the same session in a child process of its own): the speed map
downloaded, its obstacle cells listed on the host (list_s, once per N), a constant map
uploaded and dymu_solve_seeds_device run to convergence on it with one seed per obstacle
cell (device ms from its statistics, which leave the staging of the seeds out; wall_s
around the call, which includes it).

Prints one JSON object (kept as profiles/clearance.json).

    python tools/clearance_bench.py [--ns 1024,4096,16384] [--rds 4,16] [--reps 3]
                                    [--base-libdir DIR]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "planning-path_planning_amd"))


def spread(v):
    return {"min": round(min(v), 4), "median": round(float(np.median(v)), 4),
            "max": round(max(v), 4)}


def med(st, key):
    return int(np.median([s[key] for s in st]))


def leg(args):
    """One leg in this process: a JSON list of rows on stdout."""
    import dymu

    eng = dymu.Engine(device=int(os.environ.get("LOCAL_RANK", "0")))
    lib = eng._lib
    rows = []
    for N in args.ns:
        dF, dW, dS = (eng.alloc(8 * N * N) for _ in range(3))
        eng.synth_speed(dF, N, N, N, 0, 1, args.obst, 3, N // 2, N // 2)
        seeds = None
        list_s = 0.0
        if args.leg == "base":
            t0 = time.perf_counter()
            F = np.empty((N, N))
            eng.d2h(F, dF)
            jj, ii = np.nonzero(~(F < np.inf))
            seeds = np.zeros(len(ii), dtype=dymu.SEED_DTYPE)
            seeds["i"], seeds["j"] = ii, jj
            list_s = time.perf_counter() - t0
            del F, ii, jj
        for rd in args.rds:
            c = 1.0 / rd
            row = {"n": N, "risk_distance_cells": rd}
            st, wall = [], []
            for _ in range(args.reps + 1):
                t0 = time.perf_counter()
                if args.leg == "base":
                    eng.h2d(dW, np.full(N * N, c))
                    s = dymu.DymuStats()
                    dymu._check(lib.dymu_solve_seeds_device(eng.ctx, dW, dS, N, N, N,
                                                            seeds.ctypes.data, len(seeds), None,
                                                            ctypes.byref(s)), eng.ctx)
                    st.append(s.as_dict())
                else:
                    st.append(eng.clearance_device(dF, dW, dS, N, N, N, c))
                wall.append(time.perf_counter() - t0)
            st, wall = st[1:], wall[1:]
            row.update(ms=spread([s["ms"] for s in st]), passes=med(st, "passes"),
                       tile_visits=med(st, "tile_visits"), kernel=st[0]["kernel"],
                       wall_s=round(float(np.median(wall)), 4))
            if args.leg == "base":
                row.update(obstacle_cells=int(len(seeds)), list_s=round(list_s, 3))
            else:
                # the entry is asynchronous: K back-to-back launches and a copy of one cell,
                # which waits for them, on the host's clock (launch overhead included)
                K = 10 if N >= 8192 else 50 if N >= 2048 else 200
                one = np.empty(1)
                eng.inflate_speed(dF, dS, dW, N, N, N, 2.0)  # untimed
                eng.d2h(one, dW)
                t0 = time.perf_counter()
                for _ in range(K):
                    eng.inflate_speed(dF, dS, dW, N, N, N, 2.0)
                eng.d2h(one, dW)
                row["inflate_ms"] = round((time.perf_counter() - t0) * 1e3 / K, 4)
                row["inflate_launches"] = K
            rows.append(row)
            print(f"[clearance_bench] {args.leg} {row}", file=sys.stderr, flush=True)
        for p in (dF, dW, dS):
            eng.free(p)
    eng.close()
    print(json.dumps(rows))


def child(args, which, libdir):
    env = dict(os.environ)
    if libdir:
        env["DYMU_LIBDIR"] = os.path.abspath(libdir)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", which, "--reps", str(args.reps),
           "--ns", ",".join(map(str, args.ns)), "--rds", ",".join(map(str, args.rds)),
           "--obst", str(args.obst), "--inflate-reps", str(args.inflate_reps)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, check=True, timeout=args.timeout)
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def nums(s):
    return [float(v) if "." in v else int(v) for v in str(s).split(",") if v != ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="1024,4096,16384")
    ap.add_argument("--rds", default="4,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inflate-reps", type=int, default=10)
    ap.add_argument("--obst", type=float, default=0.02)
    ap.add_argument("--base-libdir", default="")
    ap.add_argument("--timeout", type=float, default=900.0)
    ap.add_argument("--leg", choices=["base", "clearance"], default="")
    args = ap.parse_args()
    args.ns, args.rds = nums(args.ns), nums(args.rds)
    if args.leg:
        return leg(args)
    base = {(r["n"], r["risk_distance_cells"]): r
            for r in child(args, "base", args.base_libdir)}
    rows = child(args, "clearance", "")
    for r in rows:
        b = base[(r["n"], r["risk_distance_cells"])]
        r["seeds_from_host"] = {k: b[k] for k in ("ms", "passes", "tile_visits", "kernel",
                                                  "wall_s", "obstacle_cells", "list_s")}
    print(json.dumps({
        "tool": "clearance_bench",
        "workload": f"config 3: N^2, U(1,5) speed, {args.obst:.0%} obstacles; c = 1 / risk "
                    "distance in cells",
        "reps": args.reps,
        "base_leg": ("another build: " + args.base_libdir) if args.base_libdir else "this build",
        "rows": rows,
    }))


if __name__ == "__main__":
    main()
