#!/usr/bin/env python3
"""Batched path extraction against looped getPath, after one config-3 solve.

One N^2 config-3 grid (bench.py's workload: splitmix64 U(1,5) speed, 2 % obstacles, goal
at the centre) is solved once through the class surface; then, for M uniformly random
interior starts, Planner.getPaths (the device route: k_extract_paths next to the map) is
timed as a whole call (host clock; the call ends after its downloads) and by its kernel
time (HIP events), and the same starts are timed through a loop of Planner.getPath -- the
only way before getPaths -- which walks the host mirror and pays its block downloads.
The device calls run first, so the mirror is cold for the host loop's first paths, as
it is for a caller.  Prints one JSON line (kept under profiles/).

    python tools/paths_bench.py [--n 16384] [--sizes 1,256,4096] [--reps 3]
                                [--host-limit K] [--stride S]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "planning-path_planning_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--sizes", default="1,256,4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--obst", type=float, default=0.02)
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--host-limit", type=int, default=0,
                    help="time at most this many of the starts through getPath (0 = all); "
                         "the total is then scaled and marked as extrapolated")
    args = ap.parse_args()
    import dymu

    N = args.n
    g = (N // 2, N // 2)
    dev = int(os.environ.get("LOCAL_RANK", "0"))
    eng = dymu.Engine(device=dev)
    dF = eng.alloc(8 * N * N)
    eng.synth_speed(dF, N, N, N, 0, 1, args.obst, 3, g[0], g[1])
    F = np.empty((N, N))
    eng.d2h(F, dF)
    eng.free(dF)
    eng.close()
    cost = np.where(np.isfinite(F), F, -1.0)
    del F
    p = dymu.Planner(risk_distance=0.5, device=dev)
    p.initGlobalLayer(1.0, 0.5, N, N)
    p.setCostMap(cost)
    del cost
    assert p.setGoal(g)
    t0 = time.perf_counter()
    assert p.computeEntireTotalCostMap()
    solve_ms = (time.perf_counter() - t0) * 1e3
    p.getPaths([(g[0] + 3.5, g[1] + 2.5)])  # first launch: code object load
    assert p.lastPathsOnDevice()

    rng = np.random.default_rng(7)
    rows = []
    for M in [int(s) for s in args.sizes.split(",")]:
        starts = [(x, y, 0.0, 0.0) for x, y in rng.uniform(2, N - 3, (M, 2))]
        call_ms, kern_ms = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            paths, status = p.getPaths(starts, stride=args.stride)
            call_ms.append((time.perf_counter() - t0) * 1e3)
            kern_ms.append(p.lastPathsKernelMs())
            assert p.lastPathsOnDevice()
        lens = np.array([len(q) for q in paths])
        k = M if args.host_limit <= 0 else min(M, args.host_limit)
        t0 = time.perf_counter()
        host = [p.getPath(s) for s in starts[:k]]
        host_ms = (time.perf_counter() - t0) * 1e3
        same = None
        if args.stride == 1:
            same = all(a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
                       for a, b in zip(paths, host))
        rows.append({
            "M": M,
            "getPaths_call_ms": {"min": round(min(call_ms), 3),
                                 "median": round(float(np.median(call_ms)), 3)},
            "getPaths_kernel_ms": {"min": round(min(kern_ms), 3),
                                   "median": round(float(np.median(kern_ms)), 3)},
            "looped_getPath_ms": round(host_ms * M / k, 3),
            "looped_getPath_timed_starts": k,
            "looped_getPath_extrapolated": k < M,
            "waypoints": {"total": int(lens.sum()), "median": int(np.median(lens)),
                          "max": int(lens.max())},
            "not_at_sink": int((status != 1).sum()),
            "device_equals_host": same,
        })
        del paths, host
        print(f"[paths_bench] M={M}: {rows[-1]}", file=sys.stderr, flush=True)
    p.close()
    print(json.dumps({
        "tool": "paths_bench",
        "workload": f"config 3: {N}x{N}, U(1,5) speed, {args.obst:.0%} obstacles, goal centre; "
                    f"uniformly random interior starts (seed 7), stride {args.stride}",
        "solve_ms_first_call": round(solve_ms, 2),
        "reps": args.reps,
        "note": "looped getPath runs after the device calls on a cold host mirror: its time "
                "includes the 128x128-cell block downloads of the cells it walks",
        "rows": rows,
    }))


if __name__ == "__main__":
    main()
