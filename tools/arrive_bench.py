#!/usr/bin/env python3
"""The arriving descent against the reference's descent after one config-3 solve.

One N^2 config-3 grid (bench.py's workload: splitmix64 U(1,5) speed, 2 % obstacles, goal
at the centre) is solved once through the class surface.  Then, for M uniformly random
interior starts (tools/paths_bench.py's), in alternating rounds in one process:

  A  Planner.getArrivingStats   against   B  Planner.getPathStats     (records only)
  C  Planner.getArrivingPaths   against   D  Planner.getPaths         (waypoints)

Per call: the whole call (host clock) and its kernel (HIP events), the outcomes by status,
the share of node-to-node hops among the steps, the median and the largest waypoint count.
The one comparison of kernels is the time per step walked -- kernel ms over the longest
path's waypoints, the chain a lane-per-path kernel waits for -- of k_arrive_paths against
k_path_stats in the same run.  Prints one JSON line and writes it to
profiles/arrive_paths.json.

    python tools/arrive_bench.py [--n 16384] [--sizes 1,256,4096] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "planning-path_planning_amd"))


def ms_stats(v):
    return {"min": round(min(v), 3), "median": round(float(np.median(v)), 3),
            "max": round(max(v), 3)}


def by_status(st):
    return {str(int(k)): int(n) for k, n in zip(*np.unique(st, return_counts=True))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--sizes", default="1,256,4096")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--obst", type=float, default=0.02)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arrive_paths.json"))
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
    p = dymu.Planner(risk_distance=0.5, device=dev)
    p.initGlobalLayer(1.0, 0.5, N, N)
    p.setCostMap(np.where(np.isfinite(F), F, -1.0))
    del F
    assert p.setGoal(g)
    assert p.computeEntireTotalCostMap()
    warm = [(g[0] + 3.5, g[1] + 2.5)]  # first launches: code object loads
    for call in (p.getPaths, p.getPathStats, p.getArrivingPaths, p.getArrivingStats):
        call(warm)
        assert p.lastPathsOnDevice()

    rng = np.random.default_rng(7)
    rows = []
    for M in [int(s) for s in args.sizes.split(",")]:
        starts = [(x, y, 0.0, 0.0) for x, y in rng.uniform(2, N - 3, (M, 2))]
        wall = {k: [] for k in "ABCD"}
        kern = {k: [] for k in "ABCD"}

        def timed(key, call):
            t0 = time.perf_counter()
            out = call(starts)
            wall[key].append((time.perf_counter() - t0) * 1e3)
            kern[key].append(p.lastPathsKernelMs())
            assert p.lastPathsOnDevice()
            return out

        for _ in range(args.rounds):
            arr = timed("A", p.getArrivingStats)
            q5 = timed("B", p.getPathStats)
            paths, status, rec = timed("C", p.getArrivingPaths)
            assert rec.tobytes() == arr.tobytes(), "stored and records-only calls differ"
            assert [len(w) for w in paths] == list(rec["count"])
            del paths
            qpaths, qstatus = timed("D", p.getPaths)
            assert [len(w) for w in qpaths] == list(q5["count"])
            del qpaths
        steps = int(arr["count"].sum())
        q5_arrived = int(((q5["status"] == 1) & (q5["last_hop"] <= 2.4)).sum())
        a_step = float(np.median(kern["A"])) / max(int(arr["count"].max()), 1)
        b_step = float(np.median(kern["B"])) / max(int(q5["count"].max()), 1)
        rows.append({
            "M": M,
            "getArrivingStats": {"call_ms": ms_stats(wall["A"]), "kernel_ms": ms_stats(kern["A"])},
            "getPathStats": {"call_ms": ms_stats(wall["B"]), "kernel_ms": ms_stats(kern["B"])},
            "getArrivingPaths": {"call_ms": ms_stats(wall["C"]), "kernel_ms": ms_stats(kern["C"])},
            "getPaths": {"call_ms": ms_stats(wall["D"]), "kernel_ms": ms_stats(kern["D"])},
            "arriving": {"by_status": by_status(arr["status"]),
                         "hops": int(arr["hops"].sum()), "steps": steps,
                         "hops_share": round(float(arr["hops"].sum()) / max(steps, 1), 5),
                         "count_median": int(np.median(arr["count"])),
                         "count_max": int(arr["count"].max()),
                         "length_median": round(float(np.median(arr["length"])), 1)},
            "reference_descent": {"by_status": by_status(q5["status"]),
                                  "arrived_last_hop_le_2.4": q5_arrived,
                                  "count_median": int(np.median(q5["count"])),
                                  "count_max": int(q5["count"].max())},
            "kernel_us_per_step_of_longest_path": {"k_arrive_paths": round(1e3 * a_step, 4),
                                                   "k_path_stats": round(1e3 * b_step, 4)},
        })
        print(f"[arrive_bench] M={M}: {rows[-1]}", file=sys.stderr, flush=True)
    p.close()
    line = json.dumps({
        "tool": "arrive_bench",
        "workload": f"config 3: {N}x{N}, U(1,5) speed, {args.obst:.0%} obstacles, goal centre; "
                    f"uniformly random interior starts (seed 7)",
        "rounds": args.rounds,
        "note": "alternating rounds in one process; min / median / max over the rounds is the "
                "spread.  Kernel times are HIP events around the kernels alone (summed over "
                "the batches of a stored call).",
        "rows": rows,
    })
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
