#!/usr/bin/env python3
"""getPathStats against getPaths plus the same reduction on the host, and the stats
kernel's work queue against one lane per path, after one config-3 solve.

One N^2 config-3 grid (bench.py's workload: splitmix64 U(1,5) speed, 2 % obstacles, goal
at the centre) is solved once through the class surface.  Then, for M uniformly random
interior starts (tools/paths_bench.py's), in alternating pairs:

  A  Planner.getPathStats          -- the whole call (host clock) and its kernel (HIP events)
  B  Planner.getPaths, then the record's figures from the waypoints in numpy (segment
     lengths, nearest-node speed samples, per-path sums by np.add.reduceat) -- the only
     way to the same row before getPathStats

and on an engine map of the same speed, in alternating rounds, the kernel time of
Engine.path_stats with n_lanes >= M (one path per lane), with n_lanes = M / 4 (every lane
refills from the queue about four times) and with the default.  Prints one JSON line and
writes it to profiles/path_stats.json.

    python tools/path_stats_bench.py [--n 16384] [--sizes 1,256,4096] [--pairs 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "planning-path_planning_amd"))


def reduce_on_host(paths, F, res):
    """length, speed integral and skipped samples per path from the waypoints (vectorised:
    the sums are not in the record's order, which is fine for a timing)."""
    ny, nx = F.shape
    cnt = np.array([len(q) for q in paths])
    xy = np.concatenate([q[:, :2] for q in paths if len(q)]) if cnt.sum() else np.zeros((0, 2))
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    seg = np.zeros(len(xy))
    if len(xy) > 1:
        d = xy[:-1] - xy[1:]
        seg[:-1] = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    last = first + cnt - 1
    seg[last[cnt > 0]] = 0.0  # no segment from a path's last waypoint to the next path
    i = (xy[:, 0] / res + 0.5).astype(np.int64)
    j = (xy[:, 1] / res + 0.5).astype(np.int64)
    on = (i >= 0) & (i < nx) & (j >= 0) & (j < ny)
    v = np.full(len(xy), np.inf)
    v[on] = F[j[on], i[on]]
    counts = np.isfinite(v)
    w = np.where(counts, v, 0.0) * seg
    length = np.zeros(len(paths))
    integral = np.zeros(len(paths))
    skipped = np.zeros(len(paths), dtype=np.int64)
    nz = cnt > 0
    if nz.any():
        length[nz] = np.add.reduceat(seg, first[nz])
        integral[nz] = np.add.reduceat(w, first[nz])
        skipped[nz] = np.add.reduceat((~counts).astype(np.int64), first[nz])
    return length, integral, skipped


def ms_stats(v):
    return {"min": round(min(v), 3), "median": round(float(np.median(v)), 3),
            "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--sizes", default="1,256,4096")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--obst", type=float, default=0.02)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_stats.json"))
    args = ap.parse_args()
    import dymu

    N = args.n
    g = (N // 2, N // 2)
    dev = int(os.environ.get("LOCAL_RANK", "0"))
    eng = dymu.Engine(device=dev)
    dF = eng.alloc(8 * N * N)
    dT = eng.alloc(8 * N * N)
    eng.synth_speed(dF, N, N, N, 0, 1, args.obst, 3, g[0], g[1])
    F = np.empty((N, N))
    eng.d2h(F, dF)
    eng.solve_device(dF, dT, N, N, N, g[0], g[1])
    p = dymu.Planner(risk_distance=0.5, device=dev)
    p.initGlobalLayer(1.0, 0.5, N, N)
    p.setCostMap(np.where(np.isfinite(F), F, -1.0))
    assert p.setGoal(g)
    assert p.computeEntireTotalCostMap()
    warm = [(g[0] + 3.5, g[1] + 2.5)]  # first launches: code object loads
    p.getPaths(warm)
    p.getPathStats(warm)
    assert p.lastPathsOnDevice()
    eng.path_stats(dT, N, N, N, 1.0, g[0], g[1], 0.4, np.array(warm), 1 << 20, [(dF, N)])

    rng = np.random.default_rng(7)
    rows = []
    for M in [int(s) for s in args.sizes.split(",")]:
        xy = rng.uniform(2, N - 3, (M, 2))
        starts = [(x, y, 0.0, 0.0) for x, y in xy]
        a_call, a_kern, b_call, b_paths, b_kern = [], [], [], [], []
        for _ in range(args.pairs):
            t0 = time.perf_counter()
            stats = p.getPathStats(starts)
            a_call.append((time.perf_counter() - t0) * 1e3)
            a_kern.append(p.lastPathsKernelMs())
            assert p.lastPathsOnDevice()
            t0 = time.perf_counter()
            paths, status = p.getPaths(starts)
            t1 = time.perf_counter()
            length, integral, skipped = reduce_on_host(paths, F, 1.0)
            b_call.append((time.perf_counter() - t0) * 1e3)
            b_paths.append((t1 - t0) * 1e3)
            b_kern.append(p.lastPathsKernelMs())
        cnt = np.array([len(q) for q in paths])
        same = bool(np.array_equal(stats["status"], status) and
                    np.array_equal(stats["count"], cnt) and
                    np.array_equal(stats["skipped"][:, 0], skipped))
        rel = float(np.max(np.abs(stats["length"] - length) / np.maximum(length, 1e-300)))
        del paths
        lanes = {"static": (M + 63) // 64 * 64, "queued_quarter": max(64, M // 4), "default": 0}
        k_ms = {k: [] for k in lanes}
        ref = None
        for _ in range(args.pairs):
            for k, nl in lanes.items():
                s = eng.path_stats(dT, N, N, N, 1.0, g[0], g[1], 0.4, xy, 1 << 20, [(dF, N)],
                                   n_lanes=nl)
                k_ms[k].append(eng.last_path_stats_ms())
                ref = s if ref is None else ref
                assert s.tobytes() == ref.tobytes(), "records depend on n_lanes"
        arrived = int(((stats["status"] == 1) & (stats["last_hop"] <= 2.4)).sum())
        rows.append({
            "M": M,
            "getPathStats_call_ms": ms_stats(a_call),
            "getPathStats_kernel_ms": ms_stats(a_kern),
            "getPaths_plus_reduction_ms": ms_stats(b_call),
            "getPaths_call_ms": ms_stats(b_paths),
            "getPaths_kernel_ms": ms_stats(b_kern),
            "stats_kernel_ms_by_lanes": {k: dict(ms_stats(v), n_lanes=lanes[k])
                                         for k, v in k_ms.items()},
            "waypoints": {"total": int(cnt.sum()), "median": int(np.median(cnt)),
                          "max": int(cnt.max())},
            "arrived": arrived,
            "cut_short_or_failed": M - arrived,
            "status_count_skipped_equal_to_reduction": same,
            "length_max_rel_diff_to_reduction": rel,
        })
        print(f"[path_stats_bench] M={M}: {rows[-1]}", file=sys.stderr, flush=True)
    p.close()
    eng.free(dF)
    eng.free(dT)
    eng.close()
    line = json.dumps({
        "tool": "path_stats_bench",
        "workload": f"config 3: {N}x{N}, U(1,5) speed, {args.obst:.0%} obstacles, goal centre; "
                    f"uniformly random interior starts (seed 7)",
        "pairs": args.pairs,
        "note": "alternating pairs in one process; min / median / max over the pairs is the "
                "spread.  The lane comparison runs Engine.path_stats on an engine map of the "
                "same speed; its kernel times are HIP events around the kernel alone.",
        "rows": rows,
    })
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
