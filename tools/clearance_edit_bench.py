#!/usr/bin/env python3
"""Freeing an obstacle block with trackObstacleRemoval on and off,
measured through the planner.

Maps: N^2 config 3 (bench.py's workload: splitmix64 U(1,5) speed, 2 % obstacles) for N in
--ns, global risk on with risk distances of --rds cells and ratio 2.  One planner per
(N, rd), solved once for a goal in the middle; then 2 * --rounds 9x9 blocks of cost +inf are
added through setCostMapWindow, each at a place of its own, and the map is solved again, so
that the map really holds the blocks an edit frees (a cost <= 0 marks a node an obstacle
for good; a cost of +inf is an obstacle of the mask that a finite cost frees).  Then
--rounds rounds in the same process and build, alternating, each edit freeing one block:

  (a) trackObstacleRemoval(True):  setCostMapWindow(finite costs) + computeEntireTotalCostMap
      -- the box's rows re-packed, the field raised and re-propagated
      (dymu_clearance_edit_device), the rows of the reported box downloaded, the total-cost
      map re-propagated from the changed window;
  (b) trackObstacleRemoval(False): the same two calls -- the freed cell marks R stale: every
      obstacle listed on the host, the whole clearance solve, all of S downloaded.

Per leg: wall seconds of the two calls together, device ms of the risk step (the engine's
statistics: HIP events), its passes, tile visits and box, the raise's passes, visits and
cells invalidated, and how the total-cost step ran and its device ms.  Prints one JSON
object (kept as profiles/clearance_edit.json); the summary gives min and max over the rounds.

    python tools/clearance_edit_bench.py [--ns 4096,16384] [--rds 4,16] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "planning-path_planning_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from clearance_update_bench import BLOCK, config3_cost  # noqa: E402


def leg(p, call):
    t0 = time.perf_counter()
    assert call()
    assert p.computeEntireTotalCostMap()
    wall = time.perf_counter() - t0
    risk, solve, raised = p.lastRiskUpdate(), p.lastStats(), p.lastRiskRaise()
    return {"wall_s": round(wall, 4), "risk_kind": p.lastRiskUpdateKind(),
            "risk_ms": round(risk["ms"], 4), "risk_passes": risk["passes"],
            "risk_tile_visits": risk["tile_visits"], "risk_box": list(risk["box"]),
            "raise_passes": raised["raise_passes"], "raise_visits": raised["raise_visits"],
            "cells_invalidated": raised["cells_invalidated"],
            "solve_kind": p.lastSolveKind(), "solve_ms": round(solve["ms"], 4)}


def span(rows, key):
    v = [r[key] for r in rows]
    return [min(v), max(v)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="4096,16384")
    ap.add_argument("--rds", default="4,16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--obst", type=float, default=0.02)
    args = ap.parse_args()
    import dymu

    rows = []
    rng = np.random.default_rng(1)
    for N in (int(v) for v in args.ns.split(",")):
        cost0 = config3_cost(dymu, N, args.obst)
        for rd in (float(v) for v in args.rds.split(",")):
            p = dymu.Planner(risk_distance=0.5)
            assert p.initGlobalLayer(1.0, 0.5, N, N)
            assert p.setCostMap(cost0)
            assert p.setGlobalRisk(rd, 2.0)
            assert p.setGoal((N // 2, N // 2, 0.0, 0.0))
            assert p.computeEntireTotalCostMap()
            # the blocks: two per round, a quarter of the map from the goal, apart from each other
            places = []
            for k in range(args.rounds):
                places.append((N // 4 + 64 * k, N // 4 + 32 * k))
                places.append((3 * N // 4 - 64 * k, 3 * N // 4 - 32 * k))
            for i, j in places:
                assert p.setCostMapWindow(i, j, np.full((BLOCK, BLOCK), np.inf))
            t0 = time.perf_counter()
            assert p.computeEntireTotalCostMap()
            added = {"wall_s": round(time.perf_counter() - t0, 4),
                     "risk_kind": p.lastRiskUpdateKind()}
            a, b = [], []
            for k in range(args.rounds):
                free = rng.uniform(1.0, 5.0, (BLOCK, BLOCK))
                (ia, ja), (ib, jb) = places[2 * k], places[2 * k + 1]
                p.trackObstacleRemoval(True)
                a.append(leg(p, lambda: p.setCostMapWindow(ia, ja, free)))
                p.trackObstacleRemoval(False)
                b.append(leg(p, lambda: p.setCostMapWindow(ib, jb, free)))
                print(f"[clearance_edit_bench] N={N} rd={rd} round {k}: (a) {a[-1]} (b) {b[-1]}",
                      file=sys.stderr, flush=True)
            p.close()
            assert all(r["risk_kind"] == 3 for r in a) and all(r["risk_kind"] == 1 for r in b)
            rows.append({"n": N, "risk_distance_cells": rd, "blocks_added": added,
                         "tracked": a, "untracked": b,
                         "wall_s": {"tracked": span(a, "wall_s"), "untracked": span(b, "wall_s")},
                         "risk_ms": {"tracked": span(a, "risk_ms"),
                                     "untracked": span(b, "risk_ms")},
                         "solve_ms": {"tracked": span(a, "solve_ms"),
                                      "untracked": span(b, "solve_ms")}})
    print(json.dumps({
        "tool": "clearance_edit_bench",
        "workload": f"config 3: N^2, U(1,5) speed, {args.obst:.0%} obstacles, global risk ratio 2; "
                    f"a {BLOCK}x{BLOCK} block of cost +inf freed per edit",
        "rounds": args.rounds,
        "rows": rows,
    }))


if __name__ == "__main__":
    main()
