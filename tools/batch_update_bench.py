#!/usr/bin/env python3
"""Windowed update of a solved batch against the cold batch solve.

One N^2 config-3 map (bench.py's workload: splitmix64 U(1,5) speed, 2 % obstacles) shared
by B goals placed as tools/batch_bench.py places them, for N in --ns and B in --bs.  The
change is config 5's: a hazard disc of radius 20 (speed x 2: hazard 0 -> 1 in F = res *
cost * (2 + hazard - traff)) plus its 1-cell ring (x 1.1), 30 % of the way from goal 0
(the centre) to the far corner; the same window in every plane.  Per case:

  update  dymu_update_batch_window_device of the solved stack to the new speed;
  clear   the decrease-only update back to the old speed (the hazard cleared);
  cold    dymu_solve_batch_device of the new speed -- from another build when --cold-libdir
          names its lib directory (the parent commit's), side by side in the same session.

update and clear alternate, so every update starts from the converged map of the old speed
and every clear from that of the new one.  Times are device times from HIP events
(dymu_stats.ms), the median over --reps after one untimed round; passes and tile visits
are the engine's counters, reset_cells is dymu_last_update_stats' out[2].  Each leg runs in
a child process of its own.  Prints one JSON object (kept as profiles/batch_update.json).

    python tools/batch_update_bench.py [--ns 512,1024,2048] [--bs 4,16,64] [--reps 5]
                                       [--cold-libdir DIR]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "planning-path_planning_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from batch_bench import goals_for, spread  # noqa: E402


def hazard(F, goal0, radius=20):
    """(new speed, window): the disc x 2, its ring x 1.1."""
    ny, nx = F.shape
    cx = int(goal0[0] + 0.3 * (nx - 1 - goal0[0]))
    cy = int(goal0[1] + 0.3 * (ny - 1 - goal0[1]))
    j, i = np.mgrid[0:ny, 0:nx]
    d2 = (i - cx) ** 2 + (j - cy) ** 2
    inner, ring = d2 <= radius * radius, (d2 > radius * radius) & (d2 <= (radius + 1) ** 2)
    F1 = F.copy()
    F1[inner] *= 2.0
    F1[ring] *= 1.1
    jj, ii = np.nonzero(inner | ring)
    return F1, (int(ii.min()), int(jj.min()), int(ii.max() - ii.min() + 1),
                int(jj.max() - jj.min() + 1))


def med(st, key):
    return int(np.median([s[key] for s in st]))


def leg(args):
    """One leg in this process: a JSON list of rows on stdout."""
    import dymu

    eng = dymu.Engine(device=int(os.environ.get("LOCAL_RANK", "0")))
    rows = []
    for N in args.ns:
        src0, src1 = eng.alloc(8 * N * N), eng.alloc(8 * N * N)
        eng.synth_speed(src0, N, N, N, 0, 1, args.obst, 3, N // 2, N // 2)
        F = np.empty((N, N))
        eng.d2h(F, src0)
        F1, win = hazard(F, (N // 2, N // 2))
        eng.h2d(src1, F1)
        P = dymu.batch_plane_rows(N)
        for B in args.bs:
            seeds = [(b, gi, gj) for b, (gi, gj) in enumerate(goals_for(F, B))]
            dF, dT = eng.alloc(8 * B * P * N), eng.alloc(8 * B * P * N)
            row = {"n": N, "B": B, "window": list(win)}
            if args.leg == "cold":
                eng.stack_speed(src1, N, 0, N, N, B, dF, N)
                st = [eng.solve_batch_device(dF, dT, N, N, B, N, seeds)
                      for _ in range(args.reps + 1)][1:]
                row.update(ms=spread([s["ms"] for s in st]), passes=med(st, "passes"),
                           tile_visits=med(st, "tile_visits"))
            else:
                wins = [(b, *win) for b in range(B)]
                eng.stack_speed(src0, N, 0, N, N, B, dF, N)
                eng.solve_batch_device(dF, dT, N, N, B, N, seeds)
                up, cl, cells = [], [], []
                for _ in range(args.reps + 1):
                    eng.stack_speed(src1, N, 0, N, N, B, dF, N)
                    up.append(eng.update_batch_window_device(dF, dT, N, N, B, N, seeds, wins))
                    cells.append(eng.last_update_stats()["cells_invalidated"])
                    eng.stack_speed(src0, N, 0, N, N, B, dF, N)
                    cl.append(eng.update_batch_window_device(dF, dT, N, N, B, N, seeds, wins,
                                                             decrease_only=True))
                up, cl = up[1:], cl[1:]
                row.update(update_ms=spread([s["ms"] for s in up]),
                           update_passes=med(up, "passes"),
                           update_tile_visits=med(up, "tile_visits"),
                           reset_cells=int(np.median(cells[1:])),
                           clear_ms=spread([s["ms"] for s in cl]),
                           clear_passes=med(cl, "passes"),
                           clear_tile_visits=med(cl, "tile_visits"))
            rows.append(row)
            print(f"[batch_update_bench] {args.leg} {row}", file=sys.stderr, flush=True)
            eng.free(dF)
            eng.free(dT)
        eng.free(src0)
        eng.free(src1)
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
    ap.add_argument("--bs", default="4,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--obst", type=float, default=0.02)
    ap.add_argument("--cold-libdir", default="")
    ap.add_argument("--timeout", type=float, default=500.0)
    ap.add_argument("--leg", choices=["cold", "update"], default="")
    args = ap.parse_args()
    args.ns = [int(s) for s in str(args.ns).split(",")]
    args.bs = [int(s) for s in str(args.bs).split(",")]
    if args.leg:
        return leg(args)
    cold = child(args, "cold", args.cold_libdir)
    upd = child(args, "update", "")
    rows = []
    for c, u in zip(cold, upd):
        assert (c["n"], c["B"]) == (u["n"], u["B"])
        u.update(cold_ms=c["ms"], cold_passes=c["passes"], cold_tile_visits=c["tile_visits"],
                 cold_over_update=round(c["ms"]["median"] / u["update_ms"]["median"], 3),
                 cold_over_clear=round(c["ms"]["median"] / u["clear_ms"]["median"], 3))
        rows.append(u)
    print(json.dumps({
        "tool": "batch_update_bench",
        "workload": f"config 3: N^2, U(1,5) speed, {args.obst:.0%} obstacles, one map shared by "
                    "B goals (tools/batch_bench.py's); config 5's change: a hazard disc of "
                    "radius 20 (x 2) and its ring (x 1.1), 30 % from goal 0 to the far corner",
        "reps": args.reps,
        "cold_leg": ("another build: " + args.cold_libdir) if args.cold_libdir else "this build",
        "rows": rows,
    }))


if __name__ == "__main__":
    main()
