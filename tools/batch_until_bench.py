#!/usr/bin/env python3
"""Early exit on target cells against the full solves.

Stacks: one N^2 config-3 map (bench.py's workload: splitmix64 U(1,5) speed, 2 % obstacles)
shared by B goals, for N in --ns and B in --bs, with three target layouts:

  box    the site matrix in a box: the B goals are free cells of the N/4-cell box at the
         centre and every goal's cell is a target in every plane (B x B targets);
  rover  rover to sites: tools/batch_bench.py's goals (anywhere) and ONE target cell, the
         same in every plane, N/5 cells from the centre;
  far    the worst case: the same goals and the far corner of every plane as its target.

Per row: dymu_solve_batch_until_device at the default cadence (device ms from HIP events,
the median over --reps after one untimed run; passes, tile visits, t_closed), the same
with a check after every pass (its passes are the fewest any cadence can run: `overshoot`
is the difference), one timing per cadence of --cadences (DYMU_UNTIL_BATCH, a fresh
context each), and the baseline: dymu_solve_batch_device of the same goals from the
build --base-libdir names (the parent commit's), run in the same session in a child
process of its own.

Single map (--single-n, 0 = skip): dymu_solve_seeds_until_device at that size for K in
--ks random goals, with a target 250 cells from goal 0 and one 3/4 of the way from the
centre to the edge; baseline: the other build's dymu_solve_seeds_device.

Prints one JSON object (kept as profiles/batch_until.json).

    python tools/batch_until_bench.py [--ns 512,1024,2048] [--bs 4,16,64] [--reps 5]
                                      [--cadences 4,8,16,32,64] [--single-n 16384]
                                      [--ks 1,16,256] [--base-libdir DIR]
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

LAYOUTS = ("box", "rover", "far")


def free_from(F, i, j):
    """(i, j) moved right to the next free cell of its row."""
    return i + int(np.argmax(np.isfinite(F[j, i:]))), j


def box_goals(F, B):
    """B distinct free interior cells of the N/4 box at the centre (seed 13)."""
    ny, nx = F.shape
    rng = np.random.default_rng(13)
    x0, y0, w = nx // 2 - nx // 8, ny // 2 - ny // 8, nx // 4
    out = {}
    while len(out) < B:
        i, j = int(rng.integers(x0, x0 + w)), int(rng.integers(y0, y0 + w))
        if np.isfinite(F[j - 1:j + 2, i - 1:i + 2]).all():
            out[(i, j)] = None
    return list(out)


def layout(F, B, name):
    """(goals, targets (plane, i, j))."""
    ny, nx = F.shape
    if name == "box":
        goals = box_goals(F, B)
        return goals, [(b, i, j) for b in range(B) for i, j in goals]
    goals = goals_for(F, B)
    cell = free_from(F, nx // 2 + nx // 5, ny // 2 + 3) if name == "rover" else \
        free_from(F[:, ::-1], 0, ny - 1)
    if name == "far":
        cell = (nx - 1 - cell[0], cell[1])
    return goals, [(b, *cell) for b in range(B)]


def med(st, key):
    return int(np.median([s[key] for s in st]))


def stack_rows(args, eng_of):
    import dymu

    eng = eng_of({})
    rows = []
    for N in args.ns:
        src = eng.alloc(8 * N * N)
        eng.synth_speed(src, N, N, N, 0, 1, args.obst, 3, N // 2, N // 2)
        F = np.empty((N, N))
        eng.d2h(F, src)
        P = dymu.batch_plane_rows(N)
        for B in args.bs:
            dF, dT = eng.alloc(8 * B * P * N), eng.alloc(8 * B * P * N)
            eng.stack_speed(src, N, 0, N, N, B, dF, N)
            for name in LAYOUTS:
                goals, tg = layout(F, B, name)
                seeds = [(b, gi, gj) for b, (gi, gj) in enumerate(goals)]
                row = {"n": N, "B": B, "layout": name, "targets": len(tg)}
                if args.leg == "base":
                    if name == "far":
                        continue  # rover's goals
                    st = [eng.solve_batch_device(dF, dT, N, N, B, N, seeds)
                          for _ in range(args.reps + 1)][1:]
                    row.update(ms=spread([s["ms"] for s in st]), passes=med(st, "passes"),
                               tile_visits=med(st, "tile_visits"))
                else:
                    def run(e):
                        return [e.solve_batch_until_device(dF, dT, N, N, B, N, seeds, tg)
                                for _ in range(args.reps + 1)][1:]
                    r = run(eng)
                    st = [x[2] for x in r]
                    row.update(ms=spread([s["ms"] for s in st]), passes=med(st, "passes"),
                               tile_visits=med(st, "tile_visits"), t_closed=r[0][0],
                               cadence=f"{eng_of.first}+{eng_of.batch}")
                    e1 = eng_of({"passes_per_check": 1})
                    one = e1.solve_batch_until_device(dF, dT, N, N, B, N, seeds, tg)[2]
                    e1.close()
                    row.update(min_passes=one["passes"], overshoot=row["passes"] - one["passes"],
                               every_pass_ms=round(one["ms"], 4))
                    cad = {}
                    for k in args.cadences:
                        ek = eng_of({}, until_batch=k)
                        sk = [x[2] for x in run(ek)]
                        ek.close()
                        cad[str(k)] = {"ms": round(float(np.median([s["ms"] for s in sk])), 4),
                                       "passes": med(sk, "passes")}
                    row["by_cadence"] = cad
                rows.append(row)
                print(f"[batch_until_bench] {args.leg} {row}", file=sys.stderr, flush=True)
            eng.free(dF)
            eng.free(dT)
        eng.free(src)
    eng.close()
    return rows


def single_rows(args, eng_of):
    N = args.single_n
    if not N:
        return []
    eng = eng_of({})
    dF, dT = eng.alloc(8 * N * N), eng.alloc(8 * N * N)
    eng.synth_speed(dF, N, N, N, 0, 1, args.obst, 3, N // 2, N // 2)
    one = np.empty(1)

    def free_cell(i, j):  # moved right to the next finite-speed cell (no download of F)
        while True:
            eng._lib.dymu_memcpy_d2h(eng.ctx, one.ctypes.data, dF + 8 * (j * N + i), 8)
            if np.isfinite(one[0]):
                return i, j
            i += 1

    rng = np.random.default_rng(17)
    rows = []
    for K in args.ks:
        goals = [(N // 2, N // 2)] + [tuple(int(v) for v in rng.integers(2, N - 2, 2))
                                      for _ in range(K - 1)]
        seeds = [(i, j, 0.0) for i, j in goals]
        g = np.array(goals, dtype=np.float64)
        if args.leg == "base":
            st = [eng.solve_seeds_device(dF, dT, N, N, N, seeds) for _ in range(args.reps + 1)][1:]
            rows.append({"n": N, "K": K, "ms": spread([s["ms"] for s in st]),
                         "passes": med(st, "passes"), "tile_visits": med(st, "tile_visits")})
        else:
            for name, cell in (("250 cells", free_cell(N // 2 + 250, N // 2)),
                               ("3/4 to the edge", free_cell(N // 2 + 3 * N // 8, N // 2))):
                r = [eng.solve_seeds_until_device(dF, dT, N, N, N, seeds, [cell])
                     for _ in range(args.reps + 1)][1:]
                st = [x[1] for x in r]
                e1 = eng_of({"passes_per_check": 1})
                one_p = e1.solve_seeds_until_device(dF, dT, N, N, N, seeds, [cell])[1]
                e1.close()
                rows.append({"n": N, "K": K, "target": name, "cell": list(cell),
                             "nearest_goal_cells": round(float(np.hypot(
                                 g[:, 0] - cell[0], g[:, 1] - cell[1]).min()), 1),
                             "ms": spread([s["ms"] for s in st]), "passes": med(st, "passes"),
                             "tile_visits": med(st, "tile_visits"), "t_closed": r[0][0],
                             "min_passes": one_p["passes"],
                             "overshoot": med(st, "passes") - one_p["passes"],
                             "cadence": f"{eng_of.first}+{eng_of.batch}"})
        print(f"[batch_until_bench] {args.leg} {rows[-1]}", file=sys.stderr, flush=True)
    eng.free(dF)
    eng.free(dT)
    eng.close()
    return rows


def leg(args):
    """One leg in this process: a JSON object on stdout."""
    import dymu

    dev = int(os.environ.get("LOCAL_RANK", "0"))

    def eng_of(opts, until_batch=None):
        # DYMU_UNTIL_BATCH is read when a context is made
        old = os.environ.get("DYMU_UNTIL_BATCH")
        if until_batch:
            os.environ["DYMU_UNTIL_BATCH"] = str(until_batch)
        try:
            return dymu.Engine(device=dev, **opts)
        finally:
            if until_batch:
                os.environ.pop("DYMU_UNTIL_BATCH")
                if old is not None:
                    os.environ["DYMU_UNTIL_BATCH"] = old

    eng_of.first = int(os.environ.get("DYMU_FIRST_BATCH", "16"))
    eng_of.batch = int(os.environ.get("DYMU_UNTIL_BATCH", "16"))
    print(json.dumps({"stacks": stack_rows(args, eng_of), "single": single_rows(args, eng_of)}))


def child(args, which, libdir):
    env = dict(os.environ)
    if libdir:
        env["DYMU_LIBDIR"] = os.path.abspath(libdir)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", which, "--reps", str(args.reps),
           "--ns", ",".join(map(str, args.ns)), "--bs", ",".join(map(str, args.bs)),
           "--cadences", ",".join(map(str, args.cadences)), "--single-n", str(args.single_n),
           "--ks", ",".join(map(str, args.ks)), "--obst", str(args.obst)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, check=True, timeout=args.timeout)
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def ints(s):
    return [int(v) for v in str(s).split(",") if v != ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="512,1024,2048")
    ap.add_argument("--bs", default="4,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cadences", default="4,8,16,32,64")
    ap.add_argument("--single-n", type=int, default=16384)
    ap.add_argument("--ks", default="1,16,256")
    ap.add_argument("--obst", type=float, default=0.02)
    ap.add_argument("--base-libdir", default="")
    ap.add_argument("--timeout", type=float, default=900.0)
    ap.add_argument("--leg", choices=["base", "until"], default="")
    args = ap.parse_args()
    args.ns, args.bs, args.cadences, args.ks = (ints(args.ns), ints(args.bs),
                                                ints(args.cadences), ints(args.ks))
    if args.leg:
        return leg(args)
    base = child(args, "base", args.base_libdir)
    unt = child(args, "until", "")
    full = {(r["n"], r["B"], r["layout"]): r for r in base["stacks"]}
    for r in unt["stacks"]:
        f = full[(r["n"], r["B"], "box" if r["layout"] == "box" else "rover")]
        r.update(full_ms=f["ms"], full_passes=f["passes"], full_tile_visits=f["tile_visits"],
                 full_over_until=round(f["ms"]["median"] / r["ms"]["median"], 3))
    fs = {r["K"]: r for r in base["single"]}
    for r in unt["single"]:
        f = fs[r["K"]]
        r.update(full_ms=f["ms"], full_passes=f["passes"], full_tile_visits=f["tile_visits"],
                 full_over_until=round(f["ms"]["median"] / r["ms"]["median"], 3))
    print(json.dumps({
        "tool": "batch_until_bench",
        "workload": f"config 3: N^2, U(1,5) speed, {args.obst:.0%} obstacles, one map shared by "
                    "B goals; layouts box / rover / far (see the tool's docstring)",
        "reps": args.reps,
        "base_leg": ("another build: " + args.base_libdir) if args.base_libdir else "this build",
        "stacks": unt["stacks"],
        "single": unt["single"],
    }))


if __name__ == "__main__":
    main()
