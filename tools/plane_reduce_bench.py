#!/usr/bin/env python3
"""Combining the planes of a batch on the device against downloading them.

One N^2 config-3 map (bench.py's workload: splitmix64 U(1,5) speed, 2 % obstacles) shared by
B goals, for N in --ns and B in --bs, on a planner that holds the solved batch.  Per shape
five questions, each answered by two routes:

  device  combineTotalCostMaps("sum" / "max" / "min") over all planes, viaCorridor(0, 1,
          slack) and rendezvous(minimax) -- one kernel over the stack, the result downloaded
          (the combined map, the mask, or the cell);
  host    what a caller does without them: batchTotalCost(b) for every plane the question
          uses, then the same fold in numpy, in the same order and in place.

Both routes download into host arrays allocated once per shape: a fresh numpy array per
download adds the allocator's and the runtime's page-pinning cost to whichever route runs
next (stalls of 20-30 ms were measured that way, on both routes), which says nothing about
either.  The two routes' results are compared bit for bit before anything is timed.  Then
--rounds alternating rounds of (device, host) per question, in one process; wall times are
reported min-max over the rounds.  kernel_ms is the HIP-event time of the reduction's
kernels (lastCombineKernelMs; the corridor's level-mask kernel is not in it), stack_gbps
the bytes of the planes it read divided by that time, next to the 6300 GB/s a copy reaches
on this device.
Prints one JSON object (kept as profiles/plane_reduce.json).

    python tools/plane_reduce_bench.py [--ns 512,1024,2048] [--bs 2,4,16,64] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "planning-path_planning_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_bench import goals_for  # noqa: E402

INF = np.inf
COPY_GBPS = 6300.0
SLACK = 0.05


class Buffers:
    """Host arrays allocated once per shape and reused by both routes."""

    def __init__(self, N, B):
        self.planes = [np.empty((N, N)) for _ in range(B)]
        self.acc, self.out = np.empty((N, N)), np.empty((N, N))
        self.arg, self.dev_arg = (np.empty((N, N), dtype=np.uint32) for _ in range(2))
        self.m = np.empty((N, N), dtype=bool)
        self.mask, self.dev_mask = (np.empty((N, N), dtype=np.uint8) for _ in range(2))


def fold(planes, op, w):
    """The header's fold in place: acc and arg of w."""
    np.copyto(w.acc, planes[0])
    w.arg.fill(0)
    for b, T in enumerate(planes[1:], 1):
        if op == "sum":
            np.add(w.acc, T, out=w.acc)
        else:
            (np.greater if op == "max" else np.less)(T, w.acc, out=w.m)
            np.copyto(w.acc, T, where=w.m)
            w.arg[w.m] = b
    if op == "min":
        w.arg[w.acc == INF] = 0xFFFFFFFF
    return w.acc, w.arg


def argmin_cell(D):
    """The lowest row-major cell that holds the minimum below +inf (argmin's first hit)."""
    k = int(np.argmin(D))
    return k % D.shape[1], k // D.shape[1], float(D.ravel()[k])


def questions(p, B, w):
    """name -> (planes read, device route, host route); both return comparable results."""
    def host_planes(ids):
        for b in ids:  # what batchTotalCost does, into a buffer allocated once
            assert p._lib.dymu_planner_copy_batch_total_cost(p.h, b, w.planes[b], 1) == 1
        return [w.planes[b] for b in ids]

    def dev_combine(op):
        def run():
            s = p.combineTotalCostMaps(op)
            out = p.combinedTotalCost(out=w.out)
            arg = None if op == "sum" else p.combinedPlanes(out=w.dev_arg)
            return out, arg, (s["min_i"], s["min_j"], s["min_value"])
        return run

    def host_combine(op):
        def run():
            out, arg = fold(host_planes(range(B)), op, w)
            return out, None if op == "sum" else arg, argmin_cell(out)
        return run

    def dev_corridor():
        mask, info = p.viaCorridor(0, 1, SLACK, mask=w.dev_mask)
        return mask, None, (info["cell"][0], info["cell"][1], info["D_min"], info["bound"],
                            info["count"], info["box"])

    def host_corridor():
        Ta, Tb = host_planes((0, 1))
        D = np.add(Ta, Tb, out=w.acc)
        i, j, d = argmin_cell(D)
        bound = d * (1.0 + SLACK)
        np.less_equal(D, bound, out=w.m)
        np.copyto(w.mask, w.m, casting="unsafe")
        rows, cols = np.flatnonzero(w.m.any(axis=1)), np.flatnonzero(w.m.any(axis=0))
        return w.mask, None, (i, j, d, bound, int(np.count_nonzero(w.m)),
                              (int(cols[0]), int(rows[0]), int(cols[-1]), int(rows[-1])))

    def dev_rendezvous():
        return None, None, p.rendezvous(minimax=True)

    def host_rendezvous():
        return None, None, argmin_cell(fold(host_planes(range(B)), "max", w)[0])

    q = {op: (B, dev_combine(op), host_combine(op)) for op in ("sum", "max", "min")}
    q["corridor"] = (2, dev_corridor, host_corridor)
    q["rendezvous"] = (B, dev_rendezvous, host_rendezvous)
    return q


def same(a, b):
    for x, y in zip(a[:2], b[:2]):
        if (x is None) != (y is None):
            return False
        if x is not None and not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
            return False
    return tuple(a[2]) == tuple(b[2])


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="512,1024,2048")
    ap.add_argument("--bs", default="2,4,16,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--obst", type=float, default=0.02)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import dymu

    dev = int(os.environ.get("LOCAL_RANK", "0"))
    rows = []
    for N in (int(s) for s in args.ns.split(",")):
        with dymu.Engine(device=dev) as eng:
            src = eng.alloc(8 * N * N)
            eng.synth_speed(src, N, N, N, 0, 1, args.obst, 3, N // 2, N // 2)
            F = np.empty((N, N))
            eng.d2h(F, src)
            eng.free(src)
        p = dymu.Planner(risk_distance=0.5, device=dev)
        assert p.initGlobalLayer(1.0, 0.5, N, N)
        assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
        for B in (int(s) for s in args.bs.split(",")):
            goals = [(float(i), float(j), 0.0, 0.0) for i, j in goals_for(F, B)]
            assert p.computeTotalCostMaps(goals), "the batch does not fit"
            solve_ms = p.lastBatchStats()["ms"]
            for name, (n_read, dev_fn, host_fn) in questions(p, B, Buffers(N, B)).items():
                assert same(dev_fn(), host_fn()), f"{name}: the two routes differ"
                dev_ms, host_ms, k_ms = [], [], []
                for _ in range(args.rounds):
                    dev_ms.append(timed(dev_fn))
                    k_ms.append(p.lastCombineKernelMs())
                    host_ms.append(timed(host_fn))
                k = float(np.median(k_ms))
                gbps = n_read * N * N * 8 / (k * 1e-3) / 1e9
                rows.append({"n": N, "B": B, "question": name, "planes_read": n_read,
                             "batch_solve_ms": round(solve_ms, 4),
                             "device_wall_ms": [round(min(dev_ms), 3), round(max(dev_ms), 3)],
                             "host_wall_ms": [round(min(host_ms), 3), round(max(host_ms), 3)],
                             "host_over_device": round(float(np.median(host_ms) /
                                                             np.median(dev_ms)), 2),
                             "kernel_ms": [round(min(k_ms), 4), round(max(k_ms), 4)],
                             "stack_gbps": round(gbps, 1),
                             "of_copy_rate": round(gbps / COPY_GBPS, 3)})
                print(f"[plane_reduce_bench] {rows[-1]}", file=sys.stderr, flush=True)
        p.close()
    doc = {
        "tool": "plane_reduce_bench",
        "workload": f"config 3: N^2, U(1,5) speed, {args.obst:.0%} obstacles, one map shared by "
                    "B goals (the centre, then uniformly random free interior cells, seed 11); "
                    "questions: sum / max / min over all planes, viaCorridor(0, 1, "
                    f"{SLACK}), rendezvous(minimax)",
        "rounds": args.rounds,
        "routes": {"device": "combineTotalCostMaps / viaCorridor / rendezvous, result downloaded",
                   "host": "batchTotalCost of every plane used, then the same fold in numpy"},
        "checked": "both routes bit-identical before timing",
        "copy_rate_gbps": COPY_GBPS,
        "rows": rows,
    }
    text = json.dumps(doc)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
