#!/usr/bin/env python3
"""dymu_route_fields_device -- every cell's node route at once -- after one config-3 solve.

One N^2 config-3 grid (bench.py's workload: splitmix64 U(1,5) speed, obstacles, goal at the
centre) is solved once on the engine.  Then, in alternating rounds in one process:

  a  route_fields: sink, axis and diag only
  b  ... plus one field's integral, minimum and maximum (the speed)
  c  ... plus four fields (the speed and three more U(1,5) maps without obstacles)
  L  dymu_goal_labels_device on the same map: the nearest existing kernel of this shape
  S  dymu_arrive_paths_device, records only, for M = 4096 starts: what getArrivingStats
     runs, the only way to these numbers so far

Per request: the whole call (host clock from the call to the last kernel's event), its
stages by HIP events (init and roots, the rounds with their counter reads, finalize), the
download of the outputs into host memory, the rounds, the bytes a round moves by
construction -- every cell's state read, the state at its pointer read, the new state
written: an upper bound, a finished cell moves 8 bytes -- and that figure over the mean
round's time against the copy rate the README quotes.  Every run also compares `length` with
the arriving descent's length from the same 4096 starts; the run to read that from is the
one without obstacles (--obst 0), where the octile metric's 8.2 % is the expectation.
Prints one JSON line and writes it to --out.

    python tools/route_fields_bench.py [--n 16384] [--rounds 3] [--obst 0.02]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "planning-path_planning_amd"))

COPY_RATE_TBS = 6.3  # README: the device-to-device copy rate measured on this part


def spread(v):
    return {"min": round(min(v), 3), "median": round(float(np.median(v)), 3),
            "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--obst", type=float, default=0.02)
    ap.add_argument("--paths", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "route_fields.json"))
    args = ap.parse_args()
    import dymu

    N = args.n
    n = N * N
    g = (N // 2, N // 2)
    eng = dymu.Engine(device=int(os.environ.get("LOCAL_RANK", "0")))
    dF, dT = eng.alloc(8 * n), eng.alloc(8 * n)
    eng.synth_speed(dF, N, N, N, 0, 1, args.obst, 3, g[0], g[1])
    more = [eng.alloc(8 * n) for _ in range(3)]
    for k, d in enumerate(more):
        eng.synth_speed(d, N, N, N, 0, 11 + k, 0.0, 3, g[0], g[1])
    solve = eng.solve_device(dF, dT, N, N, N, *g)
    seeds = [g + (0.0,)]
    fields = [(dF, N)] + [(d, N) for d in more]

    # the outputs of the largest request, allocated once (plain cached memory, like the
    # workspace); a request uses the first of them
    u32 = [eng.alloc_cached(4 * n) for _ in range(3)]
    f64 = [eng.alloc_cached(8 * n) for _ in range(1 + 12)]
    requests = {
        "a": (0, dymu.Engine.route_out(N, sink=u32[0], axis=u32[1], diag=u32[2])),
        "b": (1, dymu.Engine.route_out(N, sink=u32[0], axis=u32[1], diag=u32[2],
                                       integral=f64[1:2], vmin=f64[5:6], vmax=f64[9:10])),
        "c": (4, dymu.Engine.route_out(N, sink=u32[0], axis=u32[1], diag=u32[2],
                                       integral=f64[1:5], vmin=f64[5:9], vmax=f64[9:13])),
    }
    need = {k: eng.route_fields_workspace(N, N, nf, o) for k, (nf, o) in requests.items()}
    ws_bytes = max(need.values())
    ws = eng.alloc_cached(ws_bytes)
    d_label = eng.alloc_cached(4 * n)
    host = np.empty(n, dtype=np.float64)  # one host buffer, reused by every download

    rng = np.random.default_rng(7)
    xy = rng.uniform(2, N - 3, (args.paths, 2))

    def run_route(key, download=True):
        nf, out = requests[key]
        t0 = time.perf_counter()
        r = eng.route_fields(dT, N, N, N, 1.0, seeds, fields[:nf], out, ws, ws_bytes)
        ms = eng.last_route_fields_ms()  # waits for the last kernel
        wall = (time.perf_counter() - t0) * 1e3
        st = eng.last_route_fields_stages()
        t0 = time.perf_counter()
        if download:
            for d in u32:
                eng.d2h(host[:n // 2].view(np.uint32), d)
            for d in f64[1:1 + nf] + f64[5:5 + nf] + f64[9:9 + nf]:
                eng.d2h(host, d)
        down = (time.perf_counter() - t0) * 1e3
        return r, wall, ms, st, down

    for key in requests:  # first launches: code object loads
        run_route(key, download=False)
    eng.goal_labels_device(dT, N, N, N, seeds, d_label=d_label, download=False)
    eng.arrive_paths(dT, N, N, N, 1.0, g[0], g[1], 0.4, xy[:64], 1 << 20, store=False)

    acc = {k: {"call": [], "kernels": [], "init": [], "rounds_ms": [], "final": [], "down": [],
               "rounds": 0} for k in requests}
    lab = {"call": [], "kernels": [], "rounds": 0}
    arr = {"call": [], "kernel": []}
    rec = None
    for _ in range(args.rounds):
        for key in requests:
            r, wall, ms, st, down = run_route(key)
            a = acc[key]
            a["rounds"] = r
            a["call"].append(wall)
            a["kernels"].append(ms)
            a["init"].append(st[0])
            a["rounds_ms"].append(st[1])
            a["final"].append(st[2])
            a["down"].append(down)
        t0 = time.perf_counter()
        _, lab["rounds"] = eng.goal_labels_device(dT, N, N, N, seeds, d_label=d_label,
                                                  download=False)
        lab["call"].append((time.perf_counter() - t0) * 1e3)
        lab["kernels"].append(eng.last_labels_ms())
        t0 = time.perf_counter()
        _, _, rec = eng.arrive_paths(dT, N, N, N, 1.0, g[0], g[1], 0.4, xy, 1 << 20, store=False)
        arr["call"].append((time.perf_counter() - t0) * 1e3)
        arr["kernel"].append(eng.last_arrive_ms())

    rows = {}
    for key, (nf, out) in requests.items():
        a = acc[key]
        carried = 4 + 8 + 24 * nf  # next, the two counts, three aggregates a field
        per_round = 3 * carried * n
        round_ms = float(np.median(a["rounds_ms"])) / a["rounds"]
        rows[key] = {
            "fields": nf, "rounds": a["rounds"], "workspace_GB": round(need[key] / 1e9, 2),
            "call_ms": spread(a["call"]), "kernels_ms": spread(a["kernels"]),
            "init_ms": spread(a["init"]), "rounds_ms": spread(a["rounds_ms"]),
            "finalize_ms": spread(a["final"]), "download_ms": spread(a["down"]),
            "state_bytes_per_cell": carried,
            "round_bytes_upper_GB": round(per_round / 1e9, 2),
            "mean_round_ms": round(round_ms, 3),
            "round_TBs_upper": round(per_round / round_ms / 1e9, 3),
            "share_of_copy_rate_upper": round(per_round / round_ms / 1e9 / COPY_RATE_TBS, 3),
        }
    result = {
        "tool": "route_fields_bench",
        "workload": f"config 3: {N}x{N}, U(1,5) speed, {args.obst:.0%} obstacles, goal centre",
        "solve": {"ms": round(solve["ms"], 2), "passes": solve["passes"]},
        "alternating_rounds": args.rounds,
        "note": "min / median / max over the alternating rounds of one process is the spread. "
                "round_bytes_upper: 3 x the carried state of every cell (own state read, the "
                "state at the pointer gathered, the new state written); a finished cell moves "
                "8 bytes, so the rate is an upper bound of what a round moves.",
        "copy_rate_TBs": COPY_RATE_TBS,
        "route_fields": rows,
        "goal_labels": {"rounds": lab["rounds"], "call_ms": spread(lab["call"]),
                        "kernels_ms": spread(lab["kernels"])},
        "arrive_stats": {"M": args.paths, "call_ms": spread(arr["call"]),
                         "kernel_ms": spread(arr["kernel"]),
                         "arrived": int((rec["status"] == 1).sum())},
        "lds_stage": "not tried",
    }
    # the route's outputs against the arriving descent's records at the same starts' nodes
    nf, out = requests["a"]
    full = dymu.Engine.route_out(N, sink=u32[0], axis=u32[1], diag=u32[2], length=f64[0])
    assert eng.route_fields_workspace(N, N, 0, full) <= ws_bytes
    eng.route_fields(dT, N, N, N, 1.0, seeds, [], full, ws, ws_bytes)
    eng.d2h(host, f64[0])
    ni, nj = (xy[:, 0] + 0.5).astype(np.int64), (xy[:, 1] + 0.5).astype(np.int64)
    length = host.reshape(N, N)[nj, ni].copy()
    ok = (rec["status"] == 1) & np.isfinite(length) & (rec["length"] > 0)
    ratio = length[ok] / rec["length"][ok]
    result["length_vs_arriving_descent"] = {
        "starts": int(ok.sum()),
        "arrived_iff_routed": bool(np.array_equal(rec["status"] == 1, np.isfinite(length))),
        "ratio_median": round(float(np.median(ratio)), 4),
        "ratio_max": round(float(ratio.max()), 4), "ratio_min": round(float(ratio.min()), 4),
        "note": "route length (octile, from the start's node) over the arriving descent's "
                "length (from the start itself, at most 0.71 res from its node)"}
    for d in [dF, dT, ws, d_label] + more + u32 + f64:
        eng.free(d)
    eng.close()
    line = json.dumps(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
