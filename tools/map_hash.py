"""SHA-256 of the maps of the deterministic schedule (dymu_opts.deterministic = 1:
bit-reproducible), to compare two builds bit for bit: the config-3 grid (bench.py's
workload) at N and the serpentine maze (tools/maze_bench.py) at M.  Run once per
build (DYMU_LIBDIR selects another build) and compare the lines.
usage: python tools/map_hash.py [N = 16384] [M = 4096]"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "planning-path_planning_amd"), os.path.join(ROOT, "tests"),
                os.path.join(ROOT, "tools")]


def digest(T):
    h = hashlib.sha256()
    for r0 in range(0, T.shape[0], 1024):
        h.update(T[r0:r0 + 1024].tobytes())
    return h.hexdigest()


def main():
    import dymu
    import oracle_ffi
    from maze_bench import serpentine

    N = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    M = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    out = {"lib": os.environ.get("DYMU_LIBDIR", "tree")}
    eng = dymu.Engine(deterministic=1)
    for name, n in (("config3", N), ("maze", M)):
        g = (n // 2, n // 2)
        dF, dT = eng.alloc(8 * n * n), eng.alloc(8 * n * n)
        if name == "config3":
            eng.synth_speed(dF, n, n, n, 0, 1, 0.02, 3, g[0], g[1])
        else:
            o = oracle_ffi.load()
            eng.h2d(dF, serpentine(o.synth_speed(n, n, seed=1, obst_frac=0.02, obst_seed=3, goal=g), 64))
        st = eng.solve_device(dF, dT, n, n, n, g[0], g[1])
        T = np.empty((n, n))
        eng.d2h(T, dT)
        eng.free(dF)
        eng.free(dT)
        out[name] = {"grid": n, "sha256": digest(T), "passes": st["passes"],
                     "tile_visits": st["tile_visits"], "inner_sweeps": st["inner_sweeps"]}
        del T
    eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
