"""References for goal sets, in plain Python / numpy.

* ``fmm_seeds``  -- the reference FMM over a list of seeds: oracle.c's fmm_heap (pop key
  (T, first-insertion sequence), nb4 order, the oracle's Eikonal update) with T initialised
  to the smallest t0 per seed cell instead of 0 at one goal.
* ``labels_from_T`` -- the nearest-goal label of every cell from a total-cost map alone,
  by the definition in include/dymu_fim.h.
* ``planner_case`` -- the map, goals and starts shared by the CPU and the GPU planner tests.
"""
import heapq

import numpy as np

NONE = 0xFFFFFFFF


def fmm_seeds(oracle, F, seeds):
    """T of the converged multi-source FMM.  seeds: (i, j, t0) tuples."""
    F = np.ascontiguousarray(F, dtype=np.float64)
    ny, nx = F.shape
    inf = float("inf")
    T = [inf] * (nx * ny)
    Fl = F.ravel().tolist()
    closed = bytearray(nx * ny)
    seq = {}
    for i, j, t0 in seeds:
        k = j * nx + i
        if k not in seq:
            seq[k] = len(seq)
        T[k] = min(T[k], float(t0))
    heap = [(T[k], s, k) for k, s in seq.items()]
    heapq.heapify(heap)
    eik = oracle.eikonal
    while heap:
        t, _, node = heapq.heappop(heap)
        if closed[node] or t != T[node]:
            continue  # stale entry
        closed[node] = 1
        i, j = node % nx, node // nx
        for ii, jj in ((i, j - 1), (i - 1, j), (i + 1, j), (i, j + 1)):
            if ii < 0 or jj < 0 or ii >= nx or jj >= ny:
                continue
            nb = jj * nx + ii
            if closed[nb] or not Fl[nb] < inf:
                continue
            ts = T[nb - nx] if jj > 0 else inf
            tn = T[nb + nx] if jj + 1 < ny else inf
            tw = T[nb - 1] if ii > 0 else inf
            te = T[nb + 1] if ii + 1 < nx else inf
            tc = eik(min(tw, te), min(tn, ts), Fl[nb])
            if tc < T[nb]:
                if T[nb] == inf:
                    seq[nb] = len(seq)
                T[nb] = tc
                heapq.heappush(heap, (tc, seq[nb], nb))
    return np.array(T).reshape(ny, nx)


def labels_from_T(T, seeds):
    """uint32 [ny, nx]: the seed each cell drains to, NONE for none.
    parent(c): the first of (i,j-1), (i-1,j), (i+1,j), (i,j+1) holding the smallest T, if
    strictly below T[c]; a root is a seed cell whose T is bitwise its (smallest) t0, lowest
    index first; everything else takes its parent's label, in ascending T."""
    T = np.ascontiguousarray(T, dtype=np.float64)
    ny, nx = T.shape
    n = nx * ny
    t = T.ravel()
    pad = np.full((ny + 2, nx + 2), np.inf)
    pad[1:-1, 1:-1] = T
    nbv = np.stack([pad[:-2, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:], pad[2:, 1:-1]]).reshape(4, n)
    first = np.argmin(nbv, axis=0)  # the first smallest
    best = nbv[first, np.arange(n)]
    idx = np.arange(n)
    par = np.stack([idx - nx, idx - 1, idx + 1, idx + nx])[first, idx]
    has = np.isfinite(t) & (best < t)
    lab = np.full(n, NONE, dtype=np.uint32)
    root = np.zeros(n, dtype=bool)
    for k in range(len(seeds) - 1, -1, -1):  # descending: the lowest index is written last
        i, j, t0 = seeds[k]
        c = j * nx + i
        if np.float64(t[c]).tobytes() == np.float64(t0 + 0.0).tobytes():
            lab[c] = k
            root[c] = True
    order = np.argsort(t, kind="stable")
    for c in order:
        if not t[c] < np.inf:
            break
        if root[c] or not has[c]:
            continue
        lab[c] = lab[par[c]]
    return lab.reshape(ny, nx)


# ---- the planner case shared by tests/test_goal_sets_host.py and test_gpu_goal_sets.py ----
OFF = (100.0, 200.0)
RD = 0.5  # risk_distance: tau = min(0.4, RD)
NX, NY = 97, 61
GOALS_IJ = [(70, 40), (12, 9), (30, 50)]
HEADINGS = [1.25, -0.5, 2.0]
OFFSETS = [0.0, 6.5, 0.0]


def planner_case(dymu, oracle):
    """(planner, F, seeds, goals, starts): 97x61, U(1,5) speed with 2 % obstacles (none
    next to a goal), three goals -- one with an offset -- and 200 uniform starts."""
    F = oracle.synth_speed(NX, NY, seed=21, obst_frac=0.02, goal=GOALS_IJ[0])
    for gi, gj in GOALS_IJ:
        blk = F[gj - 1:gj + 2, gi - 1:gi + 2]
        blk[~np.isfinite(blk)] = 3.0
    p = dymu.Planner(risk_distance=RD)
    assert p.initGlobalLayer(1.0, 0.5, NX, NY, offset=OFF)
    assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
    goals = [(OFF[0] + i, OFF[1] + j, 0.0, h) for (i, j), h in zip(GOALS_IJ, HEADINGS)]
    seeds = [(i, j, t0) for (i, j), t0 in zip(GOALS_IJ, OFFSETS)]
    rng = np.random.default_rng(7)
    xy = np.stack([rng.uniform(2, NX - 3, 200), rng.uniform(2, NY - 3, 200)], axis=1)
    starts = [(OFF[0] + x, OFF[1] + y, 0.0, 0.01 * k) for k, (x, y) in enumerate(xy)]
    return p, F, seeds, goals, starts
