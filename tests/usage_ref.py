"""How much of the map drains through every cell, in plain Python / numpy:
the definition of include/dymu_fim.h, a function of the total-cost map T, a seed list and an
optional weight map alone.  It sits on route_ref's parents and roots: the cells are taken in
descending T, each added into its parent (a child is strictly higher than its parent, so it
is complete by then), and the same order backwards hands the sinks down from the roots."""
import numpy as np

import route_ref

NONE = route_ref.NONE


def forest(T, seeds):
    """(par [n] int64 with -1 for none and for the roots, root {cell: k})"""
    par, _ = route_ref.parents(T)
    root = route_ref.roots(T, seeds)
    par = par.copy()
    for c in root:
        par[c] = -1  # a root is terminal even with a lower neighbour
    return par, root


def route_usage(T, seeds, weights=None):
    """dict of [ny, nx] maps usage (uint64), far (float64), sink (uint32) and catchment
    (uint64 per seed), by the definition."""
    T = np.ascontiguousarray(T, dtype=np.float64)
    ny, nx = T.shape
    n = nx * ny
    t = T.ravel()
    par, root = forest(T, seeds)
    with np.errstate(invalid="ignore"):
        live = t < np.inf
    w = np.ones(n, dtype=np.uint64) if weights is None else \
        np.ascontiguousarray(weights, dtype=np.uint32).ravel().astype(np.uint64)
    # plain Python lists and integers: no overflow, and quick enough for 2e6 cells
    par_l, live_l, t_l = par.tolist(), live.tolist(), t.tolist()
    usage = [wc if lv else 0 for wc, lv in zip(w.tolist(), live_l)]
    far = [tc if lv else 0.0 for tc, lv in zip(t_l, live_l)]
    order = [c for c in np.argsort(t, kind="stable").tolist() if live_l[c]]
    for c in reversed(order):
        p = par_l[c]
        if p >= 0:
            usage[p] += usage[c]
            if far[c] > far[p]:
                far[p] = far[c]
    sink = [NONE] * n
    for c, k in root.items():
        sink[c] = k
    for c in order:
        if par_l[c] >= 0:
            sink[c] = sink[par_l[c]]
    sink = np.array(sink, dtype=np.uint32)
    has = sink != NONE
    usage = np.where(has, np.array(usage, dtype=np.uint64), np.uint64(0))
    far = np.where(has, np.array(far, dtype=np.float64), np.nan)
    catchment = np.zeros(len(seeds), dtype=np.uint64)
    for c, k in root.items():
        catchment[k] = usage[c]
    shape = (ny, nx)
    return {"usage": usage.reshape(shape), "far": far.reshape(shape),
            "sink": sink.reshape(shape), "catchment": catchment}
