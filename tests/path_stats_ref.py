"""The per-path record (include/dymu_fim.h, dymu_path_stat) rebuilt in numpy from the
waypoints getPaths returns: test infrastructure for getPathStats.  Every sum is sequential
(np.add.accumulate), in the order the definition gives; products and square roots are
single IEEE operations, so the result is the host loop's bit for bit."""
import numpy as np

PATH_FIELDS = 4


def grid_u32(d):
    """The reference's (uint) cast of a double: through int64, then the low 32 bits."""
    d = np.asarray(d, dtype=np.float64)
    ok = (d > -9.2e18) & (d < 9.2e18)  # NaN fails both
    t = np.where(ok, d, 0.0).astype(np.int64)  # truncation toward zero
    return (t & 0xFFFFFFFF).astype(np.int64)


def nearest_nodes(xy, res, nx, ny):
    """(i, j, on_grid) of every waypoint's nearest node by nearestIndex's rule."""
    i = grid_u32(xy[:, 0] / res + 0.5)
    j = grid_u32(xy[:, 1] / res + 0.5)
    return i, j, (i < nx) & (j < ny)


def _seq_sum(a):
    """0.0 + a[0] + a[1] + ... added left to right."""
    if len(a) == 0:
        return 0.0
    return float(np.add.accumulate(np.concatenate([[0.0], a]))[-1])


def empty_record():
    return dict(count=0, length=0.0, last_hop=0.0, integral=[0.0] * PATH_FIELDS,
                vmin=[np.inf] * PATH_FIELDS, vmax=[-np.inf] * PATH_FIELDS,
                skipped=[0] * PATH_FIELDS)


def path_record(xy, res, fields):
    """The record of the waypoints xy (n, 2; grid-local metres) over `fields`, a list of
    [ny, nx] arrays (slot 0 first): a dict of count, length, last_hop and per-slot lists."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    r = empty_record()
    n = len(xy)
    r["count"] = n
    if n == 0:
        return r
    dx = xy[:-1, 0] - xy[1:, 0]
    dy = xy[:-1, 1] - xy[1:, 1]
    seg = np.sqrt(dx * dx + dy * dy)
    r["length"] = _seq_sum(seg)
    r["last_hop"] = float(seg[-1]) if n >= 2 else 0.0
    for f, fld in enumerate(fields):
        ny, nx = fld.shape
        i, j, on = nearest_nodes(xy, res, nx, ny)
        v = np.full(n, np.nan)
        v[on] = fld[j[on], i[on]]
        counts = on & np.isfinite(v)
        r["skipped"][f] = int((~counts).sum())
        with np.errstate(invalid="ignore"):  # inf * 0 of a sample that does not count
            prod = v[:-1] * seg
        r["integral"][f] = _seq_sum(prod[counts[:-1]])
        m, M = np.inf, -np.inf
        for u in v[counts]:
            m = u if u < m else m
            M = u if u > M else M
        r["vmin"][f], r["vmax"][f] = float(m), float(M)
    return r


def same_record(rec, ref):
    """None if the structured record `rec` equals the dict `ref` in every member exactly,
    else the name of the first member that differs."""
    if int(rec["count"]) != ref["count"]:
        return "count"
    for k in ("length", "last_hop"):
        if float(rec[k]) != ref[k]:
            return k
    for k in ("integral", "vmin", "vmax", "skipped"):
        for f in range(PATH_FIELDS):
            if rec[k][f] != ref[k][f]:
                return f"{k}[{f}]"
    return None


def close_record(rec, ref, rel):
    """same_record with the float members within `rel` relative."""
    if int(rec["count"]) != ref["count"]:
        return "count"
    for k in ("length", "last_hop"):
        if abs(float(rec[k]) - ref[k]) > rel * max(abs(ref[k]), 1e-300):
            return k
    for f in range(PATH_FIELDS):
        if rec["skipped"][f] != ref["skipped"][f]:
            return f"skipped[{f}]"
        for k in ("integral", "vmin", "vmax"):
            a, b = float(rec[k][f]), float(ref[k][f])
            if a != b and not abs(a - b) <= rel * abs(b):
                return f"{k}[{f}]"
    return None


def off_grid_map(nx=32, ny=16):
    """A loaded map on which a stored waypoint has its nearest node off the grid.

    Towards the east (a ramp T = nx - 1 - i) that cannot happen: a step starts in a cell
    with x / res < nx - 1 and is at most 0.4 cell, so x / res + 0.5 < nx - 0.1 -- the
    descent leaves the grid, but every stored waypoint still has a node (asserted
    below).  Towards the west it can: positions with x / res in (-1, 0) still truncate
    to cell 0, where the bilinear form extrapolates, so a step can exceed 0.5 cell and
    land below x / res = -1.5, whose nearest index wraps past the grid.  Columns 0 .. 2
    hold 0, 10, 0.1 (a steep gradient along x at node 0, a flat one at node 1) on a
    slope of 1 per row.  Returns (T, goal, start)."""
    base = np.array([0.0, 10.0, 0.1] + [30.0 + 20.0 * k for k in range(nx - 3)])
    T = base[None, :] + np.arange(ny, dtype=float)[:, None]
    return T, (20, 8), (0.65, 8.3, 0.0, 0.0)
