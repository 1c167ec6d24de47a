"""Every cell's node route to the goal, in plain Python / numpy: the
definition of include/dymu_fim.h, a function of the total-cost map T and a seed list alone.

``parents`` evaluates the hop rule at every node, ``route_fields`` takes the cells in
ascending T, each from its parent (the integral as w(c) + integral[rp(c)]), and ``walk``
replays one cell's chain node by node for the tests that check the route itself."""
import numpy as np

NONE = 0xFFFFFFFF
DIAG = 0.7071067811865476   # a diagonal hop's score per unit of T
SQRT2 = 1.4142135623730951  # a diagonal hop's length per res
# the rule's neighbour order, (di, dj)
ORDER = ((0, -1), (-1, 0), (1, 0), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))


def rmin(a, b):
    """the minimum with -0.0 below +0.0"""
    return b if (b < a or (b == a and np.signbit(b))) else a


def rmax(a, b):
    return b if (b > a or (b == a and not np.signbit(b))) else a


def parents(T):
    """(par [n] int64, kind [n] int8): the route parent of every cell as a flat index
    (-1: none -- +inf, NaN or a dead end) and the hop's kind (0 axis, 1 diagonal)."""
    T = np.ascontiguousarray(T, dtype=np.float64)
    ny, nx = T.shape
    pad = np.full((ny + 2, nx + 2), np.inf)
    pad[1:-1, 1:-1] = T

    def nb(di, dj):
        return pad[1 + dj:1 + dj + ny, 1 + di:1 + di + nx]

    best = np.full((ny, nx), -1.0)
    par = np.full((ny, nx), -1, dtype=np.int64)
    kind = np.zeros((ny, nx), dtype=np.int8)
    idx = np.arange(nx * ny, dtype=np.int64).reshape(ny, nx)
    with np.errstate(invalid="ignore"):
        live = T < np.inf
        for di, dj in ORDER:
            tm = nb(di, dj)
            ok = live & (tm < T)
            d = di != 0 and dj != 0
            if d:  # no corner is cut: both side nodes are finite
                ok &= (nb(di, 0) < np.inf) & (nb(0, dj) < np.inf)
            s = (T - tm) * DIAG if d else T - tm
            take = ok & (s > best)  # the first of the largest score wins
            best = np.where(take, s, best)
            par = np.where(take, idx + dj * nx + di, par)
            kind = np.where(take, np.int8(d), kind)
    return par.ravel(), kind.ravel()


def roots(T, seeds):
    """{cell: k}: seed k's cell is a root iff its T is bitwise t0_k; among duplicates the
    smallest t0 (only it can match T), the lowest k among equal ones."""
    T = np.ascontiguousarray(T, dtype=np.float64)
    nx = T.shape[1]
    out = {}
    for k in range(len(seeds) - 1, -1, -1):  # descending: the lowest k is written last
        i, j, t0 = seeds[k][0], seeds[k][1], (seeds[k][2] if len(seeds[k]) > 2 else 0.0)
        if np.float64(T[j, i]).tobytes() == np.float64(t0 + 0.0).tobytes():
            out[j * nx + i] = k
    return out


def route_fields(T, res, seeds, fields=()):
    """dict of [ny, nx] maps sink, axis, diag, length and [len(fields), ny, nx] maps
    integral, vmin, vmax, by the definition."""
    T = np.ascontiguousarray(T, dtype=np.float64)
    ny, nx = T.shape
    n = nx * ny
    t = T.ravel()
    fl = [np.ascontiguousarray(f, dtype=np.float64).ravel() for f in fields]
    nf = len(fl)
    par, kind = parents(T)
    root = roots(T, seeds)
    sink = np.full(n, NONE, dtype=np.uint32)
    axis = np.zeros(n, dtype=np.uint32)
    diag = np.zeros(n, dtype=np.uint32)
    integ = np.zeros((nf, n))
    vmin = np.full((nf, n), np.inf)
    vmax = np.full((nf, n), -np.inf)
    res = np.float64(res)
    seg = (res, res * np.float64(SQRT2))
    for c, k in root.items():
        sink[c] = k
        for f in range(nf):
            if np.isfinite(fl[f][c]):
                vmin[f, c] = vmax[f, c] = fl[f][c]
    for c in np.argsort(t, kind="stable"):
        if not t[c] < np.inf:
            break  # +inf and NaN sort last
        if c in root or par[c] < 0:
            continue
        p = par[c]
        if sink[p] == NONE:
            continue  # drains to a dead end
        sink[c] = sink[p]
        axis[c] = axis[p] + (1 - kind[c])
        diag[c] = diag[p] + kind[c]
        for f in range(nf):
            v = fl[f][c]
            cnt = np.isfinite(v)
            integ[f, c] = (v * seg[kind[c]] if cnt else np.float64(0.0)) + integ[f, p]
            vmin[f, c] = rmin(v if cnt else np.inf, vmin[f, p])
            vmax[f, c] = rmax(v if cnt else -np.inf, vmax[f, p])
    has = sink != NONE
    length = np.where(has, res * axis.astype(np.float64) + seg[1] * diag.astype(np.float64),
                      np.nan)
    integ[:, ~has] = np.nan
    shape = (ny, nx)
    return {"sink": sink.reshape(shape), "axis": axis.reshape(shape), "diag": diag.reshape(shape),
            "length": length.reshape(shape), "integral": integ.reshape((nf,) + shape),
            "vmin": vmin.reshape((nf,) + shape), "vmax": vmax.reshape((nf,) + shape)}


def walk(T, seeds, i, j):
    """the nodes (i, j) of the cell's route, and how it ends: a root's k, or None"""
    T = np.ascontiguousarray(T, dtype=np.float64)
    nx = T.shape[1]
    par, _ = parents(T)
    root = roots(T, seeds)
    c = j * nx + i
    nodes = [(i, j)]
    if not T[j, i] < np.inf:
        return nodes, None
    while c not in root:
        if par[c] < 0:
            return nodes, None
        c = int(par[c])
        nodes.append((c % nx, c // nx))
    return nodes, root[c]


def abs_integral(T, res, seeds, field):
    """[ny, nx]: the integral of |field| along every route (0 without one) -- the scale of
    the rounding bound between two orders of the same sum"""
    r = route_fields(T, res, seeds, [np.abs(np.asarray(field, dtype=np.float64))])
    return np.where(r["sink"] != NONE, r["integral"][0], 0.0)
