"""The arriving descent in plain Python: the rule of DESIGN.md s5.15 restated on a [ny, nx]
array T (T[j, i], +inf for an obstacle), one IEEE double operation per Python operation and
in the rule's order, so the planner's host loop and the kernel must reproduce it bit for
bit.  descend() returns the record and the kept slots (x, y, dcx, dcy), post_pass() turns
slots into getPaths' waypoints (x, y, z, heading), check_path() tests the invariants the
rule guarantees on any sequence of waypoints."""
import math

import numpy as np

INF = math.inf
HOPS = ((0, -1), (-1, 0), (1, 0), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))
DIAG = 0.7071067811865476


def node(v, res, n):
    """nearestIndex's rounding on one axis; None off a grid of n nodes."""
    if not v >= 0.0:  # negative or NaN
        return None
    g = v / res + 0.5
    if not g < 4294967296.0:
        return None
    i = int(g)
    return i if i < n else None


def cell(g, n):
    """The cell of grid coordinate g, None when it or its +1 neighbour is off the grid."""
    if not (g > -9.2e18 and g < 9.2e18):
        return None
    c = int(g)  # truncation
    return c if c >= 0 and c + 1 < n else None


def _gradient(T, i, j):
    """The reference's gradientNode: a one-sided difference beside the edge or an obstacle,
    a central one otherwise, normalised."""
    ny, nx = T.shape
    hw, he, hs, hn = i > 0, i + 1 < nx, j > 0, j + 1 < ny
    t = float(T[j, i])
    tw = float(T[j, i - 1]) if hw else INF
    te = float(T[j, i + 1]) if he else INF
    ts = float(T[j - 1, i]) if hs else INF
    tn = float(T[j + 1, i]) if hn else INF

    def one(h0, h1, t0, t1):
        if (not h0 and not h1) or (h0 and h1 and t0 == INF and t1 == INF):
            return 0.0
        if not h0 or t0 == INF:
            return t1 - t
        if not h1 or t1 == INF:
            return t - t0
        return (t1 - t0) * 0.5

    with np.errstate(all="ignore"):
        dx, dy = np.float64(one(hw, he, tw, te)), np.float64(one(hs, hn, ts, tn))
        if dx == 0 and dy == 0:
            return 0.0, 0.0
        r = np.sqrt(dx * dx + dy * dy)
        return float(dx / r), float(dy / r)


def _bilinear(a, b, g00, g01, g10, g11):
    return g00 + (g10 - g00) * a + (g01 - g00) * b + (g11 + g00 - g10 - g01) * a * b


def _dist(ax, ay, bx, by):
    dx, dy = ax - bx, ay - by
    return math.sqrt(dx * dx + dy * dy) if dx == dx and dy == dy else math.nan


def candidate(T, res, tau, x, y):
    """nextWaypoint: (cx, cy, dcx, dcy); NaN coordinates where (x, y) is in no cell."""
    ny, nx = T.shape
    gx, gy = x / res, y / res
    cx, cy = cell(gx, nx), cell(gy, ny)
    if cx is None or cy is None:
        return math.nan, math.nan, 0.0, 0.0
    ax, ay = gx - float(cx), gy - float(cy)
    g00, g10 = _gradient(T, cx, cy), _gradient(T, cx + 1, cy)
    g01, g11 = _gradient(T, cx, cy + 1), _gradient(T, cx + 1, cy + 1)
    with np.errstate(all="ignore"):
        f = np.float64
        dcx = float(_bilinear(f(ax), f(ay), f(g00[0]), f(g01[0]), f(g10[0]), f(g11[0])))
        dcy = float(_bilinear(f(ax), f(ay), f(g00[1]), f(g01[1]), f(g10[1]), f(g11[1])))
    return x - res * tau * dcx, y - res * tau * dcy, dcx, dcy


def empty_record():
    return dict(status=-1, sink=-1, count=0, hops=0, length=0.0, start_cost=0.0)


def descend(T, res, tau, start, goal=None, labels=None, goals_ij=None, max_wp=1 << 20,
            stride=1):
    """The rule from `start` (grid-local x, y).  goal = (i, j): the single sink; labels
    ([ny, nx] uint32) with goals_ij: a goal set.  Returns (record dict, slots [k, 4])."""
    ny, nx = T.shape
    rec = empty_record()
    x, y = float(start[0]), float(start[1])
    ni, nj = node(x, res, nx), node(y, res, ny)
    if ni is None or nj is None:
        return rec, np.zeros((0, 4))

    def t_at(i, j):
        return float(T[j, i]) if 0 <= i < nx and 0 <= j < ny else INF

    def sink_of(i, j):
        """(k, sink x, sink y, the sink's node) for node (i, j); k = -1: no sink."""
        if labels is None:
            return 0, res * float(goal[0]), res * float(goal[1]), (goal[0], goal[1])
        k = int(labels[j, i])
        if not k < len(goals_ij):
            return -1, 0.0, 0.0, None
        sx, sy = res * float(goals_ij[k][0]), res * float(goals_ij[k][1])
        return k, sx, sy, (node(sx, res, nx), node(sy, res, ny))

    if not t_at(ni, nj) < INF or sink_of(ni, nj)[0] < 0:
        return rec, np.zeros((0, 4))
    rec["start_cost"] = t_at(ni, nj)
    stall = 0.01 * tau * res
    limit = max_wp * stride
    slots, same, status = [], 0, 0
    pdx = pdy = 0.0
    prev = None
    w = 0
    while True:
        if prev is not None:
            rec["length"] = rec["length"] + _dist(prev[0], prev[1], x, y)
        rec["count"] += 1
        if w % stride == 0:
            slots.append((x, y, pdx, pdy))
        prev = (x, y)
        k, sx, sy, snode = sink_of(ni, nj)
        if k >= 0 and snode == (ni, nj):  # 1. arrived
            status = 1
            break
        if w + 1 == limit:
            status = -3
            break
        tn = t_at(ni, nj)
        cx, cy, dcx, dcy = candidate(T, res, tau, x, y)  # 2. the continuous candidate
        ok = cx == cx and cy == cy and _dist(x, y, cx, cy) >= stall
        mi = mj = None
        if ok:
            mi, mj = node(cx, res, nx), node(cy, res, ny)
            ok = mi is not None and mj is not None and abs(mi - ni) <= 1 and abs(mj - nj) <= 1
        if ok:
            ok = t_at(mi, mj) < INF
            if (mi, mj) == (ni, nj):
                ok = ok and same < 8
            else:
                ok = ok and t_at(mi, mj) < tn
            if mi != ni and mj != nj:
                ok = ok and t_at(mi, nj) < INF and t_at(ni, mj) < INF
        if ok:
            same = same + 1 if (mi, mj) == (ni, nj) else 0
            x, y, ni, nj, pdx, pdy = cx, cy, mi, mj, dcx, dcy
        else:  # 3. a hop
            best, to = -1.0, None
            for di, dj in HOPS:
                tm = t_at(ni + di, nj + dj)
                if not tm < tn:
                    continue
                if di and dj and not (t_at(ni + di, nj) < INF and t_at(ni, nj + dj) < INF):
                    continue
                s = (tn - tm) * DIAG if di and dj else tn - tm
                if s > best:
                    best, to = s, (di, dj)
            if to is None:
                break  # stalled: status 0
            pdx, pdy = float(-to[0]), float(-to[1])
            ni, nj = ni + to[0], nj + to[1]
            x, y = res * float(ni), res * float(nj)
            same = 0
            rec["hops"] += 1
        w += 1
    if status == 1:
        if len(slots) < max_wp:
            rec["length"] = rec["length"] + _dist(prev[0], prev[1], sx, sy)
            rec["count"] += 1
            slots.append((sx, sy, 0.0, 0.0))
            rec["sink"] = k
        else:
            status = -3
    rec["status"] = status
    return rec, np.array(slots, dtype=np.float64).reshape(-1, 4)


def post_pass(slots, status, start, sink_wp, elev, res, off=(0.0, 0.0)):
    """getPaths' host post-pass: slots (grid-local) into waypoints (x, y, z, heading) with
    the offset added.  start = the caller's (x, y, z, heading); sink_wp = the sink's
    waypoint, offset included; elev [ny, nx]."""
    ny, nx = elev.shape
    out = np.zeros((len(slots), 4))
    for k, (x, y, dcx, dcy) in enumerate(slots):
        if status == 1 and k + 1 == len(slots):
            out[k] = sink_wp
            continue
        z, h = (start[2], start[3]) if k == 0 else (0.0, math.atan2(-dcy, -dcx))
        gx, gy = x / res, y / res
        cx, cy = cell(gx, nx), cell(gy, ny)
        if cx is not None and cy is not None:
            ax, ay = gx - float(cx), gy - float(cy)
            z = _bilinear(ax, ay, float(elev[cy, cx]), float(elev[cy, cx + 1]),
                          float(elev[cy + 1, cx]), float(elev[cy + 1, cx + 1]))
        out[k] = (x + off[0], y + off[1], z, h)
    return out


def same_record(got, want):
    """None when the structured record `got` equals the dict `want` bit for bit, else the
    first differing member."""
    for name in ("status", "sink", "count", "hops"):
        if int(got[name]) != int(want[name]):
            return name, int(got[name]), int(want[name])
    for name in ("length", "start_cost"):
        if np.float64(got[name]).tobytes() != np.float64(want[name]).tobytes():
            return name, float(got[name]), float(want[name])
    return None


def check_path(T, xy, res):
    """The invariants of a stride-1 path xy [k, 2] (grid-local): every waypoint's node is on
    the grid and finite, T at the nodes never rises, consecutive nodes are neighbours, and
    no diagonal move has an obstacle side node.  None, or a description of the violation."""
    ny, nx = T.shape
    last = None
    for k, (x, y) in enumerate(xy):
        i, j = node(float(x), res, nx), node(float(y), res, ny)
        if i is None or j is None:
            return f"waypoint {k} is off the grid"
        if not T[j, i] < INF:
            return f"waypoint {k} is on the obstacle node ({i}, {j})"
        if last is not None:
            a, b = last
            if abs(i - a) > 1 or abs(j - b) > 1:
                return f"waypoint {k} skips from node ({a}, {b}) to ({i}, {j})"
            if T[j, i] > T[b, a]:
                return f"T rises from node ({a}, {b}) to ({i}, {j})"
            if i != a and j != b and not (T[b, i] < INF and T[j, a] < INF):
                return f"waypoint {k} cuts the corner between ({a}, {b}) and ({i}, {j})"
        last = (i, j)
    return None
