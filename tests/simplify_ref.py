"""The simplification rule of getSimplifiedPaths (stated in
include/dymu_fim.h with dymu_arrive_simplified_device) in plain Python on a waypoint array:
one IEEE double operation per Python operation and in the rule's order, so the planner's
host loop and the kernel (csrc/path_simplify.h) must keep the same waypoints.  simplify()
returns the numbers of the kept waypoints, check() tests what the rule guarantees on any
kept set: the ends are there and every dropped waypoint is within eps of its segment."""
import math

import numpy as np


def _cross(ax, ay, bx, by):
    return ax * by - ay * bx


def simplify(xy, eps):
    """The rule on the waypoints xy [n, 2] walked (the sink excluded): the strictly
    increasing numbers of the kept ones, a uint32 array."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    n = len(xy)
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    eps = float(eps)
    eps2 = eps * eps
    kept = [0]
    ax, ay = float(xy[0, 0]), float(xy[0, 1])
    lx = ly = hx = hy = 0.0
    is_open, far2 = True, 0.0
    for k in range(1, n):
        x, y = float(xy[k, 0]), float(xy[k, 1])
        while True:
            vx, vy = x - ax, y - ay
            d2 = vx * vx + vy * vy
            ok = d2 >= far2 and (is_open or (_cross(lx, ly, vx, vy) >= 0 and
                                             _cross(vx, vy, hx, hy) >= 0))
            if ok:
                break
            # the previous waypoint is kept and becomes the anchor
            kept.append(k - 1)
            ax, ay = float(xy[k - 1, 0]), float(xy[k - 1, 1])
            is_open, far2 = True, 0.0
        far2 = d2
        if d2 > eps2:
            c = math.sqrt(d2 - eps2)
            tlx, tly = vx * c + vy * eps, vy * c - vx * eps
            thx, thy = vx * c - vy * eps, vy * c + vx * eps
            if is_open:
                lx, ly, hx, hy, is_open = tlx, tly, thx, thy, False
            else:
                if _cross(lx, ly, tlx, tly) > 0:
                    lx, ly = tlx, tly
                if _cross(thx, thy, hx, hy) > 0:
                    hx, hy = thx, thy
    if kept[-1] != n - 1:
        kept.append(n - 1)
    return np.array(kept, dtype=np.uint32)


def simplify_slots(slots, status, eps):
    """The rule on arrive_ref.descend's slots [k, 4] at stride 1 (with status 1 the last one
    is the sink, which is no walked waypoint and follows the kept ones): the numbers of the
    kept slots."""
    walked = len(slots) - (1 if status == 1 else 0)
    idx = simplify(slots[:walked, :2], eps)
    if status == 1:
        idx = np.append(idx, np.uint32(walked))
    return idx.astype(np.uint32)


def seg_dist(p, a, b):
    """The distance of point p from the segment a-b."""
    px, py = float(p[0]) - float(a[0]), float(p[1]) - float(a[1])
    sx, sy = float(b[0]) - float(a[0]), float(b[1]) - float(a[1])
    s2 = sx * sx + sy * sy
    t = 0.0 if s2 == 0.0 else min(1.0, max(0.0, (px * sx + py * sy) / s2))
    return math.hypot(px - t * sx, py - t * sy)


def worst(full_xy, index):
    """The largest distance of a dropped waypoint from the segment between the kept
    waypoints on either side of it (0.0 when nothing is dropped)."""
    full_xy = np.asarray(full_xy, dtype=np.float64).reshape(-1, 2)
    w = 0.0
    for a, b in zip(index[:-1], index[1:]):
        for k in range(int(a) + 1, int(b)):
            w = max(w, seg_dist(full_xy[k], full_xy[int(a)], full_xy[int(b)]))
    return w


def check(full_xy, index, eps):
    """None when `index` is a valid simplification of the walked waypoints full_xy [n, 2]
    within eps, else a description of the violation."""
    full_xy = np.asarray(full_xy, dtype=np.float64).reshape(-1, 2)
    idx = [int(i) for i in index]
    n = len(full_xy)
    if n == 0:
        return None if not idx else "waypoints kept of an empty walk"
    if any(b <= a for a, b in zip(idx[:-1], idx[1:])):
        return "the indices do not increase strictly"
    if not idx or idx[0] != 0 or idx[-1] != n - 1:
        return "the first or the last walked waypoint is missing"
    w = worst(full_xy, idx)
    if not w <= eps * (1 + 1e-9):
        return f"a dropped waypoint lies {w} from its segment, eps = {eps}"
    return None
