"""The arriving descent's rule (tests/arrive_ref.py) on hand-built maps:
what it must do where the reference's descent cannot go on.  The maps are exact 4-connected
step counts (every finite node but the goal has a strictly smaller 4-neighbour) or the exact
distance of a constant-speed map; no library of the project is loaded."""
import numpy as np
import pytest

import arrive_ref as ref

RES, TAU = 1.0, 0.4


def steps_map(free, goal):
    """T[j, i] = 4-connected steps from goal (i, j) over the free nodes, +inf elsewhere."""
    ny, nx = free.shape
    T = np.full((ny, nx), np.inf)
    T[goal[1], goal[0]] = 0.0
    front = [goal]
    while front:
        nxt = []
        for i, j in front:
            for a, b in ((i, j - 1), (i - 1, j), (i + 1, j), (i, j + 1)):
                if 0 <= a < nx and 0 <= b < ny and free[b, a] and T[b, a] == np.inf:
                    T[b, a] = T[j, i] + 1.0
                    nxt.append((a, b))
        front = nxt
    return T


def walk(T, start, goal, **kw):
    rec, slots = ref.descend(T, RES, TAU, start, goal=goal, **kw)
    nodes = [(ref.node(x, RES, T.shape[1]), ref.node(y, RES, T.shape[0])) for x, y in slots[:, :2]]
    return rec, slots, nodes


def test_diagonal_gap_is_not_a_passage():
    """An anti-diagonal wall: its nodes touch only at corners, so an 8-connected walker
    slips through anywhere.  The one real opening is at (3, 12); every path from above the
    wall must cross there, and no move may pass between two wall nodes."""
    n = 16
    free = np.ones((n, n), dtype=bool)
    for k in range(n):
        free[n - 1 - k, k] = False
    free[12, 3] = True  # the opening
    goal = (4, 4)
    T = steps_map(free, goal)
    assert np.isfinite(T[free]).all()
    for start in ((12.3, 12.6), (14.0, 9.2), (8.4, 8.3), (2.2, 14.1), (13.5, 2.5 + 10)):
        rec, slots, nodes = walk(T, start, goal)
        assert rec["status"] == 1 and rec["sink"] == 0, (start, rec)
        assert ref.check_path(T, slots[:, :2], RES) is None, ref.check_path(T, slots[:, :2], RES)
        side = [i + j - (n - 1) for i, j in nodes]  # > 0 above the wall, < 0 below, 0 on it
        on_wall = [nd for nd, s in zip(nodes, side) if s == 0]
        assert on_wall and set(on_wall) == {(3, 12)}, (start, on_wall)
        assert side[0] > 0 and side[-1] < 0
        assert rec["hops"] > 0  # beside the wall the continuous direction is NaN


def test_two_touching_obstacles_alone():
    """Just two obstacle nodes that touch at a corner, on the straight line from the start
    to the goal: the path goes round, not between."""
    n = 12
    free = np.ones((n, n), dtype=bool)
    free[6, 5] = free[5, 6] = False  # (5, 6) and (6, 5)
    goal = (2, 2)
    T = steps_map(free, goal)
    rec, slots, nodes = walk(T, (9.0, 9.0), goal)
    assert rec["status"] == 1
    assert ref.check_path(T, slots[:, :2], RES) is None
    for (a, b), (i, j) in zip(nodes, nodes[1:]):
        assert {(a, b), (i, j)} != {(6, 6), (5, 5)}, "passed between the two obstacles"


def test_dead_end_pocket():
    """A pocket open away from the goal: the path leaves it by the mouth and arrives."""
    nx, ny = 20, 14
    free = np.ones((ny, nx), dtype=bool)
    free[3:11, 6] = False      # the pocket's back wall, towards the goal
    free[3, 6:13] = False      # its two side walls
    free[10, 6:13] = False
    goal = (2, 7)
    T = steps_map(free, goal)
    rec, slots, nodes = walk(T, (8.3, 6.6), goal)
    assert rec["status"] == 1 and rec["count"] == len(slots)
    assert ref.check_path(T, slots[:, :2], RES) is None
    assert max(i for i, _ in nodes) >= 13  # it went out through the mouth at i = 13
    assert rec["length"] > 20.0            # the straight line is about 6
    assert nodes[-1] == goal and nodes[-2] == goal  # the last segment is in the sink's square


def test_goal_next_to_obstacles():
    n = 12
    free = np.ones((n, n), dtype=bool)
    free[6, 7] = free[7, 6] = free[7, 7] = False  # east, north and north-east of the goal
    goal = (6, 6)
    T = steps_map(free, goal)
    for start in ((10.2, 10.4), (10.0, 6.0), (6.3, 10.0), (1.5, 2.5)):
        rec, slots, nodes = walk(T, start, goal)
        assert rec["status"] == 1, (start, rec)
        assert ref.check_path(T, slots[:, :2], RES) is None
        assert nodes[-2] == goal and tuple(slots[-1, :2]) == (6.0, 6.0)
        assert np.hypot(*(slots[-1, :2] - slots[-2, :2])) <= np.sqrt(0.5) * RES


def test_constant_speed_map_needs_no_hop():
    """The exact distance map of a constant speed: the continuous step is always valid."""
    nx, ny, goal = 40, 30, (25, 12)
    j, i = np.mgrid[0:ny, 0:nx].astype(float)
    T = np.hypot(i - goal[0], j - goal[1])
    rng = np.random.default_rng(3)
    for x, y in zip(rng.uniform(1, nx - 2, 40), rng.uniform(1, ny - 2, 40)):
        rec, slots, _ = walk(T, (x, y), goal)
        assert rec["status"] == 1 and rec["hops"] == 0, ((x, y), rec)
        assert ref.check_path(T, slots[:, :2], RES) is None
        # the path is straight: its length is the distance, within the last steps' slack
        assert abs(rec["length"] - np.hypot(x - goal[0], y - goal[1])) < 1.0
        assert rec["start_cost"] == T[int(y + 0.5), int(x + 0.5)]


def test_statuses_and_stride():
    n, goal = 16, (3, 3)
    T = steps_map(np.ones((n, n), dtype=bool), goal)
    T[8, 8] = np.inf
    for bad in ((8.2, 7.9), (-0.3, 5.0), (5.0, float("nan")), (n - 0.4, 5.0), (5.0, 1e300)):
        rec, slots, _ = walk(T, bad, goal)
        assert rec == ref.empty_record() and len(slots) == 0, bad
    full, fslots, _ = walk(T, (12.3, 13.1), goal)
    assert full["status"] == 1 and full["count"] == len(fslots) > 20
    for m in (1, 7, len(fslots) - 1):
        rec, slots, _ = walk(T, (12.3, 13.1), goal, max_wp=m)
        assert rec["status"] == -3 and rec["count"] == m and rec["sink"] == -1
        assert np.array_equal(slots, fslots[:m])
    rec, slots, _ = walk(T, (12.3, 13.1), goal, max_wp=len(fslots))
    assert rec == full and np.array_equal(slots, fslots)
    rec, slots, _ = walk(T, (12.3, 13.1), goal, stride=3)
    assert rec == full  # the record is that of stride 1
    assert np.array_equal(slots, np.vstack([fslots[:-1][::3], fslots[-1:]]))
    # a plateau: no continuous step and no smaller neighbour
    P = np.full((n, n), 5.0)
    P[goal[1], goal[0]] = 0.0
    rec, slots, _ = walk(P, (10.2, 10.7), goal)
    assert rec["status"] == 0 and rec["count"] == 1 and len(slots) == 1 and rec["sink"] == -1


def test_goal_set_sink_is_the_label_of_the_last_node():
    n = 16
    goals = [(3, 3), (12, 4), (8, 13)]
    maps = [steps_map(np.ones((n, n), dtype=bool), g) for g in goals]
    T = np.minimum.reduce(maps)
    labels = np.argmin(np.stack(maps), axis=0).astype(np.uint32)
    rng = np.random.default_rng(5)
    seen = set()
    for x, y in zip(rng.uniform(0, n - 1, 30), rng.uniform(0, n - 1, 30)):
        rec, slots = ref.descend(T, RES, TAU, (x, y), labels=labels, goals_ij=goals)
        assert rec["status"] == 1
        k = rec["sink"]
        assert tuple(slots[-1, :2]) == (float(goals[k][0]), float(goals[k][1]))
        seen.add(k)
    assert seen == {0, 1, 2}
    labels[5, 5] = 0xFFFFFFFF
    rec, slots = ref.descend(T, RES, TAU, (5.1, 4.9), labels=labels, goals_ij=goals)
    assert rec == ref.empty_record() and len(slots) == 0


@pytest.mark.parametrize("xy, want", [((0.0, 0.49), (0, 0)), ((0.5, 1.5), (1, 2)),
                                      ((-0.0, 2.4999), (0, 2)), ((-1e-300, 0.0), (None, 0))])
def test_node_rule(xy, want):
    assert (ref.node(xy[0], RES, 8), ref.node(xy[1], RES, 8)) == want
