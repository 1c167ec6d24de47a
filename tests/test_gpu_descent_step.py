"""The three path kernels run one descent step (csrc/descent_step.h), so on the same
starts they must agree with each other wherever their definitions coincide: getPathStats'
count and length are those of getPaths' waypoints, and getArrivingPaths' waypoints are
getPaths' for as long as the arriving descent only takes continuous steps.  Each map is
built once, holds an obstacle wall, a start in the last row and a start whose first cell
has no label (no cost), and every query runs once."""
import numpy as np
import pytest

import path_stats_ref as ref

pytestmark = pytest.mark.gpu

RD = 0.5  # risk_distance: tau = min(0.4, RD) = 0.4
RES = 1.0

# name: nx, ny, the goals (i, j), their offsets (None: a single goal), the wall
# (i0, i1, j0, j1) and the 3x3 pocket's lower corner
MAPS = {
    "48x40": (48, 40, [(34, 20)], None, (13, 14, 10, 30), (3, 3)),
    "33x47-goals": (33, 47, [(25, 38), (6, 8)], [0.0, 3.0], (5, 28, 23, 24), (14, 4)),
}


def speed_map(nx, ny, wall, pocket):
    """A smooth speed in [1, 3], an obstacle wall, and a 3x3 pocket of free cells inside a
    ring of obstacles: no cost reaches it, so under a goal set its cells have no label."""
    j, i = np.mgrid[0:ny, 0:nx].astype(float)
    F = 2.0 + np.sin(0.37 * i) * np.cos(0.23 * j)
    i0, i1, j0, j1 = wall
    F[j0:j1, i0:i1] = np.inf
    pi, pj = pocket
    F[pj - 1:pj + 4, pi - 1:pi + 4] = np.inf
    F[pj:pj + 3, pi:pi + 3] = 2.0
    return F


def starts_of(nx, ny, pocket):
    """96 uniform starts and four placed ones: on the last row of nodes (in no cell), in
    the last row of cells (a clamped stencil), in the pocket, and in the first cell."""
    rng = np.random.default_rng(11)
    xy = np.stack([rng.uniform(1, nx - 2, 96), rng.uniform(1, ny - 2, 96)], axis=1)
    placed = [(10.3, ny - 1.0), (nx - 5.8, ny - 1.4), (pocket[0] + 1.2, pocket[1] + 1.3),
              (0.2, 0.3)]
    xy = np.concatenate([xy, placed])
    return xy, [(x, y, 0.0, 0.01 * k) for k, (x, y) in enumerate(xy)]


def configure(p, name):
    """The map `name` and its goal or goals on planner p; returns (F, xy, starts)."""
    nx, ny, goals, offsets, wall, pocket = MAPS[name]
    F = speed_map(nx, ny, wall, pocket)
    assert p.initGlobalLayer(RES, 0.5, nx, ny)
    assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
    if offsets is None:
        assert p.setGoal((goals[0][0], goals[0][1], 0.0, 1.25))
    else:
        assert p.setGoals([(float(i), float(j), 0.0, 0.1 * k) for k, (i, j) in enumerate(goals)],
                          offsets)
    xy, starts = starts_of(nx, ny, pocket)
    return F, xy, starts


def continuous_class(status, rec):
    """The starts whose arriving descent arrived on continuous steps alone."""
    return (np.asarray(status) == 1) & (rec["hops"] == 0)


def common_prefix(path, arriving):
    """The waypoints both descents store before either end rule acts: all but the sink
    that each appends, as far as the shorter one goes."""
    k = min(len(path), len(arriving)) - 1
    return path[:k], arriving[:k]


class Case:
    pass


@pytest.fixture(scope="module", params=sorted(MAPS))
def case(request, dymu):
    c = Case()
    c.name = request.param
    p = dymu.Planner(risk_distance=RD)
    c.F, c.xy, c.starts = configure(p, c.name)
    assert p.computeEntireTotalCostMap()
    c.paths, c.status = p.getPaths(c.starts)
    c.paths_on_device = p.lastPathsOnDevice()
    c.stats = p.getPathStats(c.starts)
    c.stats_on_device = p.lastPathsOnDevice()
    c.apaths, c.astatus, c.arec = p.getArrivingPaths(c.starts)
    c.arrive_on_device = p.lastPathsOnDevice()
    c.T = p.totalCostRaw()
    yield c
    p.close()


def test_the_map_holds_its_cases(case):
    _, _, _, offsets, _, pocket = MAPS[case.name]
    assert case.paths_on_device and case.stats_on_device and case.arrive_on_device
    assert not np.isfinite(case.T[pocket[1] + 1, pocket[0] + 1])  # the pocket: no cost, no label
    # ... so no descent leaves it: under a goal set the first cell has no label (-1), under
    # one goal the gradient of an all-infinite stencil is zero and the path stalls (0)
    assert case.astatus[98] == -1 and case.status[98] == (0 if offsets is None else -1)
    assert case.status[96] == -1  # the last row of nodes is in no cell: getPaths has no step
    assert case.astatus[96] == 1 and case.arec["hops"][96] > 0  # the arriving descent hops
    assert case.status[97] == 1 and case.status[99] == 1  # the clamped stencils descend
    assert (case.arec["hops"] > 0).sum() >= 10  # the wall: descents that getPaths cuts short


def test_path_stats_are_the_record_of_the_stored_waypoints(case):
    assert np.array_equal(case.stats["status"], case.status)
    for q in range(len(case.starts)):
        r = ref.path_record(case.paths[q][:, :2], RES, [case.F])
        assert int(case.stats["count"][q]) == r["count"], q
        assert float(case.stats["length"][q]) == r["length"], q  # the host's summation order
    assert np.median(case.stats["count"]) > 20


def test_arriving_paths_are_the_paths_while_the_steps_are_continuous(case):
    cls = continuous_class(case.astatus, case.arec)
    # a condition on the map, met by the host routes alone: half of the starts compare
    assert 2 * int(cls.sum()) >= len(case.starts), int(cls.sum())
    compared = 0
    for q in np.flatnonzero(cls):
        # every step the arriving descent took is the continuous one, at least the stall
        # length and never NaN: getPaths took the same steps and ended on its sink
        assert case.status[q] == 1, q
        a, b = common_prefix(case.paths[q], case.apaths[q])
        assert len(a) >= 1 and a.tobytes() == b.tobytes(), q  # x, y, z and the heading
        compared += len(a)
    assert compared >= 20 * int(cls.sum())
