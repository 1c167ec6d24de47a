"""getPathStats without a device: the record the host descent accumulates must be the
numpy record (tests/path_stats_ref.py) of the waypoints getPaths returns, bit for bit.  No
engine is ever created: the maps are the oracle's FMM maps installed by loadTotalCostMap.
A case (planner, paths, records, references) is built once and shared by its tests."""
import numpy as np
import pytest

import path_stats_ref as ref

RD = 0.5  # risk_distance: tau = min(0.4, RD) = 0.4
RES = 1.0
CASES = {"96x96": (96, 96, (70, 60)), "97x61": (97, 61, (70, 40))}
# paths of 200 with a last hop beyond 2.4 res / with skipped[0] > 0 at 2 % obstacles
EXPECT = {"96x96": (22, 50), "97x61": (15, 73)}


class Case:
    pass


def _planner(dymu, oracle, nx, ny, goal, obst, off=(0.0, 0.0)):
    F = oracle.synth_speed(nx, ny, seed=21, obst_frac=obst, goal=goal)
    p = dymu.Planner(risk_distance=RD)
    assert p.initGlobalLayer(RES, 0.5, nx, ny, offset=off)
    assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
    assert p.setGoal((off[0] + goal[0], off[1] + goal[1], 0.0, 1.25))
    T, _ = oracle.fmm(F, goal)
    assert p.loadTotalCostMap(T)
    return p, F


def _elevation(nx, ny):
    j, i = np.mgrid[0:ny, 0:nx].astype(float)
    return 0.3 * np.sin(0.3 * i) + 0.1 * np.cos(0.2 * j) + 0.01 * i


@pytest.fixture(scope="module", params=[(s, o) for s in sorted(CASES) for o in (0.0, 0.02)],
                ids=lambda p: f"{p[0]}-obst{p[1]}")
def case(request, dymu, oracle):
    shape, obst = request.param
    nx, ny, goal = CASES[shape]
    c = Case()
    c.shape, c.obst, c.nx, c.ny, c.goal = shape, obst, nx, ny, goal
    c.p, c.F = _planner(dymu, oracle, nx, ny, goal, obst)
    rng = np.random.default_rng(7)
    c.xy = np.stack([rng.uniform(2, nx - 3, 200), rng.uniform(2, ny - 3, 200)], axis=1)
    c.starts = [(x, y, 0.0, 0.01 * k) for k, (x, y) in enumerate(c.xy)]
    c.elev = _elevation(nx, ny)
    c.paths, c.status = c.p.getPaths(c.starts)
    c.sinks = c.p.lastPathSinks()
    assert not c.p.lastPathsOnDevice()
    c.stats = c.p.getPathStats(c.starts, field=c.elev, host=True)
    assert not c.p.lastPathsOnDevice() and c.p.lastPathsKernelMs() == 0
    c.ref = [ref.path_record(q[:, :2], RES, [c.F, c.elev]) for q in c.paths]
    yield c
    c.p.close()


def test_bit_exact_against_numpy_record(case):
    assert case.stats.shape == (200,)
    assert np.array_equal(case.stats["status"], case.status)
    assert np.array_equal(case.stats["count"], [len(q) for q in case.paths])
    assert np.array_equal(case.stats["sink"], case.sinks)
    assert np.median(case.stats["count"]) > 30
    for q in range(200):
        assert ref.same_record(case.stats[q], case.ref[q]) is None, \
            (q, ref.same_record(case.stats[q], case.ref[q]), case.status[q])


def test_without_the_callers_field_slot_one_is_empty(case):
    s = case.p.getPathStats(case.starts[:40], host=True)
    for q in range(40):
        r = dict(case.ref[q])
        for k, v in (("integral", 0.0), ("vmin", np.inf), ("vmax", -np.inf), ("skipped", 0)):
            r[k] = [r[k][0], v, v, v]
        assert ref.same_record(s[q], r) is None, q
    assert np.array_equal(s["status"], case.status[:40])


def test_conditions_that_keep_the_cases_meaningful(case):
    s = case.stats
    arrived = (s["status"] == 1) & (s["last_hop"] <= 2.4 * RES * (1 + 1e-12))
    cut = (s["status"] == 1) & ~arrived
    skipped0 = s["skipped"][:, 0] > 0
    print(f"{case.shape} obst {case.obst}: {int(arrived.sum())} arrived, {int(cut.sum())} cut "
          f"short, {int(skipped0.sum())} with skipped[0] > 0")
    if case.obst == 0.0:
        assert (s["last_hop"] <= 2.4 * RES * (1 + 1e-12)).all()
        assert not skipped0.any()
    else:
        assert (int(cut.sum()), int(skipped0.sum())) == EXPECT[case.shape]
        assert cut.sum() >= 10 and arrived.sum() >= 150 and skipped0.sum() >= 20


def test_callers_field(case):
    """A smooth elevation-like field: exact (test_bit_exact covers slot 1 too), every
    waypoint has a node, and the extrema are the field's along the path."""
    s = case.stats
    assert (s["skipped"][:, 1] == 0).all()
    ok = s["count"] > 0
    assert (s["vmin"][ok, 1] >= case.elev.min()).all() and (s["vmax"][ok, 1] <= case.elev.max()).all()
    assert (s["vmin"][ok, 1] <= s["vmax"][ok, 1]).all()
    assert np.abs(s["integral"][ok, 1]).max() > 1.0


def test_max_wp_cuts_the_record(case):
    q = int(np.argmax([len(w) if st == 1 else 0 for w, st in zip(case.paths, case.status)]))
    full = case.paths[q]
    assert len(full) > 40
    fields = [case.F, case.elev]
    for m, st in ((8, -3), (len(full) - 1, -3), (len(full), 1)):
        (r,) = case.p.getPathStats([case.starts[q]], max_wp=m, field=case.elev, host=True)
        assert r["status"] == st and r["count"] == m
        assert r["sink"] == (0 if st == 1 else -1)
        assert ref.same_record(r, ref.path_record(full[:m, :2], RES, fields)) is None, m


@pytest.mark.parametrize("shape", sorted(CASES))
def test_offset_case(dymu, oracle, shape):
    """With an offset the returned coordinates are not the grid-local ones bit for bit
    (adding and subtracting the offset rounds): counts and statuses are exact, the float
    members within the project's path tolerance."""
    nx, ny, goal = CASES[shape]
    off = (100.0, 200.0)
    p, F = _planner(dymu, oracle, nx, ny, goal, 0.02, off)
    try:
        rng = np.random.default_rng(7)
        xy = np.stack([rng.uniform(2, nx - 3, 200), rng.uniform(2, ny - 3, 200)], axis=1)
        starts = [(off[0] + x, off[1] + y, 0.0, 0.0) for x, y in xy]
        elev = _elevation(nx, ny)
        paths, status = p.getPaths(starts)
        s = p.getPathStats(starts, field=elev, host=True)
        assert np.array_equal(s["status"], status)
        assert np.array_equal(s["count"], [len(q) for q in paths])
        for q in range(200):
            r = ref.path_record(paths[q][:, :2] - np.array(off), RES, [F, elev])
            assert ref.close_record(s[q], r, 1e-9) is None, (q, ref.close_record(s[q], r, 1e-9))
    finally:
        p.close()


def test_off_grid_samples(dymu):
    """The descent walks off the grid, and the waypoint whose nearest node is off the
    grid counts as skipped in every slot; the record matches the reference exactly."""
    nx, ny = 32, 16
    ones, field = np.ones((ny, nx)), _elevation(nx, ny)
    west = ref.off_grid_map(nx, ny)
    east = (np.tile(nx - 1.0 - np.arange(nx), (ny, 1)), (2, 8), (nx - 3.7, 8.3, 0.0, 0.0))
    for name, (T, goal, start) in (("west", west), ("east", east)):
        p = dymu.Planner(risk_distance=RD)
        try:
            assert p.initGlobalLayer(RES, 0.5, nx, ny)
            assert p.setCostMap(ones)
            assert p.setGoal((float(goal[0]), float(goal[1]), 0.0, 0.0))
            assert p.loadTotalCostMap(T)
            (w,), (st,) = p.getPaths([start])
            assert st == 1 and len(w) > 3
            _, _, on = ref.nearest_nodes(w[:, :2], RES, nx, ny)
            if name == "west":
                assert (~on).sum() >= 1  # first from the reference: a sample is off the grid
            else:
                assert w[-2, 0] >= nx - 1 and on.all()  # off the last cell, still on a node
            r = ref.path_record(w[:, :2], RES, [ones, field])
            assert r["skipped"][0] == r["skipped"][1] == int((~on).sum())
            (s,) = p.getPathStats([start], field=field, host=True)
            assert s["status"] == 1 and s["sink"] == 0
            assert ref.same_record(s, r) is None, (name, ref.same_record(s, r))
            assert s["last_hop"] > 2.4 * RES  # the jump from the edge back to the sink
        finally:
            p.close()


def test_degenerate_calls(dymu, oracle):
    nx, ny, goal = CASES["96x96"]
    p, _ = _planner(dymu, oracle, nx, ny, goal, 0.0)
    try:
        with pytest.raises(dymu.DymuError):
            p.getPathStats([(5.0, 5.0)], max_wp=0, host=True)
        s = p.getPathStats([], host=True)
        assert s.shape == (0,) and s.dtype == dymu.PATH_STAT_DTYPE
        with pytest.raises(ValueError):
            p.getPathStats([(5.0, 5.0)], field=np.zeros((3, 3)), host=True)
        # rejected starts: the empty record, next to a good one that is what it is alone
        (good,) = p.getPathStats([(10.25, 12.5)], host=True)
        s = p.getPathStats([(10.25, 12.5), (float("nan"), 5.0), (-3.0, 5.0), (nx - 0.5, 5.0),
                            (1e300, 5.0), (10.25, 12.5)], host=True)
        assert s[0] == good and s[-1] == good and good["status"] == 1
        for r in s[1:-1]:
            assert r["status"] == -1 and r["sink"] == -1
            assert ref.same_record(r, ref.empty_record()) is None
    finally:
        p.close()
    q = dymu.Planner(risk_distance=RD)
    try:
        assert q.initGlobalLayer(RES, 0.5, 16, 16)
        assert q.setCostMap(np.ones((16, 16)))
        s = q.getPathStats([(5.0, 5.0), (6.0, 7.0)], host=True)  # no goal
        assert (s["status"] == -1).all() and (s["count"] == 0).all()
        assert all(ref.same_record(r, ref.empty_record()) is None for r in s)
    finally:
        q.close()


def test_symbols_and_record_layout(dymu):
    fim, pl = dymu.load_fim(), dymu.load_planner()
    for n in ("dymu_path_stats_device", "dymu_last_path_stats_ms"):
        assert hasattr(fim, n) and n in dymu.FIM_SYMBOLS, n
    for n in ("dymu_planner_get_path_stats", "dymu_planner_get_path_stats_to"):
        assert hasattr(pl, n) and n in dymu.PLANNER_SYMBOLS, n
    d = dymu.PATH_STAT_DTYPE
    assert d.itemsize == 144 and d.fields["length"][1] == 16 and d.fields["skipped"][1] == 128
    assert fim.dymu_path_stats_device(None, None, 8, 8, 8, 1.0, 1, 1, None, None, 0, 0.4, None, 0,
                                      4, None, None, 0, 0, None, None) == -1
