"""getArrivingPaths / getArrivingStats without a device: the planner's host rule
(DyMuPathPlanner::descendArriving) must be tests/arrive_ref.py bit for bit, arrive from
every start on a finite node, and keep the rule's invariants -- on the maps on which the
reference's descent is cut short.  No engine is ever created: the maps are the oracle's FMM
maps installed by loadTotalCostMap.  A case is built once and shared by its tests."""
import numpy as np
import pytest

import arrive_ref as ref
import goalset_ref

RD = 0.5  # risk_distance: tau = min(0.4, RD) = 0.4
TAU = 0.4
RES = 1.0
HEADING = 1.25
CASES = {"96x96": (96, 96, (70, 60)), "97x61": (97, 61, (70, 40))}
OFFS = {"96x96": (0.0, 0.0), "97x61": (100.0, 200.0)}  # one grid with an offset


class Case:
    pass


def _planner(dymu, oracle, nx, ny, goal, obst, off=(0.0, 0.0)):
    F = oracle.synth_speed(nx, ny, seed=21, obst_frac=obst, goal=goal)
    p = dymu.Planner(risk_distance=RD)
    assert p.initGlobalLayer(RES, 0.5, nx, ny, offset=off)
    assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
    assert p.setGoal((off[0] + goal[0], off[1] + goal[1], 0.0, HEADING))
    T, _ = oracle.fmm(F, goal)
    assert p.loadTotalCostMap(T)
    return p, T


def _local(starts, off):
    """the grid-local (x, y) of the starts, by the planner's own subtraction"""
    return [(s[0] - off[0], s[1] - off[1]) for s in starts]


@pytest.fixture(scope="module", params=[(s, o) for s in sorted(CASES) for o in (0.0, 0.02)],
                ids=lambda p: f"{p[0]}-obst{p[1]}")
def case(request, dymu, oracle):
    shape, obst = request.param
    nx, ny, goal = CASES[shape]
    c = Case()
    c.shape, c.obst, c.nx, c.ny, c.goal, c.off = shape, obst, nx, ny, goal, OFFS[shape]
    c.p, c.T = _planner(dymu, oracle, nx, ny, goal, obst, c.off)
    rng = np.random.default_rng(7)
    xy = np.stack([rng.uniform(2, nx - 3, 200), rng.uniform(2, ny - 3, 200)], axis=1)
    c.starts = [(c.off[0] + x, c.off[1] + y, 0.5, 0.01 * k) for k, (x, y) in enumerate(xy)]
    c.local = _local(c.starts, c.off)
    c.paths, c.status, c.rec = c.p.getArrivingPaths(c.starts)
    c.sinks = c.p.lastPathSinks()
    assert not c.p.lastPathsOnDevice() and c.p.lastPathsKernelMs() == 0
    c.stats = c.p.getArrivingStats(c.starts, host=True)
    c.ref = [ref.descend(c.T, RES, TAU, s, goal=goal) for s in c.local]
    c.finite = np.array([np.isfinite(c.T[int(y + 0.5), int(x + 0.5)]) for x, y in c.local])
    yield c
    c.p.close()


def test_equals_the_reference_rule_exactly(case):
    assert case.rec.dtype == case.stats.dtype and case.rec.shape == (200,)
    assert case.rec.tobytes() == case.stats.tobytes()
    assert np.array_equal(case.rec["status"], case.status)
    assert np.array_equal(case.rec["sink"], case.sinks)
    elev = np.zeros((case.ny, case.nx))  # setCostMap leaves the elevation zero
    sink = (case.off[0] + case.goal[0], case.off[1] + case.goal[1], 0.0, HEADING)
    for q in range(200):
        r, slots = case.ref[q]
        assert ref.same_record(case.rec[q], r) is None, (q, ref.same_record(case.rec[q], r))
        want = ref.post_pass(slots, r["status"], case.starts[q], sink, elev, RES, case.off)
        assert case.paths[q].shape == want.shape, q
        assert case.paths[q].tobytes() == want.tobytes(), q  # x, y, z and heading
        assert r["count"] == len(slots)
    assert np.median(case.rec["count"]) > 30


def test_every_start_on_a_finite_node_arrives(case):
    assert np.array_equal(case.status == 1, case.finite)
    assert np.array_equal(case.status == -1, ~case.finite)
    if case.obst:
        assert 1 <= (~case.finite).sum() <= 10  # the -1 starts on obstacle nodes are there
    for q in np.flatnonzero(case.finite):
        xy = case.paths[q][:, :2] - np.array(case.off)
        assert ref.check_path(case.T, xy, RES) is None, (q, ref.check_path(case.T, xy, RES))
        # the path ends in its sink's square, on the sink
        assert tuple(xy[-1]) == (float(case.goal[0]), float(case.goal[1]))
        assert np.abs(xy[-2] - xy[-1]).max() <= 0.5 * RES + 1e-9
        assert case.rec["start_cost"][q] == case.T[int(case.local[q][1] + 0.5),
                                                   int(case.local[q][0] + 0.5)]
    print(f"{case.shape} obst {case.obst}: {int(case.finite.sum())} arrive, hops "
          f"{int(case.rec['hops'].sum())} of {int(case.rec['count'].sum())} waypoints")


def test_new_ground_where_the_reference_descent_is_cut_short(case):
    """The starts from which getPaths' descent ends early and jumps to the sink (last hop
    beyond 2.4 res: test_path_stats_host's EXPECT cases) arrive with this descent."""
    paths, status = case.p.getPaths(case.starts)
    cut = [q for q in range(200) if status[q] == 1 and case.finite[q] and
           np.hypot(*(paths[q][-1, :2] - paths[q][-2, :2])) > 2.4 * RES]
    if case.obst == 0.0:
        assert not cut
        return
    assert len(cut) >= 10
    for q in cut:
        assert case.status[q] == 1
        a = case.paths[q][:, :2]
        assert np.hypot(*(a[-1] - a[-2])) <= np.sqrt(0.5) * RES + 1e-9
        assert len(a) > len(paths[q])
    assert case.rec["hops"].sum() > 0


def test_rejected_starts(case):
    nx, ny, off = case.nx, case.ny, case.off
    oj, oi = np.argwhere(np.isinf(case.T))[0] if case.obst else (None, None)
    good = case.starts[3]
    bad = [(off[0] - 0.2, off[1] + 5.0), (off[0] + 5.0, off[1] - 1.5),
           (float("nan"), off[1] + 5.0), (off[0] + nx - 0.5, off[1] + 5.0),
           (off[0] + 5.0, off[1] + ny + 40.0), (off[0] + 1e300, off[1] + 5.0)]
    if case.obst:
        bad.append((off[0] + oi + 0.2, off[1] + oj - 0.3))
    paths, status, rec = case.p.getArrivingPaths([good] + bad + [good])
    assert paths[0].tobytes() == case.paths[3].tobytes() == paths[-1].tobytes()
    assert rec[0] == case.rec[3] and rec[-1] == case.rec[3]
    assert (status[1:-1] == -1).all() and all(len(q) == 0 for q in paths[1:-1])
    for r in rec[1:-1]:
        assert ref.same_record(r, ref.empty_record()) is None
    assert (case.p.lastPathSinks()[1:-1] == -1).all()
    # the last column and row are nodes like any other: a start there arrives
    edge = [(off[0] + nx - 1.0, off[1] + 7.3), (off[0] + 9.4, off[1] + ny - 1.0),
            (off[0] + nx - 0.6, off[1] + ny - 0.6), (off[0] + 0.0, off[1] + 0.0)]
    paths, status, rec = case.p.getArrivingPaths(edge)
    for s, q, st, r in zip(_local(edge, off), paths, status, rec):
        want, slots = ref.descend(case.T, RES, TAU, s, goal=case.goal)
        assert ref.same_record(r, want) is None and st == want["status"]
        assert np.array_equal(q[:, :2], slots[:, :2] + np.array(off))
        if np.isfinite(case.T[int(s[1] + 0.5), int(s[0] + 0.5)]):
            assert st == 1


def test_max_wp_and_stride(case, dymu):
    q = int(np.argmax(case.rec["count"]))
    full, rfull = case.paths[q], case.rec[q]
    assert rfull["status"] == 1 and len(full) == rfull["count"] > 40
    for m in (1, 8, len(full) - 1):
        (cut,), (st,), (r,) = case.p.getArrivingPaths([case.starts[q]], max_wp=m)
        assert st == -3 and cut.tobytes() == full[:m].tobytes()
        want, _ = ref.descend(case.T, RES, TAU, case.local[q], goal=case.goal, max_wp=m)
        assert ref.same_record(r, want) is None and r["count"] == m and r["sink"] == -1
        (s,) = case.p.getArrivingStats([case.starts[q]], max_wp=m, host=True)
        assert s == r
    (exact,), (st,), (r,) = case.p.getArrivingPaths([case.starts[q]], max_wp=len(full))
    assert st == 1 and exact.tobytes() == full.tobytes() and r == rfull
    (thin,), (st,), (r,) = case.p.getArrivingPaths([case.starts[q]], stride=3)
    assert st == 1 and r == rfull  # the record is that of stride 1
    assert thin.tobytes() == np.vstack([full[:-1][::3], full[-1:]]).tobytes()
    with pytest.raises(dymu.DymuError):
        case.p.getArrivingPaths([case.starts[q]], max_wp=0)
    with pytest.raises(dymu.DymuError):
        case.p.getArrivingStats([case.starts[q]], max_wp=0, host=True)
    s = case.p.getArrivingStats([], host=True)
    assert s.shape == (0,)


def test_current_path_is_not_touched(case):
    assert len(case.p.getPath(case.starts[5])) > 3
    marker = case.p.current_path
    case.p.getArrivingPaths(case.starts[:10])
    case.p.getArrivingStats(case.starts[:10], host=True)
    assert np.array_equal(case.p.current_path, marker)


def test_stalled_on_a_loaded_plateau(dymu):
    n, goal = 24, (6, 6)
    p = dymu.Planner(risk_distance=RD)
    try:
        assert p.initGlobalLayer(RES, 0.5, n, n)
        assert p.setCostMap(np.ones((n, n)))
        assert p.setGoal((float(goal[0]), float(goal[1]), 0.0, 0.0))
        T = np.full((n, n), 5.0)
        T[goal[1], goal[0]] = 0.0
        T[10:, 10:] = 7.0  # a step down onto the plateau, then nothing lower
        assert p.loadTotalCostMap(T)
        starts = [(15.2, 15.7), (10.0, 12.3), (3.0, 3.0)]
        paths, status, rec = p.getArrivingPaths(starts)
        for s, q, st, r in zip(starts, paths, status, rec):
            want, slots = ref.descend(T, RES, TAU, s, goal=goal)
            assert st == 0 == want["status"] and r["sink"] == -1
            assert ref.same_record(r, want) is None
            assert np.array_equal(q[:, :2], slots[:, :2]) and len(q) == r["count"] >= 1
        assert rec["count"][1] >= 2 and rec["count"][2] == 1  # stepped down, then stalled
    finally:
        p.close()


def test_no_goal(dymu):
    p = dymu.Planner(risk_distance=RD)
    try:
        assert p.initGlobalLayer(RES, 0.5, 16, 16)
        assert p.setCostMap(np.ones((16, 16)))
        paths, status, rec = p.getArrivingPaths([(5.0, 5.0), (6.0, 7.0)])
        assert (status == -1).all() and all(len(q) == 0 for q in paths)
        assert all(ref.same_record(r, ref.empty_record()) is None for r in rec)
    finally:
        p.close()


def test_z_and_heading_on_a_terrain(dymu, oracle):
    """A planner with a non-trivial elevation: z and heading are getPaths' post-pass of the
    rule's slots."""
    N, goal, off = 64, (40, 36), (100.0, 200.0)
    j, i = np.mgrid[0:N, 0:N].astype(float)
    elev = 0.3 * np.sin(0.3 * i) + 0.1 * np.cos(0.2 * j)
    terr = 1.0 + (i > N // 2)
    lut = np.array([50.0] * 6 + [1, 2, 4, 2, 2.5, 3] + [3, 3, 3, 1, 5, 9], dtype=float)
    p = dymu.Planner(risk_distance=RD)
    try:
        assert p.initGlobalLayer(RES, 0.5, N, N, offset=off)
        assert p.computeCostMap(lut, np.array([0.0, 10.0, 20.0]), ["Wheel", "Walk"], elev, terr)
        assert p.setGoal((off[0] + goal[0], off[1] + goal[1], 0.0, HEADING))
        G = p.getGlobalCostMatrix()
        T, _ = oracle.fmm(np.where(G < 0, np.inf, G), goal)
        assert p.loadTotalCostMap(T)
        rng = np.random.default_rng(11)
        starts = [(off[0] + x, off[1] + y, 0.5, 0.1 * k)
                  for k, (x, y) in enumerate(rng.uniform(2, N - 3, size=(40, 2)))]
        paths, status, rec = p.getArrivingPaths(starts)
        sink = (off[0] + goal[0], off[1] + goal[1], float(elev[goal[1], goal[0]]), HEADING)
        arrived = 0
        for s, q, st, r in zip(starts, paths, status, rec):
            want, slots = ref.descend(T, RES, TAU, (s[0] - off[0], s[1] - off[1]), goal=goal)
            assert ref.same_record(r, want) is None and st == want["status"]
            assert q.tobytes() == ref.post_pass(slots, st, s, sink, elev, RES, off).tobytes()
            arrived += st == 1
        assert arrived >= 30 and any(np.abs(q[:, 2]).max() > 0.05 for q in paths if len(q))
    finally:
        p.close()


def test_goal_set_sink_is_the_label_of_the_last_node(dymu, oracle):
    g = goalset_ref
    p, F, seeds, goals, starts = g.planner_case(dymu, oracle)
    try:
        assert p.setGoals(goals, g.OFFSETS)
        T = g.fmm_seeds(oracle, F, seeds)
        assert p.loadTotalCostMap(T)
        labels = g.labels_from_T(T, seeds)
        paths, status, rec = p.getArrivingPaths(starts)
        sinks = p.lastPathSinks()
        assert not p.lastPathsOnDevice()
        assert np.array_equal(rec["sink"], sinks) and np.array_equal(rec["status"], status)
        assert p.getArrivingStats(starts, host=True).tobytes() == rec.tobytes()
        assert set(sinks[status == 1]) == {0, 1, 2}
        for s, q, st, k, r in zip(starts, paths, status, sinks, rec):
            loc = (s[0] - g.OFF[0], s[1] - g.OFF[1])
            want, slots = ref.descend(T, RES, min(0.4, g.RD), loc, labels=labels,
                                      goals_ij=g.GOALS_IJ)
            assert ref.same_record(r, want) is None, (s, ref.same_record(r, want))
            lab = labels[int(loc[1] + 0.5), int(loc[0] + 0.5)]
            assert (st == 1) == (lab != g.NONE)  # every labelled start arrives
            if st != 1:
                assert st == -1 and k == -1 and len(q) == 0
                continue
            gi, gj = g.GOALS_IJ[k]
            assert tuple(q[-1]) == (g.OFF[0] + gi, g.OFF[1] + gj, 0.0, g.HEADINGS[k])
            assert np.array_equal(q[:, :2], slots[:, :2] + np.array(g.OFF))
            xy = q[:, :2] - np.array(g.OFF)
            end = (ref.node(xy[-2, 0], RES, g.NX), ref.node(xy[-2, 1], RES, g.NY))
            assert end == (gi, gj) and labels[gj, gi] == k
    finally:
        p.close()


def test_symbols_and_record_layout(dymu):
    fim, pl = dymu.load_fim(), dymu.load_planner()
    for n in ("dymu_arrive_paths_device", "dymu_last_arrive_ms"):
        assert hasattr(fim, n) and n in dymu.FIM_SYMBOLS, n
    for n in ("dymu_planner_get_arriving_paths", "dymu_planner_get_arriving_paths_to",
              "dymu_planner_get_arriving_stats", "dymu_planner_get_arriving_stats_to"):
        assert hasattr(pl, n) and n in dymu.PLANNER_SYMBOLS, n
    d = dymu.ARRIVE_STAT_DTYPE
    assert d.itemsize == 32 and d.fields["hops"][1] == 12 and d.fields["start_cost"][1] == 24
    assert fim.dymu_arrive_paths_device(None, None, 8, 8, 8, 1.0, 1, 1, None, None, 0, 0.4, None,
                                        0, 4, 1, None, None, None, None) == -1
    assert pl.dymu_planner_get_arriving_stats(None, None, 0, 4, 1, None) == -1
