"""The arriving descent on the device (k_arrive_paths, csrc/arrive_kernels.hip): records
and waypoints equal the host rule's on the engine's own map exactly, every start on a
finite node arrives, and the rule's invariants hold.  The host side of each comparison is a
second planner that never creates an engine and holds the first one's map.  A case's maps,
starts and references are computed once and shared by its tests."""
import numpy as np
import pytest

import arrive_ref as ref

pytestmark = pytest.mark.gpu

RD = 0.5  # risk_distance: tau = min(0.4, RD) = 0.4
TAU = 0.4
RES = 1.0
HEADING = 1.25
CASES = {"96x96": (96, 96, (70, 60)), "97x61": (97, 61, (70, 40))}


class Case:
    pass


def _same(a, b):
    """Two structured record arrays, bit for bit."""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_paths(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes()
                                    for x, y in zip(a, b))


def _host_twin(dymu, F, T, goal=None, goals=None, offsets=None):
    """A planner without an engine that holds the map T: its calls take the host route."""
    ny, nx = F.shape
    h = dymu.Planner(risk_distance=RD)
    assert h.initGlobalLayer(RES, 0.5, nx, ny)
    assert h.setCostMap(np.where(np.isfinite(F), F, -1.0))
    assert h.setGoals(goals, offsets) if goals else h.setGoal((goal[0], goal[1], 0.0, HEADING))
    assert h.loadTotalCostMap(T)
    return h


def _starts(nx, ny, n=200):
    rng = np.random.default_rng(7)
    xy = np.stack([rng.uniform(2, nx - 3, n), rng.uniform(2, ny - 3, n)], axis=1)
    return xy, [(x, y, 0.5, 0.01 * k) for k, (x, y) in enumerate(xy)]


@pytest.fixture(scope="module", params=[(s, o) for s in sorted(CASES) for o in (0.0, 0.02)],
                ids=lambda p: f"{p[0]}-obst{p[1]}")
def case(request, dymu, oracle):
    shape, obst = request.param
    nx, ny, goal = CASES[shape]
    c = Case()
    c.shape, c.obst, c.nx, c.ny, c.goal = shape, obst, nx, ny, goal
    c.F = oracle.synth_speed(nx, ny, seed=21, obst_frac=obst, goal=goal)
    p = dymu.Planner(risk_distance=RD)
    assert p.initGlobalLayer(RES, 0.5, nx, ny)
    assert p.setCostMap(np.where(np.isfinite(c.F), c.F, -1.0))
    assert p.setGoal((goal[0], goal[1], 0.0, HEADING))
    assert p.computeEntireTotalCostMap()
    c.xy, c.starts = _starts(nx, ny)
    c.paths, c.status, c.rec = p.getArrivingPaths(c.starts)
    c.on_device, c.kernel_ms = p.lastPathsOnDevice(), p.lastPathsKernelMs()
    c.sinks = p.lastPathSinks()
    c.stats = p.getArrivingStats(c.starts)
    c.stats_on_device, c.stats_ms = p.lastPathsOnDevice(), p.lastPathsKernelMs()
    c.T = p.totalCostRaw()
    c.h = _host_twin(dymu, c.F, c.T, goal=goal)
    c.hpaths, c.hstatus, c.hrec = c.h.getArrivingPaths(c.starts)
    c.host_on_device = c.h.lastPathsOnDevice()
    c.finite = np.array([np.isfinite(c.T[int(y + 0.5), int(x + 0.5)]) for x, y in c.xy])
    c.p = p
    yield c
    p.close()
    c.h.close()


def test_device_equals_host_exactly(case):
    assert case.on_device and case.kernel_ms > 0 and not case.host_on_device
    for name in case.rec.dtype.names:
        d, h = case.rec[name], case.hrec[name]
        assert np.array_equal(d, h), (name, np.argwhere(d != h)[:4])
    assert _same(case.rec, case.hrec)  # byte for byte
    assert np.array_equal(case.status, case.hstatus)
    assert np.array_equal(case.rec["status"], case.status)
    assert np.array_equal(case.rec["sink"], case.sinks)
    assert _same_paths(case.paths, case.hpaths)  # x, y, z, heading and the counts
    assert np.array_equal(case.rec["count"], [len(q) for q in case.paths])
    assert np.median(case.rec["count"]) > 30
    # ... and both are the plain-Python rule
    for q in range(0, 200, 7):
        r, slots = ref.descend(case.T, RES, TAU, case.xy[q], goal=case.goal)
        assert ref.same_record(case.rec[q], r) is None, (q, ref.same_record(case.rec[q], r))
        assert np.array_equal(case.paths[q][:, :2], slots[:, :2])


def test_records_only_call_equals_the_stored_call(case):
    assert case.stats_on_device and case.stats_ms > 0
    assert _same(case.stats, case.rec)
    assert _same(case.h.getArrivingStats(case.starts, host=True), case.rec)
    assert _same(case.p.getArrivingStats(case.starts, host=True), case.rec)
    assert not case.p.lastPathsOnDevice()


def test_arrival_and_invariants_on_the_engines_map(case):
    assert np.array_equal(case.status == 1, case.finite)
    assert np.array_equal(case.status == -1, ~case.finite)
    for q in np.flatnonzero(case.finite):
        xy = case.paths[q][:, :2]
        assert ref.check_path(case.T, xy, RES) is None, (q, ref.check_path(case.T, xy, RES))
        assert tuple(xy[-1]) == (float(case.goal[0]), float(case.goal[1]))
        assert np.abs(xy[-2] - xy[-1]).max() <= 0.5 * RES
    # the ground getPaths cannot cover: its descent is cut short from these starts
    paths, status = case.p.getPaths(case.starts)
    cut = [q for q in range(200) if status[q] == 1 and case.finite[q] and
           np.hypot(*(paths[q][-1, :2] - paths[q][-2, :2])) > 2.4 * RES]
    print(f"{case.shape} obst {case.obst}: {int(case.finite.sum())} arrive, {len(cut)} of them "
          f"cut short by getPaths; hops {int(case.rec['hops'].sum())} of "
          f"{int(case.rec['count'].sum())} waypoints; kernel {case.kernel_ms:.3f} ms stored, "
          f"{case.stats_ms:.3f} ms records only")
    if case.obst:
        assert len(cut) >= 10 and case.rec["hops"].sum() > 0
    else:
        assert not cut


@pytest.mark.parametrize("m", [1, 65])
def test_small_batches(case, m):
    paths, status, rec = case.p.getArrivingPaths(case.starts[:m])
    assert case.p.lastPathsOnDevice()
    assert _same(rec, case.rec[:m]) and _same_paths(paths, case.paths[:m])
    assert _same(case.p.getArrivingStats(case.starts[:m]), case.rec[:m])


class Arena:
    """Device copies of a case's map, unpadded and with a pitch above nx, freed together."""

    def __init__(self, engine, case):
        self.engine, self.ptrs = engine, []
        self.T = self.put(case.T)
        self.ld = case.nx + 5
        padded = np.full((case.ny, self.ld), -7.0)  # never read: below every value of T
        padded[:, :case.nx] = case.T
        self.Tp = self.put(padded)

    def put(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        d = self.engine.alloc(a.nbytes)
        self.ptrs.append(d)
        self.engine.h2d(d, a)
        return d

    def close(self):
        for d in self.ptrs:
            self.engine.free(d)


@pytest.fixture(scope="module")
def arena(case, engine):
    a = Arena(engine, case)
    yield a
    a.close()


def _engine_paths(engine, case, dT, ld, xy, max_wp, **kw):
    return engine.arrive_paths(dT, case.nx, case.ny, ld, RES, case.goal[0], case.goal[1], TAU, xy,
                               max_wp=max_wp, **kw)


def test_engine_entry_pitch_stride_and_capacity(case, engine, arena, dymu):
    nx = case.nx
    cap = int(case.rec["count"].max())
    out, cnt, rec = _engine_paths(engine, case, arena.Tp, arena.ld, case.xy[:130], cap)
    assert engine.last_arrive_ms() > 0
    assert _same(rec, case.rec[:130])
    assert np.array_equal(cnt, case.rec["count"][:130])
    for q in range(130):
        assert np.array_equal(out[q, :cnt[q], :2], case.paths[q][:, :2]), q
    none, nocnt, only = _engine_paths(engine, case, arena.Tp, arena.ld, case.xy[:130], cap,
                                      store=False)
    assert none is None and nocnt is None and _same(only, rec)
    # a slot capacity below a path's length: status -3, the first slots kept, the record
    # covering them; the same starts again with more slots give the whole paths (the
    # planner's re-run of overflowing paths)
    small = 16
    o16, c16, r16 = _engine_paths(engine, case, arena.T, nx, case.xy[:130], small)
    over = case.rec["count"][:130] > small
    assert over.sum() > 100
    assert np.array_equal(r16["status"], np.where(over, -3, case.rec["status"][:130]))
    assert np.array_equal(c16, np.minimum(case.rec["count"][:130], small))
    assert (r16["sink"][over] == -1).all() and np.array_equal(r16["count"], c16)
    assert np.array_equal(o16[:, :small], out[:, :small])
    for q in np.flatnonzero(over)[:20]:
        want, _ = ref.descend(case.T, RES, TAU, case.xy[q], goal=case.goal, max_wp=small)
        assert ref.same_record(r16[q], want) is None, q
    # stride 3: waypoints 0, 3, 6, ... and the sink; the record is that of stride 1
    o3, c3, r3 = _engine_paths(engine, case, arena.T, nx, case.xy[:65], cap, stride=3)
    assert _same(r3, case.rec[:65])
    for q in range(65):
        if case.status[q] == 1:
            want = np.vstack([case.paths[q][:-1][::3], case.paths[q][-1:]])[:, :2]
            assert c3[q] == len(want) and np.array_equal(o3[q, :c3[q], :2], want), q
    for kw in (dict(max_wp=0), dict(stride=0), dict(ld=nx - 1), dict(goal_i=nx), dict(res=0.0),
               dict(tau=float("nan")), dict(d_label=arena.T, goals_ij=np.zeros((0, 2)))):
        a = dict(dT=arena.T, nx=nx, ny=case.ny, ld=nx, res=RES, goal_i=1, goal_j=1, tau=TAU,
                 starts_xy=case.xy[:2], max_wp=16)
        a.update(kw)
        with pytest.raises(dymu.DymuError) as e:
            engine.arrive_paths(**a)
        assert e.value.status == -1, kw


def test_rejected_starts_at_the_grid_edge(case):
    """Starts whose node is off the grid or an obstacle end with status -1 and the empty
    record before any load; starts on the last row and column are nodes like any other."""
    nx, ny = case.nx, case.ny
    bad = [(float("nan"), 5.0), (5.0, float("nan")), (-0.2, 5.0), (5.0, -3.0), (1e300, 5.0),
           (-1e300, 5.0), (nx - 0.5, 5.0), (5.0, ny - 0.5), (nx - 0.5, ny - 0.5),
           (4294967296.0 + 5.5, 5.0), (float("inf"), float("-inf"))]
    if case.obst:
        oj, oi = np.argwhere(np.isinf(case.T))[-1]
        bad.append((oi - 0.3, oj + 0.2))
    edge = [(nx - 1.0, 7.3), (9.4, ny - 1.0), (nx - 0.6, ny - 0.6), (0.0, 0.0), (nx - 1.4, 0.2)]
    batch = []
    for k, b in enumerate(bad):
        batch += [case.starts[k], b]
    batch += edge
    paths, status, rec = case.p.getArrivingPaths(batch)
    assert case.p.lastPathsOnDevice()
    hpaths, hstatus, hrec = case.h.getArrivingPaths(batch)
    assert _same(rec, hrec) and _same_paths(paths, hpaths) and np.array_equal(status, hstatus)
    assert _same(case.p.getArrivingStats(batch), rec)
    for k in range(len(bad)):
        assert rec[2 * k] == case.rec[k] and paths[2 * k].tobytes() == case.paths[k].tobytes()
        assert ref.same_record(rec[2 * k + 1], ref.empty_record()) is None, bad[k]
        assert status[2 * k + 1] == -1 and len(paths[2 * k + 1]) == 0
    for s, st in zip(edge, status[2 * len(bad):]):
        if np.isfinite(case.T[int(s[1] + 0.5), int(s[0] + 0.5)]):
            assert st == 1, s


def test_goal_set(dymu, oracle):
    nx, ny, _ = CASES["97x61"]
    goals_ij = [(70, 40), (12, 9), (30, 50)]
    F = oracle.synth_speed(nx, ny, seed=21, obst_frac=0.02, goal=goals_ij[0])
    for gi, gj in goals_ij:
        blk = F[gj - 1:gj + 2, gi - 1:gi + 2]
        blk[~np.isfinite(blk)] = 3.0
    goals = [(float(i), float(j), 0.0, 0.1 * k) for k, (i, j) in enumerate(goals_ij)]
    p = dymu.Planner(risk_distance=RD)
    h = None
    try:
        assert p.initGlobalLayer(RES, 0.5, nx, ny)
        assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
        offsets = [0.0, 6.5, 0.0]
        assert p.setGoals(goals, offsets)
        assert p.computeEntireTotalCostMap()
        xy, starts = _starts(nx, ny)
        paths, status, rec = p.getArrivingPaths(starts)
        assert p.lastPathsOnDevice() and p.lastPathsKernelMs() > 0
        sinks = p.lastPathSinks()
        stats = p.getArrivingStats(starts)
        assert p.lastPathsOnDevice() and _same(stats, rec)
        T, labels = p.totalCostRaw(), p.goalLabels()
        h = _host_twin(dymu, F, T, goals=goals, offsets=offsets)
        assert np.array_equal(h.goalLabels(), labels)
        hpaths, hstatus, hrec = h.getArrivingPaths(starts)
        assert not h.lastPathsOnDevice()
        assert _same(rec, hrec) and _same_paths(paths, hpaths) and np.array_equal(status, hstatus)
        assert np.array_equal(rec["sink"], sinks) and np.array_equal(sinks, h.lastPathSinks())
        assert set(sinks[status == 1]) == {0, 1, 2}
        for q in range(200):
            lab = labels[int(xy[q][1] + 0.5), int(xy[q][0] + 0.5)]
            assert (status[q] == 1) == (lab != dymu.LABEL_NONE), q
            if status[q] == 1:
                gi, gj = goals_ij[sinks[q]]
                assert tuple(paths[q][-1]) == (float(gi), float(gj), 0.0, 0.1 * sinks[q])
                end = paths[q][-2, :2]
                assert (ref.node(end[0], RES, nx), ref.node(end[1], RES, ny)) == (gi, gj)
                assert ref.check_path(T, paths[q][:, :2], RES) is None, q
        for q in range(0, 200, 9):
            r, slots = ref.descend(T, RES, TAU, xy[q], labels=labels, goals_ij=goals_ij)
            assert ref.same_record(rec[q], r) is None, q
    finally:
        p.close()
        if h:
            h.close()


def test_batch_planes(dymu, oracle):
    nx, ny, goal = CASES["97x61"]
    F = oracle.synth_speed(nx, ny, seed=21, obst_frac=0.02, goal=goal)
    other = (20, 15)
    blk = F[other[1] - 1:other[1] + 2, other[0] - 1:other[0] + 2]
    blk[~np.isfinite(blk)] = 3.0
    targets = [(goal[0], goal[1], 0.0, 0.0), (other[0], other[1], 0.0, 0.3)]
    p = dymu.Planner(risk_distance=RD)
    try:
        assert p.initGlobalLayer(RES, 0.5, nx, ny)
        assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
        assert p.computeTotalCostMaps(targets)
        xy, starts = _starts(nx, ny, 130)
        for b in (1, 0):
            paths, status, rec = p.getArrivingPathsTo(b, starts)
            assert p.lastPathsOnDevice() and p.lastPathsKernelMs() > 0
            stats = p.getArrivingStatsTo(b, starts)
            assert p.lastPathsOnDevice() and p.lastPathsKernelMs() > 0 and _same(stats, rec)
            T = p.batchTotalCost(b)
            g = (int(targets[b][0]), int(targets[b][1]))
            h = _host_twin(dymu, F, T, goal=g)
            try:
                hpaths, hstatus, hrec = h.getArrivingPaths(starts)
            finally:
                h.close()
            assert _same(rec, hrec) and np.array_equal(status, hstatus)
            for q in range(130):  # the twin's sink heading is its own goal's
                assert np.array_equal(paths[q][:, :3], hpaths[q][:, :3]), (b, q)
                assert np.array_equal(paths[q][:-1, 3], hpaths[q][:-1, 3]), (b, q)
                if status[q] == 1:
                    assert paths[q][-1, 3] == targets[b][3]
                    assert ref.check_path(T, paths[q][:, :2], RES) is None, (b, q)
            fin = np.array([np.isfinite(T[int(y + 0.5), int(x + 0.5)]) for x, y in xy])
            assert np.array_equal(status == 1, fin) and fin.sum() > 100
            assert np.array_equal(p.lastPathSinks(), np.where(status == 1, 0, -1))
        with pytest.raises(dymu.DymuError):
            p.getArrivingStatsTo(2, starts)
        with pytest.raises(dymu.DymuError):
            p.getArrivingPathsTo(0, starts, max_wp=0)
    finally:
        p.close()
