"""getPathStats on the device (k_path_stats, csrc/path_stats_kernels.hip): every member of
every record equals the host route's on the same map exactly, whatever the number of
lanes the work queue feeds.  The maps, starts and references of a case are computed once
and shared by its tests."""
import numpy as np
import pytest

import path_stats_ref as ref

pytestmark = pytest.mark.gpu

RD = 0.5  # risk_distance: tau = min(0.4, RD) = 0.4
RES = 1.0
HEADING = 1.25
CASES = {"96x96": (96, 96, (70, 60)), "97x61": (97, 61, (70, 40))}


class Case:
    pass


def _elevation(nx, ny):
    j, i = np.mgrid[0:ny, 0:nx].astype(float)
    return 0.3 * np.sin(0.3 * i) + 0.1 * np.cos(0.2 * j) + 0.01 * i


def _same(a, b):
    """Two structured record arrays, bit for bit."""
    return a.shape == b.shape and a.tobytes() == b.tobytes()


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
    rng = np.random.default_rng(7)
    c.xy = np.stack([rng.uniform(2, nx - 3, 200), rng.uniform(2, ny - 3, 200)], axis=1)
    c.starts = [(x, y, 0.0, 0.01 * k) for k, (x, y) in enumerate(c.xy)]
    c.elev = _elevation(nx, ny)
    c.stats = p.getPathStats(c.starts, field=c.elev)
    c.on_device = p.lastPathsOnDevice()
    c.kernel_ms = p.lastPathsKernelMs()
    c.host = p.getPathStats(c.starts, field=c.elev, host=True)
    c.host_on_device = p.lastPathsOnDevice()
    c.paths, c.status = p.getPaths(c.starts)
    c.T = p.totalCostRaw()
    c.p = p
    yield c
    p.close()


def test_device_equals_host_exactly(case):
    assert case.on_device and case.kernel_ms > 0 and not case.host_on_device
    d, h = case.stats, case.host
    assert d.shape == (200,)
    for name in d.dtype.names:
        assert np.array_equal(d[name], h[name]), (name, np.argwhere(d[name] != h[name])[:4])
    assert _same(d, h)
    assert np.array_equal(d["status"], case.status)
    assert np.array_equal(d["count"], [len(q) for q in case.paths])
    assert np.median(d["count"]) > 30
    # ... and both are the numpy record of getPaths' waypoints (offset 0: exact)
    for q in range(0, 200, 7):
        r = ref.path_record(case.paths[q][:, :2], RES, [case.F, case.elev])
        assert ref.same_record(d[q], r) is None, (q, ref.same_record(d[q], r))
    # the conditions that keep the case meaningful, on the engine's map
    arrived = (d["status"] == 1) & (d["last_hop"] <= 2.4 * RES * (1 + 1e-12))
    cut = (d["status"] == 1) & ~arrived
    skipped0 = d["skipped"][:, 0] > 0
    print(f"{case.shape} obst {case.obst}: {int(arrived.sum())} arrived, {int(cut.sum())} cut "
          f"short, {int(skipped0.sum())} with skipped[0] > 0; kernel {case.kernel_ms:.3f} ms")
    if case.obst == 0.0:
        assert (d["last_hop"] <= 2.4 * RES * (1 + 1e-12)).all()
    else:
        assert cut.sum() >= 10 and arrived.sum() >= 150 and skipped0.sum() >= 20
    assert (d["skipped"][:, 1] == 0).all()


@pytest.mark.parametrize("m", [1, 65, 130])
def test_batch_sizes(case, m):
    s = case.p.getPathStats(case.starts[:m], field=case.elev)
    assert case.p.lastPathsOnDevice()
    assert _same(s, case.stats[:m])


def test_second_call_is_bit_equal(case):
    assert _same(case.p.getPathStats(case.starts, field=case.elev), case.stats)
    # without the caller's field slot 1 is the unused one and slot 0 is unchanged
    s = case.p.getPathStats(case.starts)
    assert case.p.lastPathsOnDevice()
    for name in ("status", "sink", "count", "length", "last_hop"):
        assert np.array_equal(s[name], case.stats[name])
    for name, v in (("integral", 0.0), ("vmin", np.inf), ("vmax", -np.inf), ("skipped", 0)):
        assert np.array_equal(s[name][:, 0], case.stats[name][:, 0])
        assert (s[name][:, 1:] == v).all()


class Arena:
    """Device copies of a case's maps, unpadded and padded, freed together."""

    def __init__(self, engine, case):
        self.engine, self.ptrs = engine, []
        nx, ny = case.nx, case.ny
        self.T = self.put(case.T)
        self.F = self.put(case.F)
        self.E = self.put(case.elev)
        self.ld, self.fld = nx + 5, nx + 3
        self.Tp = self.put(self.padded(case.T, self.ld))
        self.Fp = self.put(self.padded(case.F, self.ld))
        self.Ep = self.put(self.padded(case.elev, self.fld))

    @staticmethod
    def padded(a, ld):
        out = np.full((a.shape[0], ld), -7.0)  # never a valid value of any of the maps
        out[:, :a.shape[1]] = a
        return out

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


def _engine_stats(engine, case, dT, ld, fields, n_lanes=0, m=200):
    return engine.path_stats(dT, case.nx, case.ny, ld, RES, case.goal[0], case.goal[1], 0.4,
                             case.xy[:m], max_wp=1 << 20, fields=fields, n_lanes=n_lanes)


def test_work_queue(case, engine, arena):
    """64 lanes for 200 paths: every lane takes a second path and some a fourth; 256 lanes:
    one path per lane.  The records are those of the planner's call either way."""
    nx = case.nx
    fields = [(arena.F, nx), (arena.E, nx)]
    queued = _engine_stats(engine, case, arena.T, nx, fields, n_lanes=64)
    assert engine.last_path_stats_ms() > 0
    static = _engine_stats(engine, case, arena.T, nx, fields, n_lanes=256)
    default = _engine_stats(engine, case, arena.T, nx, fields)
    one = _engine_stats(engine, case, arena.T, nx, fields, n_lanes=1)  # rounded up to a wave
    assert _same(queued, static) and _same(default, static) and _same(one, static)
    assert _same(static, case.stats)


def test_padded_pitches(case, engine, arena):
    nx = case.nx
    s = _engine_stats(engine, case, arena.Tp, arena.ld, [(arena.Fp, arena.ld), (arena.Ep, arena.fld)],
                      n_lanes=64, m=130)
    assert _same(s, case.stats[:130])


def test_field_slots_and_argument_errors(case, engine, arena, dymu):
    nx = case.nx
    # four slots, and none: a slot's figures do not depend on the others
    four = _engine_stats(engine, case, arena.T, nx, [(arena.E, nx), (arena.F, nx), (arena.E, nx),
                                                     (arena.F, nx)], m=65)
    none = _engine_stats(engine, case, arena.T, nx, [], m=65)
    for name in ("integral", "vmin", "vmax", "skipped"):
        for slot, src in enumerate((1, 0, 1, 0)):
            assert np.array_equal(four[name][:, slot], case.stats[name][:65, src]), (name, slot)
        assert np.array_equal(none[name], ref_unused(65, name))
    for name in ("status", "sink", "count", "length", "last_hop"):
        assert np.array_equal(four[name], case.stats[name][:65])
        assert np.array_equal(none[name], case.stats[name][:65])
    for kw in (dict(max_wp=0), dict(fields=[(arena.F, nx)] * 5), dict(fields=[(arena.F, nx - 1)]),
               dict(fields=[(0, nx)]), dict(ld=nx - 1), dict(goal_i=nx), dict(res=0.0),
               dict(tau=float("nan"))):
        a = dict(dT=arena.T, nx=nx, ny=case.ny, ld=nx, res=RES, goal_i=1, goal_j=1, tau=0.4,
                 starts_xy=case.xy[:2], max_wp=16, fields=[(arena.F, nx)])
        a.update(kw)
        with pytest.raises(dymu.DymuError) as e:
            engine.path_stats(**a)
        assert e.value.status == -1, kw


def ref_unused(n, name):
    v = {"integral": 0.0, "vmin": np.inf, "vmax": -np.inf, "skipped": 0}[name]
    return np.full((n, 4), v)


def test_max_wp_cuts_the_record(case):
    q = int(np.argmax([len(w) if st == 1 else 0 for w, st in zip(case.paths, case.status)]))
    full = case.paths[q]
    assert len(full) > 40
    for m, st in ((8, -3), (len(full) - 1, -3), (len(full), 1)):
        (d,) = case.p.getPathStats([case.starts[q]], max_wp=m, field=case.elev)
        assert case.p.lastPathsOnDevice()
        (h,) = case.p.getPathStats([case.starts[q]], max_wp=m, field=case.elev, host=True)
        assert d == h and d["status"] == st and d["count"] == m
        r = ref.path_record(full[:m, :2], RES, [case.F, case.elev])
        assert ref.same_record(d, r) is None, m


def test_rejected_starts_leave_the_batch_alone(case):
    """NaN, negative, huge and last-cell starts end with status -1 and the empty record
    (the kernel tests the cell in 64-bit before any load); the valid ones are unchanged."""
    nx, ny = case.nx, case.ny
    bad = [(float("nan"), 5.0), (5.0, float("nan")), (-0.5 - 1.0, 5.0), (5.0, -3.0),
           (1e300, 5.0), (-1e300, 5.0), (nx - 1 + 0.5, 5.0), (5.0, ny - 1 + 0.25),
           (4294967296.0 + 5.5, 5.0), (float("inf"), float("-inf"))]
    batch = []
    for k, b in enumerate(bad):
        batch += [case.starts[k], b]
    batch.append(case.starts[len(bad)])
    # x / res = -0.5 truncates to cell 0: getPaths accepts such a start, and so do both routes
    batch.append((-0.5, 5.0, 0.0, 0.0))
    s = case.p.getPathStats(batch, field=case.elev)
    assert case.p.lastPathsOnDevice()
    assert _same(s, case.p.getPathStats(batch, field=case.elev, host=True))
    for k in range(len(bad)):
        assert s[2 * k] == case.stats[k]
        r = s[2 * k + 1]
        assert r["status"] == -1 and r["sink"] == -1, bad[k]
        assert ref.same_record(r, ref.empty_record()) is None, bad[k]
    assert s[-2] == case.stats[len(bad)]
    (w,), (st,) = case.p.getPaths([batch[-1]])
    assert s[-1]["status"] == st and s[-1]["count"] == len(w)


def test_off_grid_samples_on_the_device(dymu):
    """The loaded map whose descent leaves the grid westwards (path_stats_ref): with an
    engine loadTotalCostMap uploads it, and the device counts the off-grid sample as the
    host does."""
    nx, ny = 32, 16
    T, goal, start = ref.off_grid_map(nx, ny)
    p = dymu.Planner(risk_distance=RD)
    try:
        assert p.initGlobalLayer(RES, 0.5, nx, ny)
        assert p.setCostMap(np.ones((ny, nx)))
        assert p.setGoal((float(goal[0]), float(goal[1]), 0.0, 0.0))
        assert p.computeEntireTotalCostMap()  # creates the engine and packs the speed
        assert p.loadTotalCostMap(T)
        field = _elevation(nx, ny)
        (d,) = p.getPathStats([start], field=field)
        assert p.lastPathsOnDevice()
        (h,) = p.getPathStats([start], field=field, host=True)
        (w,), _ = p.getPaths([start])
        _, _, on = ref.nearest_nodes(w[:, :2], RES, nx, ny)
        assert (~on).sum() >= 1
        assert d == h and d["skipped"][0] == d["skipped"][1] == (~on).sum()
        assert ref.same_record(d, ref.path_record(w[:, :2], RES, [np.ones((ny, nx)), field])) is None
    finally:
        p.close()


def test_goal_set(dymu, oracle):
    nx, ny, _ = CASES["96x96"]
    goals = [(70, 60), (15, 20), (40, 85)]
    F = oracle.synth_speed(nx, ny, seed=21, obst_frac=0.02, goal=goals[0])
    for g in goals:
        F[g[1], g[0]] = 1.0 if not np.isfinite(F[g[1], g[0]]) else F[g[1], g[0]]
    p = dymu.Planner(risk_distance=RD)
    try:
        assert p.initGlobalLayer(RES, 0.5, nx, ny)
        assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
        assert p.setGoals([(g[0], g[1], 0.0, 0.1 * k) for k, g in enumerate(goals)])
        assert p.computeEntireTotalCostMap()
        rng = np.random.default_rng(7)
        starts = [(x, y, 0.0, 0.0) for x, y in rng.uniform(2, 92, (200, 2))]
        elev = _elevation(nx, ny)
        d = p.getPathStats(starts, field=elev)
        assert p.lastPathsOnDevice() and p.lastPathsKernelMs() > 0
        h = p.getPathStats(starts, field=elev, host=True)
        assert not p.lastPathsOnDevice()
        paths, status = p.getPaths(starts)
        sinks = p.lastPathSinks()
        assert _same(d, h)
        assert np.array_equal(d["sink"], sinks) and np.array_equal(d["status"], status)
        assert len(set(sinks[sinks >= 0])) >= 2  # more than one goal drains starts
        for q in range(0, 200, 9):
            r = ref.path_record(paths[q][:, :2], RES, [F, elev])
            assert ref.same_record(d[q], r) is None, q
    finally:
        p.close()


def test_batch_plane(dymu, oracle):
    nx, ny, goal = CASES["97x61"]
    F = oracle.synth_speed(nx, ny, seed=21, obst_frac=0.02, goal=goal)
    other = (20, 15)
    F[other[1], other[0]] = 1.0 if not np.isfinite(F[other[1], other[0]]) else F[other[1], other[0]]
    p = dymu.Planner(risk_distance=RD)
    try:
        assert p.initGlobalLayer(RES, 0.5, nx, ny)
        assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
        assert p.computeTotalCostMaps([(goal[0], goal[1], 0.0, 0.0), (other[0], other[1], 0.0, 0.3)])
        rng = np.random.default_rng(7)
        starts = [(x, y, 0.0, 0.0) for x, y in
                  np.stack([rng.uniform(2, nx - 3, 130), rng.uniform(2, ny - 3, 130)], axis=1)]
        elev = _elevation(nx, ny)
        for b in (1, 0):
            d = p.getPathStatsTo(b, starts, field=elev)
            assert p.lastPathsOnDevice() and p.lastPathsKernelMs() > 0
            paths, status = p.getPathsTo(b, starts)
            assert np.array_equal(d["status"], status)
            assert np.array_equal(d["sink"], np.where(status == 1, 0, -1))
            for q in range(130):
                r = ref.path_record(paths[q][:, :2], RES, [F, elev])
                assert ref.same_record(d[q], r) is None, (b, q, ref.same_record(d[q], r))
        assert (d["status"] == 1).sum() > 100
        with pytest.raises(dymu.DymuError):
            p.getPathStatsTo(2, starts)
        with pytest.raises(dymu.DymuError):
            p.getPathStatsTo(0, starts, max_wp=0)
    finally:
        p.close()
