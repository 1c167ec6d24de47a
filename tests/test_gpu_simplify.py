"""getSimplifiedPaths on the device (k_arrive_paths' simplified instantiations,
csrc/arrive_kernels.hip with csrc/path_simplify.h): paths, indices, counts and records equal
the host route's on the engine's own map exactly, and the plain-Python rule's.  The host
side of each comparison is a second planner that never creates an engine and holds the
first one's map.  A case's maps, starts and references are computed once and shared by its
tests; eps is given in multiples of res."""
import numpy as np
import pytest

import arrive_ref as aref
import simplify_ref as sref

pytestmark = pytest.mark.gpu

RD = 0.5  # risk_distance: tau = min(0.4, RD) = 0.4
TAU = 0.4
RES = 1.0
HEADING = 1.25
CASES = {"96x96": (96, 96, (70, 60)), "97x61": (97, 61, (70, 40))}
EPS = (0.05, 0.25, 1.0)
TINY = 1e-6  # nearly every waypoint is kept: the first slot capacity overflows


class Case:
    pass


def _same(a, b):
    """Two arrays (structured or not), bit for bit."""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_lists(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _same_result(a, b):
    """(paths, status, records, indices) twice: counts, x, y, z, heading, numbers, records."""
    return (_same_lists(a[0], b[0]) and np.array_equal(a[1], b[1]) and _same(a[2], b[2]) and
            _same_lists(a[3], b[3]))


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
    c.got, c.on_device, c.kernel_ms, c.reruns, c.bytes = {}, {}, {}, {}, {}
    for e in EPS + (TINY,):
        c.got[e] = p.getSimplifiedPaths(c.starts, e * RES)
        c.on_device[e], c.kernel_ms[e] = p.lastPathsOnDevice(), p.lastPathsKernelMs()
        c.reruns[e], c.bytes[e] = p.lastSimplifiedReruns(), p.lastSimplifiedBytes()
    c.full, c.fstatus, c.frec = p.getArrivingPaths(c.starts)
    c.stats = p.getArrivingStats(c.starts)
    c.T = p.totalCostRaw()
    c.h = _host_twin(dymu, c.F, c.T, goal=goal)
    c.hgot = {e: c.h.getSimplifiedPaths(c.starts, e * RES) for e in EPS + (TINY,)}
    c.host_on_device = c.h.lastPathsOnDevice()
    c.p = p
    yield c
    p.close()
    c.h.close()


@pytest.mark.parametrize("eps", EPS)
def test_device_equals_host_exactly(case, eps):
    assert case.on_device[eps] and case.kernel_ms[eps] > 0 and not case.host_on_device
    paths, status, rec, index = case.got[eps]
    hpaths, hstatus, hrec, hindex = case.hgot[eps]
    for name in rec.dtype.names:
        assert np.array_equal(rec[name], hrec[name]), (name, np.argwhere(rec[name] != hrec[name])[:4])
    assert _same(rec, hrec)  # byte for byte
    assert np.array_equal(status, hstatus) and np.array_equal(rec["status"], status)
    assert [len(i) for i in index] == [len(i) for i in hindex]  # the counts
    assert _same_lists(index, hindex)
    assert _same_lists(paths, hpaths)  # x, y, z, heading
    assert all(i.dtype == np.uint32 and len(i) == len(q) for i, q in zip(index, paths))
    # records equal getArrivingStats' and getArrivingPaths'; the paths are a subsequence
    assert _same(rec, case.stats) and _same(rec, case.frec)
    for q in range(200):
        assert _same(paths[q], case.full[q][index[q]]), q
        assert len(index[q]) < 2 or (np.diff(index[q].astype(np.int64)) > 0).all()
    # ... and all of it is the plain-Python rule on the plain-Python descent
    for q in range(0, 200, 7):
        r, slots = aref.descend(case.T, RES, TAU, case.xy[q], goal=case.goal)
        assert aref.same_record(rec[q], r) is None, (q, aref.same_record(rec[q], r))
        want = sref.simplify_slots(slots, r["status"], eps * RES)
        assert _same(index[q], want), q
        assert np.array_equal(paths[q][:, :2], slots[want, :2])
        n = len(slots) - (1 if r["status"] == 1 else 0)
        k = len(want) - (1 if r["status"] == 1 else 0)
        assert sref.check(slots[:n, :2], want[:k], eps * RES) is None
    walked = int(rec["count"].sum())
    kept = sum(len(i) for i in index)
    print(f"{case.shape} obst {case.obst} eps {eps}: {walked} waypoints, {kept} kept, "
          f"{case.reruns[eps]} reruns, {case.bytes[eps]} bytes down, kernel "
          f"{case.kernel_ms[eps]:.3f} ms")
    assert case.bytes[eps] >= 36 * 200 + 36 * kept


@pytest.mark.parametrize("m", [1, 65])
def test_partial_waves(case, m):
    for eps in EPS:
        got = case.p.getSimplifiedPaths(case.starts[:m], eps * RES)
        assert case.p.lastPathsOnDevice() and case.p.lastPathsKernelMs() > 0
        assert _same_result(got, tuple(x[:m] for x in case.got[eps]))


def test_rerun_of_paths_that_overflow_the_first_capacity(case):
    """eps so small that nearly every waypoint is kept: paths from far starts keep more than
    the first slot capacity and run again with the capacity they reported."""
    assert case.on_device[TINY] and case.reruns[TINY] > 0
    paths, status, rec, index = case.got[TINY]
    assert _same_result(case.got[TINY], case.hgot[TINY])
    kept = np.array([len(i) for i in index])
    # the first capacity is a guess of 64 slots at the least, here below the longest paths
    assert (kept > 64).sum() >= case.reruns[TINY] > 0
    assert kept.sum() > 0.9 * rec["count"].sum()
    for q in range(200):
        assert _same(paths[q], case.full[q][index[q]]), q
    # nothing overflows at the eps of the other tests on a grid this small or it would show
    assert all(case.reruns[e] <= case.reruns[TINY] for e in EPS)
    print(f"{case.shape} obst {case.obst}: {case.reruns[TINY]} of 200 paths rerun, longest "
          f"{kept.max()} kept")


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


def _engine_call(engine, case, dT, ld, xy, eps, max_steps, max_kept, **kw):
    return engine.arrive_simplified(dT, case.nx, case.ny, ld, RES, case.goal[0], case.goal[1], TAU,
                                    xy, eps, max_steps, max_kept, **kw)


def test_engine_entry_counts_capacity_and_count_only(case, engine, arena, dymu):
    nx, eps, m = case.nx, 0.25 * RES, 130
    paths, status, rec, index = case.got[0.25]
    kept = np.array([len(i) for i in index[:m]])
    cap = int(kept.max())
    out, idx, cnt, r = _engine_call(engine, case, arena.Tp, arena.ld, case.xy[:m], eps, 1 << 20, cap)
    assert engine.last_arrive_simplified_ms() > 0
    assert _same(r, rec[:m]) and np.array_equal(cnt, kept)
    for q in range(m):
        assert np.array_equal(out[q, :cnt[q], :2], paths[q][:, :2]), q
        assert np.array_equal(idx[q, :cnt[q]], index[q]), q
        assert not out[q, cnt[q]:].any() and not idx[q, cnt[q]:].any()
    # two calls are byte-identical
    out2, idx2, cnt2, r2 = _engine_call(engine, case, arena.T, nx, case.xy[:m], eps, 1 << 20, cap)
    assert _same(out, out2) and _same(idx, idx2) and _same(cnt, cnt2) and _same(r, r2)
    # four slots: the count is still what the rule keeps, the first four are stored, and
    # neither the status nor the record changes
    o4, i4, c4, r4 = _engine_call(engine, case, arena.T, nx, case.xy[:m], eps, 1 << 20, 4)
    assert (kept > 4).sum() > 100
    assert np.array_equal(c4, kept) and _same(r4, rec[:m])
    for q in range(m):
        k = min(4, kept[q])
        assert _same(o4[q, :k], out[q, :k]) and _same(i4[q, :k], idx[q, :k]), q
    # count only: no slots, no numbers
    none, noidx, c0, r0 = _engine_call(engine, case, arena.T, nx, case.xy[:m], eps, 1 << 20, 0,
                                       store=False, with_index=False)
    assert none is None and noidx is None and np.array_equal(c0, kept) and _same(r0, rec[:m])
    # slots without numbers
    o5, no5, c5, r5 = _engine_call(engine, case, arena.T, nx, case.xy[:m], eps, 1 << 20, cap,
                                   with_index=False)
    assert no5 is None and _same(o5, out) and _same(c5, cnt) and _same(r5, r)
    # the walk limit: status -3, the record covers the waypoints walked, the last is kept
    steps = 16
    o16, i16, c16, r16 = _engine_call(engine, case, arena.T, nx, case.xy[:m], eps, steps, steps)
    over = rec["count"][:m] > steps
    assert over.sum() > 100
    assert np.array_equal(r16["status"], np.where(over, -3, rec["status"][:m]))
    for q in np.flatnonzero(over)[:20]:
        want, slots = aref.descend(case.T, RES, TAU, case.xy[q], goal=case.goal, max_wp=steps)
        assert aref.same_record(r16[q], want) is None, q
        widx = sref.simplify_slots(slots, -3, eps)
        assert c16[q] == len(widx) and np.array_equal(i16[q, :c16[q]], widx), q
        assert widx[-1] == steps - 1
        assert np.array_equal(o16[q, :c16[q]], slots[widx]), q  # x, y and the direction
    base = dict(dT=arena.T, nx=nx, ny=case.ny, ld=nx, res=RES, goal_i=1, goal_j=1, tau=TAU,
                starts_xy=case.xy[:2], eps=eps, max_steps=16, max_kept=16)
    for kw in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")),
               dict(max_steps=0), dict(max_kept=0), dict(max_kept=0, store=False),
               dict(ld=nx - 1), dict(goal_i=nx), dict(res=0.0), dict(tau=float("nan")),
               dict(d_label=arena.T, goals_ij=np.zeros((0, 2)))):
        a = dict(base)
        a.update(kw)
        with pytest.raises(dymu.DymuError) as e:
            engine.arrive_simplified(**a)
        assert e.value.status == -1, kw


def test_rejected_starts(case):
    nx, ny = case.nx, case.ny
    bad = [(float("nan"), 5.0), (-0.2, 5.0), (5.0, -3.0), (1e300, 5.0), (nx - 0.5, 5.0),
           (5.0, ny - 0.5), (float("inf"), float("-inf"))]
    if case.obst:
        oj, oi = np.argwhere(np.isinf(case.T))[-1]
        bad.append((oi - 0.3, oj + 0.2))
    edge = [(nx - 1.0, 7.3), (9.4, ny - 1.0), (nx - 0.6, ny - 0.6), (0.0, 0.0)]
    batch = []
    for k, b in enumerate(bad):
        batch += [case.starts[k], b]
    batch += edge
    got = case.p.getSimplifiedPaths(batch, 0.25 * RES)
    assert case.p.lastPathsOnDevice()
    assert _same_result(got, case.h.getSimplifiedPaths(batch, 0.25 * RES))
    for k in range(len(bad)):
        assert _same(got[0][2 * k], case.got[0.25][0][k])
        assert got[1][2 * k + 1] == -1 and len(got[0][2 * k + 1]) == 0 == len(got[3][2 * k + 1])
        assert aref.same_record(got[2][2 * k + 1], aref.empty_record()) is None


def test_bad_arguments_raise(case, dymu):
    for eps in (0.0, -0.25, float("nan"), float("inf")):
        with pytest.raises(dymu.DymuError):
            case.p.getSimplifiedPaths(case.starts[:2], eps)
    with pytest.raises(dymu.DymuError):
        case.p.getSimplifiedPaths(case.starts[:2], 0.25, max_wp=0)
    with pytest.raises(dymu.DymuError):
        case.p.getSimplifiedPathsTo(0, case.starts[:2], 0.25)  # no batch


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
        got = p.getSimplifiedPaths(starts, 0.25 * RES)
        assert p.lastPathsOnDevice() and p.lastPathsKernelMs() > 0
        sinks = p.lastPathSinks()
        full, fstatus, frec = p.getArrivingPaths(starts)
        assert _same(got[2], frec) and np.array_equal(sinks, p.lastPathSinks())
        T, labels = p.totalCostRaw(), p.goalLabels()
        h = _host_twin(dymu, F, T, goals=goals, offsets=offsets)
        assert _same_result(got, h.getSimplifiedPaths(starts, 0.25 * RES))
        assert not h.lastPathsOnDevice() and np.array_equal(sinks, h.lastPathSinks())
        assert set(sinks[got[1] == 1]) == {0, 1, 2}
        for q in range(200):
            assert _same(got[0][q], full[q][got[3][q]]), q
            if got[1][q] == 1:
                gi, gj = goals_ij[sinks[q]]
                assert tuple(got[0][q][-1]) == (float(gi), float(gj), 0.0, 0.1 * sinks[q])
        for q in range(0, 200, 9):
            r, slots = aref.descend(T, RES, TAU, xy[q], labels=labels, goals_ij=goals_ij)
            assert aref.same_record(got[2][q], r) is None, q
            assert _same(got[3][q], sref.simplify_slots(slots, r["status"], 0.25 * RES)), q
        tiny = p.getSimplifiedPaths(starts, TINY * RES)  # the rerun under a goal set
        assert p.lastSimplifiedReruns() > 0
        assert _same_result(tiny, h.getSimplifiedPaths(starts, TINY * RES))
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
            paths, status, rec, index = p.getSimplifiedPathsTo(b, starts, 0.25 * RES)
            assert p.lastPathsOnDevice() and p.lastPathsKernelMs() > 0
            assert np.array_equal(p.lastPathSinks(), np.where(status == 1, 0, -1))
            assert _same(p.getArrivingStatsTo(b, starts), rec)
            full, _, _ = p.getArrivingPathsTo(b, starts)
            T = p.batchTotalCost(b)
            g = (int(targets[b][0]), int(targets[b][1]))
            h = _host_twin(dymu, F, T, goal=g)
            try:
                hpaths, hstatus, hrec, hindex = h.getSimplifiedPaths(starts, 0.25 * RES)
            finally:
                h.close()
            assert _same(rec, hrec) and np.array_equal(status, hstatus)
            assert _same_lists(index, hindex)
            for q in range(130):  # the twin's sink heading is its own goal's
                assert np.array_equal(paths[q][:, :3], hpaths[q][:, :3]), (b, q)
                assert np.array_equal(paths[q][:-1, 3], hpaths[q][:-1, 3]), (b, q)
                assert _same(paths[q], full[q][index[q]]), (b, q)
                if status[q] == 1:
                    assert paths[q][-1, 3] == targets[b][3]
            assert (status == 1).sum() > 100
        with pytest.raises(dymu.DymuError):
            p.getSimplifiedPathsTo(2, starts, 0.25)
        with pytest.raises(dymu.DymuError):
            p.getSimplifiedPathsTo(0, starts, 0.0)
    finally:
        p.close()
