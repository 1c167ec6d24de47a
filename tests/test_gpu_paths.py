"""getPaths on the device (k_extract_paths, csrc/path_kernels.hip): bit-identical to the
host descent on the same map, within the project's path tolerance of the oracle, and
safe on starts it must reject.  The maps, starts and looped-getPath references of a
case are computed once and shared by its tests."""
import math
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OFF = (100.0, 200.0)
RD = 0.5  # risk_distance: tau = min(0.4, RD) = 0.4
HEADING = 1.25
CASES = {"96x96": (96, 96, (70, 60)), "97x61": (97, 61, (70, 40))}


class Case:
    pass


@pytest.fixture(scope="module", params=[(s, o) for s in sorted(CASES) for o in (0.0, 0.02)],
                ids=lambda p: f"{p[0]}-obst{p[1]}")
def case(request, dymu, oracle):
    shape, obst = request.param
    nx, ny, goal = CASES[shape]
    c = Case()
    c.nx, c.ny, c.goal = nx, ny, goal
    c.F = oracle.synth_speed(nx, ny, seed=21, obst_frac=obst, goal=goal)
    p = dymu.Planner(risk_distance=RD)
    assert p.initGlobalLayer(1.0, 0.5, nx, ny, offset=OFF)
    assert p.setCostMap(np.where(np.isfinite(c.F), c.F, -1.0))
    assert p.setGoal((OFF[0] + goal[0], OFF[1] + goal[1], 0.0, HEADING))
    assert p.computeEntireTotalCostMap()
    rng = np.random.default_rng(7)
    c.xy = np.stack([rng.uniform(2, nx - 3, 200), rng.uniform(2, ny - 3, 200)], axis=1)
    c.starts = [(OFF[0] + x, OFF[1] + y, 0.0, 0.01 * k) for k, (x, y) in enumerate(c.xy)]
    c.paths, c.status = p.getPaths(c.starts)
    c.on_device = p.lastPathsOnDevice()
    c.kernel_ms = p.lastPathsKernelMs()
    c.host = [p.getPath(s) for s in c.starts]  # through the host mirror of the same map
    c.p = p
    yield c
    p.close()


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_device_equals_host_exactly(case):
    assert case.on_device and case.kernel_ms > 0
    assert len(case.paths) == 200
    for q, (d, h) in enumerate(zip(case.paths, case.host)):
        assert d.shape == h.shape, (q, case.status[q], d.shape, h.shape)
        assert np.array_equal(d, h, equal_nan=True), (q, case.status[q])
    assert np.median([len(h) for h in case.host]) > 30


def test_device_against_oracle(case, oracle):
    T = case.p.totalCostRaw()
    worst = 0.0
    for q, (x, y) in enumerate(case.xy):
        n, wp = oracle.global_path(T, case.goal, res=1.0, start=(x, y, 0.01 * q),
                                   risk_distance=RD, goal_heading=HEADING)
        d, st = case.paths[q], case.status[q]
        assert (n == -1) == (st == -1), (q, n, st)
        assert (n == -2) == (st == 0), (q, n, st)
        if n < 0:
            continue
        assert st == 1 and n == len(d), (q, n, len(d))
        wp[:, 0] += OFF[0]
        wp[:, 1] += OFF[1]
        worst = max(worst, np.abs(d[:, :2] - wp[:, :2]).max(), np.abs(d[:, 3] - wp[:, 3]).max())
    print(f"max |device - oracle| over x, y, heading: {worst:.3e}")
    assert worst < 1e-9


def test_outcome_cap(case):
    bad = int((case.status != 1).sum())
    print(f"starts not ending at the sink: {bad}/200")
    assert bad <= 10  # 5 %


@pytest.mark.parametrize("m", [1, 65, 130])
def test_batch_sizes(case, m):
    paths, status = case.p.getPaths(case.starts[:m])
    assert case.p.lastPathsOnDevice()
    assert len(paths) == m and np.array_equal(status, case.status[:m])
    assert all(_same(a, b) for a, b in zip(paths, case.paths))


def test_second_call_is_bit_equal(case):
    paths, status = case.p.getPaths(case.starts)
    assert np.array_equal(status, case.status)
    assert all(_same(a, b) for a, b in zip(paths, case.paths))


def test_engine_call_with_padded_rows(case, engine):
    """dymu_extract_paths_device on a map with leading dimension nx + 5."""
    nx, ny = case.nx, case.ny
    ld = nx + 5
    T = case.p.totalCostRaw()
    Tp = np.full((ny, ld), -7.0)  # the padding is never a valid total cost
    Tp[:, :nx] = T
    dT = engine.alloc(Tp.nbytes)
    try:
        engine.h2d(dT, Tp)
        m = 65
        # grid-local starts as getPath forms them: the offset added, then removed
        xy = np.array([(s[0] - OFF[0], s[1] - OFF[1]) for s in case.starts[:m]])
        out, cnt, st = engine.extract_paths(dT, nx, ny, ld, 1.0, case.goal[0], case.goal[1], 0.4,
                                            xy, max_wp=1024)
        assert engine.last_paths_ms() > 0
    finally:
        engine.free(dT)
    assert np.array_equal(st, case.status[:m])
    for q in range(m):
        h = case.host[q]
        assert cnt[q] == len(h), q
        assert np.array_equal(out[q, :cnt[q], 0] + OFF[0], h[:, 0], equal_nan=True)
        assert np.array_equal(out[q, :cnt[q], 1] + OFF[1], h[:, 1], equal_nan=True)
        if len(h) > 1:  # the heading comes from the stored direction
            for k in range(1, len(h) - 1 if st[q] == 1 else len(h)):  # libm's atan2, as the host's
                assert math.atan2(-out[q, k, 3], -out[q, k, 2]) == h[k, 3], (q, k)


def test_engine_argument_errors(case, engine, dymu):
    with pytest.raises(dymu.DymuError) as e:
        engine.extract_paths(0, 8, 8, 8, 1.0, 1, 1, 0.4, np.zeros((1, 2)), max_wp=4)
    assert e.value.status == -1
    dT = engine.alloc(8 * 64)
    try:
        for kw in (dict(ld=7), dict(goal_i=8), dict(res=0.0), dict(tau=float("nan")),
                   dict(max_wp=0), dict(stride=0)):
            a = dict(dT=dT, nx=8, ny=8, ld=8, res=1.0, goal_i=1, goal_j=1, tau=0.4,
                     starts_xy=np.zeros((1, 2)), max_wp=4, stride=1)
            a.update(kw)
            with pytest.raises(dymu.DymuError) as e:
                engine.extract_paths(**a)
            assert e.value.status == -1, kw
    finally:
        engine.free(dT)


def test_start_next_to_the_goal(case):
    s = (OFF[0] + case.goal[0] + 0.5, OFF[1] + case.goal[1] + 0.7, 0.0, 0.3)
    (d,), (st,) = case.p.getPaths([s])
    assert st == 1 and len(d) == 2
    assert tuple(d[0, [0, 1, 3]]) == (s[0], s[1], 0.3)
    assert tuple(d[1, [0, 1, 3]]) == (OFF[0] + case.goal[0], OFF[1] + case.goal[1], HEADING)
    assert _same(d, case.p.getPath(s))


def _long_path(case):
    q = int(np.argmax([len(h) if s == 1 else 0 for h, s in zip(case.host, case.status)]))
    assert len(case.host[q]) > 40
    return case.starts[q], case.host[q]


def test_max_wp_cuts_the_path(case):
    s, full = _long_path(case)
    (d,), (st,) = case.p.getPaths([s], max_wp=8)
    assert st == -3 and _same(d, full[:8])
    (d,), (st,) = case.p.getPaths([s], max_wp=len(full))
    assert st == 1 and _same(d, full)
    (d,), (st,) = case.p.getPaths([s], max_wp=len(full) - 1)
    assert st == -3 and _same(d, full[:-1])


def test_stride_keeps_every_fourth_and_the_sink(case):
    s, full = _long_path(case)
    (d,), (st,) = case.p.getPaths([s], stride=4)
    assert st == 1 and _same(d, np.vstack([full[:-1][::4], full[-1:]]))
    (d,), (st,) = case.p.getPaths([s], max_wp=8, stride=4)
    assert st == -3 and _same(d, full[:-1][::4][:8])


def test_rejected_starts_leave_the_batch_alone(case):
    """Border cell, off the grid, negative, huge and NaN starts end with status -1 and no
    waypoint (the kernel tests the cell in 64-bit before any load); their neighbours in
    the batch are what they are alone."""
    nx, ny = case.nx, case.ny
    bad = [(OFF[0] + nx - 1 + 0.5, OFF[1] + 5.0), (OFF[0] + 5.0, OFF[1] + ny - 1 + 0.25),
           (OFF[0] + nx + 40.0, OFF[1] + 5.0), (OFF[0] + 5.0, OFF[1] + 3.0e9),
           (OFF[0] - 1.5, OFF[1] + 5.0), (OFF[0] + 5.0, OFF[1] - 1.5),
           (OFF[0] - 30.0, OFF[1] - 30.0), (OFF[0] - 4294967296.5, OFF[1] + 5.0),
           (OFF[0] + 4294967296.0 + 5.5, OFF[1] + 5.0), (OFF[0] + 1e300, OFF[1] + 5.0),
           (-1e300, OFF[1] + 5.0), (float("nan"), OFF[1] + 5.0), (OFF[0] + 5.0, float("nan")),
           (float("inf"), float("-inf"))]
    batch = []
    for k, b in enumerate(bad):
        batch += [case.starts[k], b]
    batch.append(case.starts[len(bad)])
    paths, status = case.p.getPaths(batch)
    assert case.p.lastPathsOnDevice()
    for k in range(len(bad)):
        assert _same(paths[2 * k], case.paths[k]) and status[2 * k] == case.status[k]
        assert len(paths[2 * k + 1]) == 0 and status[2 * k + 1] == -1, bad[k]
    assert _same(paths[-1], case.paths[len(bad)])


def test_state_changes(dymu, oracle):
    """After the early exit the device map is the host's (scatters / exact replay upload);
    after propagateGlobalNode only the host copy is current: the host route runs."""
    nx, ny, goal = CASES["96x96"]
    F = oracle.synth_speed(nx, ny, seed=21, obst_frac=0.02, goal=goal)
    p = dymu.Planner(risk_distance=RD)
    try:
        p.initGlobalLayer(1.0, 0.5, nx, ny, offset=OFF)
        p.setCostMap(np.where(np.isfinite(F), F, -1.0))
        assert p.setGoal((OFF[0] + goal[0], OFF[1] + goal[1], 0.0, HEADING))
        # a start whose node has no obstacle in its 3x3 (computeTotalCostMap's isSafeNode)
        ob = ~np.isfinite(F)
        si, sj = next((i, j) for j in range(45, 60) for i in range(38, 50)
                      if not ob[j - 1:j + 2, i - 1:i + 2].any())
        start = (OFF[0] + si + 0.3, OFF[1] + sj - 0.4, 0.0, 0.2)
        assert p.computeTotalCostMap(start)
        (d,), (st,) = p.getPaths([start])
        assert p.lastPathsOnDevice() and st == 1
        ref = p.getPath(start)
        assert len(ref) > 20 and _same(d, ref)
        # a never-reached free node next to a reached one: propagateGlobalNode lowers it
        T = p.totalCostRaw()
        fin = np.isfinite(T)
        nb = np.zeros_like(fin)
        nb[1:] |= fin[:-1]
        nb[:-1] |= fin[1:]
        nb[:, 1:] |= fin[:, :-1]
        nb[:, :-1] |= fin[:, 1:]
        j, i = np.argwhere(~fin & nb & np.isfinite(F))[0]
        p.propagateGlobalNode(int(i), int(j))
        assert np.isfinite(p.totalCostRaw()[j, i])
        (d,), (st,) = p.getPaths([start])
        assert not p.lastPathsOnDevice()
        assert st == 1 and _same(d, p.getPath(start))
        # the next solve makes the device map current again
        assert p.computeEntireTotalCostMap()
        (d,), _ = p.getPaths([start])
        assert p.lastPathsOnDevice() and _same(d, p.getPath(start))
        # loadTotalCostMap with an engine uploads the map
        assert p.loadTotalCostMap(T)
        (d,), _ = p.getPaths([start])
        assert p.lastPathsOnDevice() and _same(d, ref)
        p.resetGlobalNarrowBand()
        p.getPaths([start])
        assert not p.lastPathsOnDevice()
    finally:
        p.close()


def test_elevation_and_heading_post_pass(dymu):
    """z comes from the host's interpolate call on the elevation: a map from
    computeCostMap (non-trivial elevation), device against looped getPath."""
    N = 64
    j, i = np.mgrid[0:N, 0:N].astype(float)
    elev = 0.3 * np.sin(0.3 * i) + 0.1 * np.cos(0.2 * j)
    terr = 1.0 + (i > N // 2)
    lut = np.array([50.0] * 6 + [1, 2, 4, 2, 2.5, 3] + [3, 3, 3, 1, 5, 9], dtype=float)
    p = dymu.Planner(risk_distance=RD)
    try:
        p.initGlobalLayer(1.0, 0.5, N, N, offset=OFF)
        assert p.computeCostMap(lut, np.array([0.0, 10.0, 20.0]), ["Wheel", "Walk"], elev, terr)
        assert p.setGoal((OFF[0] + 40, OFF[1] + 36, 0.0, HEADING))
        assert p.computeEntireTotalCostMap()
        rng = np.random.default_rng(11)
        starts = [(OFF[0] + x, OFF[1] + y, 0.7, 0.1) for x, y in rng.uniform(2, N - 3, (66, 2))]
        paths, status = p.getPaths(starts)
        assert p.lastPathsOnDevice() and (status == 1).sum() > 50
        assert max(np.abs(q[:, 2]).max() for q in paths if len(q)) > 0.05
        for s, d in zip(starts, paths):
            assert _same(d, p.getPath(s))
    finally:
        p.close()


def test_larger_grid(dymu, oracle):
    """1024^2 config-3 terrain (U(1,5), 2 % obstacles), 4096 starts in one call."""
    N = 1024
    g = (N // 2, N // 2)
    F = oracle.synth_speed(N, N, seed=1, obst_frac=0.02, obst_seed=3, goal=g)
    p = dymu.Planner(risk_distance=RD)
    try:
        p.initGlobalLayer(1.0, 0.5, N, N)
        p.setCostMap(np.where(np.isfinite(F), F, -1.0))
        assert p.setGoal((g[0], g[1], 0.0, HEADING))
        assert p.computeEntireTotalCostMap()
        rng = np.random.default_rng(5)
        starts = [(x, y, 0.0, 0.0) for x, y in rng.uniform(2, N - 3, (4096, 2))]
        t0 = time.perf_counter()
        paths, status = p.getPaths(starts)
        ms = (time.perf_counter() - t0) * 1e3
        assert p.lastPathsOnDevice()
        n_wp = sum(len(q) for q in paths)
        print(f"1024^2, 4096 paths, {n_wp} waypoints: {ms:.1f} ms the call, "
              f"{p.lastPathsKernelMs():.2f} ms the kernel; "
              f"{int((status != 1).sum())} not ending at the sink")
        assert (status != 1).sum() <= 0.05 * 4096
        for q in rng.choice(4096, 64, replace=False):
            assert _same(paths[q], p.getPath(starts[q])), q
    finally:
        p.close()
