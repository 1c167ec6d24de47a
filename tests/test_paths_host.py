"""getPaths without a device: the host route (DyMuPathPlanner::getPaths' fallback) must
give exactly what a loop of getPath gives, and the wrap-free range check of
computeNextGlobalWaypoint must reject starts just below the grid."""
import numpy as np
import pytest

OFF = (100.0, 200.0)


def _terrain_planner(dymu, oracle, N=64, goal=(40, 36)):
    """A planner with a non-trivial elevation (so z is checked) and the oracle's FMM map
    installed by loadTotalCostMap: no engine is ever created."""
    j, i = np.mgrid[0:N, 0:N].astype(float)
    elev = 0.3 * np.sin(0.3 * i) + 0.1 * np.cos(0.2 * j)
    terr = 1.0 + (i > N // 2)
    lut = np.array([50.0] * 6 + [1, 2, 4, 2, 2.5, 3] + [3, 3, 3, 1, 5, 9], dtype=float)
    slopes = np.array([0.0, 10.0, 20.0])
    p = dymu.Planner(risk_distance=0.5)
    assert p.initGlobalLayer(1.0, 0.5, N, N, offset=OFF)
    assert p.computeCostMap(lut, slopes, ["Wheel", "Walk"], elev, terr)
    assert p.setGoal((OFF[0] + goal[0], OFF[1] + goal[1], 0.0, 1.25))
    G = p.getGlobalCostMatrix()
    F = np.where(G < 0, np.inf, G)
    T, _ = oracle.fmm(F, goal)
    assert p.loadTotalCostMap(T)
    return p, N


def test_fallback_equals_looped_get_path(dymu, oracle):
    p, N = _terrain_planner(dymu, oracle)
    try:
        rng = np.random.default_rng(7)
        xy = rng.uniform(2, N - 3, size=(200, 2))
        starts = [(OFF[0] + x, OFF[1] + y, 0.5, 0.1 * k) for k, (x, y) in enumerate(xy)]
        # a path left in current_path must survive the batched call
        assert len(p.getPath(starts[3])) > 3
        marker = p.current_path  # grid-local (getPath adds the offset to its copy)
        paths, status = p.getPaths(starts)
        assert not p.lastPathsOnDevice()
        assert np.array_equal(p.current_path, marker)
        assert len(paths) == 200 and status.shape == (200,)
        assert (status == 1).sum() > 150
        assert max(len(q) for q in paths) > 20
        assert any(np.abs(q[:, 2]).max() > 0.05 for q in paths if len(q))  # z is exercised
        for s, q, st in zip(starts, paths, status):
            ref = p.getPath(s)
            assert q.shape == ref.shape, (s, st)
            assert np.array_equal(q, ref, equal_nan=True), (s, st)
            assert st in (1, 0, -1)
            assert (st == -1) == (len(ref) == 0)
    finally:
        p.close()


def test_fallback_max_wp_and_stride(dymu, oracle):
    p, N = _terrain_planner(dymu, oracle)
    try:
        s = (OFF[0] + 5.3, OFF[1] + 7.8, 0.0, 0.2)
        full = p.getPath(s)
        assert len(full) > 40
        (cut,), (st,) = p.getPaths([s], max_wp=8)
        assert st == -3 and np.array_equal(cut, full[:8])
        (exact,), (st,) = p.getPaths([s], max_wp=len(full))
        assert st == 1 and np.array_equal(exact, full)
        (thin,), (st,) = p.getPaths([s], stride=4)
        assert st == 1 and np.array_equal(thin, np.vstack([full[:-1][::4], full[-1:]]))
        with pytest.raises(dymu.DymuError):
            p.getPaths([s], max_wp=0)
    finally:
        p.close()


@pytest.mark.parametrize("axis", [0, 1])
def test_wrap_free_range_check(dymu, oracle, axis):
    """x / res in (-2, -1] truncates to -1: as an unsigned cell its + 1 wrapped to 0 and
    passed the range check; such a start is off the grid like any other."""
    p, N = _terrain_planner(dymu, oracle)
    try:
        s = [OFF[0] + 10.25, OFF[1] + 12.5, 0.0, 0.0]
        s[axis] = OFF[axis] - 1.5 * 1.0
        paths, status = p.getPaths([tuple(s)])
        assert len(paths[0]) == 0 and status[0] == -1
        assert len(p.getPath(tuple(s))) == 0
        # and the other rejected inputs, next to a good start that is unaffected
        good = (OFF[0] + 10.25, OFF[1] + 12.5, 0.0, 0.0)
        ref = p.getPath(good)
        bad = [(OFF[0] + N - 1 + 0.5, OFF[1] + 5.0), (OFF[0] + 5.0, OFF[1] + N + 40.0),
               (OFF[0] - 30.0, OFF[1] + 5.0), (float("nan"), OFF[1] + 5.0),
               (OFF[0] + 2.0 ** 32 + 5.5, OFF[1] + 5.0), (OFF[0] + 1e300, OFF[1] + 5.0)]
        paths, status = p.getPaths([good] + bad + [good])
        assert np.array_equal(paths[0], ref) and np.array_equal(paths[-1], ref)
        assert status[0] == 1 and status[-1] == 1
        assert all(len(q) == 0 for q in paths[1:-1]) and (status[1:-1] == -1).all()
    finally:
        p.close()
