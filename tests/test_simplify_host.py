"""getSimplifiedPaths without a device: the planner's host route (descendArriving with the
rule of csrc/path_simplify.h) must be tests/simplify_ref.py applied to tests/arrive_ref.py
byte for byte, return exact copies of getArrivingPaths' waypoints, and keep the rule's
guarantee.  No engine is ever created: the maps are the oracle's FMM maps installed by
loadTotalCostMap.  A case is built once and shared by its tests."""
import ctypes

import numpy as np
import pytest

import arrive_ref as aref
import goalset_ref
import simplify_ref as sref

RD = 0.5  # risk_distance: tau = min(0.4, RD) = 0.4
TAU = 0.4
RES = 1.0
HEADING = 1.25
CASES = {"96x96": (96, 96, (70, 60)), "97x61": (97, 61, (70, 40))}
EPS = (0.05, 0.25, 1.0)  # in multiples of res


class Case:
    pass


def _planner(dymu, oracle, nx, ny, goal, obst, res=RES, off=(0.0, 0.0)):
    F = oracle.synth_speed(nx, ny, seed=21, obst_frac=obst, goal=goal)
    p = dymu.Planner(risk_distance=RD)
    assert p.initGlobalLayer(res, 0.5, nx, ny, offset=off)
    assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
    assert p.setGoal((off[0] + res * goal[0], off[1] + res * goal[1], 0.0, HEADING))
    T, _ = oracle.fmm(F, goal)
    T = T * res  # the arrival time on a grid of this spacing
    assert p.loadTotalCostMap(T)
    return p, T


def _walked(slots, status):
    return len(slots) - (1 if status == 1 else 0)


def _compare(got, starts, local, refs, full, eps, sink, elev, res, off):
    """(paths, status, records, indices) of getSimplifiedPaths against the Python rule on
    the Python descent and against getArrivingPaths' paths `full`; returns (walked, kept)
    summed over the paths, sinks excluded."""
    paths, status, rec, index = got
    walked = kept = 0
    for q in range(len(starts)):
        r, slots = refs[q]
        assert aref.same_record(rec[q], r) is None, (q, aref.same_record(rec[q], r))
        assert status[q] == r["status"]
        want_idx = sref.simplify_slots(slots, r["status"], eps)
        assert index[q].dtype == np.uint32 and index[q].tobytes() == want_idx.tobytes(), q
        want = aref.post_pass(slots, r["status"], starts[q], sink, elev, res, off)[want_idx]
        assert paths[q].shape == want.shape, q  # the count
        assert paths[q].tobytes() == want.tobytes(), q  # x, y, z and heading
        assert paths[q].tobytes() == full[q][index[q]].tobytes(), q
        n = _walked(slots, r["status"])
        k = len(want_idx) - (1 if r["status"] == 1 else 0)
        assert sref.check(slots[:n, :2], want_idx[:k], eps) is None, \
            (q, sref.check(slots[:n, :2], want_idx[:k], eps))
        walked += n
        kept += k
    return walked, kept


@pytest.fixture(scope="module", params=[(s, o) for s in sorted(CASES) for o in (0.0, 0.02)],
                ids=lambda p: f"{p[0]}-obst{p[1]}")
def case(request, dymu, oracle):
    shape, obst = request.param
    nx, ny, goal = CASES[shape]
    c = Case()
    c.shape, c.obst, c.nx, c.ny, c.goal = shape, obst, nx, ny, goal
    c.p, c.T = _planner(dymu, oracle, nx, ny, goal, obst)
    rng = np.random.default_rng(7)
    xy = np.stack([rng.uniform(2, nx - 3, 200), rng.uniform(2, ny - 3, 200)], axis=1)
    c.starts = [(x, y, 0.5, 0.01 * k) for k, (x, y) in enumerate(xy)]
    c.local = [(s[0], s[1]) for s in c.starts]
    c.full, c.status, c.rec = c.p.getArrivingPaths(c.starts)
    c.stats = c.p.getArrivingStats(c.starts, host=True)
    c.ref = [aref.descend(c.T, RES, TAU, s, goal=goal) for s in c.local]
    c.got = {e: c.p.getSimplifiedPaths(c.starts, e * RES) for e in EPS}
    assert not c.p.lastPathsOnDevice() and c.p.lastPathsKernelMs() == 0
    assert c.p.lastSimplifiedReruns() == 0 and c.p.lastSimplifiedBytes() == 0
    yield c
    c.p.close()


@pytest.mark.parametrize("eps", EPS)
def test_equals_the_reference_rule_exactly(case, eps):
    paths, status, rec, index = case.got[eps]
    assert rec.dtype == case.stats.dtype and rec.shape == (200,)
    assert rec.tobytes() == case.stats.tobytes() == case.rec.tobytes()
    assert np.array_equal(status, case.status)
    elev = np.zeros((case.ny, case.nx))  # setCostMap leaves the elevation zero
    sink = (float(case.goal[0]), float(case.goal[1]), 0.0, HEADING)
    walked, kept = _compare(case.got[eps], case.starts, case.local, case.ref, case.full,
                            eps * RES, sink, elev, RES, (0.0, 0.0))
    assert (status == 1).sum() >= 190
    if case.obst:
        assert (status == -1).sum() >= 1  # the starts on obstacle nodes are there, and empty
        assert all(len(paths[q]) == 0 and len(index[q]) == 0 for q in np.flatnonzero(status == -1))
    print(f"{case.shape} obst {case.obst} eps {eps}: walked {walked}, kept {kept}, "
          f"ratio {walked / kept:.2f}")
    if eps == 0.25:
        assert 3 * kept <= walked


def test_sinks_and_ends(case):
    paths, status, rec, index = case.got[0.25]
    for q in np.flatnonzero(status == 1):
        assert tuple(paths[q][-1]) == (float(case.goal[0]), float(case.goal[1]), 0.0, HEADING)
        assert index[q][0] == 0 and index[q][-1] == rec["count"][q] - 1
        assert index[q][-2] == rec["count"][q] - 2  # the last walked waypoint is kept
        assert tuple(paths[q][0, :2]) == tuple(case.starts[q][:2])


def test_eps_orders_the_thinning(case):
    n = {e: sum(len(i) for i in case.got[e][3]) for e in EPS}
    assert n[1.0] < n[0.25] < n[0.05] < sum(len(f) for f in case.full)


def test_walk_limit_is_status_minus_3(case):
    q = int(np.argmax(case.rec["count"]))
    full, rfull = case.full[q], case.rec[q]
    assert rfull["status"] == 1 and len(full) == rfull["count"] > 40
    for m in (1, 2, 9, len(full) - 1):
        (cut,), (st,), (r,), (idx,) = case.p.getSimplifiedPaths([case.starts[q]], 0.25, max_wp=m)
        want, slots = aref.descend(case.T, RES, TAU, case.local[q], goal=case.goal, max_wp=m)
        assert st == -3 and aref.same_record(r, want) is None and r["count"] == m
        assert idx.tobytes() == sref.simplify_slots(slots, -3, 0.25).tobytes()
        assert idx[0] == 0 and idx[-1] == m - 1  # the last waypoint walked is kept
        assert cut.tobytes() == full[idx].tobytes()
        (s,) = case.p.getArrivingStats([case.starts[q]], max_wp=m, host=True)
        assert s == r
    (exact,), (st,), (r,), (idx,) = case.p.getSimplifiedPaths([case.starts[q]], 0.25,
                                                              max_wp=len(full))
    assert st == 1 and r == rfull
    assert exact.tobytes() == case.got[0.25][0][q].tobytes()


def test_bad_arguments_raise(case, dymu):
    one = [case.starts[0]]
    for eps in (0.0, -0.25, float("nan"), float("inf")):
        with pytest.raises(dymu.DymuError):
            case.p.getSimplifiedPaths(one, eps)
    with pytest.raises(dymu.DymuError):
        case.p.getSimplifiedPaths(one, 0.25, max_wp=0)
    with pytest.raises(dymu.DymuError):
        case.p.getSimplifiedPathsTo(0, one, 0.25)  # no batch without an engine
    paths, status, rec, index = case.p.getSimplifiedPaths([], 0.25)
    assert paths == [] and status.shape == (0,) and rec.shape == (0,) and index == []


def test_rejected_starts_are_empty(case):
    nx, ny = case.nx, case.ny
    bad = [(-0.2, 5.0), (5.0, -1.5), (float("nan"), 5.0), (nx - 0.5, 5.0), (1e300, 5.0)]
    good = case.starts[3]
    paths, status, rec, index = case.p.getSimplifiedPaths([good] + bad + [good], 0.25)
    assert paths[0].tobytes() == case.got[0.25][0][3].tobytes() == paths[-1].tobytes()
    assert (status[1:-1] == -1).all()
    assert all(len(q) == 0 for q in paths[1:-1]) and all(len(i) == 0 for i in index[1:-1])
    for r in rec[1:-1]:
        assert aref.same_record(r, aref.empty_record()) is None
    assert (case.p.lastPathSinks()[1:-1] == -1).all()


def test_current_path_is_not_touched(case):
    assert len(case.p.getPath(case.starts[5])) > 3
    marker = case.p.current_path
    case.p.getSimplifiedPaths(case.starts[:10], 0.25)
    assert np.array_equal(case.p.current_path, marker)


def test_flat_abi_two_call_form(case, dymu):
    pl, h = dymu.load_planner(), case.p.h
    paths, status, rec, index = case.got[0.25]
    n = 50
    s = np.ascontiguousarray(case.starts[:n], dtype=np.float64)
    cnt, st = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    r = np.zeros(n, dtype=dymu.ARRIVE_STAT_DTYPE)
    fn = pl.dymu_planner_get_simplified_paths
    assert fn(h, s.ctypes.data, n, 0.25, 1 << 20, None, None, cnt.ctypes.data, st.ctypes.data,
              r.ctypes.data) == n
    assert np.array_equal(cnt, [len(q) for q in paths[:n]]) and np.array_equal(st, status[:n])
    assert r.tobytes() == rec[:n].tobytes()
    total = int(cnt.sum())
    out, idx = np.zeros((total, 4)), np.zeros(total, dtype=np.uint32)
    assert fn(h, None, n + 1, 0.0, 0, out.ctypes.data, idx.ctypes.data, None, None, None) == -1
    assert fn(h, None, n, 0.0, 0, out.ctypes.data, idx.ctypes.data, None, None, None) == n
    assert out.tobytes() == np.vstack(paths[:n]).tobytes()
    assert idx.tobytes() == np.concatenate(index[:n]).tobytes()
    # the held result is released: a second copy has nothing to copy
    assert fn(h, None, n, 0.0, 0, out.ctypes.data, idx.ctypes.data, None, None, None) == -1
    # one call that does both, without the optional outputs
    out2 = np.zeros((total, 4))
    assert fn(h, s.ctypes.data, n, 0.25, 1 << 20, out2.ctypes.data, None, None, None, None) == n
    assert out2.tobytes() == out.tobytes()
    for eps, max_wp in ((0.0, 16), (-1.0, 16), (float("nan"), 16), (float("inf"), 16), (0.25, 0)):
        assert fn(h, s.ctypes.data, n, eps, max_wp, None, None, cnt.ctypes.data, None, None) == -1
    assert fn(None, s.ctypes.data, n, 0.25, 16, None, None, None, None, None) == -1
    rr, bb = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert pl.dymu_planner_last_simplified(h, ctypes.byref(rr), ctypes.byref(bb)) == 0
    assert rr.value == 0 and bb.value == 0


def test_offset_and_res_not_one(dymu, oracle):
    nx, ny, goal, res, off = 97, 61, (70, 40), 0.5, (100.0, 200.0)
    p, T = _planner(dymu, oracle, nx, ny, goal, 0.02, res=res, off=off)
    try:
        rng = np.random.default_rng(9)
        xy = np.stack([rng.uniform(2, nx - 3, 60), rng.uniform(2, ny - 3, 60)], axis=1) * res
        starts = [(off[0] + x, off[1] + y, 0.5, 0.01 * k) for k, (x, y) in enumerate(xy)]
        local = [(s[0] - off[0], s[1] - off[1]) for s in starts]
        full, _, _ = p.getArrivingPaths(starts)
        refs = [aref.descend(T, res, TAU, s, goal=goal) for s in local]
        sink = (off[0] + res * goal[0], off[1] + res * goal[1], 0.0, HEADING)
        for e in EPS:
            got = p.getSimplifiedPaths(starts, e * res)
            walked, kept = _compare(got, starts, local, refs, full, e * res, sink,
                                    np.zeros((ny, nx)), res, off)
            assert kept < walked
        # eps is in map units, not cells: 0.25 is half a cell here and keeps fewer waypoints
        # than a quarter of a cell
        assert sum(map(len, p.getSimplifiedPaths(starts, 0.25 * res)[3])) > \
            sum(map(len, p.getSimplifiedPaths(starts, 0.25)[3]))
    finally:
        p.close()


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
        full, _, _ = p.getArrivingPaths(starts)
        paths, status, rec, index = p.getSimplifiedPaths(starts, 0.25)
        for s, f, q, st, r, i in zip(starts, full, paths, status, rec, index):
            want, slots = aref.descend(T, RES, TAU, s, goal=goal)
            assert st == 0 == want["status"] and r["sink"] == -1
            assert aref.same_record(r, want) is None
            assert i.tobytes() == sref.simplify_slots(slots, 0, 0.25).tobytes()
            assert q.tobytes() == f[i].tobytes() and i[-1] == r["count"] - 1
        assert len(paths[2]) == 1 and list(index[2]) == [0]  # a single waypoint
    finally:
        p.close()


def test_no_goal(dymu):
    p = dymu.Planner(risk_distance=RD)
    try:
        assert p.initGlobalLayer(RES, 0.5, 16, 16)
        assert p.setCostMap(np.ones((16, 16)))
        paths, status, rec, index = p.getSimplifiedPaths([(5.0, 5.0), (6.0, 7.0)], 0.25)
        assert (status == -1).all() and all(len(q) == 0 for q in paths)
        assert all(len(i) == 0 for i in index)
    finally:
        p.close()


def test_goal_set(dymu, oracle):
    g = goalset_ref
    p, F, seeds, goals, starts = g.planner_case(dymu, oracle)
    try:
        assert p.setGoals(goals, g.OFFSETS)
        T = g.fmm_seeds(oracle, F, seeds)
        assert p.loadTotalCostMap(T)
        labels = g.labels_from_T(T, seeds)
        full, fstatus, frec = p.getArrivingPaths(starts)
        fsinks = p.lastPathSinks()
        paths, status, rec, index = p.getSimplifiedPaths(starts, 0.25)
        assert not p.lastPathsOnDevice()
        assert rec.tobytes() == frec.tobytes() and np.array_equal(status, fstatus)
        assert np.array_equal(p.lastPathSinks(), fsinks)
        assert set(fsinks[status == 1]) == {0, 1, 2}
        for q, s in enumerate(starts):
            loc = (s[0] - g.OFF[0], s[1] - g.OFF[1])
            want, slots = aref.descend(T, RES, min(0.4, g.RD), loc, labels=labels,
                                       goals_ij=g.GOALS_IJ)
            assert aref.same_record(rec[q], want) is None
            assert index[q].tobytes() == sref.simplify_slots(slots, want["status"], 0.25).tobytes()
            assert paths[q].tobytes() == full[q][index[q]].tobytes()
            if status[q] == 1:
                gi, gj = g.GOALS_IJ[fsinks[q]]
                assert tuple(paths[q][-1]) == (g.OFF[0] + gi, g.OFF[1] + gj, 0.0,
                                               g.HEADINGS[fsinks[q]])
    finally:
        p.close()


def test_symbols(dymu):
    fim, pl = dymu.load_fim(), dymu.load_planner()
    for n in ("dymu_arrive_simplified_device", "dymu_last_arrive_simplified_ms"):
        assert hasattr(fim, n) and n in dymu.FIM_SYMBOLS, n
    for n in ("dymu_planner_get_simplified_paths", "dymu_planner_get_simplified_paths_to",
              "dymu_planner_last_simplified"):
        assert hasattr(pl, n) and n in dymu.PLANNER_SYMBOLS, n
    assert fim.dymu_arrive_simplified_device(None, None, 8, 8, 8, 1.0, 1, 1, None, None, 0, 0.4,
                                             None, 0, 0.25, 4, 4, None, None, None, None,
                                             None) == -1
