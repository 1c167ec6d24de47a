"""Goal sets without a device: the reference helpers pinned to the
oracle, and the planner's host routes -- setGoals, the host label routine, getPath /
getPaths with per-path sinks -- on a map installed by loadTotalCostMap (no engine is
ever created)."""
import numpy as np
import pytest

import goalset_ref as ref


def test_helper_fmm_is_the_oracle_for_one_seed(oracle):
    F = oracle.synth_speed(96, 96, seed=21, obst_frac=0.02, goal=(70, 60))
    T_ref, _ = oracle.fmm(F, (70, 60))
    T = ref.fmm_seeds(oracle, F, [(70, 60, 0.0)])
    assert np.array_equal(T.view(np.uint64), T_ref.view(np.uint64))
    lab = ref.labels_from_T(T, [(70, 60, 0.0)])
    assert np.array_equal(lab == ref.NONE, np.isinf(T))
    assert (lab[np.isfinite(T)] == 0).all()


class Case:
    pass


@pytest.fixture(scope="module")
def case(dymu, oracle):
    c = Case()
    c.p, c.F, c.seeds, c.goals, c.starts = ref.planner_case(dymu, oracle)
    assert c.p.setGoals(c.goals, ref.OFFSETS)
    c.T = ref.fmm_seeds(oracle, c.F, c.seeds)
    assert c.p.loadTotalCostMap(c.T)
    c.labels = ref.labels_from_T(c.T, c.seeds)
    yield c
    c.p.close()


def test_set_goals_state(case):
    p = case.p
    assert p.goalCount() == 3
    g0 = p.getGlobalNode(*ref.GOALS_IJ[0])
    assert g0 is not None


def test_host_labels_equal_the_definition(case):
    lab = case.p.goalLabels()
    assert lab.dtype == np.uint32 and lab.shape == (ref.NY, ref.NX)
    assert np.array_equal(lab, case.labels)
    assert set(np.unique(lab)) == {0, 1, 2, ref.NONE}  # every goal owns a region
    assert np.array_equal(lab == ref.NONE, np.isinf(case.T))
    for (i, j), k in zip(ref.GOALS_IJ, range(3)):
        assert case.p.goalLabel((ref.OFF[0] + i + 0.2, ref.OFF[1] + j - 0.3)) == k
    oi, oj = np.argwhere(np.isinf(case.T))[0][::-1]
    assert case.p.goalLabel((ref.OFF[0] + oi, ref.OFF[1] + oj)) == -1
    assert case.p.goalLabel((ref.OFF[0] - 50.0, ref.OFF[1] + 3.0)) == -1


def test_paths_end_on_their_goal(case):
    p = case.p
    paths, status = p.getPaths(case.starts)
    sinks = p.lastPathSinks()
    assert not p.lastPathsOnDevice()
    assert len(paths) == 200 and sinks.shape == (200,)
    bad = int((status != 1).sum())
    print(f"starts not ending at a sink: {bad}/200")
    assert bad <= 10  # 5 %, the cap of the single-goal tests
    assert set(sinks[status == 1]) == {0, 1, 2}
    for s, q, st, k in zip(case.starts, paths, status, sinks):
        looped = p.getPath(s)
        assert q.shape == looped.shape and np.array_equal(q, looped, equal_nan=True), (s, st)
        assert (st == 1) == (k >= 0)
        if st == 1:
            gi, gj = ref.GOALS_IJ[k]
            assert tuple(q[-1]) == (ref.OFF[0] + gi, ref.OFF[1] + gj, 0.0, ref.HEADINGS[k])
    # a start's own label is usually its sink (not always: the sink follows the cells)
    own = [case.labels[int(s[1] - ref.OFF[1]), int(s[0] - ref.OFF[0])] for s in case.starts]
    agree = sum(1 for o, k, st in zip(own, sinks, status) if st == 1 and o == k)
    assert agree >= 0.9 * (status == 1).sum()


def test_set_goals_rejects_and_keeps_the_previous(dymu, oracle):
    p, F, seeds, goals, starts = ref.planner_case(dymu, oracle)
    try:
        assert p.setGoal(goals[1])
        assert p.goalCount() == 1
        oj, oi = np.argwhere(np.isinf(F))[0]
        border = (ref.OFF[0] + 0.0, ref.OFF[1] + 20.0, 0.0, 0.0)
        obstacle = (ref.OFF[0] + oi, ref.OFF[1] + oj, 0.0, 0.0)
        assert not p.setGoals([goals[0], border])
        assert not p.setGoals([goals[0], obstacle])
        assert not p.setGoals(goals, [0.0, -1.0, 0.0])
        assert not p.setGoals(goals, [0.0, float("nan"), 0.0])
        assert not p.setGoals(goals, [0.0, float("inf"), 0.0])
        assert not p.setGoals(goals, [0.0, 1.0])
        assert not p.setGoals([])
        assert p.goalCount() == 1
        g = p.getGlobalNode(*ref.GOALS_IJ[1])
        T1, _ = oracle.fmm(F, ref.GOALS_IJ[1])
        assert p.loadTotalCostMap(T1)
        path = p.getPath(starts[0])
        assert tuple(path[-1][:2]) == (ref.OFF[0] + ref.GOALS_IJ[1][0], ref.OFF[1] + ref.GOALS_IJ[1][1])
        assert path[-1][3] == ref.HEADINGS[1] and g is not None
    finally:
        p.close()


def test_set_goal_after_set_goals_is_single_goal(dymu, oracle):
    p, F, seeds, goals, starts = ref.planner_case(dymu, oracle)
    q = dymu.Planner(risk_distance=ref.RD)
    try:
        assert p.setGoals(goals, ref.OFFSETS) and p.goalCount() == 3
        assert p.setGoal(goals[2]) and p.goalCount() == 1
        assert q.initGlobalLayer(1.0, 0.5, ref.NX, ref.NY, offset=ref.OFF)
        assert q.setCostMap(np.where(np.isfinite(F), F, -1.0))
        assert q.setGoal(goals[2])
        T2, _ = oracle.fmm(F, ref.GOALS_IJ[2])
        assert p.loadTotalCostMap(T2) and q.loadTotalCostMap(T2)
        a, sa = p.getPaths(starts[:40])
        b, sb = q.getPaths(starts[:40])
        assert np.array_equal(sa, sb)
        assert all(x.shape == y.shape and np.array_equal(x, y, equal_nan=True)
                   for x, y in zip(a, b))
        assert set(p.lastPathSinks()[sa == 1]) == {0}
        lab = p.goalLabels()  # one goal: 0 wherever the map is finite
        assert np.array_equal(lab == 0, np.isfinite(T2))
    finally:
        p.close()
        q.close()


def test_goal_set_state_is_a_converged_full_solve(case):
    p = case.p
    st = p.nodeStates()
    assert np.array_equal(st.astype(bool), np.isfinite(case.T))  # every finite node CLOSED
    assert len(p.globalNarrowband()) == 0
    order = p.globalPropagatedNodes()
    t = case.T.ravel()
    fin = np.flatnonzero(np.isfinite(t))
    want = fin[np.lexsort((fin, t[fin]))]  # by (total cost, grid index)
    got = order[:, 1].astype(np.int64) * ref.NX + order[:, 0]
    assert np.array_equal(got, want)
    # resetGlobalNarrowBand: every root goal in the band, at its offset
    p.resetGlobalNarrowBand()
    band = {(int(i), int(j)) for i, j in p.globalNarrowband()}
    assert band == set(ref.GOALS_IJ)
    assert p.totalCostRaw()[ref.GOALS_IJ[1][1], ref.GOALS_IJ[1][0]] == ref.OFFSETS[1]


def test_local_repair_declines_a_goal_set(dymu, oracle):
    """computeLocalPlanning / repairPath toward more than one goal are out of scope: they
    return false / -1 and leave the path and the hazard map alone."""
    p, F, seeds, goals, starts = ref.planner_case(dymu, oracle)
    try:
        assert p.setGoals(goals, ref.OFFSETS)
        assert p.loadTotalCostMap(ref.fmm_seeds(oracle, F, seeds))
        path = p.getPath(starts[0])
        assert len(path) > 3
        cur, hz = p.current_path, p.getHazardDensityMatrix()
        img = np.zeros((40, 40), dtype=np.uint8)
        img[18:22, 18:22] = 1
        ok, traj, _ = p.computeLocalPlanning(tuple(path[1]), img, 0.1)
        assert not ok and len(traj) == 0
        assert p.repairPath(tuple(path[1]), 1) == -1
        assert np.array_equal(p.current_path, cur)
        assert np.array_equal(p.getHazardDensityMatrix(), hz)
        assert p.setGoals(goals[:1])  # one goal in a set: the local layer is available
        assert p.goalCount() == 1
    finally:
        p.close()
