"""setCostMapWindow on the planner: a box of costs applied by setCostMap's
per-cell rule, followed by the windowed re-propagation and, with setGlobalRisk on, by the
incremental update of R when the box only adds obstacles.

Yardsticks, as in test_gpu_global_risk.py: the oracle FMM of the (effective) speed built in
numpy, within |dT| <= 1e-12 max(1, T) and with the same +inf mask; R within 1e-12 absolute of
what a second planner computes whole from the edited map given through setCostMap.
"""
import numpy as np
import pytest

from test_gpu_global_risk import (INF, RATIO, RD, check_parity, effective, new_planner, risk_ref,
                                  speed, wp)

pytestmark = pytest.mark.gpu

NX, NY = 128, 96
GOAL, GOALS = (90, 60), [(90, 60), (20, 20), (100, 15), (30, 80)]
FREEABLE = (40, 50)  # cost +inf: an obstacle of the mask that a finite cost frees


class Case:
    pass


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def case(oracle):
    """128x96, 2 % obstacles (none next to a goal), one cell of cost +inf, and a 3x3 box in
    clear terrain (R = 0, away from the goals and from every obstacle's reach)."""
    c = Case()
    F = oracle.synth_speed(NX, NY, seed=33, obst_frac=0.02, obst_seed=17, goal=GOAL)
    for gi, gj in GOALS:
        blk = F[gj - 1:gj + 2, gi - 1:gi + 2]
        blk[~np.isfinite(blk)] = 3.0
    c.cost = np.where(np.isfinite(F), F, -1.0)
    c.cost[FREEABLE[1], FREEABLE[0]] = INF
    c.R_ref = risk_ref(oracle, ~(speed(c.cost) < INF))
    clear = c.R_ref == 0
    c.box = next((i, j) for j in range(8, NY - 11) for i in range(8, NX - 11)
                 if clear[j - 4:j + 7, i - 4:i + 7].all()
                 and all(abs(i - g[0]) + abs(j - g[1]) > 16 for g in GOALS))
    i, j = c.box
    c.block = np.full((3, 3), -1.0)
    c.block[1, 1] = 0.0  # both forms of an obstacle cost
    c.cost1 = c.cost.copy()
    c.cost1[j:j + 3, i:i + 3] = c.block
    for a in (c.cost, c.cost1, c.R_ref, c.block):
        a.setflags(write=False)
    return c


def obstacles(cost):
    return ~(speed(cost) < INF)


def test_risk_off(dymu, oracle, case):
    i, j = case.box
    p, q = new_planner(dymu, case.cost, risk=None), new_planner(dymu, case.cost1, risk=None)
    try:
        assert p.setGoal(wp(*GOAL)) and p.computeEntireTotalCostMap()
        assert p.lastSolveKind() == 0
        assert p.setCostMapWindow(i, j, case.block)
        assert p.computeEntireTotalCostMap()
        assert p.lastSolveKind() == 1
        assert p.lastRiskUpdateKind() == 0
        T = p.totalCostRaw()
        check_parity(T, oracle.fmm(speed(case.cost1), GOAL)[0])
        assert q.setGoal(wp(*GOAL)) and q.computeEntireTotalCostMap()
        check_parity(T, q.totalCostRaw())
        assert np.array_equal(bits(p.getGlobalCostMatrix()), bits(q.getGlobalCostMatrix()))
    finally:
        p.close()
        q.close()


def whole_map_risk(dymu, cost):
    q = new_planner(dymu, cost)
    try:
        R = q.getGlobalRiskMatrix()
        assert q.lastRiskUpdateKind() == 1
        return R
    finally:
        q.close()


def check_risk_and_map(p, oracle, dymu, cost):
    """R against the whole-map planner's and the reference; the solved map against the oracle
    on this planner's own effective speed."""
    R = p.getGlobalRiskMatrix()
    err = np.abs(R - whole_map_risk(dymu, cost)).max()
    print(f"max |R - R of the whole-map planner| = {err:.3e}")
    assert err <= 1e-12
    assert np.abs(R - risk_ref(oracle, obstacles(cost))).max() <= 1e-12
    assert p.computeEntireTotalCostMap()
    check_parity(p.totalCostRaw(), oracle.fmm(effective(speed(cost), R), GOAL)[0])
    return R


def test_risk_on_block_added_then_freed(dymu, oracle, case):
    i, j = case.box
    p = new_planner(dymu, case.cost)
    try:
        assert p.lastRiskUpdateKind() == 0
        assert p.setGoal(wp(*GOAL)) and p.computeEntireTotalCostMap()
        assert p.lastRiskUpdateKind() == 1
        R0 = p.getGlobalRiskMatrix()
        assert np.abs(R0 - case.R_ref).max() <= 1e-12
        # obstacles added: the incremental route
        assert p.setCostMapWindow(i, j, case.block)
        R1 = check_risk_and_map(p, oracle, dymu, case.cost1)
        assert p.lastRiskUpdateKind() == 2
        assert (R1[j:j + 3, i:i + 3] == 1.0).all() and R1[j + 1, i + 3] > 0.0
        assert (R0[j - 4:j + 7, i - 4:i + 7] == 0.0).all()
        # finite costs only: R is not touched and no refresh runs
        fi, fj = FREEABLE[0] + 6, FREEABLE[1] - 1
        assert (case.cost1[fj:fj + 2, fi:fi + 2] > 0).all()
        cost2 = case.cost1.copy()
        cost2[fj:fj + 2, fi:fi + 2] = [[1.5, 2.5], [3.5, 4.5]]
        assert p.setCostMapWindow(fi, fj, cost2[fj:fj + 2, fi:fi + 2])
        assert np.array_equal(bits(p.getGlobalRiskMatrix()), bits(R1))
        assert p.computeEntireTotalCostMap() and p.lastSolveKind() == 1
        assert p.lastRiskUpdateKind() == 2
        check_parity(p.totalCostRaw(), oracle.fmm(effective(speed(cost2), R1), GOAL)[0])
        # an obstacle freed (with another one added beside it): the whole recompute
        cost3 = cost2.copy()
        cost3[FREEABLE[1], FREEABLE[0]:FREEABLE[0] + 2] = [2.0, -1.0]
        assert obstacles(cost2)[FREEABLE[1], FREEABLE[0]]
        assert not obstacles(cost3)[FREEABLE[1], FREEABLE[0]]
        assert p.setCostMapWindow(FREEABLE[0], FREEABLE[1],
                                  cost3[FREEABLE[1]:FREEABLE[1] + 1, FREEABLE[0]:FREEABLE[0] + 2])
        R3 = check_risk_and_map(p, oracle, dymu, cost3)
        assert p.lastRiskUpdateKind() == 1
        assert R3[FREEABLE[1], FREEABLE[0]] < 1.0 and R3[FREEABLE[1], FREEABLE[0] + 1] == 1.0
    finally:
        p.close()


def test_two_boxes_before_one_synchronisation(dymu, oracle, case):
    i, j = case.box
    p = new_planner(dymu, case.cost)
    try:
        assert p.setGoal(wp(*GOAL)) and p.computeEntireTotalCostMap()
        cost = case.cost1.copy()
        cost[5:7, 120:123] = -1.0
        assert p.setCostMapWindow(i, j, case.block)
        assert p.setCostMapWindow(120, 5, cost[5:7, 120:123])
        check_risk_and_map(p, oracle, dymu, cost)
        assert p.lastRiskUpdateKind() == 2
    finally:
        p.close()


def test_rejected_boxes_change_nothing(dymu, case):
    p = new_planner(dymu, case.cost)
    try:
        assert p.setGoal(wp(*GOAL)) and p.computeEntireTotalCostMap()
        before = (p.getGlobalCostMatrix(), p.getGlobalRiskMatrix(), p.totalCostRaw())
        blk = np.full((3, 3), -1.0)
        assert p.setCostMapWindow(NX - 2, 10, blk) is False
        assert p.setCostMapWindow(10, NY - 2, blk) is False
        assert p.setCostMapWindow(NX, 0, blk) is False
        assert p._lib.dymu_planner_set_cost_map_window(None, 0, 0, 3, 3, blk) == -1
        assert p._lib.dymu_planner_last_risk_update_kind(None) == -1
        assert p.computeEntireTotalCostMap() and p.lastSolveKind() == 2  # nothing to do
        assert p.lastRiskUpdateKind() == 1
        after = (p.getGlobalCostMatrix(), p.getGlobalRiskMatrix(), p.totalCostRaw())
        for a, b in zip(before, after):
            assert np.array_equal(bits(a), bits(b))
    finally:
        p.close()


@pytest.mark.parametrize("risk", [None, (RD, RATIO)], ids=["risk-off", "risk-on"])
def test_batches_follow_the_box(dymu, oracle, case, risk):
    i, j = case.box
    p = new_planner(dymu, case.cost, risk=risk)
    try:
        p.trackSpeedChanges(True)
        goals = [wp(*g) for g in GOALS]
        assert p.computeTotalCostMaps(goals)
        assert p.lastBatchSolveKind() == 0
        assert p.setCostMapWindow(i, j, case.block)
        assert p.computeTotalCostMaps(goals)
        assert p.lastBatchSolveKind() == 1
        F = speed(case.cost1)
        if risk:
            assert p.lastRiskUpdateKind() == 2
            F = effective(F, p.getGlobalRiskMatrix())
        for b, g in enumerate(GOALS):
            check_parity(p.batchTotalCost(b), oracle.fmm(F, g)[0])
    finally:
        p.close()
