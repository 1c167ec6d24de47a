"""Obstacle clearance for the global plan on the planner.

With setGlobalRisk(risk_distance, risk_ratio) every global solve runs on the effective
speed F * (risk_ratio * R + 1), R = max(1 - S, 0), S the clearance field of the obstacles on
the global map.  The yardsticks: S_ref = goalset_ref.fmm_seeds on the constant map
global_res / risk_distance with one seed at 0 per obstacle cell (|R - R_ref| <= 1e-12), and
the oracle FMM of the effective speed built in numpy from the planner's own R (the parity
bound |dT| <= 1e-12 max(1, T), same +inf mask).  References are computed once per shape.
"""
import ctypes

import numpy as np
import pytest

import goalset_ref as ref

pytestmark = pytest.mark.gpu

OFF = (100.0, 200.0)
RES = 1.0
RD, RATIO = 3.5, 2.0  # risk distance in metres (3.5 cells), risk ratio
SHAPES = {"97x61": ((97, 61), (70, 40), (12, 9)), "160x128": ((160, 128), (101, 77), (20, 30))}
INF = np.inf


class Case:
    pass


def check_parity(T, T_ref):
    assert np.array_equal(np.isinf(T), np.isinf(T_ref))
    fin = np.isfinite(T_ref)
    rel = (np.abs(T[fin] - T_ref[fin]) / np.maximum(1.0, T_ref[fin])).max()
    print(f"max |dT| / max(1, T) = {rel:.3e}")
    assert rel <= 1e-12


def risk_ref(oracle, obst, rd=RD):
    seeds = [(int(i), int(j), 0.0) for j, i in np.argwhere(obst)]
    S = ref.fmm_seeds(oracle, np.full(obst.shape, RES / rd), seeds)
    return np.maximum(1.0 - S, 0.0)


def speed(cost, hazard=0.0, traff=1.0):
    """The planner's raw speed (:527-528) for its non-obstacle cells, +inf for the others."""
    return np.where(cost > 0, (RES * cost) * (2 + hazard - traff), INF)


def effective(F, R, ratio=RATIO):
    return F * (ratio * R + 1.0)


def new_planner(dymu, cost, risk=(RD, RATIO), deterministic=False):
    ny, nx = cost.shape
    p = dymu.Planner(risk_distance=0.5)
    if deterministic:
        o = dymu.DymuOpts(-1, 0, 0, 0, 0, 0, 0, 0, 1)
        assert p._lib.dymu_planner_set_engine_options(p.h, ctypes.byref(o)) == 0
    assert p.initGlobalLayer(RES, 0.5, nx, ny, offset=OFF)
    assert p.setCostMap(cost)
    if risk is not None:
        assert p.setGlobalRisk(*risk)
    return p


def wp(i, j):
    return (OFF[0] + RES * i, OFF[1] + RES * j, 0.0, 0.0)


@pytest.fixture(scope="module", params=sorted(SHAPES))
def case(request, oracle):
    """A 2 % obstacle map (none next to a goal), its risk reference and cost map."""
    c = Case()
    (c.nx, c.ny), c.goal, c.goal2 = SHAPES[request.param]
    F = oracle.synth_speed(c.nx, c.ny, seed=33, obst_frac=0.02, obst_seed=17, goal=c.goal)
    for gi, gj in (c.goal, c.goal2):
        blk = F[gj - 1:gj + 2, gi - 1:gi + 2]
        blk[~np.isfinite(blk)] = 3.0
    c.cost = np.where(np.isfinite(F), F, -1.0)
    c.F = speed(c.cost)
    c.R_ref = risk_ref(oracle, c.cost <= 0)
    assert ((c.R_ref > 0) & (c.R_ref < 1)).any() and (c.R_ref == 0).any()
    for a in (c.cost, c.F, c.R_ref):
        a.setflags(write=False)
    return c


def test_risk_and_every_solve(dymu, oracle, case):
    p = new_planner(dymu, case.cost)
    try:
        R = p.getGlobalRiskMatrix()  # stale: computed here, before any solve
        err = np.abs(R - case.R_ref).max()
        print(f"max |R - R_ref| = {err:.3e}")
        assert err <= 1e-12
        assert (R[case.cost <= 0] == 1.0).all()
        Fe = effective(case.F, R)
        # single goal
        assert p.setGoal(wp(*case.goal)) and p.computeEntireTotalCostMap()
        assert p.lastSolveKind() == 0
        check_parity(p.totalCostRaw(), oracle.fmm(Fe, case.goal)[0])
        assert np.array_equal(p.getGlobalRiskMatrix().view(np.uint64), R.view(np.uint64))
        # a goal set with an offset
        seeds = [(*case.goal, 0.0), (*case.goal2, 6.5)]
        assert p.setGoals([wp(*case.goal), wp(*case.goal2)], [0.0, 6.5])
        assert p.computeEntireTotalCostMap()
        check_parity(p.totalCostRaw(), ref.fmm_seeds(oracle, Fe, seeds))
        # a batch of two goals
        assert p.computeTotalCostMaps([wp(*case.goal), wp(*case.goal2)])
        for b, g in enumerate((case.goal, case.goal2)):
            check_parity(p.batchTotalCost(b), oracle.fmm(Fe, g)[0])
    finally:
        p.close()


def test_hazard_window_is_repropagated(dymu, oracle, case):
    p = new_planner(dymu, case.cost)
    try:
        assert p.setGoal(wp(*case.goal)) and p.computeEntireTotalCostMap()
        R = p.getGlobalRiskMatrix()
        i0, j0 = case.goal2[0] - 3, case.goal2[1] - 3
        hd = np.array(p.getHazardDensityMatrix())
        hd[j0:j0 + 6, i0:i0 + 6] = np.where(case.cost[j0:j0 + 6, i0:i0 + 6] > 0, 0.5, 1.0)
        assert p.setHazardDensityWindow(i0, j0, hd[j0:j0 + 6, i0:i0 + 6])
        assert p.computeEntireTotalCostMap()
        assert p.lastSolveKind() == 1  # a windowed update, not a cold solve
        traff = np.array(p.getTrafficabilityMatrix())
        Fe = effective(speed(case.cost, hd, traff), R)
        assert (Fe[j0:j0 + 6, i0:i0 + 6] != effective(case.F, R)[j0:j0 + 6, i0:i0 + 6]).any()
        check_parity(p.totalCostRaw(), oracle.fmm(Fe, case.goal)[0])
        assert np.array_equal(p.getGlobalRiskMatrix().view(np.uint64), R.view(np.uint64))
    finally:
        p.close()


def test_new_obstacle_recomputes_the_risk(dymu, oracle, case):
    p = new_planner(dymu, case.cost)
    try:
        assert p.setGoal(wp(*case.goal)) and p.computeEntireTotalCostMap()
        R0 = p.getGlobalRiskMatrix()
        # a cell that is clear of every obstacle so far, away from the goal
        far = np.argwhere((case.R_ref == 0) & (case.cost > 0))
        j, i = next((j, i) for j, i in far
                    if abs(i - case.goal[0]) + abs(j - case.goal[1]) > 12 and 2 < i < case.nx - 3
                    and 2 < j < case.ny - 3)
        cost = case.cost.copy()
        cost[j, i] = -1.0
        assert p.setCostMap(cost)
        R1 = p.getGlobalRiskMatrix()
        assert R0[j, i] == 0.0 and R1[j, i] == 1.0 and R1[j, i + 1] > 0.0
        assert np.abs(R1 - risk_ref(oracle, cost <= 0)).max() <= 1e-12
        assert p.computeEntireTotalCostMap()
        check_parity(p.totalCostRaw(), oracle.fmm(effective(speed(cost), R1), case.goal)[0])
        # another distance and ratio: stale again, the map follows
        assert p.setGlobalRisk(2.0, 0.75)
        R2 = p.getGlobalRiskMatrix()
        assert np.abs(R2 - risk_ref(oracle, cost <= 0, rd=2.0)).max() <= 1e-12
        assert p.computeEntireTotalCostMap()
        check_parity(p.totalCostRaw(),
                     oracle.fmm(effective(speed(cost), R2, 0.75), case.goal)[0])
        # and off again: the plain speed
        assert p.setGlobalRisk(0.0, 0.75)
        assert not p.getGlobalRiskMatrix().any()
        assert p.computeEntireTotalCostMap()
        check_parity(p.totalCostRaw(), oracle.fmm(speed(cost), case.goal)[0])
    finally:
        p.close()


def test_risk_refresh_leaves_the_synchronised_speed_alone(dymu, oracle, case):
    """A held batch with a pending box is re-propagated from the device copy of the speed
    last synchronised; reading a stale risk in between must not disturb that copy."""
    p = new_planner(dymu, case.cost)
    try:
        p.trackSpeedChanges(True)
        goals = [wp(*case.goal), wp(*case.goal2)]
        assert p.computeTotalCostMaps(goals)
        R = p.getGlobalRiskMatrix()
        i0, j0 = case.goal2[0] - 3, case.goal2[1] - 3
        hd = np.array(p.getHazardDensityMatrix())
        hd[j0:j0 + 6, i0:i0 + 6] = np.where(case.cost[j0:j0 + 6, i0:i0 + 6] > 0, 0.5, 1.0)
        assert p.setHazardDensityWindow(i0, j0, hd[j0:j0 + 6, i0:i0 + 6])
        assert p.setGoal(wp(*case.goal)) and p.computeEntireTotalCostMap()  # synchronises
        Fe = effective(speed(case.cost, hd, np.array(p.getTrafficabilityMatrix())), R)
        # a new obstacle, not synchronised yet: the risk is stale and is recomputed here
        far = np.argwhere((case.R_ref == 0) & (case.cost > 0))
        j, i = next((j, i) for j, i in far
                    if abs(i - case.goal[0]) + abs(j - case.goal[1]) > 12 and 2 < i < case.nx - 3
                    and 2 < j < case.ny - 3)
        cost = case.cost.copy()
        cost[j, i] = -1.0
        assert p.setCostMap(cost)
        assert p.getGlobalRiskMatrix()[j, i] == 1.0
        for b, g in enumerate((case.goal, case.goal2)):  # the batch of the synchronised speed
            check_parity(p.batchTotalCost(b), oracle.fmm(Fe, g)[0])
        assert p.lastBatchSolveKind() == 1
    finally:
        p.close()


def test_off_is_bit_identical(dymu, case):
    """Never called, called with a 0 distance, called with a 0 ratio: one deterministic map."""
    maps = []
    for risk in (None, (0.0, RATIO), (RD, 0.0)):
        p = new_planner(dymu, case.cost, risk=risk, deterministic=True)
        try:
            assert p.setGoal(wp(*case.goal)) and p.computeEntireTotalCostMap()
            assert not p.getGlobalRiskMatrix().any()
            maps.append(p.totalCostRaw())
        finally:
            p.close()
    for m in maps[1:]:
        assert np.array_equal(m.view(np.uint64), maps[0].view(np.uint64))


def test_propagate_global_node_uses_the_effective_speed(dymu, oracle, case):
    p = new_planner(dymu, case.cost)
    try:
        assert p.setGoal(wp(*case.goal)) and p.computeEntireTotalCostMap()
        R = p.getGlobalRiskMatrix()
        T = p.totalCostRaw()
        inner = np.zeros(T.shape, dtype=bool)
        inner[1:-1, 1:-1] = True
        cand = np.argwhere((R > 0.2) & (R < 1) & np.isfinite(T) & inner)
        j, i = (int(v) for v in cand[len(cand) // 2])
        T0 = T.copy()
        T0[j, i] = INF
        assert p.loadTotalCostMap(T0)
        p.propagateGlobalNode(i, j)
        got = p.totalCostRaw()[j, i]
        tx, ty = min(T[j, i - 1], T[j, i + 1]), min(T[j - 1, i], T[j + 1, i])
        want = oracle.eikonal(tx, ty, effective(case.F, R)[j, i])
        plain = oracle.eikonal(tx, ty, case.F[j, i])
        print(f"cell ({i}, {j}): R = {R[j, i]:.3f}, got {got!r}, effective {want!r}, "
              f"plain {plain!r}")
        assert abs(got - want) <= 1e-12 * max(1.0, want)
        assert abs(got - plain) > 1e-6
    finally:
        p.close()
