"""setCostMapWindow and the clearance update without a device: the exported
entries, the per-cell rule against setCostMap's on the node fields, and a planner that has no
device engine (a device ordinal no machine has, so the same holds with and without a GPU)."""
import ctypes

import numpy as np

FIM_ENTRIES = ("dymu_clearance_update_device",)
PLANNER_ENTRIES = ("dymu_planner_set_cost_map_window", "dymu_planner_last_risk_update_kind")
NX, NY = 48, 40


def test_symbols_exported_and_abi_unchanged(dymu):
    fim, pl = dymu.load_fim(), dymu.load_planner()
    for n in FIM_ENTRIES:
        assert hasattr(fim, n) and n in dymu.FIM_SYMBOLS, n
    for n in PLANNER_ENTRIES:
        assert hasattr(pl, n) and n in dymu.PLANNER_SYMBOLS, n
    assert fim.dymu_abi_version() == 5
    assert callable(dymu.Engine.clearance_update_device)
    for m in ("setCostMapWindow", "lastRiskUpdateKind"):
        assert callable(getattr(dymu.Planner, m))


def test_entries_reject_null_arguments(dymu):
    fim = dymu.load_fim()
    assert fim.dymu_clearance_update_device(None, None, None, None, 8, 8, 8, 0.5, 0, 0, 4, 4,
                                            None, None, None) == -1
    # a second handle on the library: plain prototypes, so that a null cost pointer passes
    raw = ctypes.CDLL(dymu.lib_path("libdymu_planner.so"))
    p = dymu.Planner(risk_distance=0.5, device=9999)
    try:
        assert p.initGlobalLayer(1.0, 0.5, NX, NY)
        h = ctypes.c_void_p(p.h if isinstance(p.h, int) else p.h.value)
        assert raw.dymu_planner_set_cost_map_window(h, 0, 0, 2, 2, None) == -1
        assert raw.dymu_planner_set_cost_map_window(None, 0, 0, 2, 2, None) == -1
        assert raw.dymu_planner_last_risk_update_kind(None) == -1
    finally:
        p.close()


def nodes(p):
    return [tuple(sorted(p.getGlobalNode(i, j).items())) for j in range(NY) for i in range(NX)]


def test_per_cell_rule_is_setcostmaps(dymu, oracle):
    """The box written through the window and the whole edited map written through setCostMap
    leave the same node fields; cells outside the box keep theirs."""
    F = oracle.synth_speed(NX, NY, seed=3, obst_frac=0.02, goal=(20, 20))
    cost = np.where(np.isfinite(F), F, -1.0)
    box = np.array([[2.5, -1.0, 0.0, 7.0], [np.inf, 1.25, -0.0, np.nan], [3.0, 3.0, -2.0, 0.5]])
    i0, j0 = 9, 30
    cost[j0, i0] = -1.0  # an obstacle the box gives a positive cost: it stays one
    edited = cost.copy()
    edited[j0:j0 + 3, i0:i0 + 4] = box
    a = dymu.Planner(risk_distance=0.5, device=9999)
    b = dymu.Planner(risk_distance=0.5, device=9999)
    try:
        for p in (a, b):
            assert p.initGlobalLayer(1.0, 0.5, NX, NY)
            assert p.setCostMap(cost)
        before = nodes(a)
        for bad in ((NX - 3, j0), (i0, NY - 2), (NX, 0), (0, NY)):
            assert a.setCostMapWindow(*bad, box) is False
        assert nodes(a) == before  # a rejected box changes nothing
        assert a.setCostMapWindow(i0, j0, box) is True
        assert b.setCostMap(edited)
        na, nb = nodes(a), nodes(b)
        assert repr(na) == repr(nb)  # repr: NaN costs compare equal
        n = a.getGlobalNode(i0, j0)
        assert n["is_obstacle"] == 1 and n["cost"] == 2.5
        n = a.getGlobalNode(i0 + 2, j0)
        assert n["is_obstacle"] == 1 and n["trafficability"] == 0.0 and n["hazard_density"] == 1.0
        changed = [k for k, (x, y) in enumerate(zip(before, na)) if repr(x) != repr(y)]
        assert changed and all(j0 <= k // NX < j0 + 3 and i0 <= k % NX < i0 + 4 for k in changed)
        assert a.setCostMapWindow(NX - 4, NY - 3, box) is True  # flush with the far corner
        assert a.setCostMapWindow(5, 5, np.empty((0, 3))) is True  # an empty box inside the grid
        assert a.lastRiskUpdateKind() == 0
    finally:
        a.close()
        b.close()


def test_risk_on_planner_without_engine(dymu, oracle):
    """No device, no global risk: the setting is refused as before, a window edit is a plain
    cost edit, and the loaded map and its paths are what they were."""
    F = oracle.synth_speed(NX, NY, seed=3, obst_frac=0.02, goal=(20, 20))
    T, _ = oracle.fmm(F, (20, 20))
    p = dymu.Planner(risk_distance=0.5, device=9999)
    try:
        assert p.initGlobalLayer(1.0, 0.5, NX, NY)
        assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
        assert p.setGoal((20, 20, 0.0, 0.75))
        assert p.loadTotalCostMap(T)
        path = p.getPath((5.3, 30.2))
        before = p.getTotalCostMatrix()
        assert p.setGlobalRisk(1.0, 2.0) is False  # a non-zero setting needs the engine
        assert p.setCostMapWindow(40, 3, np.full((2, 2), -1.0)) is True
        assert p.lastRiskUpdateKind() == 0
        R = p.getGlobalRiskMatrix()
        assert R.shape == (NY, NX) and not R.view(np.uint64).any()
        assert p.getGlobalNode(41, 4)["is_obstacle"] == 1
        assert np.array_equal(p.getTotalCostMatrix().view(np.uint64), before.view(np.uint64))
        assert np.array_equal(p.getPath((5.3, 30.2)), path)
    finally:
        p.close()
