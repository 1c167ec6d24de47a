"""The clearance edit and trackObstacleRemoval without a device: the
exported entries, an unchanged ABI version, the null-handle returns of the C forms, and a
planner that has no device engine (a device ordinal no machine has, so the same holds with
and without a GPU), on which the switch and a box that frees an obstacle are plain edits."""
import ctypes

import numpy as np

NX, NY = 48, 40


def test_symbols_exported_and_abi_unchanged(dymu):
    fim, pl = dymu.load_fim(), dymu.load_planner()
    assert hasattr(fim, "dymu_clearance_edit_device")
    assert "dymu_clearance_edit_device" in dymu.FIM_SYMBOLS
    assert hasattr(pl, "dymu_planner_track_obstacle_removal")
    assert "dymu_planner_track_obstacle_removal" in dymu.PLANNER_SYMBOLS
    assert hasattr(fim, "dymu_clearance_update_device")  # nothing renamed
    assert fim.dymu_abi_version() == 5
    assert callable(dymu.Engine.clearance_edit_device)
    assert callable(dymu.Planner.trackObstacleRemoval)
    assert "3" in dymu.Planner.lastRiskUpdateKind.__doc__


def test_entries_reject_null_handles(dymu):
    fim, pl = dymu.load_fim(), dymu.load_planner()
    assert fim.dymu_clearance_edit_device(None, None, None, None, 8, 8, 8, 0.5, 0, 0, 4, 4, None,
                                          None, None) == -1
    assert pl.dymu_planner_track_obstacle_removal(None, 1) == -1
    assert pl.dymu_planner_track_obstacle_removal(None, 0) == -1
    assert pl.dymu_planner_last_risk_raise(None, (ctypes.c_uint64 * 4)()) == -1


def test_switch_and_freeing_box_without_engine(dymu, oracle):
    """No device, so no global risk: the switch is accepted either way, a box that frees an
    obstacle of the mask is a plain cost edit, and R was never brought up to date."""
    F = oracle.synth_speed(NX, NY, seed=3, obst_frac=0.02, goal=(20, 20))
    cost = np.where(np.isfinite(F), F, -1.0)
    cost[7, 30] = np.inf  # an obstacle of the mask that a finite cost frees
    p = dymu.Planner(risk_distance=0.5, device=9999)
    try:
        assert p.initGlobalLayer(1.0, 0.5, NX, NY)
        assert p.setCostMap(cost)
        assert p.setGlobalRisk(1.0, 2.0) is False
        assert p.trackObstacleRemoval() is None
        h = ctypes.c_void_p(p.h if isinstance(p.h, int) else p.h.value)
        assert p._lib.dymu_planner_track_obstacle_removal(h, 1) == 0
        assert p.setCostMapWindow(30, 7, np.array([[2.0, -1.0]])) is True
        assert p.lastRiskUpdateKind() == 0 and not any(p.lastRiskRaise().values())
        assert p.getGlobalNode(30, 7)["cost"] == 2.0 and p.getGlobalNode(30, 7)["is_obstacle"] == 0
        assert p.getGlobalNode(31, 7)["is_obstacle"] == 1
        R = p.getGlobalRiskMatrix()
        assert R.shape == (NY, NX) and not R.view(np.uint64).any()
        p.trackObstacleRemoval(False)
        assert p.setCostMapWindow(30, 7, np.array([[np.inf]])) is True
        assert p.lastRiskUpdateKind() == 0
    finally:
        p.close()
