"""Windowed re-propagation of seeded maps and of batches without a device (DESIGN.md
s5.8): the exported entries, the window record's layout, and the planner's tracked batch
calls on a planner that has no device engine (a device ordinal no machine has, so the same
holds with and without a GPU)."""
import numpy as np

FIM_ENTRIES = ("dymu_update_seeds_window_device", "dymu_update_batch_window_device")
PLANNER_ENTRIES = ("dymu_planner_track_speed_changes", "dymu_planner_last_batch_solve_kind")


def test_symbols_exported_and_abi_unchanged(dymu):
    fim, pl = dymu.load_fim(), dymu.load_planner()
    for n in FIM_ENTRIES:
        assert hasattr(fim, n) and n in dymu.FIM_SYMBOLS, n
    for n in PLANNER_ENTRIES:
        assert hasattr(pl, n) and n in dymu.PLANNER_SYMBOLS, n
    assert fim.dymu_abi_version() == 5
    assert dymu.BATCH_WINDOW_DTYPE.itemsize == 24  # plane, i0, j0, w, h, reserved
    assert dymu.BATCH_WINDOW_DTYPE.names == ("plane", "i0", "j0", "w", "h", "reserved")
    for m in ("update_seeds_window_device", "update_batch_window_device"):
        assert callable(getattr(dymu.Engine, m))
    for m in ("trackSpeedChanges", "lastBatchSolveKind"):
        assert callable(getattr(dymu.Planner, m))


def test_engine_entries_reject_null_context(dymu):
    fim = dymu.load_fim()
    seed = np.zeros(1, dtype=dymu.SEED_DTYPE)
    bseed = np.zeros(1, dtype=dymu.BATCH_SEED_DTYPE)
    win = np.zeros(1, dtype=dymu.BATCH_WINDOW_DTYPE)
    win[0] = (0, 1, 1, 2, 2, 0)
    assert fim.dymu_update_seeds_window_device(None, None, None, 8, 8, 8, seed.ctypes.data, 1, 1,
                                               1, 2, 2, 0, None, None) == -1
    assert fim.dymu_update_batch_window_device(None, None, None, 8, 8, 1, 8, bseed.ctypes.data, 1,
                                               win.ctypes.data, 1, 0, None, None) == -1


def test_tracking_planner_without_engine(dymu, oracle):
    nx, ny = 48, 40
    F = oracle.synth_speed(nx, ny, seed=3)
    T, _ = oracle.fmm(F, (20, 20))
    p = dymu.Planner(risk_distance=0.5, device=9999)  # no such device: no engine, ever
    try:
        assert p.initGlobalLayer(1.0, 0.5, nx, ny)
        assert p.setCostMap(F)
        assert p.setGoal((20, 20, 0.0, 0.75))
        assert p.loadTotalCostMap(T)
        path = p.getPath((5.3, 30.2))
        before = (p.getTotalCostMatrix(), p.goalCount(), p.lastSolveKind(), p.current_path)
        assert p.lastBatchSolveKind() == 0
        p.trackSpeedChanges(True)
        goals = [(10, 10), (30, 25), (20, 20)]
        assert p.computeTotalCostMaps(goals) is False
        assert p.batchCount() == 0
        assert p.lastBatchSolveKind() == 0
        assert p.costMatrix(goals, [(4.5, 4.5)]) is None
        assert p.getTotalCosts([(4.5, 4.5)]) is None
        assert p.batchTotalCost(0) is None
        # the single-goal state is what it was
        assert np.array_equal(p.getTotalCostMatrix(), before[0])
        assert (p.goalCount(), p.lastSolveKind()) == before[1:3]
        assert np.array_equal(p.current_path, before[3]) and len(path) == len(before[3])
        assert np.array_equal(p.getPath((5.3, 30.2)), path)
        p.trackSpeedChanges(False)
        assert p.computeTotalCostMaps(goals) is False and p.batchCount() == 0
    finally:
        p.close()
