"""Obstacle clearance for the global plan without a device: the exported
entries, and setGlobalRisk on a planner that has no device engine (a device ordinal no
machine has, so the same holds with and without a GPU)."""
import numpy as np

FIM_ENTRIES = ("dymu_clearance_device", "dymu_inflate_speed_device")
PLANNER_ENTRIES = ("dymu_planner_set_global_risk", "dymu_planner_get_global_risk")


def test_symbols_exported_and_abi_unchanged(dymu):
    fim, pl = dymu.load_fim(), dymu.load_planner()
    for n in FIM_ENTRIES:
        assert hasattr(fim, n) and n in dymu.FIM_SYMBOLS, n
    for n in PLANNER_ENTRIES:
        assert hasattr(pl, n) and n in dymu.PLANNER_SYMBOLS, n
    assert fim.dymu_abi_version() == 5
    for m in ("clearance_device", "inflate_speed"):
        assert callable(getattr(dymu.Engine, m))
    for m in ("setGlobalRisk", "getGlobalRiskMatrix"):
        assert callable(getattr(dymu.Planner, m))


def test_engine_entries_reject_null_context(dymu):
    fim = dymu.load_fim()
    assert fim.dymu_clearance_device(None, None, None, None, 8, 8, 8, 0.5, None, None) == -1
    assert fim.dymu_inflate_speed_device(None, None, None, None, 8, 8, 8, 1.0, None) == -1


def test_planner_without_engine(dymu, oracle):
    nx, ny = 48, 40
    F = oracle.synth_speed(nx, ny, seed=3, obst_frac=0.02, goal=(20, 20))
    T, _ = oracle.fmm(F, (20, 20))
    p = dymu.Planner(risk_distance=0.5, device=9999)  # no such device: no engine, ever
    try:
        assert p.initGlobalLayer(1.0, 0.5, nx, ny)
        assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
        assert p.setGoal((20, 20, 0.0, 0.75))
        assert p.loadTotalCostMap(T)
        path = p.getPath((5.3, 30.2))
        before = (p.getTotalCostMatrix(), p.getGlobalCostMatrix(), p.lastSolveKind())
        assert p.setGlobalRisk(1.0, 2.0) is False  # a non-zero setting needs the engine
        assert p.setGlobalRisk(-1.0, 1.0) is False
        assert p.setGlobalRisk(1.0, -1.0) is False
        assert p.setGlobalRisk(np.nan, 1.0) is False
        assert p.setGlobalRisk(1.0, np.inf) is False
        assert p.setGlobalRisk(0.0, 3.0) is True and p.setGlobalRisk(3.0, 0.0) is True  # off
        R = p.getGlobalRiskMatrix()
        assert R.shape == (ny, nx) and not R.view(np.uint64).any()
        lib = dymu.load_planner()
        assert lib.dymu_planner_set_global_risk(None, 1.0, 1.0) == -1
        assert lib.dymu_planner_get_global_risk(None, R) == -1
        # the loaded state is what it was, bit for bit
        assert np.array_equal(p.getTotalCostMatrix().view(np.uint64), before[0].view(np.uint64))
        assert np.array_equal(p.getGlobalCostMatrix().view(np.uint64), before[1].view(np.uint64))
        assert p.lastSolveKind() == before[2]
        assert np.array_equal(p.getPath((5.3, 30.2)), path)
    finally:
        p.close()
