"""Batched solves without a device: the stack layout's plane pitch, the
exported entries, and the planner's batch calls on a planner that has no device engine
(a device ordinal no machine has, so the same holds with and without a GPU)."""
import numpy as np
import pytest

FIM_ENTRIES = ("dymu_batch_plane_rows", "dymu_stack_speed_device", "dymu_solve_batch_device",
               "dymu_gather_costs_device")
PLANNER_ENTRIES = ("dymu_planner_compute_total_cost_maps", "dymu_planner_batch_count",
                   "dymu_planner_copy_batch_total_cost", "dymu_planner_get_total_costs",
                   "dymu_planner_cost_matrix", "dymu_planner_get_paths_to",
                   "dymu_planner_last_batch_stats")


@pytest.mark.parametrize("ny, rows", [(15, 16), (16, 32), (61, 64), (63, 64), (96, 112)])
def test_plane_rows(dymu, ny, rows):
    assert dymu.batch_plane_rows(ny) == rows
    assert rows % 16 == 0 and rows > ny  # a tile boundary, and at least one wall row


def test_symbols_exported_and_abi_unchanged(dymu):
    fim, pl = dymu.load_fim(), dymu.load_planner()
    for n in FIM_ENTRIES:
        assert hasattr(fim, n) and n in dymu.FIM_SYMBOLS, n
    for n in PLANNER_ENTRIES:
        assert hasattr(pl, n) and n in dymu.PLANNER_SYMBOLS, n
    assert fim.dymu_abi_version() == 5
    assert dymu.BATCH_SEED_DTYPE.itemsize == 24  # plane, i, j, reserved, t0
    for m in ("stack_speed", "solve_batch_device", "gather_costs"):
        assert callable(getattr(dymu.Engine, m))


def test_engine_entries_reject_null_context(dymu):
    fim = dymu.load_fim()
    assert fim.dymu_stack_speed_device(None, None, 8, 0, 8, 8, 1, None, 8, None) == -1
    assert fim.dymu_solve_batch_device(None, None, None, 8, 8, 1, 8, None, 0, None, None) == -1
    assert fim.dymu_gather_costs_device(None, None, 8, 8, 1, 8, 1.0, None, 0, None, None) == -1


def test_planner_without_engine(dymu, oracle):
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
        goals = [(10, 10), (30, 25), (20, 20)]
        assert p.computeTotalCostMaps(goals) is False
        assert p.batchCount() == 0
        assert p.costMatrix(goals, [(4.5, 4.5)]) is None
        assert p.getTotalCosts([(4.5, 4.5)]) is None
        assert p.batchTotalCost(0) is None
        with pytest.raises(dymu.DymuError) as e:
            p.getPathsTo(0, [(5.3, 30.2)])
        assert e.value.status == -1
        # a goal setGoal would reject is refused before any engine is asked for
        assert p.computeTotalCostMaps([(0, 10)]) is False
        assert p.computeTotalCostMaps([]) is False
        # the single-goal state is what it was
        assert np.array_equal(p.getTotalCostMatrix(), before[0])
        assert (p.goalCount(), p.lastSolveKind()) == before[1:3]
        assert np.array_equal(p.current_path, before[3]) and len(path) == len(before[3])
        assert p.getTotalCost((12.25, 7.5)) == T[7, 12] + (T[7, 13] - T[7, 12]) * 0.25 + \
            (T[8, 12] - T[7, 12]) * 0.5 + (T[8, 13] + T[7, 12] - T[7, 13] - T[8, 12]) * 0.25 * 0.5
        assert np.array_equal(p.getPath((5.3, 30.2)), path)
    finally:
        p.close()
