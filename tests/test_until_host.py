"""Early exit on target cells without a device: the exported entries, the
cell types' layout, and costMatrix(..., until=True) on a planner that has no device engine
(a device ordinal no machine has, so the same holds with and without a GPU)."""
import numpy as np

FIM_ENTRIES = ("dymu_solve_seeds_until_device", "dymu_solve_batch_until_device")
PLANNER_ENTRIES = ("dymu_planner_cost_matrix_until", "dymu_planner_batch_level")


def test_symbols_exported_and_abi_unchanged(dymu):
    fim, pl = dymu.load_fim(), dymu.load_planner()
    for n in FIM_ENTRIES:
        assert hasattr(fim, n) and n in dymu.FIM_SYMBOLS, n
    for n in PLANNER_ENTRIES:
        assert hasattr(pl, n) and n in dymu.PLANNER_SYMBOLS, n
    assert fim.dymu_abi_version() == 5
    assert dymu.CELL_DTYPE.itemsize == 8          # i, j
    assert dymu.BATCH_CELL_DTYPE.itemsize == 16   # plane, i, j, reserved
    for m in ("solve_seeds_until_device", "solve_batch_until_device"):
        assert callable(getattr(dymu.Engine, m))
    assert callable(dymu.Planner.batchLevel)


def test_engine_entries_reject_null_context(dymu):
    fim = dymu.load_fim()
    assert fim.dymu_solve_seeds_until_device(None, None, None, 8, 8, 8, None, 0, None, 0, None,
                                             None, None) == -1
    assert fim.dymu_solve_batch_until_device(None, None, None, 8, 8, 1, 8, None, 0, None, 0,
                                             None, None, None, None) == -1


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
        assert p.batchLevel() == np.inf
        assert p.costMatrix(goals, [(4.5, 4.5)], until=True) is None
        assert p.costMatrix(goals, [], until=True) is None
        assert p.costMatrix([], [(4.5, 4.5)], until=True) is None
        # a goal setGoal would reject is refused as well
        assert p.costMatrix([(0, 10)], [(4.5, 4.5)], until=True) is None
        assert p.batchCount() == 0 and p.batchLevel() == np.inf
        assert p.getTotalCosts([(4.5, 4.5)]) is None
        lib = dymu.load_planner()
        assert lib.dymu_planner_cost_matrix_until(None, None, 0, None, 0, None) == -1
        assert lib.dymu_planner_batch_level(None, None) == -1
        # the single-goal state is what it was, bit for bit
        assert np.array_equal(p.getTotalCostMatrix().view(np.uint64), before[0].view(np.uint64))
        assert (p.goalCount(), p.lastSolveKind()) == before[1:3]
        assert np.array_equal(p.current_path, before[3]) and len(path) == len(before[3])
        assert p.getTotalCost((12.25, 7.5)) == T[7, 12] + (T[7, 13] - T[7, 12]) * 0.25 + \
            (T[8, 12] - T[7, 12]) * 0.5 + (T[8, 13] + T[7, 12] - T[7, 13] - T[8, 12]) * 0.25 * 0.5
        assert np.array_equal(p.getPath((5.3, 30.2)), path)
    finally:
        p.close()
