"""Combining the planes of a batch without a device: the exported entries,
their null checks, and a planner that has no device engine (a device ordinal no machine
has, so the same holds with and without a GPU): every new method refuses and changes nothing."""
import ctypes

import numpy as np

FIM_ENTRIES = ("dymu_batch_reduce_device", "dymu_level_mask_device")
PLANNER_ENTRIES = ("dymu_planner_combine_total_cost_maps", "dymu_planner_copy_combined_total_cost",
                   "dymu_planner_copy_combined_planes", "dymu_planner_via_corridor",
                   "dymu_planner_rendezvous")
NX, NY = 48, 40


def test_symbols_exported_and_abi_unchanged(dymu):
    fim, pl = dymu.load_fim(), dymu.load_planner()
    for n in FIM_ENTRIES:
        assert hasattr(fim, n) and n in dymu.FIM_SYMBOLS, n
    for n in PLANNER_ENTRIES:
        assert hasattr(pl, n) and n in dymu.PLANNER_SYMBOLS, n
    assert fim.dymu_abi_version() == 5
    for m in ("batch_reduce", "level_mask"):
        assert callable(getattr(dymu.Engine, m))
    for m in ("combineTotalCostMaps", "combinedTotalCost", "combinedPlanes", "viaCorridor",
              "rendezvous"):
        assert callable(getattr(dymu.Planner, m))
    assert ctypes.sizeof(dymu.DymuReduceSummary) == 32  # the header's layout


def test_entries_reject_null_arguments(dymu):
    fim = dymu.load_fim()
    assert fim.dymu_batch_reduce_device(None, None, 8, 8, 2, 8, 0, None, 0, None, None, None, 8,
                                        None, 0, None, None) == -1
    assert fim.dymu_level_mask_device(None, None, 8, 8, 8, 1.0, None, 8, None, None) == -1
    # a second handle on the library: plain prototypes, so that null pointers pass
    raw = ctypes.CDLL(dymu.lib_path("libdymu_planner.so"))
    raw.dymu_planner_via_corridor.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                              ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    p = dymu.Planner(risk_distance=0.5, device=9999)
    try:
        assert p.initGlobalLayer(1.0, 0.5, NX, NY)
        h = ctypes.c_void_p(p.h if isinstance(p.h, int) else p.h.value)
        assert raw.dymu_planner_combine_total_cost_maps(None, 0, None, 0, None, None, None) == -1
        assert raw.dymu_planner_combine_total_cost_maps(h, 3, None, 0, None, None, None) == -1
        assert raw.dymu_planner_copy_combined_total_cost(None, None, 1) == -1
        assert raw.dymu_planner_copy_combined_total_cost(h, None, 1) == -1
        assert raw.dymu_planner_copy_combined_planes(None, None) == -1
        assert raw.dymu_planner_copy_combined_planes(h, None) == -1
        assert raw.dymu_planner_via_corridor(None, 0, 1, 0.05, None, None) == -1
        assert raw.dymu_planner_via_corridor(h, 0, 1, 0.05, None, None) == -1
        assert raw.dymu_planner_rendezvous(None, None, 0, None, None, 1, None, None, None) == -1
        assert raw.dymu_planner_rendezvous(h, None, 0, None, None, 1, None, None, None) == -1
    finally:
        p.close()


def nodes(p):
    return [tuple(sorted(p.getGlobalNode(i, j).items())) for j in range(NY) for i in range(NX)]


def test_planner_without_engine_refuses_and_changes_nothing(dymu, oracle):
    F = oracle.synth_speed(NX, NY, seed=3, obst_frac=0.02, goal=(20, 20))
    T, _ = oracle.fmm(F, (20, 20))
    p = dymu.Planner(risk_distance=0.5, device=9999)
    try:
        assert p.initGlobalLayer(1.0, 0.5, NX, NY)
        assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
        assert p.setGoal((20, 20, 0.0, 0.75))
        assert p.loadTotalCostMap(T)
        before, nodes_before = p.getTotalCostMatrix(), nodes(p)
        assert p.computeTotalCostMaps([(20, 20), (30, 10)]) is False
        for op in ("sum", "max", "min", 0, 1, 2):
            assert p.combineTotalCostMaps(op) is False
            assert p.combineTotalCostMaps(op, planes=[0, 1], weights=[1.0, 2.0]) is False
        assert p.combinedTotalCost() is False
        assert p.combinedTotalCost(raw=False) is False
        assert p.combinedPlanes() is False
        assert p.viaCorridor(0, 1, 0.05) is False
        assert p.viaCorridor(0, 0, 0.0) is False
        assert p.rendezvous() is False
        assert p.rendezvous(planes=[0, 1], minimax=False) is False
        assert p.batchCount() == 0
        assert repr(nodes(p)) == repr(nodes_before)
        assert np.array_equal(p.getTotalCostMatrix().view(np.uint64), before.view(np.uint64))
    finally:
        p.close()
