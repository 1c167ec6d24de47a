"""getRouteUsage without a device: the planner's host route must be tests/usage_ref.py byte
for byte -- both take the cells in descending total cost, each added into its parent, and the
sums are integers.  No engine is ever created: the maps are the oracle's FMM maps installed
by loadTotalCostMap.  A case is built once and shared."""
import ctypes

import numpy as np
import pytest

import goalset_ref
import usage_ref as ref

RD = 0.5
RES = 1.0
NONE = ref.NONE
CASES = {"96x96": (96, 96, (70, 60)), "97x61": (97, 61, (70, 40))}
OFFS = {"96x96": (0.0, 0.0), "97x61": (100.0, 200.0)}  # one grid with an offset
KEYS = ("usage", "far", "sink", "catchment")
DTYPES = {"usage": np.uint64, "far": np.float64, "sink": np.uint32, "catchment": np.uint64}


def same(a, b, keys=KEYS):
    """None if the two results are the same bits, else the first differing key"""
    for k in keys:
        if a[k].dtype != DTYPES[k] or b[k].dtype != DTYPES[k] or a[k].shape != b[k].shape or \
                a[k].tobytes() != b[k].tobytes():
            return k
    return None


class Case:
    pass


def single_goal_case(dymu, oracle, shape, obst):
    nx, ny, goal = CASES[shape]
    off = OFFS[shape]
    c = Case()
    c.nx, c.ny, c.off, c.obst = nx, ny, off, obst
    c.F = oracle.synth_speed(nx, ny, seed=21, obst_frac=obst, goal=goal)
    c.p = dymu.Planner(risk_distance=RD)
    assert c.p.initGlobalLayer(RES, 0.5, nx, ny, offset=off)
    assert c.p.setCostMap(np.where(np.isfinite(c.F), c.F, -1.0))
    assert c.p.setGoal((off[0] + goal[0], off[1] + goal[1], 0.0, 1.25))
    c.T, _ = oracle.fmm(c.F, goal)
    assert c.p.loadTotalCostMap(c.T)
    c.seeds = [goal + (0.0,)]
    c.goals_ij = [goal]
    return c


# three goals, one with an offset, and a fourth that the first dominates: two cells away
# with an offset of 50 its cell ends far below its t0
GS_GOALS = goalset_ref.GOALS_IJ + [(68, 38)]
GS_OFFSETS = goalset_ref.OFFSETS + [50.0]


def goal_set_case(dymu, oracle):
    g = goalset_ref
    c = Case()
    c.nx, c.ny, c.off, c.obst = g.NX, g.NY, g.OFF, 0.02
    c.F = oracle.synth_speed(g.NX, g.NY, seed=21, obst_frac=0.02, goal=GS_GOALS[0])
    for gi, gj in GS_GOALS:
        blk = c.F[gj - 1:gj + 2, gi - 1:gi + 2]
        blk[~np.isfinite(blk)] = 3.0
    c.p = dymu.Planner(risk_distance=RD)
    assert c.p.initGlobalLayer(RES, 0.5, g.NX, g.NY, offset=g.OFF)
    assert c.p.setCostMap(np.where(np.isfinite(c.F), c.F, -1.0))
    c.goals = [(g.OFF[0] + i, g.OFF[1] + j, 0.0, 0.1 * k) for k, (i, j) in enumerate(GS_GOALS)]
    assert c.p.setGoals(c.goals, GS_OFFSETS)
    c.seeds = [(i, j, t0) for (i, j), t0 in zip(GS_GOALS, GS_OFFSETS)]
    c.T = g.fmm_seeds(oracle, c.F, c.seeds)
    assert c.p.loadTotalCostMap(c.T)
    c.goals_ij = GS_GOALS
    return c


PARAMS = [(s, o) for s in sorted(CASES) for o in (0.0, 0.02)] + [("goalset", 0.02)]


@pytest.fixture(scope="module", params=PARAMS, ids=lambda p: f"{p[0]}-obst{p[1]}")
def case(request, dymu, oracle):
    shape, obst = request.param
    c = goal_set_case(dymu, oracle) if shape == "goalset" else \
        single_goal_case(dymu, oracle, shape, obst)
    c.shape = shape
    rng = np.random.default_rng(7)
    c.w = rng.integers(0, 2 ** 32, size=(c.ny, c.nx), dtype=np.uint64).astype(np.uint32)
    c.got = c.p.getRouteUsage()
    assert not c.p.lastPathsOnDevice() and c.p.lastPathsKernelMs() == 0 and c.got["rounds"] == 0
    c.got_w = c.p.getRouteUsage(weights=c.w)
    c.ref = ref.route_usage(c.T, c.seeds)
    c.ref_w = ref.route_usage(c.T, c.seeds, c.w)
    yield c
    c.p.close()


def test_host_equals_the_reference_byte_for_byte(case):
    assert same(case.got, case.ref) is None, same(case.got, case.ref)
    assert same(case.got_w, case.ref_w) is None, same(case.got_w, case.ref_w)
    assert case.got["usage"].shape == (case.ny, case.nx)
    assert case.got["catchment"].shape == (len(case.seeds),)
    # host=True is the same route, and a subset of outputs the same maps
    again = case.p.getRouteUsage(weights=case.w, host=True)
    assert same(again, case.got_w) is None
    part = case.p.getRouteUsage(outputs=("far", "catchment"))
    assert sorted(part) == ["catchment", "far", "rounds"]
    assert same(part, case.got, ("far", "catchment")) is None
    part = case.p.getRouteUsage(weights=case.w, outputs=("usage",))
    assert sorted(part) == ["rounds", "usage"]
    assert part["usage"].tobytes() == case.got_w["usage"].tobytes()


def test_properties_on_converged_maps(case):
    g = case.got
    has = g["sink"] != NONE
    assert np.array_equal(has, np.isfinite(case.T))
    assert (g["usage"][~has] == 0).all() and np.isnan(g["far"][~has]).all()
    assert (g["usage"][has] >= 1).all() and (g["far"][has] >= case.T[has]).all()
    assert int(g["catchment"].sum()) == int(has.sum())
    assert int(case.got_w["catchment"].astype(object).sum()) == int(case.w[has].astype(object).sum())
    if case.shape == "goalset":
        assert g["catchment"][3] == 0 and (g["catchment"][:3] > 100).all()
        for k, (gi, gj) in enumerate(case.goals_ij[:3]):
            assert g["usage"][gj, gi] == g["catchment"][k] == (g["sink"] == k).sum()
            assert g["far"][gj, gi] == case.T[g["sink"] == k].max()
    else:
        gi, gj = case.goals_ij[0]
        assert g["usage"][gj, gi] == has.sum() == g["catchment"][0]
        assert g["far"][gj, gi] == case.T[has].max()
    assert case.got_w["far"].tobytes() == g["far"].tobytes()


def test_current_path_is_not_touched(case):
    start = (case.off[0] + 20.3, case.off[1] + 20.6, 0.0, 0.0)
    assert len(case.p.getPath(start)) > 3
    marker = case.p.current_path
    case.p.getRouteUsage()
    assert np.array_equal(case.p.current_path, marker)


def test_non_seed_local_minimum_gets_zero_nan_none(dymu):
    n, goal = 24, (6, 6)
    p = dymu.Planner(risk_distance=RD)
    try:
        assert p.initGlobalLayer(RES, 0.5, n, n)
        assert p.setCostMap(np.ones((n, n)))
        assert p.setGoal((float(goal[0]), float(goal[1]), 0.0, 0.0))
        T = np.full((n, n), 5.0)
        T[goal[1], goal[0]] = 0.0
        T[10:, 10:] = 7.0
        T[15, 15] = 1.0  # a local minimum that is no seed, lower than most of the map
        assert p.loadTotalCostMap(T)
        w = np.arange(n * n, dtype=np.uint32).reshape(n, n) * 7919
        got = p.getRouteUsage(weights=w)
        want = ref.route_usage(T, [goal + (0.0,)], w)
        assert same(got, want) is None, same(got, want)
        near = np.zeros((n, n), dtype=bool)
        near[5:8, 5:8] = True
        assert (got["sink"][near] == 0).all() and (got["sink"][~near] == NONE).all()
        assert (got["usage"][~near] == 0).all() and np.isnan(got["far"][~near]).all()
        assert got["catchment"][0] == w[near].sum() and got["far"][6, 6] == 5.0
    finally:
        p.close()


def test_arguments(dymu):
    p = dymu.Planner(risk_distance=RD)
    try:
        assert p.initGlobalLayer(RES, 0.5, 8, 8)
        assert p.setCostMap(np.ones((8, 8)))
        with pytest.raises(ValueError):
            p.getRouteUsage(weights=np.ones((3, 3), dtype=np.uint32))
        with pytest.raises(ValueError):
            p.getRouteUsage(weights=np.ones((8, 8)))  # not integers
        with pytest.raises(ValueError):
            p.getRouteUsage(weights=np.full((8, 8), -1))
        with pytest.raises(ValueError):
            p.getRouteUsage(weights=np.full((8, 8), 2 ** 32, dtype=np.uint64))
        with pytest.raises(ValueError):
            p.getRouteUsage(outputs=("usage", "hops"))
        with pytest.raises(ValueError):
            p.getRouteUsage(outputs=())
        with pytest.raises(dymu.DymuError):
            p.getRouteUsageTo(0)  # no batch
        got = p.getRouteUsage()  # no goal: nothing has a route, no catchment
        assert (got["sink"] == NONE).all() and (got["usage"] == 0).all()
        assert np.isnan(got["far"]).all() and got["catchment"].shape == (0,)
    finally:
        p.close()


def test_flat_abi_and_symbols(dymu, oracle):
    fim, pl = dymu.load_fim(), dymu.load_planner()
    for n in ("dymu_route_usage_device", "dymu_route_usage_workspace", "dymu_last_route_usage_ms",
              "dymu_last_route_usage_stages", "dymu_last_route_usage_round_ms"):
        assert hasattr(fim, n) and n in dymu.FIM_SYMBOLS, n
    for n in ("dymu_planner_get_route_usage", "dymu_planner_get_route_usage_to"):
        assert hasattr(pl, n) and n in dymu.PLANNER_SYMBOLS, n
    o = dymu.DymuUsageOut()
    assert fim.dymu_route_usage_device(None, None, 8, 8, 8, None, 0, None, 0, o, None, None, 0,
                                       None, None) == -1
    # the workspace: the counters and two 4-byte entries a cell; 16 more for usage, 8 for far
    w = dymu.Engine.usage_out
    ws = lambda out=None: fim.dymu_route_usage_workspace(100, 50, out)  # noqa: E731
    n = 5000
    assert 8 * n <= ws(w(100, sink=1)) < 8 * n + 4096
    assert ws(w(100, sink=1, far=1)) - ws(w(100, sink=1)) in range(8 * n, 8 * n + 256)
    assert ws(w(100, usage=1)) - ws(w(100, sink=1)) in range(16 * n, 16 * n + 512)
    assert ws() == ws(w(100, usage=1, far=1, sink=1)) <= 32 * n + 4096
    assert fim.dymu_route_usage_workspace(0, 50, None) == 0
    assert fim.dymu_route_usage_workspace(65536, 32768, None) == 0
    # the flat ABI on one loaded map
    c = single_goal_case(dymu, oracle, "97x61", 0.02)
    try:
        n = c.nx * c.ny
        usage = np.full(n, 77, dtype=np.uint64)
        far = np.full(n, -5.0)
        cat = np.full(3, 99, dtype=np.uint64)
        rounds = ctypes.c_uint32(7)
        out = w(0, usage=usage.ctypes.data, far=far.ctypes.data)
        h = c.p.h
        assert pl.dymu_planner_get_route_usage(h, None, 0, out, cat.ctypes.data, 3, rounds) == 0
        want = ref.route_usage(c.T, c.seeds)
        assert usage.tobytes() == want["usage"].tobytes() and far.tobytes() == want["far"].tobytes()
        assert cat.tolist() == [int(want["catchment"][0]), 0, 0] and rounds.value == 0
        # argument errors: nothing is written
        usage[:] = 77
        cat[:] = 99
        assert pl.dymu_planner_get_route_usage(h, None, 0, out, cat.ctypes.data, 0, None) == -1
        assert pl.dymu_planner_get_route_usage(h, None, 0, dymu.DymuUsageOut(), None, 0, None) == -1
        assert pl.dymu_planner_get_route_usage(h, None, 0, None, cat.ctypes.data, 3, None) == -1
        assert pl.dymu_planner_get_route_usage(None, None, 0, out, None, 0, None) == -1
        assert pl.dymu_planner_get_route_usage_to(h, 0, None, out, None, 0, None) == -1
        assert (usage == 77).all() and (cat == 99).all()
    finally:
        c.p.close()
