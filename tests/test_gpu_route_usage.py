"""getRouteUsage on the device (csrc/usage_kernels.hip): how much of the map
drains through every cell, by the reverse of getRouteFields' pointer doubling -- 64-bit
integer atomic adds into a double-buffered sum, a 64-bit atomic maximum in place.  Every
output is an integer or a maximum over bit patterns, so every comparison is byte for byte:
against the planner's host twin on the engine's own map (a second planner that never creates
an engine and holds the device's T), against tests/usage_ref.py, and between two device
calls.  A case's maps and references are computed once and shared by its tests."""
import ctypes

import numpy as np
import pytest

import usage_ref

pytestmark = pytest.mark.gpu

RD = 0.5
RES = 1.0
HEADING = 1.25
NONE = 0xFFFFFFFF
CASES = {"96x96": (96, 96, (70, 60)), "97x61": (97, 61, (70, 40)),
         # more cells than one stride of the capped round grid (8192 x 256)
         "2049x1025": (2049, 1025, (1500, 700))}
MAPS = ("usage", "far", "sink")
KEYS = MAPS + ("catchment",)
DTYPES = {"usage": np.uint64, "far": np.float64, "sink": np.uint32, "catchment": np.uint64}
CANARY = {"usage": 0xA5A5A5A5A5A5A5A5, "far": -12345.0, "sink": 0xA5A5A5A5}


class Case:
    pass


def check_same(a, b, keys=KEYS):
    for k in keys:
        d, h = a[k], b[k]
        assert d.dtype == DTYPES[k] and h.dtype == DTYPES[k] and d.shape == h.shape, k
        if d.tobytes() != h.tobytes():
            view = np.uint32 if d.dtype == np.uint32 else np.uint64
            bad = np.argwhere(d.view(view) != h.view(view))
            raise AssertionError((k, len(bad), bad[:4].tolist()))


def host_twin(dymu, F, T, goal=None, goals=None, offsets=None):
    """A planner without an engine that holds the map T: its calls take the host route."""
    ny, nx = F.shape
    h = dymu.Planner(risk_distance=RD)
    assert h.initGlobalLayer(RES, 0.5, nx, ny)
    assert h.setCostMap(np.where(np.isfinite(F), F, -1.0))
    assert h.setGoals(goals, offsets) if goals else h.setGoal((goal[0], goal[1], 0.0, HEADING))
    assert h.loadTotalCostMap(T)
    return h


def weights_for(nx, ny):
    rng = np.random.default_rng(7)
    return rng.integers(0, 2 ** 32, size=(ny, nx), dtype=np.uint64).astype(np.uint32)


def build_case(dymu, oracle, shape, obst):
    nx, ny, goal = CASES[shape]
    c = Case()
    c.shape, c.obst, c.nx, c.ny, c.goal = shape, obst, nx, ny, goal
    c.F = oracle.synth_speed(nx, ny, seed=21, obst_frac=obst, goal=goal)
    c.w = weights_for(nx, ny)
    p = dymu.Planner(risk_distance=RD)
    assert p.initGlobalLayer(RES, 0.5, nx, ny)
    assert p.setCostMap(np.where(np.isfinite(c.F), c.F, -1.0))
    assert p.setGoal((goal[0], goal[1], 0.0, HEADING))
    assert p.computeEntireTotalCostMap()
    c.dev = p.getRouteUsage()
    c.on_device, c.kernel_ms = p.lastPathsOnDevice(), p.lastPathsKernelMs()
    c.dev2 = p.getRouteUsage()
    c.dev_w = p.getRouteUsage(weights=c.w)
    c.hops = p.getRouteFields(outputs=("axis", "diag"))
    c.T = p.totalCostRaw()
    c.h = host_twin(dymu, c.F, c.T, goal=goal)
    c.host = c.h.getRouteUsage()
    c.host_w = c.h.getRouteUsage(weights=c.w)
    c.host_on_device, c.host_ms = c.h.lastPathsOnDevice(), c.h.lastPathsKernelMs()
    c.p = p
    return c


@pytest.fixture(scope="module", params=[(s, o) for s in ("96x96", "97x61") for o in (0.0, 0.02)],
                ids=lambda p: f"{p[0]}-obst{p[1]}")
def case(request, dymu, oracle):
    c = build_case(dymu, oracle, *request.param)
    yield c
    c.p.close()
    c.h.close()


def device_equals_host_and_reference(case, unit_reference=True):
    assert case.on_device and case.kernel_ms > 0
    assert not case.host_on_device and case.host_ms == 0 and case.host["rounds"] == 0
    assert 1 <= case.dev["rounds"] <= 32
    check_same(case.dev, case.host)
    check_same(case.dev_w, case.host_w)
    seeds = [case.goal + (0.0,)]
    if unit_reference:
        check_same(case.dev, usage_ref.route_usage(case.T, seeds))
    check_same(case.dev_w, usage_ref.route_usage(case.T, seeds, case.w))
    # two device calls give byte-identical outputs
    assert case.dev["rounds"] == case.dev2["rounds"] == case.dev_w["rounds"]
    check_same(case.dev, case.dev2)
    # on a converged map exactly the finite cells have a route, and the goal drains them all
    has = case.dev["sink"] != NONE
    assert np.array_equal(has, np.isfinite(case.T)) and (case.dev["sink"][has] == 0).all()
    gi, gj = case.goal
    assert case.dev["usage"][gj, gi] == np.isfinite(case.T).sum() == case.dev["catchment"][0]
    assert case.dev["far"][gj, gi] == case.T[has].max()
    hops = case.hops["axis"].astype(np.int64) + case.hops["diag"]
    print(f"{case.shape} obst {case.obst}: rounds {case.dev['rounds']}, longest route "
          f"{int(hops.max())} hops, kernels {case.kernel_ms:.3f} ms")
    assert 2 ** case.dev["rounds"] >= hops.max()


def test_device_equals_host_twin_and_reference(case):
    device_equals_host_and_reference(case)


def test_grid_larger_than_one_stride_of_the_round_grid(dymu, oracle):
    """2049 x 1025 cells against 8192 x 256 lanes: the strided loops and the per-round
    counters.  The plain-Python reference is run once, with the weights (2e6 cells take it a
    few seconds); the unit-weight call is held against the host twin."""
    c = build_case(dymu, oracle, "2049x1025", 0.02)
    try:
        assert c.nx * c.ny > 8192 * 256
        device_equals_host_and_reference(c, unit_reference=False)
        assert c.dev["rounds"] >= 10
    finally:
        c.p.close()
        c.h.close()


def test_subsets_of_outputs(case):
    p = case.p
    a = p.getRouteUsage(outputs=("catchment",))
    assert p.lastPathsOnDevice() and sorted(a) == ["catchment", "rounds"]
    assert a["catchment"].tobytes() == case.dev["catchment"].tobytes()
    b = p.getRouteUsage(weights=case.w, outputs=("far", "usage"))
    assert p.lastPathsOnDevice() and sorted(b) == ["far", "rounds", "usage"]
    check_same(b, case.dev_w, ("far", "usage"))
    c = p.getRouteUsage(weights=case.w, host=True)
    assert not p.lastPathsOnDevice() and p.lastPathsKernelMs() == 0
    check_same(c, case.host_w)


class Arena:
    """Device buffers of one test, freed together."""

    def __init__(self, engine):
        self.engine, self.ptrs = engine, []

    def put(self, a):
        a = np.ascontiguousarray(a)
        d = self.alloc(a.nbytes)
        self.engine.h2d(d, a)
        return d

    def alloc(self, nbytes, cached=False):
        d = (self.engine.alloc_cached if cached else self.engine.alloc)(max(nbytes, 8))
        self.ptrs.append(d)
        return d

    def get(self, d, shape, dtype):
        a = np.empty(shape, dtype=dtype)
        self.engine.d2h(a, d)
        return a

    def close(self):
        for d in self.ptrs:
            self.engine.free(d)


@pytest.fixture()
def arena(engine):
    a = Arena(engine)
    yield a
    a.close()


def padded(a, ld, fill):
    out = np.full((a.shape[0], ld), fill, dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out


def engine_usage(dymu, engine, arena, T, seeds, want=KEYS, weights=None, ld_t=None, ld_w=None,
                 ld_o=None):
    """Engine.route_usage on uploaded copies at the given pitches: a dict of the outputs
    named in `want` cropped to nx columns, the rounds, the workspace bytes; the buffers of
    the maps not asked for and the pad columns of the others must keep their canary."""
    ny, nx = T.shape
    ld_t, ld_w, ld_o = ld_t or nx, ld_w or nx, ld_o or nx
    dT = arena.put(padded(T, ld_t, -7.0))  # the pad lies below every value of T: never read
    dW = arena.put(padded(weights, ld_w, 0x5A5A5A5A)) if weights is not None else 0
    bufs = {k: arena.put(np.full((ny, ld_o), CANARY[k], dtype=DTYPES[k])) for k in MAPS}
    out = dymu.Engine.usage_out(ld_o, **{k: bufs[k] for k in MAPS if k in want})
    # the catchment needs the sums: the size is asked with a usage pointer
    sized = dymu.Engine.usage_out(ld_o, **{k: bufs[k] for k in MAPS
                                           if k in want or (k == "usage" and "catchment" in want)})
    nbytes = engine.route_usage_workspace(nx, ny, sized)
    assert nbytes > 0
    ws = arena.alloc(nbytes, cached=True)
    r = engine.route_usage(dT, nx, ny, ld_t, seeds, out, ws, nbytes, weight=dW, weight_ld=ld_w,
                           catchment="catchment" in want)
    assert engine.last_route_usage_ms() > 0 and len(engine.last_route_usage_stages()) == 3
    assert len(engine.last_route_usage_round_ms()) >= r["rounds"]
    res = {"rounds": r["rounds"], "workspace": nbytes}
    if "catchment" in want:
        res["catchment"] = r["catchment"]
    for k in MAPS:
        a = arena.get(bufs[k], (ny, ld_o), DTYPES[k])
        if k in want:
            assert (a[:, nx:] == DTYPES[k](CANARY[k])).all(), k  # the sentinel in the pad columns
            res[k] = np.ascontiguousarray(a[:, :nx])
        else:
            assert (a == DTYPES[k](CANARY[k])).all(), k
    return res


@pytest.mark.parametrize("nx", [1025, 1000])
def test_chain_carries_past_32_bits(dymu, engine, arena, nx):
    """ny = 1, T[i] = i, the seed at 0: the far end is nx - 1 hops from the root -- exactly
    2^10 for nx = 1025, no power of two for nx = 1000 -- and every weight is 2^32 - 1."""
    T = np.arange(nx, dtype=np.float64).reshape(1, nx)
    w = np.full((1, nx), 0xFFFFFFFF, dtype=np.uint32)
    got = engine_usage(dymu, engine, arena, T, [(0, 0, 0.0)], weights=w)
    want = np.array([(nx - i) * (2 ** 32 - 1) for i in range(nx)], dtype=np.uint64)
    assert got["usage"][0].tobytes() == want.tobytes()
    assert (got["far"] == nx - 1).all() and (got["sink"] == 0).all()
    assert int(got["catchment"][0]) == nx * (2 ** 32 - 1)
    assert 2 ** got["rounds"] >= nx - 1 > 2 ** (got["rounds"] - 2)
    check_same(got, usage_ref.route_usage(T, [(0, 0, 0.0)], w))


def test_constant_speed_map_many_senders_per_cell(dymu, engine, arena):
    """96 x 96 at constant speed without obstacles: thousands of cells feed the few cells
    around the goal in the same round."""
    N, goal = 96, (40, 52)
    F = np.full((N, N), 2.0)
    dF, dT = arena.put(F), arena.alloc(F.nbytes)
    engine.solve_seeds_device(dF, dT, N, N, N, [goal + (0.0,)])
    T = arena.get(dT, (N, N), np.float64)
    w = weights_for(N, N)
    for weights in (None, w):
        got = engine_usage(dymu, engine, arena, T, [goal + (0.0,)], weights=weights)
        check_same(got, usage_ref.route_usage(T, [goal + (0.0,)], weights))
    assert got["catchment"][0] == w.astype(np.uint64).sum()
    # the goal's children carry the whole map between them, and one round feeds it from many
    par, _ = usage_ref.forest(T, [goal + (0.0,)])
    g = goal[1] * N + goal[0]
    kids = np.flatnonzero(par == g)
    u = got["usage"].ravel().astype(object)
    assert len(kids) >= 4 and u[kids].sum() == u[g] - int(w[goal[1], goal[0]])


def test_pitches_and_sentinels(case, dymu, engine, arena):
    nx = case.nx
    seeds = [case.goal + (0.0,)]
    got = engine_usage(dymu, engine, arena, case.T, seeds, weights=case.w, ld_t=nx + 5,
                       ld_w=nx + 3, ld_o=nx + 7)
    check_same(got, case.dev_w)  # the planner's call, byte for byte
    assert got["rounds"] == case.dev_w["rounds"]


def test_goal_set_catchments(dymu, oracle, engine, arena):
    nx, ny, _ = CASES["97x61"]
    goals_ij = [(70, 40), (12, 9), (30, 50), (68, 38)]
    offsets = [0.0, 6.5, 3.25, 50.0]  # three seeds with offsets (one of 0), the last dominated
    F = oracle.synth_speed(nx, ny, seed=21, obst_frac=0.02, goal=goals_ij[0])
    for gi, gj in goals_ij:
        blk = F[gj - 1:gj + 2, gi - 1:gi + 2]
        blk[~np.isfinite(blk)] = 3.0
    goals = [(float(i), float(j), 0.0, 0.1 * k) for k, (i, j) in enumerate(goals_ij)]
    seeds = [(i, j, t0) for (i, j), t0 in zip(goals_ij, offsets)]
    w = weights_for(nx, ny)
    p = dymu.Planner(risk_distance=RD)
    h = None
    try:
        assert p.initGlobalLayer(RES, 0.5, nx, ny)
        assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
        assert p.setGoals(goals, offsets)
        assert p.computeEntireTotalCostMap()
        dev = p.getRouteUsage(weights=w)
        assert p.lastPathsOnDevice() and p.lastPathsKernelMs() > 0
        T = p.totalCostRaw()
        h = host_twin(dymu, F, T, goals=goals, offsets=offsets)
        host = h.getRouteUsage(weights=w)
        assert not h.lastPathsOnDevice()
        check_same(dev, host)
        check_same(dev, usage_ref.route_usage(T, seeds, w))
        has = dev["sink"] != NONE
        assert np.array_equal(has, np.isfinite(T))
        assert set(np.unique(dev["sink"][has])) == {0, 1, 2}
        assert int(dev["catchment"].astype(object).sum()) == int(w[has].astype(object).sum())
        assert dev["catchment"][3] == 0 and (dev["catchment"][:3] > 0).all()
        for k, (gi, gj) in enumerate(goals_ij[:3]):
            assert dev["usage"][gj, gi] == dev["catchment"][k]
            assert int(dev["catchment"][k]) == int(w[dev["sink"] == k].astype(object).sum())
        # the engine entry on the same map gives the planner's bytes
        check_same(engine_usage(dymu, engine, arena, T, seeds, weights=w), dev)
    finally:
        p.close()
        if h:
            h.close()


def local_minimum_map():
    n, goal = 24, (6, 6)
    T = np.full((n, n), 5.0)
    T[goal[1], goal[0]] = 0.0
    T[10:, 10:] = 7.0
    T[15, 15] = 1.0  # a local minimum that is no seed, lower than most of the map
    T[0, 23] = np.inf
    T[1, 23] = np.nan
    near = np.zeros((n, n), dtype=bool)
    near[5:8, 5:8] = True
    return T, goal, near


def test_non_seed_local_minimum_gets_zero_nan_none(dymu, engine, arena):
    T, goal, near = local_minimum_map()
    w = np.arange(T.size, dtype=np.uint32).reshape(T.shape) * 7919
    got = engine_usage(dymu, engine, arena, T, [goal + (0.0,)], weights=w)
    check_same(got, usage_ref.route_usage(T, [goal + (0.0,)], w))
    assert (got["sink"][near] == 0).all() and (got["sink"][~near] == NONE).all()
    assert (got["usage"][~near] == 0).all() and np.isnan(got["far"][~near]).all()
    assert got["catchment"][0] == w[near].sum() and got["far"][6, 6] == 5.0


def test_null_output_combinations(case, dymu, engine, arena):
    seeds = [case.goal + (0.0,)]
    full = engine_usage(dymu, engine, arena, case.T, seeds, weights=case.w)
    check_same(full, case.dev_w)
    sizes = {}
    for want in (("usage",), ("far",), ("sink",), ("catchment",), ("far", "sink"),
                 ("usage", "far"), ("sink", "catchment")):
        got = engine_usage(dymu, engine, arena, case.T, seeds, want=want, weights=case.w)
        check_same(got, full, want)
        assert got["rounds"] == full["rounds"]
        sizes[want] = got["workspace"]
    n = case.nx * case.ny
    assert sizes[("sink",)] < sizes[("far",)] < sizes[("usage",)] < full["workspace"]
    assert sizes[("far", "sink")] == sizes[("far",)]
    assert sizes[("catchment",)] == sizes[("usage",)] == sizes[("sink", "catchment")]
    assert sizes[("usage", "far")] == full["workspace"]
    assert 8 * n <= sizes[("sink",)] < 8 * n + 4096 and full["workspace"] < 32 * n + 4096


def test_batch_plane_equals_the_goal_solved_alone(dymu, oracle):
    nx, ny, goal = CASES["96x96"]
    F = oracle.synth_speed(nx, ny, seed=21, obst_frac=0.02, goal=goal)
    other = (20, 15)
    blk = F[other[1] - 1:other[1] + 2, other[0] - 1:other[0] + 2]
    blk[~np.isfinite(blk)] = 3.0
    w = weights_for(nx, ny)

    def planner():
        p = dymu.Planner(risk_distance=RD)
        o = dymu.DymuOpts(-1, 0, 0, 0, 0, 0, 0, 0, 1)  # deterministic: both maps the same bits
        assert p._lib.dymu_planner_set_engine_options(p.h, ctypes.byref(o)) == 0
        assert p.initGlobalLayer(RES, 0.5, nx, ny)
        assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
        return p

    targets = [(goal[0], goal[1], 0.0, 0.0), (other[0], other[1], 0.0, 0.3)]
    pb = planner()
    try:
        assert pb.computeTotalCostMaps(targets)
        for b in (1, 0):
            dev = pb.getRouteUsageTo(b, weights=w)
            assert pb.lastPathsOnDevice() and pb.lastPathsKernelMs() > 0
            ps = planner()
            try:
                assert ps.setGoal(targets[b])
                assert ps.computeEntireTotalCostMap()
                assert ps.totalCostRaw().tobytes() == pb.batchTotalCost(b).tobytes()
                alone = ps.getRouteUsage(weights=w)
                assert ps.lastPathsOnDevice()
            finally:
                ps.close()
            check_same(dev, alone)
            assert dev["catchment"].shape == (1,)
            g = (int(targets[b][0]), int(targets[b][1]))
            assert dev["usage"][g[1], g[0]] == dev["catchment"][0] > 0
        with pytest.raises(dymu.DymuError):
            pb.getRouteUsageTo(2)
    finally:
        pb.close()


def test_argument_errors_write_nothing(case, dymu, engine, arena):
    nx, ny = case.nx, case.ny
    seeds = [case.goal + (0.0,)]
    dT = arena.put(case.T)
    dW = arena.put(case.w)
    dU = arena.put(np.full((ny, nx), CANARY["usage"], dtype=np.uint64))
    dS = arena.put(np.full((ny, nx), CANARY["sink"], dtype=np.uint32))
    out = dymu.Engine.usage_out(nx, usage=dU, sink=dS)
    need = engine.route_usage_workspace(nx, ny, out)
    ws = arena.alloc(need, cached=True)
    engine.h2d(ws, np.full(need // 8, 0x1111111111111111, dtype=np.uint64))
    small = dymu.Engine.usage_out(nx, sink=dS)
    need_small = engine.route_usage_workspace(nx, ny, small)
    assert need_small < need
    bad = [dict(workspace_bytes=need - 1), dict(workspace=0), dict(workspace=ws + 8),
           dict(ld=nx - 1), dict(nx=0), dict(dT=0), dict(seeds=[]), dict(seeds=[(nx, 1, 0.0)]),
           dict(seeds=[(1, 1, -1.0)]), dict(weight_ld=nx - 1),
           dict(out=dymu.Engine.usage_out(nx - 1, usage=dU)),
           dict(out=dymu.Engine.usage_out(nx), catchment=False),  # nothing asked for
           # a catchment needs the sums: the size of a call without them is too small
           dict(out=small, workspace_bytes=need_small, catchment=True)]
    for kw in bad:
        a = dict(dT=dT, nx=nx, ny=ny, ld=nx, seeds=seeds, out=out, workspace=ws,
                 workspace_bytes=need, weight=dW, weight_ld=nx, catchment=True)
        a.update(kw)
        with pytest.raises(dymu.DymuError) as e:
            engine.route_usage(**a)
        assert e.value.status == -1, kw
    # nothing was written: not the outputs, not the workspace
    assert (arena.get(dU, (ny, nx), np.uint64) == np.uint64(CANARY["usage"])).all()
    assert (arena.get(dS, (ny, nx), np.uint32) == CANARY["sink"]).all()
    assert (arena.get(ws, (need // 8,), np.uint64) == 0x1111111111111111).all()
    # ... and the same call without the error runs
    r = engine.route_usage(dT, nx, ny, nx, seeds, out, ws, need, weight=dW, weight_ld=nx)
    assert r["rounds"] == case.dev_w["rounds"]
    assert arena.get(dU, (ny, nx), np.uint64).tobytes() == case.dev_w["usage"].tobytes()
    assert r["catchment"].tobytes() == case.dev_w["catchment"].tobytes()
