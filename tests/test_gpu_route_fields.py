"""getRouteFields on the device (csrc/route_kernels.hip): every cell's
node route to the goal by synchronous pointer doubling, against the planner's host twin on
the engine's own map -- a second planner that never creates an engine and holds the
device's T.  sink, axis, diag, length, vmin and vmax are compared byte for byte.

The integrals add the same terms in different orders (the host each cell from its parent,
the device in a doubling tree).  Each side is a summation of at most `hops` terms and lies
within (hops - 1) * 2^-53 * sum|w| of the exact sum (Higham, Accuracy and Stability of
Numerical Algorithms, (4.4), to first order; the products w = v * seg are formed once and
are the same bits on both sides), so the two differ by at most
    1.01 * hops * 2^-52 * I_abs,   I_abs = the host-side integral of |v| along the route,
a derived bound, not a measured tolerance.  A case's maps and references are computed once
and shared by its tests."""
import numpy as np
import pytest

import route_ref

pytestmark = pytest.mark.gpu

RD = 0.5
RES = 1.0
HEADING = 1.25
NONE = 0xFFFFFFFF
CASES = {"96x96": (96, 96, (70, 60)), "97x61": (97, 61, (70, 40)),
         # more cells than one stride of the capped round grid (8192 x 256)
         "2049x1025": (2049, 1025, (1500, 700))}
EXACT = ("sink", "axis", "diag", "length", "vmin", "vmax")


class Case:
    pass


def elevation(nx, ny):
    j, i = np.mgrid[0:ny, 0:nx].astype(float)
    return 0.3 * np.sin(0.3 * i) + 0.1 * np.cos(0.2 * j) + 0.01 * i - 0.2


def host_twin(dymu, F, T, goal=None, goals=None, offsets=None):
    """A planner without an engine that holds the map T: its calls take the host route."""
    ny, nx = F.shape
    h = dymu.Planner(risk_distance=RD)
    assert h.initGlobalLayer(RES, 0.5, nx, ny)
    assert h.setCostMap(np.where(np.isfinite(F), F, -1.0))
    assert h.setGoals(goals, offsets) if goals else h.setGoal((goal[0], goal[1], 0.0, HEADING))
    assert h.loadTotalCostMap(T)
    return h


def check_exact(dev, host, keys=EXACT):
    for k in keys:
        d, h = dev[k], host[k]
        assert d.dtype == h.dtype and d.shape == h.shape, k
        if d.tobytes() != h.tobytes():
            bad = np.argwhere(d.view(np.uint64 if d.dtype == np.float64 else np.uint32) !=
                              h.view(np.uint64 if h.dtype == np.float64 else np.uint32))
            raise AssertionError((k, len(bad), bad[:4].tolist()))


def check_integral(dev, host, i_abs, what=""):
    """|device - host| <= 1.01 * hops * 2^-52 * I_abs per cell, NaN exactly where the host's is"""
    hops = host["axis"].astype(np.float64) + host["diag"]
    worst = 0.0
    for f in range(dev["integral"].shape[0]):
        d, h = dev["integral"][f], host["integral"][f]
        assert np.array_equal(np.isnan(d), np.isnan(h)), (what, f)
        has = ~np.isnan(h)
        assert np.array_equal(has, host["sink"] != NONE)
        err = np.abs(d[has] - h[has])
        bound = 1.01 * hops[has] * 2.0 ** -52 * i_abs[f][has]
        # a bound of 0 (no hop, or nothing but zeros summed) allows no difference
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0),
                         np.where(err > 0, np.inf, 0.0))
        worst = max(worst, float(ratio.max(initial=0.0)))
    print(f"{what}: largest |device - host| / bound = {worst:.4f}")
    assert worst <= 1.0, f"{what}: largest |device - host| / bound = {worst:.4f}"
    return worst


def abs_integrals(h, fields_abs):
    """I_abs per field from the twin: the integral of |v| along the same routes"""
    r = h.getRouteFields(fields=fields_abs, outputs=("sink", "integral"), host=True)
    return [np.where(r["sink"] != NONE, r["integral"][f], 0.0) for f in range(len(fields_abs))]


def build_case(dymu, oracle, shape, obst):
    nx, ny, goal = CASES[shape]
    c = Case()
    c.shape, c.obst, c.nx, c.ny, c.goal = shape, obst, nx, ny, goal
    c.F = oracle.synth_speed(nx, ny, seed=21, obst_frac=obst, goal=goal)
    c.elev = elevation(nx, ny)
    p = dymu.Planner(risk_distance=RD)
    assert p.initGlobalLayer(RES, 0.5, nx, ny)
    assert p.setCostMap(np.where(np.isfinite(c.F), c.F, -1.0))
    assert p.setGoal((goal[0], goal[1], 0.0, HEADING))
    assert p.computeEntireTotalCostMap()
    c.dev = p.getRouteFields(fields=["speed", c.elev])
    c.on_device, c.kernel_ms = p.lastPathsOnDevice(), p.lastPathsKernelMs()
    c.dev2 = p.getRouteFields(fields=["speed", c.elev])
    c.T = p.totalCostRaw()
    c.h = host_twin(dymu, c.F, c.T, goal=goal)
    c.host = c.h.getRouteFields(fields=["speed", c.elev])
    c.host_on_device, c.host_ms = c.h.lastPathsOnDevice(), c.h.lastPathsKernelMs()
    c.i_abs = abs_integrals(c.h, ["speed", np.abs(c.elev)])  # the speed is positive
    c.p = p
    return c


@pytest.fixture(scope="module", params=[(s, o) for s in ("96x96", "97x61") for o in (0.0, 0.02)],
                ids=lambda p: f"{p[0]}-obst{p[1]}")
def case(request, dymu, oracle):
    c = build_case(dymu, oracle, *request.param)
    yield c
    c.p.close()
    c.h.close()


def device_equals_host(case):
    assert case.on_device and case.kernel_ms > 0
    assert not case.host_on_device and case.host_ms == 0 and case.host["rounds"] == 0
    assert 1 <= case.dev["rounds"] <= 32
    check_exact(case.dev, case.host)
    check_integral(case.dev, case.host, case.i_abs, f"{case.shape} obst {case.obst}")
    has = case.dev["sink"] != NONE
    assert np.array_equal(has, np.isfinite(case.T)) and (case.dev["sink"][has] == 0).all()
    hops = case.dev["axis"].astype(np.int64) + case.dev["diag"]
    print(f"{case.shape} obst {case.obst}: rounds {case.dev['rounds']}, longest route "
          f"{int(hops.max())} hops, kernels {case.kernel_ms:.3f} ms")
    assert 2 ** case.dev["rounds"] >= hops.max()
    # two device calls give byte-identical outputs
    assert case.dev["rounds"] == case.dev2["rounds"]
    check_exact(case.dev, case.dev2, EXACT + ("integral",))


def test_device_equals_host_twin(case):
    device_equals_host(case)
    # ... and both are the plain-Python definition
    ref = route_ref.route_fields(case.T, RES, [case.goal + (0.0,)], [case.F, case.elev])
    check_exact(case.host, ref, EXACT + ("integral",))


def test_grid_larger_than_one_stride_of_the_round_grid(dymu, oracle):
    """2049 x 1025 cells against 8192 x 256 lanes: the strided loop and the per-round
    counters.  The host side is the planner's host twin only."""
    c = build_case(dymu, oracle, "2049x1025", 0.02)
    try:
        assert c.nx * c.ny > 8192 * 256
        device_equals_host(c)
        assert c.dev["rounds"] >= 10
    finally:
        c.p.close()
        c.h.close()


def test_subsets_of_outputs_and_fields(case):
    p = case.p
    a = p.getRouteFields(outputs=("sink",))
    assert p.lastPathsOnDevice() and sorted(a) == ["rounds", "sink"]
    assert a["sink"].tobytes() == case.dev["sink"].tobytes()
    b = p.getRouteFields(fields=[case.elev], outputs=("length", "vmax", "integral"))
    assert p.lastPathsOnDevice() and sorted(b) == ["integral", "length", "rounds", "vmax"]
    assert b["length"].tobytes() == case.dev["length"].tobytes()
    assert b["vmax"][0].tobytes() == case.dev["vmax"][1].tobytes()
    assert b["integral"][0].tobytes() == case.dev["integral"][1].tobytes()
    c = p.getRouteFields(fields=["speed", case.elev], host=True)
    assert not p.lastPathsOnDevice() and p.lastPathsKernelMs() == 0
    check_exact(c, case.host, EXACT + ("integral",))


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


def engine_route(dymu, engine, arena, T, seeds, fields, want, ld_t=None, ld_f=None, ld_o=None,
                 canary=True):
    """Engine.route_fields on uploaded copies at the given pitches: a dict of the outputs
    named in `want` (per-field ones stacked), the rounds, and the buffers of the outputs
    not asked for, which were filled with a canary."""
    ny, nx = T.shape
    ld_t, ld_f, ld_o = ld_t or nx, ld_f or nx, ld_o or nx
    dT = arena.put(padded(T, ld_t, -7.0))  # the pad lies below every value of T: never read
    dfs = [(arena.put(padded(np.ascontiguousarray(f, dtype=np.float64), ld_f, np.nan)), ld_f)
           for f in fields]
    nf = len(fields)
    kinds = {"sink": np.uint32, "axis": np.uint32, "diag": np.uint32, "length": np.float64}
    bufs, kw = {}, {}
    for name, dt in kinds.items():
        bufs[name] = arena.put(np.full((ny, ld_o), 0xA5A5A5A5 if dt == np.uint32 else -12345.0,
                                       dtype=dt))
        if name in want:
            kw[name] = bufs[name]
    for name in ("integral", "vmin", "vmax"):
        bufs[name] = [arena.put(np.full((ny, ld_o), -12345.0)) for _ in range(nf)]
        if name in want:
            kw[name] = bufs[name]
    out = dymu.Engine.route_out(ld_o, **kw)
    nbytes = engine.route_fields_workspace(nx, ny, nf, out)
    assert nbytes > 0
    ws = arena.alloc(nbytes, cached=True)
    rounds = engine.route_fields(dT, nx, ny, ld_t, RES, seeds, dfs, out, ws, nbytes)
    assert engine.last_route_fields_ms() > 0 and len(engine.last_route_fields_stages()) == 3
    res, rest = {"rounds": rounds}, {}
    for name, dt in kinds.items():
        a = arena.get(bufs[name], (ny, ld_o), dt)
        (res if name in want else rest)[name] = a
    for name in ("integral", "vmin", "vmax"):
        a = np.stack([arena.get(b, (ny, ld_o), np.float64) for b in bufs[name]]) if nf else \
            np.zeros((0, ny, ld_o))
        (res if name in want else rest)[name] = a
    # the pad columns of a written output keep the canary too
    for name, a in res.items():
        if name != "rounds" and ld_o > nx and a.size:
            pad = a[..., nx:]
            assert (pad == (0xA5A5A5A5 if a.dtype == np.uint32 else -12345.0)).all(), name
    crop = {k: (np.ascontiguousarray(v[..., :nx]) if k != "rounds" else v) for k, v in res.items()}
    return crop, rest


def test_engine_entry_pitches_canaries_and_workspace(case, dymu, engine, arena):
    nx, ny = case.nx, case.ny
    seeds = [case.goal + (0.0,)]
    allk = EXACT + ("integral",)
    got, _ = engine_route(dymu, engine, arena, case.T, seeds, [case.F, case.elev], allk,
                          ld_t=nx + 5, ld_f=nx + 3, ld_o=nx + 7)
    check_exact(got, case.dev, allk)  # the planner's call, byte for byte
    assert got["rounds"] == case.dev["rounds"]
    # outputs not requested are not written
    want = ("sink", "vmin")
    got, rest = engine_route(dymu, engine, arena, case.T, seeds, [case.elev], want, ld_o=nx + 2)
    assert got["sink"].tobytes() == case.dev["sink"].tobytes()
    assert got["vmin"][0].tobytes() == case.dev["vmin"][1].tobytes()
    for name, a in rest.items():
        assert (a == (0xA5A5A5A5 if a.dtype == np.uint32 else -12345.0)).all(), name
    # a workspace that is too small, and the other argument errors
    dT = arena.put(case.T)
    dS = arena.alloc(4 * nx * ny)
    out = dymu.Engine.route_out(nx, sink=dS)
    need = engine.route_fields_workspace(nx, ny, 0, out)
    ws = arena.alloc(need, cached=True)
    assert engine.route_fields(dT, nx, ny, nx, RES, seeds, [], out, ws, need) == case.dev["rounds"]
    assert arena.get(dS, (ny, nx), np.uint32).tobytes() == case.dev["sink"].tobytes()
    full = dymu.Engine.route_out(nx, sink=dS, axis=dS)  # asks for more than `need` holds
    assert engine.route_fields_workspace(nx, ny, 0, full) > need
    bad = [dict(out=full), dict(workspace_bytes=need - 1), dict(workspace=0),
           dict(workspace=ws + 8), dict(ld=nx - 1), dict(res=0.0), dict(seeds=[]),
           dict(seeds=[(nx, 1, 0.0)]), dict(seeds=[(1, 1, -1.0)]),
           dict(out=dymu.Engine.route_out(nx - 1, sink=dS)),
           dict(out=dymu.Engine.route_out(nx, sink=dS, vmin=[dS])),  # beyond n_fields
           dict(fields=[(dT, nx - 1)]), dict(fields=[(0, nx)]), dict(fields=[(dT, nx)] * 5)]
    for kw in bad:
        a = dict(dT=dT, nx=nx, ny=ny, ld=nx, res=RES, seeds=seeds, fields=[], out=out,
                 workspace=ws, workspace_bytes=need)
        a.update(kw)
        with pytest.raises(dymu.DymuError) as e:
            engine.route_fields(**a)
        assert e.value.status == -1, kw


def test_goal_set(dymu, oracle):
    nx, ny, _ = CASES["97x61"]
    goals_ij = [(70, 40), (12, 9), (30, 50), (68, 38)]
    offsets = [0.0, 6.5, 0.0, 50.0]  # the last is dominated by the first
    F = oracle.synth_speed(nx, ny, seed=21, obst_frac=0.02, goal=goals_ij[0])
    for gi, gj in goals_ij:
        blk = F[gj - 1:gj + 2, gi - 1:gi + 2]
        blk[~np.isfinite(blk)] = 3.0
    goals = [(float(i), float(j), 0.0, 0.1 * k) for k, (i, j) in enumerate(goals_ij)]
    elev = elevation(nx, ny)
    p = dymu.Planner(risk_distance=RD)
    h = None
    try:
        assert p.initGlobalLayer(RES, 0.5, nx, ny)
        assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
        assert p.setGoals(goals, offsets)
        assert p.computeEntireTotalCostMap()
        dev = p.getRouteFields(fields=[elev, "speed"])
        assert p.lastPathsOnDevice() and p.lastPathsKernelMs() > 0
        T = p.totalCostRaw()
        h = host_twin(dymu, F, T, goals=goals, offsets=offsets)
        host = h.getRouteFields(fields=[elev, "speed"])
        assert not h.lastPathsOnDevice()
        check_exact(dev, host)
        check_integral(dev, host, abs_integrals(h, [np.abs(elev), "speed"]), "goal set")
        has = dev["sink"] != NONE
        assert np.array_equal(has, np.isfinite(T))
        assert set(np.unique(dev["sink"][has])) == {0, 1, 2}
        for k, (gi, gj) in enumerate(goals_ij[:3]):
            assert dev["sink"][gj, gi] == k and dev["axis"][gj, gi] + dev["diag"][gj, gi] == 0
        gi, gj = goals_ij[3]
        assert dev["sink"][gj, gi] == 0 and dev["axis"][gj, gi] + dev["diag"][gj, gi] == 2
        seeds = [(i, j, t0) for (i, j), t0 in zip(goals_ij, offsets)]
        ref = route_ref.route_fields(T, RES, seeds, [elev, F])
        check_exact(host, ref, EXACT + ("integral",))
    finally:
        p.close()
        if h:
            h.close()


def test_batch_planes(dymu, oracle):
    nx, ny, goal = CASES["96x96"]
    F = oracle.synth_speed(nx, ny, seed=21, obst_frac=0.02, goal=goal)
    others = [(20, 15), (48, 80)]
    for o in others:
        blk = F[o[1] - 1:o[1] + 2, o[0] - 1:o[0] + 2]
        blk[~np.isfinite(blk)] = 3.0
    targets = [(goal[0], goal[1], 0.0, 0.0)] + [(o[0], o[1], 0.0, 0.3) for o in others]
    elev = elevation(nx, ny)
    p = dymu.Planner(risk_distance=RD)
    try:
        assert p.initGlobalLayer(RES, 0.5, nx, ny)
        assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
        assert p.computeTotalCostMaps(targets)
        for b in (2, 0, 1):
            dev = p.getRouteFieldsTo(b, fields=["speed", elev])
            assert p.lastPathsOnDevice() and p.lastPathsKernelMs() > 0
            T = p.batchTotalCost(b)
            g = (int(targets[b][0]), int(targets[b][1]))
            h = host_twin(dymu, F, T, goal=g)
            try:
                host = h.getRouteFields(fields=["speed", elev])
                i_abs = abs_integrals(h, ["speed", np.abs(elev)])
            finally:
                h.close()
            check_exact(dev, host)
            check_integral(dev, host, i_abs, f"plane {b}")
            assert dev["axis"][g[1], g[0]] + dev["diag"][g[1], g[0]] == 0
            assert dev["sink"][g[1], g[0]] == 0
            assert (dev["sink"] != NONE).sum() == np.isfinite(T).sum() > 8000
        with pytest.raises(dymu.DymuError):
            p.getRouteFieldsTo(3, fields=[elev])
    finally:
        p.close()


def test_long_chains(dymu, engine, arena):
    """The ~2000-cell serpentine corridor of test_gpu_goal_sets.py: many rounds."""
    N = 128
    F = np.full((N, N), 2.0)
    for q, j in enumerate(range(8, N, 8)):
        F[j, :] = np.inf
        F[j, N - 1 if q % 2 == 0 else 0] = 2.0  # the gap alternates sides
    seeds = [(2, 2, 0.0)]
    dF, dT = arena.put(F), arena.alloc(F.nbytes)
    engine.solve_seeds_device(dF, dT, N, N, N, seeds)
    T = arena.get(dT, (N, N), np.float64)
    elev = elevation(N, N)
    dev, _ = engine_route(dymu, engine, arena, T, seeds, [F, elev], EXACT + ("integral",))
    h = host_twin(dymu, F, T, goal=(2, 2))
    try:
        host = h.getRouteFields(fields=["speed", elev])
        i_abs = abs_integrals(h, ["speed", np.abs(elev)])
    finally:
        h.close()
    check_exact(dev, host)
    check_integral(dev, host, i_abs, "serpentine")
    hops = dev["axis"].astype(np.int64) + dev["diag"]
    print(f"serpentine: rounds {dev['rounds']}, longest route {int(hops.max())} hops")
    assert np.array_equal(dev["sink"] != NONE, np.isfinite(T))
    assert hops.max() > 1000 and dev["rounds"] >= 10
    assert 2 ** dev["rounds"] >= hops.max() > 2 ** (dev["rounds"] - 2)


@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 7), (7, 1), (2, 2)])
def test_tiny_grids(dymu, engine, arena, nx, ny):
    T = np.arange(nx * ny, dtype=np.float64).reshape(ny, nx) * 1.5
    f = elevation(nx, ny) + 1.0
    seeds = [(0, 0, 0.0)]
    dev, _ = engine_route(dymu, engine, arena, T, seeds, [f], EXACT + ("integral",))
    ref = route_ref.route_fields(T, RES, seeds, [f])
    check_exact(dev, ref)
    i_abs = [route_ref.abs_integral(T, RES, seeds, f)]
    check_integral(dev, ref, i_abs, f"{nx}x{ny}")
    assert (dev["sink"] == 0).all() and dev["rounds"] >= 1
    assert (dev["axis"] + dev["diag"]).max() == max(nx, ny) - 1
    # a map with nothing finite but the seed, and one with no root at all
    T2 = np.full((ny, nx), np.inf)
    T2[0, 0] = 0.0
    dev, _ = engine_route(dymu, engine, arena, T2, seeds, [f], EXACT + ("integral",))
    check_exact(dev, route_ref.route_fields(T2, RES, seeds, [f]), EXACT)
    assert dev["sink"][0, 0] == 0 and (dev["sink"].ravel()[1:] == NONE).all()
    dev, _ = engine_route(dymu, engine, arena, T, [(0, 0, 4.0)], [f], EXACT)  # dominated
    assert (dev["sink"] == NONE).all() and np.isnan(dev["length"]).all()
