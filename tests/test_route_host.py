"""getRouteFields without a device: the planner's host route must be tests/route_ref.py bit
for bit -- both take the cells in ascending total cost, each from its parent -- and keep the
definition's properties on converged maps.  No engine is ever created: the maps are the
oracle's FMM maps installed by loadTotalCostMap.  A case is built once and shared."""
import numpy as np
import pytest

import goalset_ref
import route_ref as ref

RD = 0.5
RES = 1.0
NONE = ref.NONE
CASES = {"96x96": (96, 96, (70, 60)), "97x61": (97, 61, (70, 40))}
OFFS = {"96x96": (0.0, 0.0), "97x61": (100.0, 200.0)}  # one grid with an offset
KEYS = ("sink", "axis", "diag", "length", "integral", "vmin", "vmax")


class Case:
    pass


def elevation(nx, ny):
    j, i = np.mgrid[0:ny, 0:nx].astype(float)
    return 0.3 * np.sin(0.3 * i) + 0.1 * np.cos(0.2 * j) + 0.01 * i - 0.2


def same(a, b):
    """None if the two results are the same bits, else the first differing key"""
    for k in KEYS:
        if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
            return k
    return None


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
    c.elev = elevation(c.nx, c.ny)
    c.got = c.p.getRouteFields(fields=["speed", c.elev])
    assert not c.p.lastPathsOnDevice() and c.p.lastPathsKernelMs() == 0 and c.got["rounds"] == 0
    c.ref = ref.route_fields(c.T, RES, c.seeds, [c.F, c.elev])
    yield c
    c.p.close()


def test_host_equals_the_reference_bit_for_bit(case):
    assert same(case.got, case.ref) is None, same(case.got, case.ref)
    assert case.got["sink"].shape == (case.ny, case.nx) and case.got["sink"].dtype == np.uint32
    assert case.got["integral"].shape == (2, case.ny, case.nx)
    # host=True is the same route, and a subset of outputs the same maps
    again = case.p.getRouteFields(fields=["speed", case.elev], host=True)
    assert same(again, case.got) is None
    part = case.p.getRouteFields(fields=[case.elev], outputs=("sink", "length", "vmax"))
    assert sorted(part) == ["length", "rounds", "sink", "vmax"]
    assert part["sink"].tobytes() == case.got["sink"].tobytes()
    assert part["length"].tobytes() == case.got["length"].tobytes()
    assert part["vmax"][0].tobytes() == case.got["vmax"][1].tobytes()
    none = case.p.getRouteFields(outputs=("axis", "diag"))
    assert sorted(none) == ["axis", "diag", "rounds"]
    assert none["diag"].tobytes() == case.got["diag"].tobytes()


def test_every_finite_cell_has_a_route(case):
    g = case.got
    has = g["sink"] != NONE
    assert np.array_equal(has, np.isfinite(case.T))
    if case.obst:
        assert 0 < (~has).sum() < 0.05 * has.size
    if case.shape == "goalset":
        assert set(np.unique(g["sink"][has])) == {0, 1, 2}  # goal 3 is dominated: no root
        k = GS_GOALS[3]
        assert g["sink"][k[1], k[0]] == 0 and g["axis"][k[1], k[0]] + g["diag"][k[1], k[0]] == 2
        lab = goalset_ref.labels_from_T(case.T, case.seeds)
        assert (lab[has] != g["sink"][has]).mean() < 0.05  # close to the 4-neighbour label
    else:
        assert (g["sink"][has] == 0).all()
    assert (g["axis"][~has] == 0).all() and (g["diag"][~has] == 0).all()
    assert np.isnan(g["length"][~has]).all() and np.isnan(g["integral"][:, ~has]).all()
    assert (g["vmin"][:, ~has] == np.inf).all() and (g["vmax"][:, ~has] == -np.inf).all()


def test_hops_and_length_bound_the_distance(case):
    g = case.got
    has = g["sink"] != NONE
    j, i = np.mgrid[0:case.ny, 0:case.nx]
    gij = np.array(case.goals_ij)[np.where(has, g["sink"], 0).astype(int)]
    dx, dy = np.abs(i - gij[..., 0]), np.abs(j - gij[..., 1])
    hops = g["axis"].astype(np.int64) + g["diag"]
    assert (hops[has] >= np.maximum(dx, dy)[has]).all()
    assert (g["length"][has] >= RES * np.hypot(dx, dy)[has] - 1e-9).all()
    want = RES * g["axis"].astype(float) + (RES * 1.4142135623730951) * g["diag"].astype(float)
    assert g["length"][has].tobytes() == want[has].tobytes()
    for k, (gi, gj) in enumerate(case.goals_ij[:3]):
        assert hops[gj, gi] == 0 and g["length"][gj, gi] == 0.0 and g["sink"][gj, gi] == k
        assert g["integral"][0][gj, gi] == 0.0 and g["vmin"][0][gj, gi] == case.F[gj, gi]
    # the speed is U(1, 5) off the obstacles: the integral lies between 1 and 5 lengths
    far = has & (hops > 0)
    assert (g["integral"][0][far] >= g["length"][far] * (1 - 1e-12)).all()
    assert (g["integral"][0][far] <= 5 * g["length"][far] * (1 + 1e-12)).all()
    assert (g["vmin"][0][has] >= 1.0).all() and (g["vmax"][0][has] <= 5.0).all()
    assert (g["vmin"][1][has] <= case.elev[has]).all() and (g["vmax"][1][has] >= case.elev[has]).all()


def test_routes_descend_and_cut_no_corner(case):
    g = case.got
    rng = np.random.default_rng(5)
    cells = np.argwhere(g["sink"] != NONE)
    T = case.T
    for j, i in cells[rng.choice(len(cells), 200, replace=False)]:
        nodes, k = ref.walk(T, case.seeds, int(i), int(j))
        assert k == g["sink"][j, i]
        assert len(nodes) - 1 == int(g["axis"][j, i]) + int(g["diag"][j, i])
        assert nodes[-1] == tuple(case.goals_ij[k])
        diag = 0
        for (a, b), (c, d) in zip(nodes, nodes[1:]):
            assert T[d, c] < T[b, a] and max(abs(c - a), abs(d - b)) == 1
            if c != a and d != b:
                diag += 1
                assert np.isfinite(T[b, c]) and np.isfinite(T[d, a])
        assert diag == g["diag"][j, i]
        elev = [case.elev[b, a] for a, b in nodes]
        assert g["vmin"][1][j, i] == min(elev) and g["vmax"][1][j, i] == max(elev)


def test_current_path_is_not_touched(case):
    start = (case.off[0] + 20.3, case.off[1] + 20.6, 0.0, 0.0)
    assert len(case.p.getPath(start)) > 3
    marker = case.p.current_path
    case.p.getRouteFields(fields=["speed"])
    assert np.array_equal(case.p.current_path, marker)


def test_loaded_plateau_and_its_drainage_get_none(dymu):
    n, goal = 24, (6, 6)
    p = dymu.Planner(risk_distance=RD)
    try:
        assert p.initGlobalLayer(RES, 0.5, n, n)
        assert p.setCostMap(np.ones((n, n)))
        assert p.setGoal((float(goal[0]), float(goal[1]), 0.0, 0.0))
        T = np.full((n, n), 5.0)
        T[goal[1], goal[0]] = 0.0
        T[10:, 10:] = 7.0  # a step down onto the plateau, then nothing lower
        assert p.loadTotalCostMap(T)
        f = elevation(n, n)
        got = p.getRouteFields(fields=[f, "speed"])
        want = ref.route_fields(T, RES, [goal + (0.0,)], [f, np.ones((n, n))])
        assert same(got, want) is None, same(got, want)
        near = np.zeros((n, n), dtype=bool)
        near[5:8, 5:8] = True
        assert (got["sink"][near] == 0).all() and (got["sink"][~near] == NONE).all()
        assert np.isnan(got["length"][~near]).all()
    finally:
        p.close()


@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 7), (2, 2), (3, 3)])
def test_tiny_grids(dymu, nx, ny):
    """No goal fits on a grid without an interior: every cell is without a route, as with
    no goal at all; the 3x3 grid has its one interior goal."""
    p = dymu.Planner(risk_distance=RD)
    try:
        assert p.initGlobalLayer(RES, 0.5, nx, ny)
        assert p.setCostMap(np.ones((ny, nx)))
        seeds = []
        if nx == 3:
            assert p.setGoal((1.0, 1.0, 0.0, 0.0))
            T = np.array([[1.4, 1.0, 1.4], [1.0, 0.0, 1.0], [1.4, 1.0, 1.4]])
            seeds = [(1, 1, 0.0)]
        else:
            assert not p.setGoal((0.0, 0.0, 0.0, 0.0))
            T = np.full((ny, nx), np.inf)
        p.loadTotalCostMap(T)
        f = elevation(nx, ny)
        got = p.getRouteFields(fields=[f])
        want = ref.route_fields(T, RES, seeds, [f])
        assert same(got, want) is None, same(got, want)
        if nx == 3:
            assert got["diag"].sum() == 4 and got["axis"].sum() == 4
        else:
            assert (got["sink"] == NONE).all()
    finally:
        p.close()


def test_arguments(dymu):
    p = dymu.Planner(risk_distance=RD)
    try:
        assert p.initGlobalLayer(RES, 0.5, 8, 8)
        assert p.setCostMap(np.ones((8, 8)))
        z = np.zeros((8, 8))
        with pytest.raises(ValueError):
            p.getRouteFields(fields=[z] * 5)
        with pytest.raises(ValueError):
            p.getRouteFields(fields=[np.zeros((3, 3))])
        with pytest.raises(ValueError):
            p.getRouteFields(fields=["hazard"])
        with pytest.raises(ValueError):
            p.getRouteFields(outputs=("sink", "hops"))
        with pytest.raises(dymu.DymuError):
            p.getRouteFieldsTo(0, fields=[z])  # no batch
        got = p.getRouteFields(fields=[z, "speed"])  # no goal: nothing has a route
        assert (got["sink"] == NONE).all() and np.isnan(got["integral"]).all()
    finally:
        p.close()


def test_symbols(dymu):
    fim, pl = dymu.load_fim(), dymu.load_planner()
    for n in ("dymu_route_fields_device", "dymu_route_fields_workspace",
              "dymu_last_route_fields_ms", "dymu_last_route_fields_stages"):
        assert hasattr(fim, n) and n in dymu.FIM_SYMBOLS, n
    for n in ("dymu_planner_get_route_fields", "dymu_planner_get_route_fields_to"):
        assert hasattr(pl, n) and n in dymu.PLANNER_SYMBOLS, n
    o = dymu.DymuRouteOut()
    assert fim.dymu_route_fields_device(None, None, 8, 8, 8, 1.0, None, 0, None, None, 0, o, None,
                                        0, None, None) == -1
    assert pl.dymu_planner_get_route_fields(None, None, 0, 1, o, None) == -1
    # the workspace: two 4-byte entries a cell and the counters at least; more per output
    w = dymu.Engine.route_out
    ws = lambda nf, out=None: fim.dymu_route_fields_workspace(100, 50, nf, out)  # noqa: E731
    n = 5000
    assert ws(0, w(100, sink=1)) >= 8 * n
    assert ws(0, w(100, sink=1, length=1)) >= ws(0, w(100, sink=1)) + 16 * n
    assert ws(2) >= 2 * (12 + 24 * 2) * n and ws(2) <= 2 * (12 + 24 * 2) * n + 65536
    assert ws(1, w(100, integral=[1])) >= ws(0, w(100, sink=1)) + 16 * n
    assert ws(5) == 0 and ws(1, w(100, vmin=[0, 1])) == 0
    assert fim.dymu_route_fields_workspace(0, 50, 0, None) == 0
    assert fim.dymu_route_fields_workspace(65536, 32768, 0, None) == 0
