"""The device code against the reference planner's recorded output, no oracle in between.

tests/golden/ref_*.npz hold what the reference's own sources produced
(tests/golden/gen_golden_ref.py); neither the reference nor its driver is needed here.
Shapes are 96x64, 64x96 and 33x47: several 16x16 tiles each way, a ragged last tile, and
a padded pitch (ld = nx + 8) next to the dense one.

Tolerances are the project's existing ones: +inf / -1 masks, node states, orders and
integer fields exact; total cost within 1e-12 * max(1, T) (tests/test_gpu_solver.py);
the cost map's real fields within 1e-13 (tests/test_gpu_costmap.py: the device atan);
waypoints within 1e-9 (tests/test_gpu_paths.py); total cost at a point exact where the
map was loaded from the fixture.
"""
import numpy as np
import pytest

import ref_cases as rc
from test_gpu_costmap import DeviceState, close, upload
from test_gpu_solver import assert_parity
from test_planner import _early_matches

pytestmark = pytest.mark.gpu

PAD = 8
POISON = 1e-3  # in the padding columns: a cheap speed that would pull T down if it were read


@pytest.fixture(scope="module")
def recorded():
    return {n: rc.load_fixture(n) for n in rc.committed_cases()}


def _goal_node(p):
    return (int((p["goal"][0] - p["offset"][0]) / p["gres"] + 0.5),
            int((p["goal"][1] - p["offset"][1]) / p["gres"] + 0.5))


def _padded(a, ld, fill):
    ny, nx = a.shape
    buf = np.full((ny, ld), fill, dtype=np.float64)
    buf[:, :nx] = a
    return buf


# ------------------------------------------------------------------ solve
ENGINES = {3: dict(kernel=3), 4: dict(kernel=4, prio_target=64), 5: dict(kernel=5, prio_target=16)}


@pytest.fixture(scope="module", params=[(k, e) for k in sorted(ENGINES) for e in (0, 1)],
                ids=lambda p: f"k{p[0]}-exact{p[1]}")
def solver(request, dymu):
    k, e = request.param
    eng = dymu.Engine(exact_sqrt=e, **ENGINES[k])
    yield eng
    eng.close()


SOLVE_MAPS = [("setcost_96x64", 0), ("setcost_96x64", PAD), ("setcost_64x96", 0),
              ("setcost_64x96", PAD), ("path_96x64", 0), ("path_96x64", PAD), ("path_64x96", 0),
              ("path_64x96", PAD), ("setcost_33x47", 0), ("path_33x47", PAD)]


@pytest.mark.parametrize("name,pad", SOLVE_MAPS, ids=lambda v: str(v))
def test_solve_device_matches_reference(solver, recorded, name, pad):
    case, want = recorded[name]
    p = case["params"]
    nx, ny, ld = p["nx"], p["ny"], p["nx"] + pad
    F = rc.speed_from_fields(want, p["gres"])
    g = tuple(int(v) for v in want["goal_node"]) if "goal_node" in want else _goal_node(p)
    dF, dT = solver.alloc(8 * ny * ld), solver.alloc(8 * ny * ld)
    try:
        solver.h2d(dF, _padded(F, ld, POISON))
        solver.solve_device(dF, dT, nx, ny, ld, g[0], g[1])
        T = np.empty((ny, ld))
        solver.d2h(T, dT)
    finally:
        solver.free(dF)
        solver.free(dT)
    assert_parity(T[:, :nx], rc._inf(want["total_cost"]))


# ------------------------------------------------------------------ device cost map
@pytest.mark.parametrize("name,pad", [("costmap_96x64", PAD), ("costmap_64x96", 0),
                                      ("costmap_40x56", PAD)])
def test_device_cost_map_matches_reference(engine, oracle, recorded, name, pad):
    case, want = recorded[name]
    p, a = case["params"], case["arrays"]
    nx, ny, ld = p["nx"], p["ny"], p["nx"] + pad
    dst = DeviceState(engine, nx, ny, ld, oracle.new_state(nx, ny))  # a fresh planner's fields
    dE, dTr = upload(engine, a["elevation"], ld), upload(engine, a["terrain"], ld)
    dF = engine.alloc(8 * ny * ld)
    try:
        for sfx in ("_1", "_2"):  # the second call compounds the smoothing (Q1)
            engine.compute_cost_map(nx, ny, ld, p["gres"], a["lut"], a["slopes"], p["n_locs"],
                                    dE, dTr, dst.ptr, dF)
            for f in ("terrain", "is_obstacle", "loc_mode", "hazard", "traff"):
                assert np.array_equal(dst.get(f), want[f + sfx]), (sfx, f)
            for f in ("slope", "raw_cost", "cost"):
                ok, err = close(dst.get(f), want[f + sfx])
                assert ok, (sfx, f, err)
            Fd = np.empty((ny, ld))
            engine.d2h(Fd, dF)
            fields = {k: want[k + sfx] for k in ("cost", "hazard", "traff", "is_obstacle")}
            ok, err = close(Fd[:, :nx], rc.speed_from_fields(fields, p["gres"]))
            assert ok, (sfx, "F", err)
    finally:
        for q in (dE, dTr, dF):
            engine.free(q)
        dst.free()


@pytest.mark.parametrize("name,pad", [("costmap_64x96", PAD), ("local_64x40", 0)])
def test_pack_speed_of_reference_fields(engine, oracle, recorded, name, pad):
    """dymu_pack_speed on the reference's own node fields (for the local case: after the
    local layer's feedback) is the reference's C (:527-528) bit for bit"""
    case, want = recorded[name]
    p = case["params"]
    nx, ny, ld = p["nx"], p["ny"], p["nx"] + pad
    if case["family"] == "local":
        ob = want["global_cost"] == -1.0
        cost = np.where(ob, 1.0, want["global_cost"])  # any cost: only the factor is tested
        fields = {"cost": cost, "hazard": want["hazard_matrix"], "traff": want["traff_matrix"],
                  "is_obstacle": ob.astype(np.int64)}
    else:
        fields = {k: want[k + "_2"] for k in ("cost", "hazard", "traff", "is_obstacle")}
    st = oracle.new_state(nx, ny)
    for k in ("cost", "hazard", "traff", "is_obstacle"):
        st[k][:] = fields[k]
    dst = DeviceState(engine, nx, ny, ld, st)
    dF = engine.alloc(8 * ny * ld)
    try:
        engine.pack_speed(nx, ny, ld, p["gres"], dst.ptr, dF)
        Fd = np.empty((ny, ld))
        engine.d2h(Fd, dF)
    finally:
        engine.free(dF)
        dst.free()
    assert np.array_equal(Fd[:, :nx], rc.speed_from_fields(fields, p["gres"]))


# ------------------------------------------------------------------ early exit
def _check_early(pl, p, want, sfx, goal, start):
    assert pl.setGoal(tuple(goal)) == bool(want["rc_setgoal" + sfx][0])
    assert pl.computeTotalCostMap(tuple(start)) == bool(want["rc" + sfx][0])
    _early_matches(pl.getTotalCostMatrix(), rc._inf(want["total_cost" + sfx]))
    assert np.array_equal(pl.nodeStates(), want["closed" + sfx])
    band = pl.globalNarrowband()
    assert np.array_equal(band, want["narrowband" + sfx])
    assert pl.lastBandSize() == len(want["narrowband" + sfx])
    assert np.array_equal(pl.globalPropagatedNodes(), want["propagated" + sfx])
    (i, j), t = pl.minCostGlobalNode()
    assert (i, j) == tuple(want["next_min" + sfx])
    assert t == pl.getTotalCostMatrix()[j, i]


@pytest.mark.parametrize("name", ["early_96x64", "early_64x96", "early_48x40"])
def test_early_exit_matches_reference(dymu, recorded, name):
    """computeTotalCostMap's exit state: the -1 mask, every node state, the band and the
    propagated list in the reference's order, the next minimum node; then a second goal
    and start on the same planner"""
    case, want = recorded[name]
    p = case["params"]
    pl = rc._new_planner(dymu, p)
    try:
        assert pl.setCostMap(case["arrays"]["cost"])
        _check_early(pl, p, want, "_1", p["goal"], p["start"])
        pl.resetTotalCostMap()
        assert (pl.getTotalCostMatrix() == -1.0).all()
        _check_early(pl, p, want, "_2", p["goal2"], p["start2"])
    finally:
        pl.close()


# ------------------------------------------------------------------ paths and costs
def _split(want):
    ends = np.cumsum(want["path_len"])
    return [want["path_wp"][e - n:e] for e, n in zip(ends, want["path_len"])]


def _check_paths(pl, case, want):
    starts = [(s[0], s[1], 0.0, s[2]) for s in case["arrays"]["starts"]]
    paths, status = pl.getPaths(starts)
    assert pl.lastPathsOnDevice()
    worst = 0.0
    for q, (d, r) in enumerate(zip(paths, _split(want))):
        if len(r) == 0:  # the reference's first step met the NaN rule: nothing pushed
            assert status[q] == -1 and len(d) == 0, (q, status[q], len(d))
            continue
        assert len(d) == len(r), (q, status[q], len(d), len(r))
        assert not np.isnan(d).any(), q
        worst = max(worst, np.abs(d[:, :2] - r[:, :2]).max(), np.abs(d[:, 3] - r[:, 3]).max(),
                    np.abs(d[:, 2] - r[:, 2]).max())
    print(f"max |device - reference| over x, y, z, heading: {worst:.3e}")
    assert worst < 1e-9


@pytest.mark.parametrize("name", ["path_96x64", "path_64x96", "path_33x47"])
def test_paths_and_costs_match_reference(dymu, engine, recorded, name):
    case, want = recorded[name]
    p, a = case["params"], case["arrays"]
    nx, ny = p["nx"], p["ny"]
    pl = rc._new_planner(dymu, p)
    try:
        assert rc._planner_costmap_once(pl, case)
        g = p["goal"]
        assert pl.setGoal((g[0], g[1], 0.0, g[2]))
        assert pl.computeEntireTotalCostMap()  # the device solve
        assert_parity(pl.totalCostRaw(), rc._inf(want["total_cost"]))
        _check_paths(pl, case, want)
        # the reference's own matrix on the device: getPaths again, and every recorded point
        assert pl.loadTotalCostMap(rc._inf(want["total_cost"]))
        _check_paths(pl, case, want)
        got = np.array([pl.getTotalCost((x, y)) for x, y in a["points"]])
        assert got.tobytes() == want["point_cost"].tobytes()
    finally:
        pl.close()
    ld = nx + PAD
    dT = engine.alloc(8 * ny * ld)
    try:
        engine.h2d(dT, _padded(rc._inf(want["total_cost"]), ld, -7.0))
        local = a["points"] - np.array(p["offset"])  # as getTotalCost removes the offset (:862)
        got = engine.gather_costs(dT, nx, ny, 1, ld, p["gres"], local)
    finally:
        engine.free(dT)
    assert got.shape == (1, len(local)) and got[0].tobytes() == want["point_cost"].tobytes()


# ------------------------------------------------------------------ feedback re-solve
@pytest.mark.parametrize("name", ["local_cons", "local_sweep", "local_64x40", "local_40x64"])
def test_resolve_after_recorded_feedback(dymu, recorded, name):
    """the solve, then the solve again on the hazard density and trafficability the
    reference's local layer left behind, against the reference's two matrices"""
    case, want = recorded[name]
    p = case["params"]
    pl = rc._new_planner(dymu, p)
    try:
        assert rc._planner_costmap_once(pl, case)
        g = p["goal"]
        assert pl.setGoal((g[0], g[1], 0.0, g[2]))
        assert pl.computeEntireTotalCostMap()
        assert_parity(pl.totalCostRaw(), rc._inf(want["total_cost"]))
        changed = (want["hazard_matrix"] != pl.getHazardDensityMatrix()) | \
                  (want["traff_matrix"] != pl.getTrafficabilityMatrix())
        assert changed.any()
        assert pl.setHazardDensity(want["hazard_matrix"])
        assert pl.setTrafficability(want["traff_matrix"])
        assert np.array_equal(pl.getGlobalCostMatrix(), want["global_cost"])
        assert pl.computeEntireTotalCostMap()
        assert pl.lastSolveKind() != 2  # not the previous map reused
        assert_parity(pl.totalCostRaw(), rc._inf(want["total_cost_2"]))
        assert not np.array_equal(want["total_cost"], want["total_cost_2"])
    finally:
        pl.close()
