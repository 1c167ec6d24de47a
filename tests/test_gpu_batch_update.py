"""Windowed re-propagation of seeded maps and of stacks of planes on the device (DESIGN.md
s5.8): dymu_update_seeds_window_device, dymu_update_batch_window_device and the planner's
trackSpeedChanges.  The yardstick is always the oracle FMM of the NEW speed (oracle.fmm for
one zero seed, goalset_ref.fmm_seeds for seed lists) under the project's bound -- the same
+inf mask and |dT| <= 1e-12 max(1, T).  The number of reset cells (dymu_last_update_stats'
out[2]) is compared with a numpy count against each plane's own theta: it is the one
observable that tells a per-plane theta from a global one.  References are computed once
per case and shared by the kernels."""
import numpy as np
import pytest

import goalset_ref as ref
from test_gpu_batch import (BLOCKED, HEADINGS, KERNELS, NX, NY, OFF, SHAPES, SITES, Case, Stack,
                            check_parity, goal_of, make_planner, seeds_for)
from test_gpu_update import disc, modified, window_of

pytestmark = pytest.mark.gpu


def theta_of(T0, wins):
    """min of the old map over every window grown by its ring, clipped; +inf for none."""
    ny, nx = T0.shape
    th = np.inf
    for i0, j0, w, h in wins:
        i1, j1 = min(i0 + w, nx), min(j0 + h, ny)
        th = min(th, T0[max(j0 - 1, 0):min(j1 + 1, ny), max(i0 - 1, 0):min(i1 + 1, nx)].min())
    return th


def reset_count(T0, theta):
    return int((np.isfinite(T0) & (T0 >= theta)).sum())


# ---- 1. a seeded single map ----

def seeded_kinds(F0, rng):
    """name -> (new speed, window, decrease_only)."""
    ny, nx = F0.shape
    out = {}
    F1 = F0.copy()
    inner, _ = disc(nx, ny, (60, 20), 5)  # a hazard disc away from every seed
    F1[inner] *= 1.5
    out["hazard"] = (F1, window_of(inner), 0)
    F1 = F0.copy()
    inner, _ = disc(nx, ny, (50, 40), 4)
    F1[inner] = np.inf
    out["blocked"] = (F1, window_of(inner), 0)
    F1 = F0.copy()
    box = F1[5:20, 40:60]
    box[~np.isfinite(box)] = 2.0
    box *= 0.5
    out["clear"] = (F1, (40, 5, 20, 15), 0)
    out["clear-decrease-only"] = (F1, (40, 5, 20, 15), 1)
    F1 = F0.copy()
    F1[30:50, 55:73] *= rng.uniform(0.5, 2.0, (20, 18))
    out["mixed"] = (F1, (55, 30, 18, 20), 0)
    F1 = F0.copy()
    F1[17:25, 17:27] *= 3.0  # over the seeds (20,20), (22,21,0.5) and the dominated (24,22,1e6)
    out["seeds"] = (F1, (17, 17, 10, 8), 0)
    F1 = F0.copy()
    F1[ny - 6:, nx - 20:] *= 2.0
    out["corner"] = (F1, (nx - 20, ny - 6, 500, 500), 0)  # clipped at the grid corner
    return out


@pytest.fixture(scope="module")
def seeded(oracle):
    c = Case()
    c.nx, c.ny = SHAPES["97x61"]
    c.seeds = seeds_for(c.nx, c.ny)
    # test_gpu_batch.py's `multi` fixture, plane 0
    c.F0 = oracle.synth_speed(c.nx, c.ny, seed=21, obst_frac=0.02, obst_seed=3, goal=(20, 20))
    for i, j, _ in c.seeds:
        if not np.isfinite(c.F0[j, i]):
            c.F0[j, i] = 3.0
    c.kinds = seeded_kinds(c.F0, np.random.default_rng(17))
    c.T1 = {k: ref.fmm_seeds(oracle, v[0], c.seeds) for k, v in c.kinds.items()
            if k != "clear-decrease-only"}
    c.T1["clear-decrease-only"] = c.T1["clear"]
    c.F2, c.T2 = {}, {}
    for k, v in c.kinds.items():  # the chained second change
        c.F2[k] = v[0].copy()
        c.F2[k][5:15, 5:25] *= 0.8
        c.T2[k] = c.T2["clear"] if k == "clear-decrease-only" else \
            ref.fmm_seeds(oracle, c.F2[k], c.seeds)
    return c


KINDS = ["hazard", "blocked", "clear", "clear-decrease-only", "mixed", "seeds", "corner"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_seeded_map_update(dymu, seeded, kernel, kind):
    c = seeded
    nx, ny = c.nx, c.ny
    F1, (i0, j0, w, h), dec = c.kinds[kind]
    T0, T = np.empty((ny, nx)), np.empty((ny, nx))
    with dymu.Engine(**KERNELS[kernel]) as eng:
        dF, dT = eng.alloc(8 * nx * ny), eng.alloc(8 * nx * ny)
        try:
            eng.h2d(dF, c.F0)
            eng.solve_seeds_device(dF, dT, nx, ny, nx, c.seeds)
            eng.d2h(T0, dT)
            eng.h2d(dF, F1)
            st = eng.update_seeds_window_device(dF, dT, nx, ny, nx, c.seeds, i0, j0, w, h,
                                                decrease_only=bool(dec))
            us = eng.last_update_stats()
            eng.d2h(T, dT)
            check_parity(T, c.T1[kind])
            # a second update chains on the first
            eng.h2d(dF, c.F2[kind])
            eng.update_seeds_window_device(dF, dT, nx, ny, nx, c.seeds, 5, 5, 20, 10)
            us2 = eng.last_update_stats()
            T2 = np.empty((ny, nx))
            eng.d2h(T2, dT)
        finally:
            eng.free(dF)
            eng.free(dT)
    assert st["kernel"] == kernel
    check_parity(T2, c.T2[kind])
    assert us["raise_passes"] == 0 and us["raise_visits"] == 0
    want = 0 if dec else reset_count(T0, theta_of(T0, [(i0, j0, w, h)]))
    print(f"{kind}: {us['cells_invalidated']} cells reset, {st['passes']} passes, "
          f"{st['tile_visits']} tile visits")
    assert us["cells_invalidated"] == want
    assert us2["cells_invalidated"] == reset_count(T, theta_of(T, [(5, 5, 20, 10)]))
    if kind == "seeds":
        # the window holds a seed of value 0, so theta = 0 and every finite cell is reset:
        # the seeds come back as boundary values, the dominated one as what propagates
        assert want == int(np.isfinite(T0).sum())
        assert T[20, 20].tobytes() == np.float64(0.0).tobytes()
        for i, j, t0 in ((22, 21, 0.5), (0, 30, 1.0), (nx - 10, ny - 12, 0.25), (24, 22, 1e6)):
            assert T[j, i] <= t0
            if c.T1[kind][j, i] == t0:  # a seed at its t0 ends at bitwise its t0
                assert T[j, i].tobytes() == np.float64(t0).tobytes()
        assert c.T1[kind][30, 0] == 1.0 and c.T1[kind][21, 22] == 0.5
        assert c.T1[kind][22, 24] < 1e6 and T[22, 24] < 1e6  # min(1e6, propagated)
        assert T[22, 24] > T0[22, 24]  # not its stale value: the cells around it got slower


# ---- 2. one zero seed: the existing single-goal path ----

@pytest.fixture(scope="module")
def single(oracle):
    c = Case()
    c.nx, c.ny, c.goal = 300, 260, (150, 200)
    c.F0 = oracle.synth_speed(c.nx, c.ny, seed=23, obst_frac=0.04, obst_seed=29, goal=c.goal)
    rng = np.random.default_rng(17)
    c.kinds = {k: modified(k, c.F0, c.goal, rng) for k in ("hazard", "goal")}
    c.T1 = {k: oracle.fmm(v[0], c.goal)[0] for k, v in c.kinds.items()}
    return c


@pytest.mark.parametrize("kind", ["hazard", "goal"])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_single_zero_seed_equals_resolve_window(dymu, single, kernel, kind):
    c = single
    nx, ny, (gi, gj) = c.nx, c.ny, c.goal
    F1, (i0, j0, w, h) = c.kinds[kind]
    Ta, Tb = np.empty((ny, nx)), np.empty((ny, nx))
    with dymu.Engine(**KERNELS[kernel]) as eng:
        ptrs = [eng.alloc(8 * nx * ny) for _ in range(3)]
        dF, dTa, dTb = ptrs
        try:
            eng.h2d(dF, c.F0)
            eng.solve_device(dF, dTa, nx, ny, nx, gi, gj)
            eng.solve_device(dF, dTb, nx, ny, nx, gi, gj)
            eng.h2d(dF, F1)
            eng.update_seeds_window_device(dF, dTa, nx, ny, nx, [(gi, gj, 0.0)], i0, j0, w, h)
            eng.resolve_window_device(dF, dTb, nx, ny, nx, gi, gj, i0, j0, w, h)
            eng.d2h(Ta, dTa)
            eng.d2h(Tb, dTb)
        finally:
            for p in ptrs:
                eng.free(p)
    assert Ta[gj, gi] == 0.0
    check_parity(Ta, c.T1[kind])
    check_parity(Ta, Tb)


# ---- 3. a stack: the planes stay isolated, theta is per plane ----

def stack_change(F0, goals):
    """(new speeds [5, ny, nx], windows (plane, i0, j0, w, h)): plane 0 a hazard disc, plane
    1 a box that includes row 0 beside the wall, the blocked plane a box, plane 3 nothing,
    plane 4 two windows."""
    _, ny, nx = F0.shape
    F1 = F0.copy()
    inner, _ = disc(nx, ny, (nx // 2, ny // 2), 6)
    F1[0][inner] *= 1.5
    wins = [(0, *window_of(inner))]
    F1[1, 0:6, 40:52] *= 1.7
    wins.append((1, 40, 0, 12, 6))
    F1[BLOCKED, 30:35, 30:35] = 2.0  # an island nothing reaches
    wins.append((BLOCKED, 30, 30, 5, 5))
    F1[4, 10:18, 10:18] *= 0.5
    F1[4, 30:40, 70:80] *= 2.0
    wins += [(4, 10, 10, 8, 8), (4, 70, 30, 10, 10)]
    return F1, wins


@pytest.fixture(scope="module", params=sorted(SHAPES))
def changed(request, oracle):
    """test_gpu_batch.py's five planes, their change, and the FMM of every new plane."""
    c = Case()
    c.nx, c.ny = SHAPES[request.param]
    c.ld = c.nx + 5 if request.param == "97x61" else c.nx  # one pitched stack
    c.goals = [goal_of(b, c.nx, c.ny) for b in range(5)]
    c.F0 = np.stack([oracle.synth_speed(c.nx, c.ny, seed=(b + 1) << 20 | 30, obst_frac=0.02,
                                        obst_seed=(b + 1) << 22 | 5, goal=c.goals[b])
                     for b in range(5)])
    c.F0[BLOCKED] = np.inf
    gi, gj = c.goals[BLOCKED]
    c.F0[BLOCKED, gj, gi] = 2.5
    c.F1, c.wins = stack_change(c.F0, c.goals)
    c.T_ref = [oracle.fmm(c.F1[b], c.goals[b])[0] for b in range(5)]
    c.seeds = [(b, *c.goals[b]) for b in range(5)]
    return c


def solve_and_update(dymu, eng, c):
    """(old planes, new planes, walls of T, walls of F, update stats, reset cells)."""
    s = Stack(dymu, eng, c.F0, ld=c.ld)
    try:
        s.solve(c.seeds)
        T0 = s.planes(s.download(s.dT))[0].copy()
        eng.h2d(s.src, c.F1)
        eng.stack_speed(s.src, c.nx, c.nx * c.ny, c.nx, c.ny, 5, s.dF, s.ld)
        st = eng.update_batch_window_device(s.dF, s.dT, c.nx, c.ny, 5, s.ld, c.seeds, c.wins)
        n_reset = eng.last_update_stats()["cells_invalidated"]
        T, Tw = s.planes(s.download(s.dT))
        Fw = s.planes(s.download(s.dF))[1]
    finally:
        s.close()
    return T0, T.copy(), Tw.copy(), Fw.copy(), st, n_reset


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_stack_isolation_and_per_plane_theta(dymu, changed, kernel):
    c = changed
    with dymu.Engine(**KERNELS[kernel]) as eng:
        T0, T, Tw, Fw, st, n_reset = solve_and_update(dymu, eng, c)
    assert st["kernel"] == kernel
    assert np.isposinf(Tw).all() and np.isposinf(Fw).all()
    for b in range(5):
        check_parity(T[b], c.T_ref[b])
    assert np.array_equal(T[3].view(np.uint64), T0[3].view(np.uint64))  # bit for bit
    theta = [theta_of(T0[b], [w[1:] for w in c.wins if w[0] == b]) for b in range(5)]
    assert np.isinf(theta[3]) and np.isinf(theta[BLOCKED]) and np.isfinite(theta[0])
    per_plane = sum(reset_count(T0[b], theta[b]) for b in range(5))
    one_theta = sum(reset_count(T0[b], min(theta)) for b in range(5))
    print(f"theta {theta}: {per_plane} cells reset per plane, {one_theta} under one theta; "
          f"{st['passes']} passes, {st['tile_visits']} tile visits")
    assert per_plane < one_theta  # the windows tell the two rules apart
    assert n_reset == per_plane


def test_stack_update_deterministic(dymu, changed):
    c = changed
    with dymu.Engine(deterministic=1) as eng:
        a = solve_and_update(dymu, eng, c)
        b = solve_and_update(dymu, eng, c)
    assert a[4]["kernel"] == 5
    assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    assert a[5] == b[5]
    for p in range(5):
        check_parity(a[1][p], c.T_ref[p])


# ---- 4. argument errors ----

def test_argument_errors(dymu, engine, changed):
    c = changed
    B, nx, ny = 3, c.nx, c.ny
    s = Stack(dymu, engine, c.F0[:B], ld=c.ld)
    lib, ctx = engine._lib, engine.ctx
    good, gwin = c.seeds[:B], [(0, 5, 5, 4, 4)]
    too_many = -(-(1 << 32) // s.P)

    def raw(seeds, wins, B_=B, ld_=c.ld, ctx_=ctx, dF=s.dF, dT=s.dT, null_seeds=False,
            null_wins=False):
        a = np.zeros(len(seeds), dtype=dymu.BATCH_SEED_DTYPE)
        for k, sd in enumerate(seeds):
            a[k] = (sd[0], sd[1], sd[2], 0, sd[3] if len(sd) > 3 else 0.0)
        wn = np.zeros(len(wins), dtype=dymu.BATCH_WINDOW_DTYPE)
        for k, q in enumerate(wins):
            wn[k] = (*q, 0)
        return lib.dymu_update_batch_window_device(
            ctx_, dF, dT, nx, ny, B_, ld_, None if null_seeds else a.ctypes.data, len(a),
            None if null_wins else wn.ctypes.data, len(wn), 0, None, None)

    def raw1(seeds, win, ld_=nx, ctx_=ctx, dF=s.dF, dT=s.dT, null_seeds=False):
        a = engine._seeds(seeds)
        return lib.dymu_update_seeds_window_device(
            ctx_, dF, dT, nx, ny, ld_, None if null_seeds else a.ctypes.data, len(a), *win, 0,
            None, None)

    one = [(5, 5, 0.0)]
    try:
        s.solve(good)
        bad = {
            "null ctx": raw(good, gwin, ctx_=None),
            "null speed": raw(good, gwin, dF=None),
            "null map": raw(good, gwin, dT=None),
            "null seeds": raw(good, gwin, null_seeds=True),
            "null windows": raw(good, gwin, null_wins=True),
            "B = 0": raw(good, gwin, B_=0),
            "ld < nx": raw(good, gwin, ld_=nx - 1),
            "seed plane >= B": raw(good + [(B, 5, 5)], gwin),
            "seed i off the plane": raw(good + [(0, nx, 5)], gwin),
            "seed j in the wall rows": raw(good + [(0, 5, ny)], gwin),
            "t0 < 0": raw(good + [(1, 5, 5, -1.0)], gwin),
            "t0 NaN": raw(good + [(1, 5, 5, float("nan"))], gwin),
            "t0 inf": raw(good + [(1, 5, 5, float("inf"))], gwin),
            "no seeds": raw([], gwin),
            "a plane without a seed": raw(good[:1] + good[2:], gwin),
            "B * P beyond uint32": raw(good, gwin, B_=too_many),
            "window plane >= B": raw(good, gwin + [(B, 5, 5, 4, 4)]),
            "w = 0": raw(good, gwin + [(1, 5, 5, 0, 4)]),
            "h = 0": raw(good, gwin + [(1, 5, 5, 4, 0)]),
            "i0 >= nx": raw(good, gwin + [(1, nx, 5, 4, 4)]),
            "j0 >= ny": raw(good, gwin + [(1, 5, ny, 4, 4)]),
            "no windows": raw(good, []),
            "1: null ctx": raw1(one, (5, 5, 4, 4), ctx_=None),
            "1: null speed": raw1(one, (5, 5, 4, 4), dF=None),
            "1: null map": raw1(one, (5, 5, 4, 4), dT=None),
            "1: null seeds": raw1(one, (5, 5, 4, 4), null_seeds=True),
            "1: no seeds": raw1([], (5, 5, 4, 4)),
            "1: ld < nx": raw1(one, (5, 5, 4, 4), ld_=nx - 1),
            "1: seed off the grid": raw1([(nx, 5, 0.0)], (5, 5, 4, 4)),
            "1: t0 < 0": raw1([(5, 5, -1.0)], (5, 5, 4, 4)),
            "1: t0 NaN": raw1([(5, 5, float("nan"))], (5, 5, 4, 4)),
            "1: w = 0": raw1(one, (5, 5, 0, 4)),
            "1: h = 0": raw1(one, (5, 5, 4, 0)),
            "1: i0 >= nx": raw1(one, (nx, 5, 4, 4)),
            "1: j0 >= ny": raw1(one, (5, ny, 4, 4)),
        }
        for what, rc in bad.items():
            assert rc == -1, what
        # the context still updates
        engine.h2d(s.src, c.F1[:B])
        engine.stack_speed(s.src, nx, nx * ny, nx, ny, B, s.dF, s.ld)
        engine.update_batch_window_device(s.dF, s.dT, nx, ny, B, s.ld, good,
                                          [w for w in c.wins if w[0] < B])
        T, _ = s.planes(s.download(s.dT))
    finally:
        s.close()
    for b in range(B):
        check_parity(T[b], c.T_ref[b])


# ---- 5. the planner's batch ----

def site_map(oracle):
    F = oracle.synth_speed(NX, NY, seed=17, obst_frac=0.02, goal=SITES[0])
    for i, j in SITES:
        blk = F[j - 1:j + 2, i - 1:i + 2]
        blk[~np.isfinite(blk)] = 3.0
    return F


def set_hazard(planners, hz, i0, j0, w, h, v):
    """hazard v on [i0, i0+w) x [j0, j0+h): F = res * cost * (2 + hazard - traff), traff = 1."""
    hz[j0:j0 + h, i0:i0 + w] = v
    for p in planners:
        assert p.setHazardDensityWindow(i0, j0, np.full((h, w), float(v)))


def test_planner_batch_tracks_speed_changes(dymu, oracle):
    F = site_map(oracle)
    hz = np.zeros((NY, NX))
    sites = [(OFF[0] + i, OFF[1] + j, 0.0, h) for (i, j), h in zip(SITES, HEADINGS)]
    p, q = make_planner(dymu, F), make_planner(dymu, F)
    try:
        assert p.lastBatchSolveKind() == 0
        p.trackSpeedChanges(True)
        assert p.setGoal(sites[1]) and p.computeEntireTotalCostMap()
        p.getPath((OFF[0] + 30.5, OFF[1] + 22.25, 0.0, 0.0))
        M = p.costMatrix(sites, sites)
        assert M is not None and p.batchCount() == 5 and p.lastBatchSolveKind() == 0
        set_hazard((p, q), hz, 47, 19, 4, 4, 0.5)  # around site 4
        assert p.computeEntireTotalCostMap()
        single = (p.getTotalCostMatrix(), (p.goalI(), p.goalJ()), p.goalCount(),
                  p.lastSolveKind(), p.current_path.copy())

        def single_untouched():
            assert np.array_equal(p.getTotalCostMatrix(), single[0])
            assert ((p.goalI(), p.goalJ()), p.goalCount(), p.lastSolveKind()) == single[1:4]
            assert np.array_equal(p.current_path, single[4])

        assert p.batchCount() == 5  # kept, with the box pending
        assert p.computeTotalCostMaps(sites) is True and p.lastBatchSolveKind() == 1
        print("windowed batch update:", p.lastBatchStats())
        assert p.lastBatchStats()["passes"] > 0
        F2 = F * (1.0 + hz)
        for b in (0, 3, 4):
            check_parity(p.batchTotalCost(b), oracle.fmm(F2, SITES[b])[0])
        M2 = p.getTotalCosts(sites)
        loop = np.empty((5, 5))
        for a, s in enumerate(sites):  # one setGoal + solve per site, on a planner of its own
            assert q.setGoal(s) and q.computeEntireTotalCostMap()
            loop[a] = [q.getTotalCost(t) for t in sites]
        assert np.array_equal(np.isinf(M2), np.isinf(loop))
        fin = np.isfinite(loop) & (loop != 0)
        rel = (np.abs(M2[fin] - loop[fin]) / np.abs(loop[fin])).max()
        print(f"cost matrix after the update: max relative difference {rel:.3e}")
        assert rel <= 1e-12
        assert M2[0, 4] > M[0, 4]  # site 4's own cell got slower
        single_untouched()
        # nothing pending: reused, values unchanged
        assert p.computeTotalCostMaps(sites) is True and p.lastBatchSolveKind() == 2
        assert np.array_equal(p.getTotalCosts(sites), M2)
        # a reader between the synchronisation and computeTotalCostMaps sees the new speed
        set_hazard((p,), hz, 60, 50, 3, 3, 0.3)
        assert p.computeEntireTotalCostMap()
        single = (p.getTotalCostMatrix(), *single[1:3], p.lastSolveKind(), single[4])
        F3 = F * (1.0 + hz)
        T0new = oracle.fmm(F3, SITES[0])[0]
        assert not np.array_equal(T0new, oracle.fmm(F2, SITES[0])[0])
        check_parity(p.batchTotalCost(0), T0new)
        assert p.lastBatchSolveKind() == 1 and p.batchCount() == 5
        assert p.computeTotalCostMaps(sites) is True and p.lastBatchSolveKind() == 2
        single_untouched()
        # another goal list: cold
        assert p.computeTotalCostMaps(sites[:3]) is True
        assert p.lastBatchSolveKind() == 0 and p.batchCount() == 3
        check_parity(p.batchTotalCost(2), oracle.fmm(F3, SITES[2])[0])
        single_untouched()
        # a change over more than half the grid: cold
        set_hazard((p,), hz, 5, 5, 80, 70, 0.1)
        assert p.computeEntireTotalCostMap()
        assert p.batchCount() == 3
        assert p.computeTotalCostMaps(sites[:3]) is True and p.lastBatchSolveKind() == 0
        check_parity(p.batchTotalCost(1), oracle.fmm(F * (1.0 + hz), SITES[1])[0])
    finally:
        p.close()
        q.close()


def test_planner_batch_untracked_is_dropped(dymu, oracle):
    F = site_map(oracle)
    sites = [(OFF[0] + i, OFF[1] + j, 0.0, h) for (i, j), h in zip(SITES, HEADINGS)]
    p = make_planner(dymu, F)
    try:
        assert p.setGoal(sites[1]) and p.computeEntireTotalCostMap()
        assert p.costMatrix(sites, sites) is not None and p.batchCount() == 5
        assert p.setHazardDensityWindow(47, 19, np.full((4, 4), 0.5))
        assert p.computeEntireTotalCostMap()
        assert p.batchCount() == 0 and p.lastBatchSolveKind() == 0
        assert p.getTotalCosts(sites) is None
    finally:
        p.close()


# ---- 6. the planner's goal set ----

def test_planner_goal_set_tracks_speed_changes(dymu, oracle):
    p, F, seeds, goals, _ = ref.planner_case(dymu, oracle)
    try:
        p.trackSpeedChanges(True)
        assert p.setGoals(goals, ref.OFFSETS)
        assert p.computeEntireTotalCostMap() and p.lastSolveKind() == 0
        assert p.setHazardDensityWindow(45, 20, np.full((5, 5), 0.5))  # away from the goals
        assert p.computeEntireTotalCostMap() and p.lastSolveKind() == 1
        F2 = F.copy()
        F2[20:25, 45:50] *= 1.5
        T = p.totalCostRaw()
        check_parity(T, ref.fmm_seeds(oracle, F2, seeds))
        assert np.array_equal(p.goalLabels(), ref.labels_from_T(T, seeds))
        assert np.array_equal(p.nodeStates().astype(bool), np.isfinite(T))
        assert p.computeEntireTotalCostMap() and p.lastSolveKind() == 2
        assert np.array_equal(p.totalCostRaw(), T)
        assert p.setGoals(goals, [0.0, 2.5, 0.0])  # another offset: another boundary value
        assert p.computeEntireTotalCostMap() and p.lastSolveKind() == 0
        seeds2 = [(i, j, t0) for (i, j, _), t0 in zip(seeds, [0.0, 2.5, 0.0])]
        check_parity(p.totalCostRaw(), ref.fmm_seeds(oracle, F2, seeds2))
    finally:
        p.close()


# ---- 7. the size a rover plans on ----

def test_eight_planes_of_1024_updated(dymu, oracle):
    N, B = 1024, 8
    goals = [(512, 512), (100, 120), (900, 80), (130, 880), (940, 930), (512, 40), (30, 512),
             (700, 300)]
    with dymu.Engine() as eng:
        P = dymu.batch_plane_rows(N)
        src, dF, dT = eng.alloc(8 * N * N), eng.alloc(8 * B * P * N), eng.alloc(8 * B * P * N)
        try:
            eng.synth_speed(src, N, N, N, 0, 1, 0.02, 3, 512, 512)
            F = np.empty((N, N))
            eng.d2h(F, src)
            goals = [(i + int(np.argmax(np.isfinite(F[j, i:]))), j) for i, j in goals]
            seeds = [(b, *g) for b, g in enumerate(goals)]
            eng.stack_speed(src, N, 0, N, N, B, dF, N)
            cold = eng.solve_batch_device(dF, dT, N, N, B, N, seeds)
            inner, _ = disc(N, N, (300, 600), 20)  # a hazard disc
            F[inner] *= 2.0
            i0, j0, w, h = window_of(inner)
            eng.h2d(src, F)
            eng.stack_speed(src, N, 0, N, N, B, dF, N)
            st = eng.update_batch_window_device(dF, dT, N, N, B, N, seeds,
                                                [(b, i0, j0, w, h) for b in range(B)])
            print(f"8 x 1024^2 update: {st['passes']} passes, {st['tile_visits']} tile visits, "
                  f"{st['ms']:.3f} ms, {eng.last_update_stats()['cells_invalidated']} cells reset "
                  f"(cold: {cold['passes']} passes, {cold['tile_visits']} visits, "
                  f"{cold['ms']:.3f} ms)")
            assert st["kernel"] == 5
            T = np.empty((P, N))
            for b in (1, 6):
                eng._lib.dymu_memcpy_d2h(eng.ctx, T.ctypes.data, dT + 8 * b * P * N, T.nbytes)
                assert np.isposinf(T[N:]).all()
                check_parity(T[:N], oracle.fmm(F, goals[b])[0])
        finally:
            for ptr in (src, dF, dT):
                eng.free(ptr)
