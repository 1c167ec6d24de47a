"""Early exit on target cells for seeded and batched solves.

The yardstick is the oracle FMM of every plane on its own, T_ref.  With the level t_closed
a solve returns and m = 1e-12 max(1, t_closed), the project's parity bound: every cell
with T_ref <= t_closed - m and every counting target (finite speed) is finite exactly
where T_ref is and within 1e-12 max(1, T_ref) of it.  Cells with t_closed - m < T_ref <=
t_closed that are no targets could fall on either side of the level; check_until asserts
that a case has none (the zone is about 1e-12 wide).  A case's references are computed
once and shared."""
import ctypes

import numpy as np
import pytest

import goalset_ref as ref
from test_gpu_batch import SHAPES, Stack, check_parity, goal_of, seeds_for

pytestmark = pytest.mark.gpu

# priority kernels with small per-pass targets, so that tiles are deferred on test-sized
# grids; every assertion about exiting early checks after every pass
KERNELS = {4: dict(kernel=4, prio_target=64), 5: dict(kernel=5, prio_target=16)}


class Case:
    pass


def until(s, seeds, targets):
    return s.eng.solve_batch_until_device(s.dF, s.dT, s.nx, s.ny, s.B, s.ld, seeds, targets)


def check_until(T, T_ref, F, t_closed, targets):
    """The yardstick on one plane; targets: that plane's (i, j)."""
    if np.isinf(t_closed):
        return check_parity(T, T_ref)
    m = 1e-12 * max(1.0, t_closed)
    tm = np.zeros(T.shape, dtype=bool)
    for i, j in targets:
        tm[j, i] = np.isfinite(F[j, i])  # the counting ones
    zone = (T_ref > t_closed - m) & (T_ref <= t_closed) & ~tm
    assert not zone.any(), np.argwhere(zone)
    sel = (T_ref <= t_closed - m) | tm
    assert np.array_equal(np.isinf(T[sel]), np.isinf(T_ref[sel]))
    fin = sel & np.isfinite(T_ref)
    rel = (np.abs(T[fin] - T_ref[fin]) / np.maximum(1.0, T_ref[fin])).max()
    print(f"level {t_closed:.6g}: {fin.sum()} of {np.isfinite(T_ref).sum()} cells final, "
          f"max |dT| / max(1, T) = {rel:.3e}")
    assert rel <= 1e-12


def plane_max(T, F, targets):
    """Bits of the largest downloaded value among a plane's counting targets (0: none)."""
    v = [T[j, i] for i, j in targets if np.isfinite(F[j, i])]
    return np.float64(max(v) if v else 0.0).view(np.uint64)


def near_targets(goal, nx, ny):
    """Four cells within about 12 cells of a goal, clipped to the plane."""
    gi, gj = goal
    cand = [(gi + 9, gj + 7), (gi - 8, gj - 6), (gi + 3, gj - 11), (gi - 5, gj + 10)]
    out = []
    for i, j in cand:
        c = (min(max(i, 0), nx - 1), min(max(j, 0), ny - 1))
        if c not in out and c != goal:
            out.append(c)
    return out


@pytest.fixture(scope="module", params=sorted(SHAPES))
def field(request, oracle):
    """Five planes of one shape, each with its own speed, obstacles and goal beside a wall,
    3-4 targets near every goal, and the FMM of each plane."""
    c = Case()
    c.nx, c.ny = SHAPES[request.param]
    c.goals = [goal_of(b, c.nx, c.ny) for b in range(5)]
    c.F = np.stack([oracle.synth_speed(c.nx, c.ny, seed=(b + 1) << 20 | 30, obst_frac=0.02,
                                       obst_seed=(b + 1) << 22 | 5, goal=c.goals[b])
                    for b in range(5)])
    c.targets = [near_targets(c.goals[b], c.nx, c.ny) for b in range(5)]
    c.far = (c.nx - 1, 0)  # plane 1's goal is on row 0 at column 11: the far corner
    c.F[1, c.far[1], c.far[0]] = 2.0
    for b in range(5):
        assert 3 <= len(c.targets[b]) <= 4
        for i, j in c.targets[b]:  # every target counts
            if not np.isfinite(c.F[b, j, i]):
                c.F[b, j, i] = 3.0
    c.T_ref = [oracle.fmm(c.F[b], c.goals[b])[0] for b in range(5)]
    return c


# ---- 1. stack parity and early exit ----
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_stack_parity_and_early_exit(dymu, field, kernel):
    B = 5
    seeds = [(b, *field.goals[b]) for b in range(B)]
    tg = [(b, i, j) for b in range(B) for i, j in field.targets[b]]
    with dymu.Engine(passes_per_check=1, **KERNELS[kernel]) as eng:
        s = Stack(dymu, eng, field.F)
        try:
            tc, tp, st = until(s, seeds, tg)
            T, walls = s.planes(s.download(s.dT).copy())
            full = s.solve(seeds)
        finally:
            s.close()
    assert st["kernel"] == kernel
    assert np.isposinf(walls).all()
    assert np.isfinite(tc) and tc == tp.max()
    for b in range(B):
        assert tp[b].view(np.uint64) == plane_max(T[b], field.F[b], field.targets[b])
        check_until(T[b], field.T_ref[b], field.F[b], tc, field.targets[b])
    print(f"passes {st['passes']} of {full['passes']}, visits {st['tile_visits']} of "
          f"{full['tile_visits']}")
    assert st["passes"] < full["passes"]


def test_plain_kernel_option_runs_a_priority_kernel(dymu, field):
    B = 2
    with dymu.Engine(kernel=3, passes_per_check=1) as eng:
        s = Stack(dymu, eng, field.F[:B])
        try:
            tc, tp, st = until(s, [(b, *field.goals[b]) for b in range(B)],
                               [(b, i, j) for b in range(B) for i, j in field.targets[b]])
            T, _ = s.planes(s.download(s.dT))
        finally:
            s.close()
    assert st["kernel"] == 4
    for b in range(B):
        check_until(T[b], field.T_ref[b], field.F[b], tc, field.targets[b])


# ---- 2. planes stop at different levels ----
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_planes_stop_at_different_levels(dymu, field, kernel):
    far, F, refs = field.far, field.F[:2], field.T_ref[:2]
    tgs = [field.targets[0], [far]]
    with dymu.Engine(passes_per_check=1, **KERNELS[kernel]) as eng:
        s = Stack(dymu, eng, F)
        try:
            tc, tp, st = until(s, [(b, *field.goals[b]) for b in range(2)],
                               [(b, i, j) for b in range(2) for i, j in tgs[b]])
            T, _ = s.planes(s.download(s.dT))
        finally:
            s.close()
    assert tp[0] < tp[1] == tc and np.isfinite(tc)
    assert tp[1].view(np.uint64) == T[1, far[1], far[0]].view(np.uint64)
    # plane 0 is final up to the stack's level, not merely up to its own
    assert (refs[0] <= tc).sum() > (refs[0] <= tp[0]).sum()
    for b in range(2):
        check_until(T[b], refs[b], F[b], tc, tgs[b])


# ---- 3. ignored and blocking targets ----
def test_ignored_and_blocking_targets(dymu, field, oracle):
    B = 3
    seeds = [(b, *field.goals[b]) for b in range(B)]
    near = [(b, i, j) for b in range(2) for i, j in field.targets[b]]  # plane 2: no target
    F = field.F[:B].copy()
    ti, tj = field.targets[0][0]
    obst = (ti + 1, tj)  # an obstacle cell beside a near target
    F[0, obst[1], obst[0]] = np.inf
    ring = (40, 30)  # plane 1: a finite-speed cell walled in by a 3x3 ring of obstacles
    F[1, ring[1] - 1:ring[1] + 2, ring[0] - 1:ring[0] + 2] = np.inf
    F[1, ring[1], ring[0]] = 2.0
    refs = [oracle.fmm(F[b], field.goals[b])[0] for b in range(B)]
    assert np.isinf(refs[1][ring[1], ring[0]])
    # bit-reproducible maps, so that "the same" below is exact
    with dymu.Engine(deterministic=1, passes_per_check=1) as eng:
        s = Stack(dymu, eng, F)
        try:
            tc0, tp0, st0 = until(s, seeds, near)
            T0, _ = s.planes(s.download(s.dT).copy())
            tc1, tp1, st1 = until(s, seeds, near + [(0, *obst)])
            tc2, tp2, st2 = until(s, seeds, near + [(1, *ring)])
            T2, walls = s.planes(s.download(s.dT).copy())
            full = s.solve(seeds)
        finally:
            s.close()
    # the obstacle target changes nothing; the plane without a target reports 0.0
    assert np.isfinite(tc0) and tc1 == tc0 and np.array_equal(tp1, tp0)
    assert tp0[2] == 0.0 and tp0[0] > 0 and tp0[1] > 0
    for b in range(B):
        check_until(T0[b], refs[b], F[b], tc0, [t[1:] for t in near if t[0] == b])
    assert st0["passes"] < full["passes"]
    # the walled-in target keeps the whole stack running to convergence
    assert np.isposinf(tc2) and np.isposinf(tp2[1]) and tp2[0] == tp0[0] and tp2[2] == 0.0
    assert np.isposinf(walls).all()
    for b in range(B):
        check_parity(T2[b], refs[b])


# ---- 4. a target on a seed ----
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_target_on_a_seed(dymu, field, kernel):
    """Two passes: the checkerboard of kernel 5 can defer the seed's tile once, then its
    visit raises every queued key above 0.5.  That presumes the visit ends converged.
    Kernel 5 caps a visit at 16 sweeps by default and re-queues a capped tile under its
    old key -- here 0.5, which the stop test has to honour (two more passes per capped
    visit: 4 passes on 97x61 and 96x63, where the goal's row is inside its tile; DESIGN.md
    s5.9).  max_inner lifts the cap to 4 (tile_w + tile_h) sweeps, the engine's own rule
    for the 8x8 kernels, so that the bound tests the stop test and not the cap."""
    B = 2
    seeds = [(b, *field.goals[b], 0.5) for b in range(B)]
    with dymu.Engine(passes_per_check=1, max_inner=4 * (16 + 16), **KERNELS[kernel]) as eng:
        s = Stack(dymu, eng, field.F[:B])
        try:
            tc, tp, st = until(s, seeds, [(0, *field.goals[0])])
            T, _ = s.planes(s.download(s.dT))
        finally:
            s.close()
    gi, gj = field.goals[0]
    assert tc == 0.5 and tp[0] == 0.5 and tp[1] == 0.0
    assert T[0, gj, gi].view(np.uint64) == np.float64(0.5).view(np.uint64)
    assert st["passes"] <= 2


# ---- 5. the single map ----
@pytest.fixture(scope="module")
def single(oracle):
    c = Case()
    c.nx, c.ny = 97, 61
    c.seeds = seeds_for(c.nx, c.ny)
    c.F = oracle.synth_speed(c.nx, c.ny, seed=21, obst_frac=0.02, goal=(20, 20))
    c.targets = [(33, 28), (c.nx - 16, c.ny - 20)]
    for i, j in [sd[:2] for sd in c.seeds] + c.targets:
        if not np.isfinite(c.F[j, i]):
            c.F[j, i] = 3.0
    c.T_ref = ref.fmm_seeds(oracle, c.F, c.seeds)
    return c


class Map:
    def __init__(self, eng, F):
        self.eng = eng
        self.ny, self.nx = F.shape
        self.dF, self.dT = eng.alloc(F.nbytes), eng.alloc(F.nbytes)
        eng.h2d(self.dF, F)

    def T(self):
        a = np.empty((self.ny, self.nx))
        self.eng.d2h(a, self.dT)
        return a

    def close(self):
        self.eng.free(self.dF)
        self.eng.free(self.dT)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_single_map(dymu, single, kernel):
    nx, ny = single.nx, single.ny
    with dymu.Engine(passes_per_check=1, **KERNELS[kernel]) as eng:
        mp = Map(eng, single.F)
        try:
            tc, st = eng.solve_seeds_until_device(mp.dF, mp.dT, nx, ny, nx, single.seeds,
                                                  single.targets)
            T = mp.T()
            full = eng.solve_seeds_device(mp.dF, mp.dT, nx, ny, nx, single.seeds)
        finally:
            mp.close()
    assert st["kernel"] == kernel and np.isfinite(tc)
    assert tc.hex() == max(T[j, i] for i, j in single.targets).hex()
    check_until(T, single.T_ref, single.F, tc, single.targets)
    assert st["passes"] < full["passes"]


def test_single_map_equals_solve_until(dymu, single):
    nx, ny = single.nx, single.ny
    goal, start = (20, 20), (60, 41)
    nb = [start, (start[0], start[1] - 1), (start[0] - 1, start[1]), (start[0] + 1, start[1]),
          (start[0], start[1] + 1)]
    F = single.F.copy()
    for i, j in nb:
        if not np.isfinite(F[j, i]):
            F[j, i] = 3.0
    with dymu.Engine(deterministic=1) as a, dymu.Engine(deterministic=1) as b:
        ma, mb = Map(a, F), Map(b, F)
        try:
            want, _ = a.solve_until_device(ma.dF, ma.dT, nx, ny, nx, *goal, *start)
            got, st = b.solve_seeds_until_device(mb.dF, mb.dT, nx, ny, nx, [(*goal, 0.0)], nb)
        finally:
            ma.close()
            mb.close()
    assert st["kernel"] == 5
    assert np.isfinite(want) and got.hex() == want.hex()


# ---- 6. pitch and ragged edge ----
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_pitch_and_ragged_edge(dymu, oracle, kernel):
    nx, ny, B = 17, 15, 3  # P = 16: one wall row, the last column a tile of its own
    goals = [(3, 3), (8, 7), (12, 2)]
    F = np.stack([oracle.synth_speed(nx, ny, seed=(b + 1) << 20 | 7) for b in range(B)])
    tgs = [[(nx - 1, 9), (5, ny - 1)], [(nx - 1, ny - 1)], [(nx - 1, 0), (0, ny - 1), (16, 14)]]
    refs = [oracle.fmm(F[b], goals[b])[0] for b in range(B)]
    with dymu.Engine(passes_per_check=1, **KERNELS[kernel]) as eng:
        s = Stack(dymu, eng, F, ld=nx + 5)
        assert s.P == 16
        try:
            tc, tp, st = until(s, [(b, *goals[b]) for b in range(B)],
                               [(b, i, j) for b in range(B) for i, j in tgs[b]])
            T, walls = s.planes(s.download(s.dT))
        finally:
            s.close()
    assert np.isposinf(walls).all()
    assert np.isfinite(tc) and tc == tp.max()
    for b in range(B):
        assert tp[b].view(np.uint64) == plane_max(T[b], F[b], tgs[b])
        check_until(T[b], refs[b], F[b], tc, tgs[b])


# ---- 7. determinism ----
def test_deterministic_runs_are_bit_identical(dymu, field):
    B = 5
    seeds = [(b, *field.goals[b]) for b in range(B)]
    tg = [(b, i, j) for b in range(B) for i, j in field.targets[b]]
    with dymu.Engine(deterministic=1, passes_per_check=1) as eng:
        s = Stack(dymu, eng, field.F)
        try:
            tc1, tp1, st1 = until(s, seeds, tg)
            T1 = s.download(s.dT).copy()
            tc2, tp2, st2 = until(s, seeds, tg)
            T2 = s.download(s.dT)
        finally:
            s.close()
    assert st1["kernel"] == 5 and st1["passes"] == st2["passes"]
    assert tc1 == tc2 and np.array_equal(tp1, tp2)
    assert np.array_equal(T1.view(np.uint64), T2.view(np.uint64))
    for b in range(B):
        check_until(s.planes(T1)[0][b], field.T_ref[b], field.F[b], tc1, field.targets[b])


# ---- 8. argument errors ----
def test_argument_errors(dymu, engine, field):
    B, nx, ny = 3, field.nx, field.ny
    s = Stack(dymu, engine, field.F[:B])
    seeds = [(b, *field.goals[b]) for b in range(B)]
    good = [(b, *field.targets[b][0]) for b in range(B)]
    bad = {
        "no targets": (seeds, []),
        "plane >= B": (seeds, good + [(B, 5, 5)]),
        "i >= nx": (seeds, good + [(0, nx, 5)]),
        "j >= ny (a wall row)": (seeds, good + [(0, 5, ny)]),
        "a plane without a seed": (seeds[:2], good),
    }
    try:
        for what, (sd, tg) in bad.items():
            with pytest.raises(dymu.DymuError) as e:
                until(s, sd, tg)
            assert e.value.status == -1, what
        with pytest.raises(dymu.DymuError) as e:
            engine.solve_seeds_until_device(s.dF, s.dT, nx, ny, nx, [(5, 5, 0.0)], [])
        assert e.value.status == -1
        with pytest.raises(dymu.DymuError) as e:
            engine.solve_seeds_until_device(s.dF, s.dT, nx, ny, nx, [(5, 5, 0.0)], [(5, ny)])
        assert e.value.status == -1
        tc, tp, st = until(s, seeds, good)  # the engine is fine afterwards
        assert np.isfinite(tc) and len(tp) == B
    finally:
        s.close()


# ---- 9. the natural kernel 5 ----
def test_natural_kernel_5_at_512(dymu, oracle):
    """Default engine and cadence: 4 planes of one shared config-3 map of 512^2, 8 target
    points within 40 cells of goal 0 in every plane."""
    N, B = 512, 4
    goals = [(256, 256), (60, 70), (450, 90), (100, 440)]
    rng = np.random.default_rng(11)
    pts = [(256 + int(dx), 256 + int(dy)) for dx, dy in rng.integers(-28, 29, size=(8, 2))]
    with dymu.Engine() as eng:
        P = dymu.batch_plane_rows(N)
        src, dF, dT = eng.alloc(8 * N * N), eng.alloc(8 * B * P * N), eng.alloc(8 * B * P * N)
        try:
            eng.synth_speed(src, N, N, N, 0, 1, 0.02, 3, 256, 256)
            F = np.empty((N, N))
            eng.d2h(F, src)
            goals = [(i + int(np.argmax(np.isfinite(F[j, i:]))), j) for i, j in goals]
            eng.stack_speed(src, N, 0, N, N, B, dF, N)
            seeds = [(b, *g) for b, g in enumerate(goals)]
            tc, tp, st = eng.solve_batch_until_device(
                dF, dT, N, N, B, N, seeds, [(b, i, j) for b in range(B) for i, j in pts])
            T = np.empty((B, P, N))
            eng.d2h(T, dT)
            full = eng.solve_batch_device(dF, dT, N, N, B, N, seeds)
        finally:
            for ptr in (src, dF, dT):
                eng.free(ptr)
    print(f"4 x 512^2 until: {st['passes']} passes, {st['tile_visits']} visits, "
          f"{st['ms']:.3f} ms; full: {full['passes']} passes, {full['tile_visits']} visits, "
          f"{full['ms']:.3f} ms; level {tc:.6g}, per plane {tp}")
    assert st["kernel"] == 5 and np.isfinite(tc) and tc == tp.max() and tp[0] < tc
    assert np.isposinf(T[:, N:]).all()
    for b in range(B):
        check_until(T[b, :N], oracle.fmm(F, goals[b])[0], F, tc, pts)


# ---- 10. the planner ----
OFF = (100.0, 200.0)


def planner_pair(dymu, F):
    out = []
    for _ in range(2):
        p = dymu.Planner(risk_distance=0.5)
        # bit-reproducible maps, so that two cold solves give the same paths
        o = dymu.DymuOpts(-1, 0, 0, 0, 0, 0, 0, 0, 1)
        assert p._lib.dymu_planner_set_engine_options(p.h, ctypes.byref(o)) == 0
        assert p.initGlobalLayer(1.0, 0.5, F.shape[1], F.shape[0], offset=OFF)
        assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
        out.append(p)
    return out


@pytest.mark.parametrize("N", ["97x61", "512x512"])
def test_planner_cost_matrix_until(dymu, oracle, N):
    nx, ny = (int(v) for v in N.split("x"))
    sites = [(30, 25), (44, 31), (36, 40), (52, 22)]
    F = oracle.synth_speed(nx, ny, seed=17, obst_frac=0.02, goal=sites[0])
    for i, j in sites:
        blk = F[j - 1:j + 2, i - 1:i + 2]
        blk[~np.isfinite(blk)] = 3.0
    oj, oi = np.nonzero(np.isinf(F[20:45, 25:55]))
    assert len(oi) > 0
    beside = (25 + oi[0] - 0.6, 20 + oj[0] - 0.7)  # a point with an obstacle corner
    goals = [(OFF[0] + i, OFF[1] + j, 0.0, 0.1 * k) for k, (i, j) in enumerate(sites)]
    targets = [(OFF[0] + i, OFF[1] + j) for i, j in sites] + \
        [(OFF[0] + 40.3, OFF[1] + 30.6), (OFF[0] + beside[0], OFF[1] + beside[1])]
    far = [(OFF[0] + nx - 4.5, OFF[1] + ny - 3.25), (OFF[0] + 2.5, OFF[1] + ny - 6.0),
           (OFF[0] + nx - 8.0, OFF[1] + 3.75)]
    starts = [(OFF[0] + x, OFF[1] + y, 0.0, 0.0) for x, y in
              np.random.default_rng(5).uniform([2, 2], [nx - 3, ny - 3], size=(12, 2))]
    p, q = planner_pair(dymu, F)
    try:
        want = q.costMatrix(goals, targets)
        got = p.costMatrix(goals, targets, until=True)
        assert got is not None and got.shape == want.shape == (4, 6)
        assert np.array_equal(np.isinf(got), np.isinf(want))
        fin = np.isfinite(want)
        rel = (np.abs(got[fin] - want[fin]) / np.maximum(1.0, want[fin])).max()
        print(f"until: {p.lastBatchStats()['passes']} passes, full: "
              f"{q.lastBatchStats()['passes']}; level {p.batchLevel():.6g}; max rel {rel:.3e}")
        assert rel <= 1e-12 and fin.sum() >= 20
        assert p.batchCount() == 4 and p.lastBatchStats()["passes"] > 0
        T0 = q.batchTotalCost(0)
        assert np.isfinite(p.batchLevel()) and p.batchLevel() < T0[np.isfinite(T0)].max()
        assert np.isposinf(q.batchLevel())
        # a reader completes the truncated batch first
        a, b = p.getTotalCosts(far), q.getTotalCosts(far)
        assert np.isposinf(p.batchLevel()) and p.lastBatchSolveKind() == 0
        assert np.array_equal(np.isinf(a), np.isinf(b))
        fa = np.isfinite(b)
        assert fa.any() and (np.abs(a[fa] - b[fa]) <= 1e-12 * np.maximum(1.0, b[fa])).all()
        # ... and so does getPathsTo, straight after another truncated solve
        assert p.costMatrix(goals, targets, until=True) is not None
        assert np.isfinite(p.batchLevel())
        paths, status = p.getPathsTo(2, starts)
        wpaths, wstatus = q.getPathsTo(2, starts)
        assert np.isposinf(p.batchLevel()) and p.lastBatchSolveKind() == 0
        assert np.array_equal(status, wstatus) and (status == 1).sum() >= 8
        for x, w in zip(paths, wpaths):
            assert np.array_equal(x, w, equal_nan=True)
        # the same goals after a truncated solve: a cold solve, never a reuse
        p.trackSpeedChanges(True)
        assert p.costMatrix(goals, targets, until=True) is not None
        assert p.computeTotalCostMaps(goals) and p.lastBatchSolveKind() == 0
        assert np.isposinf(p.batchLevel())
        assert p.computeTotalCostMaps(goals) and p.lastBatchSolveKind() == 2
    finally:
        p.close()
        q.close()
