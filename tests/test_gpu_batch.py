"""Batched solves on the device: B maps stacked into one domain behind
+inf wall rows and solved in one pass sequence.  The yardstick is the oracle FMM of every
plane on its own (goalset_ref.fmm_seeds for several seeds) under the project's bound --
the same +inf mask and |dT| <= 1e-12 max(1, T); the gather kernel is compared exactly
with Planner.getTotalCost.  A case's reference maps are computed once and shared."""
import numpy as np
import pytest

import goalset_ref as ref

pytestmark = pytest.mark.gpu

# test_gpu_goal_sets.py's kernels: small per-pass targets so that the priority kernels
# defer tiles on test-sized grids
KERNELS = {3: dict(kernel=3), 4: dict(kernel=4, prio_target=64), 5: dict(kernel=5, prio_target=16)}


def seeds_for(nx, ny):
    """test_gpu_goal_sets.py's six seeds."""
    return [(20, 20, 0.0), (22, 21, 0.5),  # two in one tile (8- and 16-cell)
            (nx - 10, ny - 12, 0.25),      # a far tile
            (0, 30, 1.0),                  # a grid-edge cell
            (20, 20, 3.0),                 # a duplicate cell with a larger t0
            (24, 22, 1e6)]                 # dominated: its cell ends far below its t0


def check_parity(T, T_ref):
    """|dT| <= 1e-12 max(1, T) and the same +inf mask (the parity bound of dymu_fim.h)."""
    assert np.array_equal(np.isinf(T), np.isinf(T_ref))
    fin = np.isfinite(T_ref)
    rel = (np.abs(T[fin] - T_ref[fin]) / np.maximum(1.0, T_ref[fin])).max()
    print(f"max |dT| / max(1, T) = {rel:.3e}")
    assert rel <= 1e-12

# 97x61: three wall rows; 96x63: exactly one; 96x96: the wall is a tile row of its own
SHAPES = {"97x61": (97, 61), "96x63": (96, 63), "96x96": (96, 96)}
BLOCKED = 2  # the plane that is all obstacles except its goal


class Case:
    pass


class Stack:
    """B planes on the device: the per-plane source maps, the stacked F and T."""

    def __init__(self, dymu, eng, F, B=None, ld=None):
        """F: [B, ny, nx] per-plane speeds, or [ny, nx] with B for one shared map."""
        self.eng = eng
        F = np.ascontiguousarray(F, dtype=np.float64)
        shared = F.ndim == 2
        self.B = B if shared else F.shape[0]
        self.ny, self.nx = F.shape[-2:]
        self.P = dymu.batch_plane_rows(self.ny)
        self.ld = ld or self.nx
        self.rows = self.B * self.P
        self.src = eng.alloc(F.nbytes)
        self.dF = eng.alloc(8 * self.rows * self.ld)
        self.dT = eng.alloc(8 * self.rows * self.ld)
        eng.h2d(self.src, F)
        eng.stack_speed(self.src, self.nx, 0 if shared else self.nx * self.ny, self.nx, self.ny,
                        self.B, self.dF, self.ld)

    def solve(self, seeds):
        return self.eng.solve_batch_device(self.dF, self.dT, self.nx, self.ny, self.B, self.ld,
                                           seeds)

    def download(self, ptr):
        a = np.empty((self.rows, self.ld))
        self.eng.d2h(a, ptr)
        return a[:, :self.nx]

    def planes(self, a):
        """([B, ny, nx] maps, [B, P - ny, nx] wall rows) of a downloaded stack."""
        a = a.reshape(self.B, self.P, self.nx)
        return a[:, :self.ny], a[:, self.ny:]

    def close(self):
        for p in (self.src, self.dF, self.dT):
            self.eng.free(p)


def goal_of(b, nx, ny):
    """Goals beside the walls: the last row of even planes, the first row of odd ones, so
    that the goals of planes b and b + 1 (b even) face each other across a wall."""
    return (11 + 13 * b, ny - 1) if b % 2 == 0 else (11 + 13 * (b - 1), 0)


@pytest.fixture(scope="module", params=sorted(SHAPES))
def field(request, oracle):
    """Five planes of one shape, each with its own speed, obstacles and goal, and the
    FMM of each."""
    c = Case()
    c.nx, c.ny = SHAPES[request.param]
    c.goals = [goal_of(b, c.nx, c.ny) for b in range(5)]
    # the generator hashes seed ^ cell: seeds apart by more than the cell count give
    # unrelated draws (nearby seeds only permute the cells)
    c.F = np.stack([oracle.synth_speed(c.nx, c.ny, seed=(b + 1) << 20 | 30, obst_frac=0.02,
                                       obst_seed=(b + 1) << 22 | 5, goal=c.goals[b])
                    for b in range(5)])
    c.F[BLOCKED] = np.inf
    gi, gj = c.goals[BLOCKED]
    c.F[BLOCKED, gj, gi] = 2.5
    c.T_ref = [oracle.fmm(c.F[b], c.goals[b])[0] for b in range(5)]
    return c


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("B", [1, 5])
def test_isolation_and_parity(dymu, field, B, kernel):
    with dymu.Engine(**KERNELS[kernel]) as eng:
        s = Stack(dymu, eng, field.F[:B])
        try:
            st = s.solve([(b, *field.goals[b]) for b in range(B)])
            T, walls = s.planes(s.download(s.dT))
            Fw = s.planes(s.download(s.dF))[1]
        finally:
            s.close()
    assert st["kernel"] == kernel
    assert s.P - field.ny == {61: 3, 63: 1, 96: 16}[field.ny]
    assert np.isposinf(walls).all() and np.isposinf(Fw).all()
    for b in range(B):
        gi, gj = field.goals[b]
        assert T[b, gj, gi] == 0.0
        check_parity(T[b], field.T_ref[b])
    if B > BLOCKED:
        T[BLOCKED, field.goals[BLOCKED][1], field.goals[BLOCKED][0]] = np.inf
        assert np.isposinf(T[BLOCKED]).all()  # 0 at its goal was all it held


def test_shared_speed_is_replicated_bitwise(dymu, engine, oracle):
    nx, ny, B = 97, 61, 4
    F = oracle.synth_speed(nx, ny, seed=9, obst_frac=0.02, goal=(40, 30))
    F[30, 40:40 + B] = 2.0  # the goals' cells
    s = Stack(dymu, engine, F, B=B, ld=nx + 5)  # a pitched stack
    try:
        planes, walls = s.planes(s.download(s.dF))
        st = s.solve([(b, 40 + b, 30) for b in range(B)])
        T, Tw = s.planes(s.download(s.dT))
    finally:
        s.close()
    for b in range(B):
        assert np.array_equal(planes[b].view(np.uint64), F.view(np.uint64))
    assert walls.shape == (B, 3, nx) and np.isposinf(walls).all() and np.isposinf(Tw).all()
    assert st["passes"] > 0
    for b in (0, B - 1):
        check_parity(T[b], oracle.fmm(F, (40 + b, 30))[0])


@pytest.fixture(scope="module")
def multi(oracle):
    """Two planes: one with the six seeds of seeds_for, one with a single seed."""
    c = Case()
    c.nx, c.ny = SHAPES["97x61"]
    c.seeds = [seeds_for(c.nx, c.ny), [(60, 5, 0.75)]]
    c.F = np.stack([oracle.synth_speed(c.nx, c.ny, seed=b << 20 | 21, obst_frac=0.02,
                                       obst_seed=b << 22 | 3, goal=(20, 20)) for b in range(2)])
    for b, sd in enumerate(c.seeds):
        for i, j, _ in sd:  # no seed on an obstacle
            if not np.isfinite(c.F[b, j, i]):
                c.F[b, j, i] = 3.0
    c.T_ref = [ref.fmm_seeds(oracle, c.F[b], c.seeds[b]) for b in range(2)]
    return c


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_multi_seed_planes(dymu, multi, kernel):
    with dymu.Engine(**KERNELS[kernel]) as eng:
        s = Stack(dymu, eng, multi.F)
        try:
            s.solve([(b, *sd) for b in range(2) for sd in multi.seeds[b]])
            T, walls = s.planes(s.download(s.dT))
        finally:
            s.close()
    assert np.isposinf(walls).all()
    for b in range(2):
        check_parity(T[b], multi.T_ref[b])
    assert T[0, 20, 20] == 0.0 and T[0, 30, 0] == 1.0 and T[1, 5, 60] == 0.75


def test_argument_errors(dymu, engine, field):
    B, nx, ny = 3, field.nx, field.ny
    s = Stack(dymu, engine, field.F[:B])
    good = [(b, *field.goals[b]) for b in range(B)]
    lib, ctx = engine._lib, engine.ctx
    too_many = -(-(1 << 32) // s.P)  # the fewest planes whose rows B * P no longer fit
    assert too_many < 1 << 32 and too_many * s.P > 0xFFFFFFFF >= (too_many - 1) * s.P

    def raw(B_, ld_, seeds):
        a = np.zeros(len(seeds), dtype=dymu.BATCH_SEED_DTYPE)
        for k, sd in enumerate(seeds):
            a[k] = (sd[0], sd[1], sd[2], 0, sd[3] if len(sd) > 3 else 0.0)
        return lib.dymu_solve_batch_device(ctx, s.dF, s.dT, nx, ny, B_, ld_, a.ctypes.data,
                                           len(a), None, None)

    try:
        bad = {
            "B = 0": (0, nx, good),
            "ld < nx": (B, nx - 1, good),
            "plane >= B": (B, nx, good + [(B, 5, 5)]),
            "i off the plane": (B, nx, good + [(0, nx, 5)]),
            "j in the wall rows": (B, nx, good + [(0, 5, ny)]),
            "t0 < 0": (B, nx, good + [(1, 5, 5, -1.0)]),
            "t0 NaN": (B, nx, good + [(1, 5, 5, float("nan"))]),
            "t0 inf": (B, nx, good + [(1, 5, 5, float("inf"))]),
            "a plane without a seed": (B, nx, good[:1] + good[2:]),
            "no seeds": (B, nx, []),
            "B * P beyond uint32": (too_many, nx, good),
        }
        for what, (B_, ld_, seeds) in bad.items():
            assert raw(B_, ld_, seeds) == -1, what
        assert engine._lib.dymu_stack_speed_device(ctx, s.src, nx, 0, nx, ny, too_many, s.dF, nx,
                                                   None) == -1
        assert engine._lib.dymu_stack_speed_device(ctx, s.src, nx - 1, 0, nx, ny, B, s.dF, nx,
                                                   None) == -1
        s.solve(good)  # the context still solves
        T, _ = s.planes(s.download(s.dT))
    finally:
        s.close()
    for b in range(B):
        check_parity(T[b], field.T_ref[b])


def test_deterministic_batches_are_bitwise_equal(dymu, field):
    seeds = [(b, *field.goals[b]) for b in range(5)]
    with dymu.Engine(deterministic=1) as eng:
        s = Stack(dymu, eng, field.F)
        try:
            st = s.solve(seeds)
            T1 = s.download(s.dT).copy()
            s.solve(seeds)
            T2 = s.download(s.dT)
        finally:
            s.close()
    assert st["kernel"] == 5
    assert np.array_equal(T1, T2)
    for b in range(5):
        check_parity(s.planes(T1)[0][b], field.T_ref[b])


def gather_points(F, res, rng):
    """About 200 query points in metres: nodes, cell interiors, points beside obstacles,
    the last row and column, and points off the grid."""
    ny, nx = F.shape
    pts = [(float(i), float(j)) for i, j in rng.integers(0, [nx, ny], size=(50, 2))]
    pts += [tuple(p) for p in rng.uniform([0, 0], [nx - 1, ny - 1], size=(70, 2))]
    oj, oi = np.nonzero(np.isinf(F))
    for k in rng.choice(len(oi), 40, replace=False):
        dx, dy = rng.uniform(-1.2, 1.2, 2)
        pts.append((oi[k] + dx, oj[k] + dy))
    pts += [(nx - 1 - u, v) for u, v in rng.uniform([0, 0], [1.0, ny - 1], size=(15, 2))]
    pts += [(u, ny - 1 - v) for u, v in rng.uniform([0, 0], [nx - 1, 1.0], size=(15, 2))]
    pts += [(nx - 1.0, ny - 1.0), (nx - 0.6, ny - 0.6), (nx - 0.4, 3.0), (3.0, ny - 0.4),
            (-0.3, 5.2), (5.2, -0.3), (-0.7, -0.7), (-5.0, 4.0), (4.0, -5.0), (nx + 10.0, 4.0),
            (4.0, ny + 10.0), (1e30, 2.0), (2.0, -1e30), (0.0, 0.0), (nx - 2.0, ny - 2.0)]
    return res * np.array(pts)


def test_gather_equals_planner_get_total_cost(dymu, engine, field):
    B, res = 3, 0.5  # planes 0, 1 and the blocked one; res != 1 keeps the a = x - i quirk
    xy = gather_points(field.F[0], res, np.random.default_rng(3))
    assert len(xy) >= 200
    s = Stack(dymu, engine, field.F[:B])
    try:
        s.solve([(b, *field.goals[b]) for b in range(B)])
        got = engine.gather_costs(s.dT, s.nx, s.ny, B, s.ld, res, xy)
        T, _ = s.planes(s.download(s.dT))
    finally:
        s.close()
    assert got.shape == (B, len(xy))
    p = dymu.Planner()
    try:
        assert p.initGlobalLayer(res, res / 2, field.nx, field.ny)
        for b in range(B):
            assert p.loadTotalCostMap(T[b])
            want = np.array([p.getTotalCost((x, y)) for x, y in xy])
            assert not np.isnan(want).any()
            assert (got[b] == want).all(), np.nonzero(got[b] != want)
            assert np.isinf(want).any() and (b == BLOCKED or np.isfinite(want).sum() > 100)
    finally:
        p.close()


# ---- the planner end to end ----
OFF = (100.0, 200.0)
NX, NY = 96, 80
SITES = [(12, 9), (70, 40), (30, 66), (85, 70), (48, 20)]
HEADINGS = [0.5, -1.0, 2.0, 0.0, 1.5]


def make_planner(dymu, F):
    p = dymu.Planner(risk_distance=0.5)
    assert p.initGlobalLayer(1.0, 0.5, NX, NY, offset=OFF)
    assert p.setCostMap(np.where(np.isfinite(F), F, -1.0))
    return p


def test_planner_cost_matrix_paths_and_state(dymu, oracle):
    F = oracle.synth_speed(NX, NY, seed=17, obst_frac=0.02, goal=SITES[0])
    for i, j in SITES:
        blk = F[j - 1:j + 2, i - 1:i + 2]
        blk[~np.isfinite(blk)] = 3.0
    sites = [(OFF[0] + i, OFF[1] + j, 0.0, h) for (i, j), h in zip(SITES, HEADINGS)]
    rng = np.random.default_rng(5)
    starts = [(OFF[0] + x, OFF[1] + y, 0.0, 0.01 * k) for k, (x, y) in
              enumerate(rng.uniform([2, 2], [NX - 3, NY - 3], size=(60, 2)))]
    p, q = make_planner(dymu, F), make_planner(dymu, F)
    try:
        assert p.batchCount() == 0 and p.getTotalCosts(sites) is None
        assert p.setGoal(sites[1]) and p.computeEntireTotalCostMap()
        p.getPath(starts[0])
        before = (p.getTotalCostMatrix(), (p.goalI(), p.goalJ()), p.goalCount(),
                  p.lastSolveKind(), p.current_path.copy())
        assert before[1] == SITES[1]
        M = p.costMatrix(sites, sites)
        assert M is not None and M.shape == (5, 5) and p.batchCount() == 5
        print("batch stats:", p.lastBatchStats())
        assert p.lastBatchStats()["passes"] > 0
        # the single-goal state is untouched
        assert np.array_equal(p.getTotalCostMatrix(), before[0])
        assert (p.goalI(), p.goalJ()) == before[1]
        assert (p.goalCount(), p.lastSolveKind()) == before[2:4]
        assert np.array_equal(p.current_path, before[4])
        # an unchanged speed: the next single-goal solve reuses its map
        assert p.computeEntireTotalCostMap() and p.lastSolveKind() == 2
        # paths to goal b on plane b == getPaths on a planner holding that plane and goal
        assert np.array_equal(p.getTotalCosts(sites), M)
        for b in (0, 3):
            Tb = p.batchTotalCost(b)
            assert Tb[SITES[b][1], SITES[b][0]] == 0.0
            check_parity(Tb, oracle.fmm(F, SITES[b])[0])
            assert np.array_equal(np.where(np.isinf(Tb), -1.0, Tb), p.batchTotalCost(b, raw=False))
            paths, status = p.getPathsTo(b, starts)
            assert p.lastPathsOnDevice()
            assert q.setGoal(sites[b]) and q.loadTotalCostMap(Tb)
            want, wstatus = q.getPaths(starts)
            assert np.array_equal(status, wstatus) and (status == 1).sum() >= 50
            assert [len(a) for a in paths] == [len(a) for a in want]
            for a, w in zip(paths, want):
                assert np.array_equal(a, w, equal_nan=True)  # x, y, z, heading
        assert np.array_equal(p.current_path, before[4])
        # the matrix against one solve per site
        loop = np.empty((5, 5))
        for a, s in enumerate(sites):
            assert p.setGoal(s) and p.computeEntireTotalCostMap()
            loop[a] = [p.getTotalCost(t) for t in sites]
        assert p.batchCount() == 5  # the speed did not change
        assert np.array_equal(np.isinf(M), np.isinf(loop))
        fin = np.isfinite(loop) & (loop != 0)
        rel = (np.abs(M[fin] - loop[fin]) / np.abs(loop[fin])).max()
        print(f"cost matrix: max relative difference {rel:.3e}")
        assert rel <= 1e-12
        assert (np.diag(M) == 0.0).all() and (np.diag(loop) == 0.0).all()
        assert (M[~np.eye(5, dtype=bool)] > 0).all()
        # a goal setGoal rejects: nothing changes
        assert p.computeTotalCostMaps(sites[:2] + [(OFF[0], OFF[1] + 5)]) is False
        assert p.batchCount() == 5
        # a hazard change followed by a solve drops the batch
        assert p.setHazardDensityWindow(47, 19, np.full((4, 4), 0.5))  # around site 4
        assert p.computeEntireTotalCostMap()
        assert p.batchCount() == 0
        assert p.getTotalCosts(sites) is None and p.batchTotalCost(0) is None
        # ... and a batch solved after it is that of the new speed
        M2 = p.costMatrix(sites[:2], sites)
        assert M2.shape == (2, 5) and p.batchCount() == 2
        assert p.setGoal(sites[0]) and p.computeEntireTotalCostMap()
        row = np.array([p.getTotalCost(t) for t in sites])
        assert np.allclose(M2[0], row, rtol=1e-12, atol=0)
        assert M2[0, 4] > M[0, 4]  # site 4's own cell got slower
    finally:
        p.close()
        q.close()


def test_batch_speed_change_reaches_the_single_goal_map(dymu, oracle):
    """A speed change first synchronised by a batch solve is not lost for the single
    goal's map: the next computeEntireTotalCostMap re-propagates it."""
    F = oracle.synth_speed(NX, NY, seed=17)
    p = make_planner(dymu, F)
    try:
        site = (OFF[0] + 20, OFF[1] + 20)
        assert p.setGoal(site) and p.computeEntireTotalCostMap()
        T0 = p.totalCostRaw()
        hd = np.full((6, 6), 1.0)
        assert p.setHazardDensityWindow(40, 30, hd)
        assert p.computeTotalCostMaps([site, (OFF[0] + 60, OFF[1] + 50)])
        assert np.array_equal(p.totalCostRaw(), T0)  # not touched by the batch
        assert p.computeEntireTotalCostMap() and p.lastSolveKind() != 2
        F2 = F.copy()
        F2[30:36, 40:46] *= 2.0  # F = res * cost * (2 + hazard - traff)
        check_parity(p.totalCostRaw(), oracle.fmm(F2, (20, 20))[0])
        check_parity(p.batchTotalCost(0), oracle.fmm(F2, (20, 20))[0])
    finally:
        p.close()


def test_eight_planes_of_1024(dymu, oracle):
    """The size a rover plans on: 8 goals on one shared config-3 map of 1024^2."""
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
            # a nominal goal on an obstacle moves right to the next free cell
            goals = [(i + int(np.argmax(np.isfinite(F[j, i:]))), j) for i, j in goals]
            assert all(np.isfinite(F[j, i]) for i, j in goals)
            eng.stack_speed(src, N, 0, N, N, B, dF, N)
            st = eng.solve_batch_device(dF, dT, N, N, B, N, [(b, *g) for b, g in enumerate(goals)])
            print(f"8 x 1024^2: {st['passes']} passes, {st['tile_visits']} tile visits, "
                  f"{st['ms']:.3f} ms")
            assert st["kernel"] == 5
            T = np.empty((P, N))
            for b in (1, 6):
                eng._lib.dymu_memcpy_d2h(eng.ctx, T.ctypes.data, dT + 8 * b * P * N, T.nbytes)
                assert np.isposinf(T[N:]).all()
                check_parity(T[:N], oracle.fmm(F, goals[b])[0])
        finally:
            for ptr in (src, dF, dT):
                eng.free(ptr)
