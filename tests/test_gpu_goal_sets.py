"""Goal sets on the device: the multi-source solve against the reference
FMM over the same seeds, the label map against the definition applied to the downloaded
device T, and Planner.setGoals end to end.  The reference maps of a case are computed
once and shared by its tests."""
import numpy as np
import pytest

import goalset_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = {"96x96": (96, 96), "97x61": (97, 61)}  # ragged against 8- and 16-cell tiles
# small per-pass targets so that the priority kernels defer tiles on test-sized grids
KERNELS = {3: dict(kernel=3), 4: dict(kernel=4, prio_target=64), 5: dict(kernel=5, prio_target=16)}


def seeds_for(nx, ny):
    return [(20, 20, 0.0), (22, 21, 0.5),  # two in one tile (8- and 16-cell)
            (nx - 10, ny - 12, 0.25),      # a far tile
            (0, 30, 1.0),                  # a grid-edge cell
            (20, 20, 3.0),                 # a duplicate cell with a larger t0
            (24, 22, 1e6)]                 # dominated: its cell ends far below its t0


class Case:
    pass


@pytest.fixture(scope="module", params=sorted(SHAPES))
def field(request, oracle):
    """Speed, seeds and the reference FMM of one shape (shared by the kernels)."""
    c = Case()
    c.nx, c.ny = SHAPES[request.param]
    c.seeds = seeds_for(c.nx, c.ny)
    c.F = oracle.synth_speed(c.nx, c.ny, seed=21, obst_frac=0.02, goal=(20, 20))
    for i, j, _ in c.seeds:  # no seed on an obstacle
        if not np.isfinite(c.F[j, i]):
            c.F[j, i] = 3.0
    c.T_ref = ref.fmm_seeds(oracle, c.F, c.seeds)
    return c


class Dev:
    """F and T of one field on the device."""

    def __init__(self, eng, F):
        self.eng, self.F = eng, np.ascontiguousarray(F)
        self.ny, self.nx = F.shape
        self.dF = eng.alloc(F.nbytes)
        self.dT = eng.alloc(F.nbytes)
        eng.h2d(self.dF, self.F)

    def solve_seeds(self, seeds):
        st = self.eng.solve_seeds_device(self.dF, self.dT, self.nx, self.ny, self.nx, seeds)
        return self.T(), st

    def T(self):
        T = np.empty((self.ny, self.nx))
        self.eng.d2h(T, self.dT)
        return T

    def labels(self, seeds):
        return self.eng.goal_labels_device(self.dT, self.nx, self.ny, self.nx, seeds)

    def close(self):
        self.eng.free(self.dF)
        self.eng.free(self.dT)


def check_parity(T, T_ref):
    """|dT| <= 1e-12 max(1, T) and the same +inf mask (the parity bound of dymu_fim.h)."""
    assert np.array_equal(np.isinf(T), np.isinf(T_ref))
    fin = np.isfinite(T_ref)
    rel = (np.abs(T[fin] - T_ref[fin]) / np.maximum(1.0, T_ref[fin])).max()
    print(f"max |dT| / max(1, T) = {rel:.3e}")
    assert rel <= 1e-12


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_solve_and_labels(dymu, field, kernel):
    with dymu.Engine(**KERNELS[kernel]) as eng:
        d = Dev(eng, field.F)
        try:
            T, st = d.solve_seeds(field.seeds)
            assert st["kernel"] == kernel
            check_parity(T, field.T_ref)
            assert T[20, 20] == 0.0 and T[21, 22] == 0.5 and T[30, 0] == 1.0
            assert T[22, 24] < 100.0
            lab, rounds = d.labels(field.seeds)
            assert eng.last_labels_ms() > 0 and 1 <= rounds <= 64
        finally:
            d.close()
    want = ref.labels_from_T(T, field.seeds)  # from the device's own T
    assert lab.dtype == np.uint32 and np.array_equal(lab, want)
    assert not (lab == 5).any()  # the dominated seed is nobody's goal
    assert not (lab == 4).any()  # nor the duplicate with the larger t0
    assert set(np.unique(lab)) == {0, 1, 2, 3, ref.NONE}
    assert (lab[np.isinf(field.F)] == ref.NONE).all()
    assert np.array_equal(lab == ref.NONE, np.isinf(T))


def test_one_seed_deterministic_is_solve_device(dymu, field):
    with dymu.Engine(deterministic=1) as eng:
        d = Dev(eng, field.F)
        try:
            T, _ = d.solve_seeds([(20, 20, 0.0)])
            eng.solve_device(d.dF, d.dT, d.nx, d.ny, d.nx, 20, 20)
            T1 = d.T()
            Tm, _ = d.solve_seeds(field.seeds)
        finally:
            d.close()
    assert np.array_equal(T.view(np.uint64), T1.view(np.uint64))
    check_parity(Tm, field.T_ref)


def test_exact_sqrt(dymu, field):
    with dymu.Engine(kernel=5, exact_sqrt=1) as eng:
        d = Dev(eng, field.F)
        try:
            T, _ = d.solve_seeds(field.seeds)
        finally:
            d.close()
    check_parity(T, field.T_ref)


def test_two_chambers(engine, oracle):
    """A full +inf wall column splits the grid; one seed per chamber."""
    F = oracle.synth_speed(96, 96, seed=5)
    F[:, 48] = np.inf
    seeds = [(10, 10, 0.0), (80, 80, 0.0)]
    d = Dev(engine, F)
    try:
        T, _ = d.solve_seeds(seeds)
        lab, _ = d.labels(seeds)
    finally:
        d.close()
    check_parity(T, ref.fmm_seeds(oracle, F, seeds))
    assert (lab[:, :48] == 0).all() and (lab[:, 49:] == 1).all()
    assert (lab[:, 48] == ref.NONE).all()


def test_long_chains(engine):
    """A serpentine corridor: one chain of ~2000 cells needs ~log2 of that many rounds."""
    N = 128
    F = np.full((N, N), 2.0)
    for q, j in enumerate(range(8, N, 8)):
        F[j, :] = np.inf
        F[j, N - 1 if q % 2 == 0 else 0] = 2.0  # the gap alternates sides
    seeds = [(2, 2, 0.0)]
    d = Dev(engine, F)
    try:
        T, _ = d.solve_seeds(seeds)
        lab, rounds = d.labels(seeds)
    finally:
        d.close()
    assert np.array_equal(np.isinf(T), np.isinf(F))
    assert T.max(where=np.isfinite(T), initial=0.0) > 2.0 * 1500  # the route winds
    assert (lab[np.isfinite(T)] == 0).all() and (lab[np.isinf(T)] == ref.NONE).all()
    print(f"pointer-jumping rounds: {rounds}")
    assert 8 <= rounds <= 64


def test_argument_errors(dymu, engine, field):
    d = Dev(engine, field.F)
    try:
        for bad in ([], [(field.nx, 3, 0.0)], [(3, field.ny, 0.0)], [(3, 3, float("nan"))],
                    [(3, 3, -1.0)], [(3, 3, float("inf"))], [(20, 20, 0.0), (5, 5, float("nan"))]):
            with pytest.raises(dymu.DymuError) as e:
                d.solve_seeds(bad)
            assert e.value.status == -1, bad
            with pytest.raises(dymu.DymuError) as e:
                d.labels(bad)
            assert e.value.status == -1, bad
        T, _ = d.solve_seeds(field.seeds)  # the context still solves
    finally:
        d.close()
    check_parity(T, field.T_ref)


# ---- Planner.setGoals on the device ----

@pytest.fixture(scope="module")
def pcase(dymu, oracle):
    c = Case()
    c.p, c.F, c.seeds, c.goals, c.starts = ref.planner_case(dymu, oracle)
    assert c.p.setGoals(c.goals, ref.OFFSETS)
    assert c.p.computeEntireTotalCostMap()
    c.kind = c.p.lastSolveKind()
    c.labels = c.p.goalLabels()
    c.paths, c.status = c.p.getPaths(c.starts)
    c.on_device = c.p.lastPathsOnDevice()
    c.sinks = c.p.lastPathSinks()
    yield c
    c.p.close()


def test_planner_solve_and_labels(pcase, oracle):
    p = pcase.p
    assert pcase.kind == 0 and p.goalCount() == 3
    T = p.totalCostRaw()
    check_parity(T, ref.fmm_seeds(oracle, pcase.F, pcase.seeds))
    assert np.array_equal(pcase.labels, ref.labels_from_T(T, pcase.seeds))
    assert set(np.unique(pcase.labels)) == {0, 1, 2, ref.NONE}
    assert np.array_equal(p.nodeStates().astype(bool), np.isfinite(T))
    assert len(p.globalNarrowband()) == 0
    order = p.globalPropagatedNodes()
    t = T.ravel()
    fin = np.flatnonzero(np.isfinite(t))
    want = fin[np.lexsort((fin, t[fin]))]
    assert np.array_equal(order[:, 1].astype(np.int64) * ref.NX + order[:, 0], want)
    assert p.computeEntireTotalCostMap() and p.lastSolveKind() == 0  # never reused


def test_planner_paths_device_equals_host(pcase):
    p = pcase.p
    assert pcase.on_device and p.lastPathsKernelMs() > 0
    bad = int((pcase.status != 1).sum())
    print(f"starts not ending at a sink: {bad}/200")
    assert bad <= 10
    assert set(pcase.sinks[pcase.status == 1]) == {0, 1, 2}
    for q, (s, d, st, k) in enumerate(zip(pcase.starts, pcase.paths, pcase.status, pcase.sinks)):
        h = p.getPath(s)  # the host descent on the mirror of the same map
        assert d.shape == h.shape, (q, st)
        assert np.array_equal(d, h, equal_nan=True), (q, st)
        assert (st == 1) == (k >= 0)
        if st == 1:
            gi, gj = ref.GOALS_IJ[k]
            assert tuple(d[-1]) == (ref.OFF[0] + gi, ref.OFF[1] + gj, 0.0, ref.HEADINGS[k])


def test_planner_rejected_starts(dymu):
    """A start off the grid and one in an unreachable pocket: status -1, nothing written."""
    N = 96
    cost = np.full((N, N), 2.0)
    cost[40:45, 40] = cost[40:45, 44] = cost[40, 40:45] = cost[44, 40:45] = -1.0  # a closed ring
    p = dymu.Planner(risk_distance=ref.RD)
    try:
        assert p.initGlobalLayer(1.0, 0.5, N, N, offset=ref.OFF)
        assert p.setCostMap(cost)
        assert p.setGoals([(ref.OFF[0] + 10, ref.OFF[1] + 10), (ref.OFF[0] + 80, ref.OFF[1] + 70)])
        assert p.computeEntireTotalCostMap()
        good = (ref.OFF[0] + 60.3, ref.OFF[1] + 20.7)
        starts = [good, (ref.OFF[0] + 42.3, ref.OFF[1] + 42.4), (ref.OFF[0] - 30.0, ref.OFF[1] + 5.0),
                  (ref.OFF[0] + 5.0, ref.OFF[1] + N + 40.0), (float("nan"), ref.OFF[1] + 5.0), good]
        paths, status = p.getPaths(starts)
        assert p.lastPathsOnDevice()
        assert list(status) == [1, -1, -1, -1, -1, 1]
        assert all(len(q) == 0 for q in paths[1:5])
        assert list(p.lastPathSinks()) == [p.lastPathSinks()[0], -1, -1, -1, -1, p.lastPathSinks()[0]]
        assert p.lastPathSinks()[0] in (0, 1)
        assert np.array_equal(paths[0], paths[-1]) and np.array_equal(paths[0], p.getPath(good))
        assert p.goalLabel((ref.OFF[0] + 42, ref.OFF[1] + 42)) == -1
        assert p.goalLabel((ref.OFF[0] + 12, ref.OFF[1] + 11)) == 0
        # out of scope for a goal set: the local layer declines, state untouched
        cur = p.current_path
        assert p.repairPath(good, 0) == -1
        assert np.array_equal(p.current_path, cur)
    finally:
        p.close()
