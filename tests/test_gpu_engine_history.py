"""What an engine carries from one solve to the next, and what a domain starts from.

An engine keeps its tile-epoch stamps, the three lists with their counters, keys and
histograms, the edge columns, the staged maps of the host path and the mailbox sequence
across solves, each behind a capacity of its own.  dymu_dom_snapshot copies that state out
of the live domain and dymu_debug_raise_epoch_base brings the epoch wrap within reach
(include/dymu_fim.h); the engines here are this file's own, each with a history.

(a) test_domain_starts_clean: whatever ran before, dom_begin leaves exactly the seed's
    tiles stamped, listed and keyed, everything else empty, and the solve meets the oracle.
(b) test_invariants_between_passes: before pass p every listed tile is inside the domain,
    listed once, and stamped eb + p + 1, and no stamp exceeds that.  Every enqueue of a pass
    -- an activation through an edge, a key- or colour-deferred entry, a capped visit
    re-queued -- goes through one path that stamps the epoch of the list it appends to
    (`enqueue` in the pass kernels), so the rule has no exception.
(c) test_epoch_wrap: the guard that restarts the 32-bit epochs must clear every stamp of the
    array, not the current domain's tiles only.
(d) test_tiny_first_grid_*: DESIGN.md s8 item 2's sequence -- a first grid of 48^2 or less,
    then the MT19937 grids at 256^2, 512^2 and 1024^2 -- through the host path and through
    device buffers of the caller's.

Parity is the project's (tests/test_gpu_solver.py): identical +inf mask and
|T - Tref| <= 1e-12 * max(1, Tref) against the oracle's FMM.
"""
import numpy as np
import pytest

from test_gpu_solver import assert_parity

pytestmark = pytest.mark.gpu

INF = np.inf
WRAP = 0xFFFFFFF0  # dom_begin's guard: a domain whose epochs could reach this restarts them

ENGINES = {
    "k3": dict(kernel=3),
    "k4": dict(kernel=4, prio_target=64),
    "k5": dict(kernel=5, prio_target=16),
    "k5det": dict(kernel=5, prio_target=16, deterministic=1),
}
# nx, ny, goal (off-centre; on tile edges of the 8- and the 16-cell tiles where marked)
GRIDS = {
    "40": (40, 40, (9, 31)),           # row 31: the last row of a tile (8 and 16)
    "64": (64, 64, (20, 44)),
    "96x80": (96, 80, (32, 17)),       # column 32: the first column of a tile (8 and 16)
    "104x88": (104, 88, (40, 23)),     # column 40: first of an 8-tile; row 23: last of one
    "200x136": (200, 136, (150, 40)),  # ragged last tile column and row; row 40: first of an 8-tile
    "256": (256, 256, (100, 175)),     # row 175: the last row of a tile (8 and 16)
}
SIDE = (120, 72, (77, 20))  # the grid of the extra steps of a history: another shape


@pytest.fixture(scope="module")
def maps(oracle):
    """Speeds (3-5 % obstacles) and their converged maps, computed once and read-only."""
    out = {}
    for k, (name, (nx, ny, goal)) in enumerate(list(GRIDS.items()) + [("side", SIDE)]):
        F = oracle.synth_speed(nx, ny, seed=31 + k, obst_frac=0.03 + 0.005 * (k % 5),
                               obst_seed=57 + k, goal=goal)
        Tref, _ = oracle.fmm(F, goal)
        F.setflags(write=False)
        Tref.setflags(write=False)
        out[name] = (F, Tref, goal)
    return out


class Buf:
    """A speed and a map of the caller's on the device (Engine.alloc), pitch nx."""

    def __init__(self, eng, F, rows=None):
        self.eng = eng
        self.ny, self.nx = F.shape
        n = 8 * self.nx * (rows or self.ny)
        self.dF, self.dT = eng.alloc(n), eng.alloc(n)
        eng.h2d(self.dF, F)

    def map(self, rows=None):
        T = np.empty((rows or self.ny, self.nx))
        self.eng.d2h(T, self.dT)
        return T

    def close(self):
        self.eng.free(self.dF)
        self.eng.free(self.dT)


def seed_tiles(variant, nx, ny, goal):
    """dom_begin's SeedTiles: the goal's tile and, for kernels 4 and 5, the tile across each
    tile edge the goal's cell lies on."""
    tw = 16 if variant == 5 else 8
    gi, gj = goal
    ntx = -(-nx // tw)
    gt = (gj // tw) * ntx + gi // tw
    t = [gt]
    if variant in (4, 5):
        if gi % tw == 0 and gi > 0:
            t.append(gt - 1)
        if gi % tw == tw - 1 and gi + 1 < nx:
            t.append(gt + 1)
        if gj % tw == 0 and gj > 0:
            t.append(gt - ntx)
        if gj % tw == tw - 1 and gj + 1 < ny:
            t.append(gt + ntx)
    return sorted(t)


def assert_stamps_clean(s, seeds):
    """Clause (a)'s tile_epoch condition: nothing above eb + 1, and eb + 1 on the seed's
    tiles only -- over the whole array, beyond the domain's tiles too."""
    ep = s["tile_epoch"].astype(np.int64)
    assert len(ep) == s["tiles_cap"] >= s["ntiles"]
    above = np.flatnonzero(ep > s["eb"] + 1)
    assert above.size == 0, (f"{above.size} stamps above eb + 1 = {s['eb'] + 1}: tiles "
                             f"{above[:8]} carry {ep[above[:8]]} (ntiles {s['ntiles']})")
    assert sorted(np.flatnonzero(ep == s["eb"] + 1)) == seeds


def assert_clean_start(eng, s, nx, ny, goal):
    """Everything clause (a) asks of the snapshot taken right after dom_begin."""
    v = s["variant"]
    tw = 16 if v == 5 else 8
    nt = (-(-nx // tw)) * (-(-ny // tw))
    assert (s["p"], s["ntiles"], s["nx"], s["ny"]) == (0, nt, nx, ny)
    seeds = seed_tiles(v, nx, ny, goal)
    assert_stamps_clean(s, seeds)
    assert sorted(s["list_tile"]) == seeds
    assert np.array_equal(s["list_raw"], s["list_tile"])  # the seed's entries carry no bin
    assert s["counts"][0].sum() == len(seeds) and not s["counts"][1:].any()
    T0 = np.empty((ny, s["ld"]))
    eng.d2h(T0, s["T"])
    T0 = T0[:, :nx]
    want = np.full((ny, nx), INF)
    want[goal[1], goal[0]] = 0.0
    assert np.array_equal(T0, want)
    if v == 3:
        assert s["keys"] is None and s["hist"] is None and s["ec"] is None
        return
    keys = np.full(nt, INF)
    keys[seeds] = 0.0
    assert np.array_equal(s["keys"][0], keys)
    assert np.all(s["keys"][1:] == INF)
    hist = np.zeros((3, 64), dtype=np.int64)
    hist[0, 0] = len(seeds)
    assert np.array_equal(s["hist"].sum(axis=1), hist)
    # k_prio_init then k_prio_seed: list 0's smallest key is the seed's 0, every origin 0
    assert np.array_equal(s["minkey"], [0.0, INF, INF])
    assert np.array_equal(s["base"], [0.0, 0.0, 0.0])
    assert 0.0 < s["delta"] < INF
    if v == 5:
        ec = np.full((nt, 2, 16), INF)
        ntx = -(-nx // 16)
        gt = (goal[1] // 16) * ntx + goal[0] // 16
        for side, col in ((0, 0), (1, 15)):
            i = (gt % ntx) * 16 + col
            for r in range(16):
                j = (gt // ntx) * 16 + r
                if i < nx and j < ny:
                    ec[gt, side, r] = T0[j, i]
        assert np.array_equal(s["ec"], ec)


def run_to_end(eng, batch=0, cap=20000):
    """The passes of a stepped domain, in batches of `batch` or, by default, in the batches
    converge() uses; the stats.  The passes launched, empty ones included, are the epochs
    the domain uses up."""
    k, done = batch or 16, 0
    while eng.dom_pending():
        assert done < cap
        eng.dom_run(k)
        done += k
        k = batch or min(2 * k, 64)
    return eng.dom_finish()


def solve_plain(eng, buf, goal):
    eng.solve_device(buf.dF, buf.dT, buf.nx, buf.ny, buf.nx, goal[0], goal[1])


def extras(dymu, eng, maps):
    """The other entries, on another shape: each stamps epochs and fills lists, keys and edge
    columns for a domain of its own.  Their results are other files' business."""
    F, Tref, g = maps["side"]
    ny, nx = F.shape
    P = dymu.batch_plane_rows(ny)
    b = Buf(eng, F, rows=3 * P)
    src = eng.alloc(F.nbytes)
    try:
        solve_plain(eng, b, g)
        F2 = F.copy()
        F2[30:38, 50:60] *= 0.5  # a windowed update, increases and decreases mixed
        F2[34, 52:56] = 7.0
        eng.h2d(b.dF, F2)
        eng.update_window_device(b.dF, b.dT, nx, ny, nx, g[0], g[1], 50, 30, 10, 8, False)
        eng.h2d(b.dF, F)
        eng.solve_seeds_device(b.dF, b.dT, nx, ny, nx, [(5, 5, 0.0), (100, 60, 1.5), (64, 15)])
        eng.clearance_device(b.dF, src, b.dT, nx, ny, nx, 0.25)
        tc, st = eng.solve_until_device(b.dF, b.dT, nx, ny, nx, g[0], g[1], g[0] + 4, g[1] + 3)
        assert np.isfinite(tc)
        # it stopped early: the front was abandoned with reachable cells not yet converged
        fin = np.isfinite(Tref)
        assert np.any(b.map()[fin] > Tref[fin] * (1 + 1e-9))
        eng.h2d(src, F)
        eng.stack_speed(src, nx, 0, nx, ny, 3, b.dF, nx)
        eng.solve_batch_device(b.dF, b.dT, nx, ny, 3, nx, [(0, 5, 5), (1, 100, 60), (2, *g)])
    finally:
        eng.free(src)
        b.close()


# name -> (the grids solved before, the grid G whose start is examined)
HISTORIES = {
    "fresh": ((), "96x80"),
    "larger_smaller": (("256",), "96x80"),            # a stale region beyond ntiles, no growth
    "smaller_larger": (("40",), "200x136"),           # every workspace grows
    "larger_smaller_larger": (("256", "96x80"), "256"),
}


def check_history(dymu, eng, maps, before, G, with_extras):
    bufs = {}
    try:
        for name in set(before) | {G}:
            bufs[name] = Buf(eng, maps[name][0])
        eng.set_stepping(False)
        for name in before:
            solve_plain(eng, bufs[name], maps[name][2])
        if with_extras:
            extras(dymu, eng, maps)
        F, Tref, goal = maps[G]
        ny, nx = F.shape
        eng.set_stepping(True)
        solve_plain(eng, bufs[G], goal)  # returns after dom_begin, the domain live
        s = eng.dom_snapshot()
        assert (s["F"], s["T"]) == (bufs[G].dF, bufs[G].dT)
        assert_clean_start(eng, s, nx, ny, goal)
        st = run_to_end(eng)
        assert st["kernel"] == s["variant"]
        assert_parity(bufs[G].map(), Tref)
        return s
    finally:
        eng.set_stepping(False)
        for b in bufs.values():
            b.close()


@pytest.mark.parametrize("with_extras", [False, True], ids=["plain", "extras"])
@pytest.mark.parametrize("history", sorted(HISTORIES))
@pytest.mark.parametrize("engine", sorted(ENGINES))
def test_domain_starts_clean(dymu, maps, engine, history, with_extras):
    before, G = HISTORIES[history]
    with dymu.Engine(**ENGINES[engine]) as eng:
        s = check_history(dymu, eng, maps, before, G, with_extras)
        assert s["variant"] == ENGINES[engine]["kernel"]


@pytest.mark.parametrize("with_extras", [False, True], ids=["plain", "extras"])
@pytest.mark.parametrize("order", ["v3_then_v5", "v5_then_v3"])
def test_domain_starts_clean_after_tile_size_switch(dymu, maps, monkeypatch, order, with_extras):
    """kernel = 0 picks the kernel per domain: below DYMU_PRIO_MIN_TILES 8x8 tiles the plain
    FIM on 8x8 tiles (variant 3), from there on kernel 5 on 16x16 tiles.  One engine, one
    tile-epoch array, two tilings: the second grid's tiles, and those of the extra steps
    (at most 135 on 8x8 tiles, 120 for the stack on 16x16), fit the first grid's capacity,
    so the array the first tiling stamped is the one the second reads.
    v3 then v5: 104x88 (143 8x8 tiles), then 200x136 (425 8x8 tiles -> kernel 5, 117 tiles).
    v5 then v3: 256^2 (1,024 -> kernel 5, 256 tiles), then 96x80 (120 8x8 tiles)."""
    monkeypatch.setenv("DYMU_PRIO_MIN_TILES", "200")
    before, G, v, cap = {"v3_then_v5": (("104x88",), "200x136", 5, 143),
                         "v5_then_v3": (("256",), "96x80", 3, 256)}[order]
    with dymu.Engine(kernel=0) as eng:
        s = check_history(dymu, eng, maps, before, G, with_extras)
        assert s["variant"] == v
        assert s["tiles_cap"] == cap  # never regrown


@pytest.mark.parametrize("grid", ["96x80", "200x136"])
@pytest.mark.parametrize("engine", ["k4", "k5"])
def test_invariants_between_passes(dymu, maps, engine, grid):
    F, Tref, goal = maps[grid]
    ny, nx = F.shape
    with dymu.Engine(**ENGINES[engine]) as eng:
        b = Buf(eng, F)
        try:
            eng.set_stepping(True)
            solve_plain(eng, b, goal)
            p, looked = 0, 0
            while True:
                pending = eng.dom_pending()
                if p < 12 or p % 8 == 0 or pending == 0:
                    s = eng.dom_snapshot()
                    looked += 1
                    assert s["p"] == p
                    tiles = s["list_tile"]
                    assert np.all(tiles < s["ntiles"])
                    assert len(np.unique(tiles)) == len(tiles)
                    assert s["counts"][p % 3].sum() == pending == len(tiles)
                    ep = s["tile_epoch"].astype(np.int64)
                    assert ep.max() <= s["eb"] + p + 1
                    assert np.all(ep[tiles] == s["eb"] + p + 1)
                if pending == 0:
                    break
                assert p < 20000
                eng.dom_run(1)
                p += 1
            assert looked > 12
            eng.dom_finish()
            assert_parity(b.map(), Tref)
        finally:
            eng.set_stepping(False)
            b.close()


@pytest.mark.parametrize("engine", ["k3", "k4", "k5"])
def test_epoch_wrap(dymu, maps, engine):
    """The base is raised to 3,000 below the guard's limit, 256^2 solved, the base raised to
    1,000 below it, 64^2 solved -- there the guard fires, for 4 * ntiles + 1,024 + 136 > 1,000
    -- and 256^2 solved again without growth: its tiles beyond the 64^2 domain's must not have
    kept the stamps of the first 256^2 solve, which lie above every epoch after the restart.

    Kernel 5 has 256 tiles at 256^2 (4 * 256 + 1,160 = 2,184 <= 3,000: the first solve stamps
    up there, as intended).  Kernels 3 and 4 have 1,024 (5,256 > 3,000), so for them the guard
    already fires in the first solve; the stamps that solve leaves are then small, but still
    above the epochs the third solve starts from after the second restart, so the sequence
    tests the same defect.  Which solves restart is asserted from that arithmetic."""
    F256, T256, g256 = maps["256"]
    F64, T64, g64 = maps["64"]
    tw = 8 if engine in ("k3", "k4") else 16

    def fires(base, n):  # dom_begin's test, default pass cap 4 * ntiles + 1024
        return base + 4 * (n // tw) ** 2 + 1024 + 128 + 8 >= WRAP

    with dymu.Engine(**ENGINES[engine]) as eng:
        big, small = Buf(eng, F256), Buf(eng, F64)
        try:
            eng.set_stepping(True)

            def solve(b, goal, Tref):
                solve_plain(eng, b, goal)
                s = eng.dom_snapshot()
                # two passes at a time: the 64^2 solve then uses up fewer epochs than the
                # first 256^2 solve stamped, for every kernel (asserted below)
                done = 0
                while eng.dom_pending():
                    assert done < 20000
                    eng.dom_run(2)
                    done += 2
                s["stamps_left"] = eng.dom_snapshot()["tile_epoch"].astype(np.int64)
                eng.dom_finish()
                assert_parity(b.map(), Tref)
                return s

            eng.raise_epoch_base(WRAP - 3000)
            s1 = solve(big, g256, T256)
            assert s1["eb"] == (0 if fires(WRAP - 3000, 256) else WRAP - 3000)
            assert fires(WRAP - 3000, 256) == (engine != "k5")
            eng.raise_epoch_base(WRAP - 1000)
            s2 = solve(small, g64, T64)
            assert fires(WRAP - 1000, 64) and s2["eb"] == 0  # the guard did fire
            s3 = solve(big, g256, T256)
            assert s3["tiles_cap"] == s1["tiles_cap"] == s3["ntiles"]  # no growth
            assert 0 < s3["eb"] < 4096
            # the test has teeth: beyond the 64^2 domain's tiles the first solve left stamps
            # above the epoch the third one seeds with, which only the guard can have cleared
            assert s1["stamps_left"][s2["ntiles"]:].max() > s3["eb"] + 1
            assert_stamps_clean(s3, seed_tiles(s3["variant"], 256, 256, g256))
        finally:
            eng.set_stepping(False)
            big.close()
            small.close()


# ---- (d) DESIGN.md s8 item 2 ----
KAT = {256: ("1.7066083890e+07", "479.2433625750"),  # tests/test_gpu_solver.py's strings
       512: ("1.3467278246e+08", "972.7322452271"),
       1024: ("1.0666255888e+09", "1913.6136177798")}
S82 = dict(kernel=5, prio_target=16)


@pytest.fixture(scope="module")
def mt(oracle):
    out = {}
    for N in KAT:
        F = oracle.mt_uniform(N * N).reshape(N, N)
        F.setflags(write=False)
        out[N] = F
    Tref, _ = oracle.fmm(out[256], (128, 128))
    Tref.setflags(write=False)
    out["Tref256"] = Tref
    return out


def assert_kat(T, N):
    M = np.where(np.isinf(T), -1.0, T)
    assert (f"{M.sum():.10e}", f"{T[1, 1]:.10f}") == KAT[N], f"N = {N}"


def host_solver(eng):
    def solve(F):
        N = F.shape[0]
        r = eng.solve(F, N // 2, N // 2)
        return r.T, r.stats
    return solve, lambda: None


def device_solver(eng):
    """The same solves on two buffers of the caller's, sized once for 1024^2: no staging."""
    n = 8 * 1024 * 1024
    dF, dT = eng.alloc(n), eng.alloc(n)

    def solve(F):
        N = F.shape[0]
        eng.h2d(dF, F)
        st = eng.solve_device(dF, dT, N, N, N, N // 2, N // 2)
        T = np.empty((N, N))
        eng.d2h(T, dT)
        return T, st

    def close():
        eng.free(dF)
        eng.free(dT)
    return solve, close


def tiny_first_sequence(dymu, mt, first, solver):
    """Three engines one after the other (the recorded rate was 6 of 7 sequences wrong), then
    a fresh engine's 1024^2 solve for the pass count -- after them, so that no engine has
    held and released buffers of the final size before the sequences run.

    DESIGN.md s8 item 2: the wrong maps follow the release of map memory that is then
    allocated again larger, and whether this sequence shows them varies from build to build
    and with what the process did before; tools/history_probe.py shows them more often."""
    passes = []
    for attempt in range(3):
        with dymu.Engine(**S82) as eng:
            solve, close = solver(eng)
            try:
                T, _ = solve(np.ones((first, first)))
                assert np.all(np.isfinite(T)) and T[first // 2, first // 2] == 0.0
                for N in (256, 512, 1024):
                    T, st = solve(mt[N])
                    print(f"first {first} attempt {attempt} N {N}: {st['passes']} passes")
                    assert_kat(T, N)
                    if N == 256:
                        assert_parity(T, mt["Tref256"])
                passes.append(st["passes"])
            finally:
                close()
    with dymu.Engine(**S82) as fresh:
        solve, close = solver(fresh)
        try:
            T, st = solve(mt[1024])
        finally:
            close()
        assert_kat(T, 1024)
        want = st["passes"]
    print(f"a fresh engine's 1024^2: {want} passes")
    assert all(abs(p - want) <= 0.02 * want for p in passes), (passes, want)


S82_OPEN = pytest.mark.xfail(strict=False, reason=(
    "DESIGN.md s8 item 2: an intermittent wrong 1024^2 map after the engine's buffers have "
    "grown; the cause is not found"))


@pytest.mark.parametrize("first", [pytest.param(16, marks=S82_OPEN),
                                   pytest.param(48, marks=S82_OPEN), 64])
def test_tiny_first_grid_host_path(dymu, mt, first):
    """Engine.solve on host arrays: the staged d_F / d_T grow with every grid (ensure_cells)
    and every upload is a pageable copy into uncached memory.  64^2 is the control."""
    tiny_first_sequence(dymu, mt, first, host_solver)


@pytest.mark.parametrize("first", [16, 48, 64])
def test_tiny_first_grid_device_path(dymu, mt, first):
    """The twin on buffers of the caller's, allocated once: only the tile workspace, the
    keys and the edge columns are freed and regrown on the way up."""
    tiny_first_sequence(dymu, mt, first, device_solver)
