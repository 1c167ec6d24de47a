"""The preparation stage of the windowed updates and the early exit's key bound, seen
between the passes (dymu_set_stepping, dymu_dom_min_key; include/dymu_fim.h).

Stage tests: with stepping on, a device-resident update returns after its preparation --
k_window_min / k_windows_min, k_reset_seed / k_reset_planes with the seeds written back,
k_seed_window / k_seed_windows, k_raise and k_cone_seed, k_theta_state /
k_theta_min_state -- and the map, the number of queued tiles and the smallest key are
compared exactly (bit patterns and integers) with tests/update_ref.py, whose references
tests/test_update_ref.py pins on the CPU.  Every case runs at ld = nx and at ld = nx + 7
with poisoned padding (T: 0.0, below every theta; F: a finite speed no cell holds) that
must come back bitwise, then runs on to dymu_dom_finish and meets the oracle's map.

Key-bound test: a solve or an update stepped one pass at a time.  Before every pass the
smallest key k_p of the list the pass reads bounds, from below, the final value of every
cell that still changes -- the rule the *_until_* entries stop by -- whatever queued the
tiles: edge keys, key- and colour-deferred entries, capped visits, seeds, theta.
"""
import ctypes
import os

import numpy as np
import pytest

import goalset_ref
import update_ref as ref
from test_gpu_solver import assert_parity
from update_ref import INF, PAD, PAD_F, PAD_T, bits

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -7
NX, NY, GOAL = ref.SHAPES[0]
P = ref.plane_rows(NY)
ROWS_MAX = 3 * P
STEP_CAP = 3000  # passes a stepped solve may take before the test fails
LIVE = 3         # engines of this file open at a time


# ---------------------------------------------------------------------------
# fixtures: engines with stepping on (a few open at a time); two device buffers
# ---------------------------------------------------------------------------
@pytest.fixture(scope="session")
def pool(dymu, ptrs):
    """get(kernel, raise_front=False, **opts): an engine with stepping on.  DYMU_RAISE is
    read when a context is created, the other knobs when a domain begins.

    A new engine first begins (and ends, without a pass) the largest domain of this file,
    the three-plane stack, so that its tile workspace, keys, edge columns and theta slots
    are allocated once at their final size: no engine frees and reallocates device memory
    between the tests (see the note on frees at tests/test_gpu_postproc.py's arena).  That
    begin overwrites the two device buffers: ask for the engines first, upload afterwards.
    At most LIVE engines are kept, the least recently used one is closed: this file asks
    for fifteen different ones, and the suite has its own contexts open besides."""
    made = {}
    wins = [(b, 0, 0, 1, 1) for b in range(3)]
    seeds = [(b, 0, 0, 0.0) for b in range(3)]

    def get(kernel, raise_front=False, **opts):
        key = (kernel, raise_front, tuple(sorted(opts.items())))
        if key in made:
            made[key] = made.pop(key)  # most recently used last
        else:
            while len(made) >= LIVE:
                made.pop(next(iter(made))).close()
            old = os.environ.get("DYMU_RAISE")
            os.environ["DYMU_RAISE"] = "1" if raise_front else "0"
            try:
                eng = dymu.Engine(kernel=kernel, **opts)
            finally:
                if old is None:
                    del os.environ["DYMU_RAISE"]
                else:
                    os.environ["DYMU_RAISE"] = old
            eng.set_stepping(True)
            flat = np.ones((ROWS_MAX, NX + PAD))
            eng.h2d(ptrs[0], flat)
            eng.h2d(ptrs[1], flat)
            eng.update_batch_window_device(ptrs[0], ptrs[1], NX, NY, 3, NX + PAD, seeds, wins,
                                           decrease_only=True)
            eng.dom_finish()
            made[key] = eng
        return made[key]

    yield get
    for eng in made.values():
        eng.close()


class Dev:
    """The speed and the map of a case on the device at pitch ld, padding poisoned."""

    def __init__(self, eng, ptrs, F, T, pad):
        self.eng = eng
        self.rows, self.nx = T.shape
        self.ld = self.nx + pad
        self.dF, self.dT = ptrs
        self.F = ref.pitched(F, self.ld, PAD_F)
        self.T = ref.pitched(T, self.ld, PAD_T)
        eng.h2d(self.dF, self.F)
        eng.h2d(self.dT, self.T)

    def map(self):
        """The map's cells; the padding of both buffers and the whole speed must be bitwise
        what was uploaded."""
        got = np.empty_like(self.T)
        self.eng.d2h(got, self.dT)
        assert np.array_equal(bits(got[:, self.nx:]), bits(self.T[:, self.nx:]))
        f = np.empty_like(self.F)
        self.eng.d2h(f, self.dF)
        assert np.array_equal(bits(f), bits(self.F))
        return got[:, :self.nx].copy()


@pytest.fixture(scope="session")
def ptrs(engine):
    n = 8 * ROWS_MAX * (NX + PAD)
    p = (engine.alloc(n), engine.alloc(n))
    yield p
    for q in p:
        engine.free(q)


@pytest.fixture(scope="session")
def world(oracle):
    """The old speeds and their converged maps, computed once: the oracle's FMM for a goal,
    goalset_ref.fmm_seeds for seeds; fin(key, fn) caches a final map by name."""
    w = {"maps": {}, "final": {}}
    for nx, ny, goal in ref.ALL_SHAPES:
        F0 = ref.base_speed(oracle, nx, ny, goal)
        w["maps"][(nx, ny, goal)] = (F0, oracle.fmm(F0, goal)[0])
    F0 = w["maps"][ref.SHAPES[0]][0]
    w["seeded"] = goalset_ref.fmm_seeds(oracle, F0, ref.SEEDS_97)

    def plane_maps(Fs):
        return ref.stacked([goalset_ref.fmm_seeds(oracle, Fs[b * P:b * P + NY],
                                                  [s[1:] for s in ref.STACK_SEEDS if s[0] == b])
                            for b in range(3)], NY, P, INF)

    def fin(key, fn):
        if key not in w["final"]:
            w["final"][key] = fn()
        return w["final"][key]

    w["plane_maps"] = plane_maps
    w["fin"] = fin
    w["stack_F0"] = ref.stack_speeds(F0)[0]
    w["stack_T0"] = plane_maps(w["stack_F0"])
    return w


def tiles_of(eng_kernel):
    return ref.tile_size(eng_kernel)


def drive(eng, batch=4):
    """The passes of a live domain to convergence, then dom_finish's statistics."""
    for _ in range(STEP_CAP):
        if eng.dom_pending() == 0:
            return eng.dom_finish()
        eng.dom_run(batch)
    pytest.fail("step cap reached")


def check_stage(eng, kernel, dev, want_T, want_tiles, want_key, tag):
    """After the begin: the map bit for bit, the queued tiles, the smallest key."""
    got = dev.map()
    diff = bits(got) != bits(want_T)
    assert not diff.any(), f"{tag}: {int(diff.sum())} cells differ, first {np.argwhere(diff)[:4]}"
    assert eng.dom_pending() == len(want_tiles), tag
    if kernel == 3:
        with pytest.raises(Exception) as e:
            eng.dom_min_key()
        assert e.value.status == ERR_STATE
    else:
        key = eng.dom_min_key()
        assert key == want_key, f"{tag}: min key {key!r}, want {want_key!r}"


STAGE_CASES = [(s, name) for s in ref.ALL_SHAPES for name in ref.cases_for(s[0], s[1])]
STAGE_IDS = [f"{s[0]}x{s[1]}g{s[2][0]}-{name}" for s, name in STAGE_CASES]


# ---------------------------------------------------------------------------
# stage tests
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pad", (0, PAD))
@pytest.mark.parametrize("kernel", (3, 4, 5))
@pytest.mark.parametrize("shape,name", STAGE_CASES, ids=STAGE_IDS)
def test_theta_reset_stage(pool, ptrs, world, oracle, shape, name, kernel, pad):
    nx, ny, goal = shape
    F0, T0 = world["maps"][shape]
    F1, win = ref.case(name, F0, goal)
    tile = tiles_of(kernel)
    want_T, tiles, theta, n_reset = ref.reset_ref(T0, F1, [win], tile, goal=goal)
    eng = pool(kernel, prio_target=16 if kernel == 5 else 64)
    dev = Dev(eng, ptrs, F1, T0, pad)
    eng.resolve_window_device(dev.dF, dev.dT, nx, ny, dev.ld, goal[0], goal[1], *win)
    check_stage(eng, kernel, dev, want_T, tiles, theta, name)
    if name == "unreached":
        assert theta == INF and not tiles
    # the single-goal theta reset does not count its cells (dymu_last_update_stats)
    assert eng.last_update_stats() == {"raise_passes": 0, "raise_visits": 0, "cells_invalidated": 0}
    drive(eng)
    Tref = world["fin"](("reset", shape, name), lambda: oracle.fmm(ref.no_nan(F1), goal)[0])
    assert_parity(dev.map(), Tref)


@pytest.mark.parametrize("pad", (0, PAD))
@pytest.mark.parametrize("kernel", (3, 4, 5))
@pytest.mark.parametrize("shape,name", STAGE_CASES, ids=STAGE_IDS)
def test_decrease_only_stage(pool, ptrs, world, oracle, shape, name, kernel, pad):
    nx, ny, goal = shape
    F0, T0 = world["maps"][shape]
    F1, win = ref.decrease_case(name, F0, goal)
    tile = tiles_of(kernel)
    eng = pool(kernel, prio_target=16 if kernel == 5 else 64)
    dev = Dev(eng, ptrs, F1, T0, pad)
    eng.update_window_device(dev.dF, dev.dT, nx, ny, dev.ld, goal[0], goal[1], *win, True)
    # nothing is written; the tiles that meet the clipped window are queued, keyed theta
    check_stage(eng, kernel, dev, T0, ref.seed_window_ref([win], nx, ny, tile),
                ref.theta_ref(T0, [win]), name)
    assert eng.last_update_stats()["cells_invalidated"] == 0
    drive(eng)
    Tref = world["fin"](("dec", shape, name), lambda: oracle.fmm(F1, goal)[0])
    assert_parity(dev.map(), Tref)


@pytest.mark.parametrize("pad", (0, PAD))
@pytest.mark.parametrize("kernel", (3, 4, 5))
@pytest.mark.parametrize("name", ref.SEEDED_CASES + ("decrease",))
def test_seeded_stage(pool, ptrs, world, oracle, name, kernel, pad):
    F0 = world["maps"][ref.SHAPES[0]][0]
    T0 = world["seeded"]
    dec = name == "decrease"
    F1, win = ref.decrease_case("interior", F0, GOAL) if dec else ref.case(name, F0, GOAL)
    tile = tiles_of(kernel)
    seeds = [(0,) + s for s in ref.SEEDS_97]
    want_T, tiles, thetas, n_reset = ref.stack_ref(T0, F1, NY, NY, [(0,) + win], seeds, tile,
                                                   decrease_only=dec, across=kernel != 3)
    eng = pool(kernel, prio_target=16 if kernel == 5 else 64)
    dev = Dev(eng, ptrs, F1, T0, pad)
    eng.update_seeds_window_device(dev.dF, dev.dT, NX, NY, dev.ld, ref.SEEDS_97, *win,
                                   decrease_only=dec)
    check_stage(eng, kernel, dev, want_T, tiles, thetas[0], name)
    assert eng.last_update_stats()["cells_invalidated"] == n_reset  # readable after the begin
    i, j, t0 = ref.SEEDS_97[1]  # the dominated seed, back at its t0 where the reset covers it
    if not dec and T0[j, i] >= thetas[0]:
        assert T0[j, i] < t0 and want_T[j, i] == t0
    if name == "unreached":
        assert thetas[0] == INF and n_reset == 0
    drive(eng)
    Tref = world["fin"](("seeded", name), lambda: goalset_ref.fmm_seeds(oracle, F1, ref.SEEDS_97))
    assert_parity(dev.map(), Tref)


@pytest.mark.parametrize("pad", (0, PAD))
@pytest.mark.parametrize("kernel", (3, 4, 5))
@pytest.mark.parametrize("dec", (False, True), ids=("reset", "decrease"))
def test_stack_stage(pool, ptrs, world, dec, kernel, pad):
    """Three planes: two windows in plane 0, none in plane 1 (bitwise untouched, theta =
    +inf), a clipped one in plane 2."""
    F0 = world["maps"][ref.SHAPES[0]][0]
    _, F1, _ = ref.stack_speeds(F0, 0.5 if dec else 1.5)
    T0 = world["stack_T0"]
    tile = tiles_of(kernel)
    want_T, tiles, thetas, n_reset = ref.stack_ref(T0, F1, NY, P, ref.STACK_WINS,
                                                   ref.STACK_SEEDS, tile, decrease_only=dec,
                                                   across=kernel != 3)
    assert thetas[1] == INF and np.array_equal(bits(want_T[P:2 * P]), bits(T0[P:2 * P]))
    eng = pool(kernel, prio_target=16 if kernel == 5 else 64)
    dev = Dev(eng, ptrs, F1, T0, pad)
    eng.update_batch_window_device(dev.dF, dev.dT, NX, NY, 3, dev.ld, ref.STACK_SEEDS,
                                   ref.STACK_WINS, decrease_only=dec)
    check_stage(eng, kernel, dev, want_T, tiles, min(thetas), "stack")
    assert eng.last_update_stats()["cells_invalidated"] == n_reset
    drive(eng)
    Tref = world["fin"](("stack", dec), lambda: world["plane_maps"](F1))
    assert_parity(dev.map(), Tref)


@pytest.mark.parametrize("pad", (0, PAD))
@pytest.mark.parametrize("kernel", (3, 4, 5))
@pytest.mark.parametrize("shape,name", STAGE_CASES, ids=STAGE_IDS)
def test_raise_stage(pool, ptrs, world, oracle, shape, name, kernel, pad):
    """DYMU_RAISE=1: the invalidated set is exactly the cells no longer supported, on the
    engine's own converged map of the old speed."""
    nx, ny, goal = shape
    F0, _ = world["maps"][shape]
    F1, win = ref.case(name, F0, goal)
    tile = tiles_of(kernel)
    eng = pool(kernel, raise_front=True, prio_target=16 if kernel == 5 else 64)
    dev = Dev(eng, ptrs, F0, np.full_like(F0, 123.0), pad)
    eng.solve_device(dev.dF, dev.dT, nx, ny, dev.ld, *goal)  # stepping: the cold begin only
    drive(eng)
    T0 = dev.map()
    # the two conditions the exact comparison rests on, asserted and not tolerated: the
    # engine's map is a fixed point of the reference update within the raise tolerance (it
    # covers the sweep sqrt), and no cell sits in the margin around the threshold
    _, S_old, m_old = ref.raise_ref(T0, F0, goal)
    assert not S_old.any() and not m_old.any(), name
    want_T, S, margin = ref.raise_ref(T0, F1, goal)
    assert not margin.any(), name
    cone_tiles, m = ref.cone_seed_ref(want_T, F1, goal, tile)
    tiles = cone_tiles | ref.seed_window_ref([win], nx, ny, tile)
    dev.F = ref.pitched(F1, dev.ld, PAD_F)
    eng.h2d(dev.dF, dev.F)
    eng.resolve_window_device(dev.dF, dev.dT, nx, ny, dev.ld, goal[0], goal[1], *win)
    check_stage(eng, kernel, dev, want_T, tiles, min(ref.theta_ref(T0, [win]), m), name)
    us = eng.last_update_stats()
    assert us["cells_invalidated"] == int(S.sum()), name
    assert us["raise_passes"] > 0
    if name not in ("unreached", "cleared"):
        assert 0 < S.sum() < np.isfinite(T0).sum()
    drive(eng)
    Tref = world["fin"](("reset", shape, name), lambda: oracle.fmm(ref.no_nan(F1), goal)[0])
    assert_parity(dev.map(), Tref)


def test_stepped_solve_is_the_default_solve(dymu, pool, ptrs, world):
    """Deterministic mode: the stepped cold solve and update end bit for bit where the
    entries themselves do."""
    F0, T0 = world["maps"][ref.SHAPES[0]]
    F1, win = ref.case("interior", F0, GOAL)
    got = []
    for stepping in (False, True):
        eng = pool(5, deterministic=1, prio_target=4)
        eng.set_stepping(stepping)
        try:
            dev = Dev(eng, ptrs, F0, np.zeros_like(F0), PAD)
            st = eng.solve_device(dev.dF, dev.dT, NX, NY, dev.ld, *GOAL)
            if stepping:
                assert st["passes"] == 0  # statistics come from dom_finish
                st = drive(eng, batch=1)
            a = dev.map()
            dev.F = ref.pitched(F1, dev.ld, PAD_F)
            eng.h2d(dev.dF, dev.F)
            eng.resolve_window_device(dev.dF, dev.dT, NX, NY, dev.ld, GOAL[0], GOAL[1], *win)
            if stepping:
                drive(eng, batch=1)
            got.append((a, dev.map(), st["passes"]))
        finally:
            eng.set_stepping(True)
    assert np.array_equal(bits(got[0][0]), bits(got[1][0]))
    assert np.array_equal(bits(got[0][1]), bits(got[1][1]))
    assert got[0][2] == got[1][2] > 0
    assert_parity(got[1][0], T0)


@pytest.mark.parametrize("kernel", (4, 5))
@pytest.mark.parametrize("shape", ref.GOAL_SHAPES, ids=("g16", "g15"))
@pytest.mark.parametrize("seeded", (False, True), ids=("goal", "seed"))
def test_goal_in_a_tile_corner_reaches_across(pool, ptrs, world, oracle, shape, kernel, seeded):
    """The goal in the corner of a tile with its two in-tile neighbours blocked: the only
    way out leads across the tile edges, through cells that are updated from the goal's
    own value, which no visit changes.  The tiles across are queued by the seed (kernels 4
    and 5; the plain FIM, kernel 3, still queues the goal's tile only and does not get out
    of such a pocket)."""
    nx, ny, goal = shape
    F = world["maps"][shape][0].copy()
    d = 1 if goal[0] % 8 == 0 else -1  # the in-tile side
    F[goal[1], goal[0] + d] = INF
    F[goal[1] + d, goal[0]] = INF
    eng = pool(kernel, prio_target=16 if kernel == 5 else 64)
    dev = Dev(eng, ptrs, F, np.full_like(F, 9.0), PAD)
    if seeded:
        eng.solve_seeds_device(dev.dF, dev.dT, nx, ny, dev.ld, [goal + (0.0,)])
    else:
        eng.solve_device(dev.dF, dev.dT, nx, ny, dev.ld, *goal)
    assert eng.dom_pending() == 3  # the goal's tile and the two across
    drive(eng)
    Tref = oracle.fmm(F, goal)[0]
    assert np.isfinite(Tref).sum() > 1000
    assert_parity(dev.map(), Tref)


# ---------------------------------------------------------------------------
# the key bound, pass by pass
# ---------------------------------------------------------------------------
# name -> (engine options, environment at the begin, kernels)
CONFIGS = {
    "defer": ({}, {}, (4, 5)),
    "deterministic": ({"deterministic": 1}, {}, (5,)),
    "no-checker": ({}, {"DYMU_CHECKER": "0"}, (5,)),
    "no-pack-bins": ({}, {"DYMU_PACK_BINS": "0"}, (5,)),
    "no-capfrac": ({}, {"DYMU_PRIO_CAPFRAC": "0"}, (5,)),
    "max-inner-1": ({"max_inner": 1}, {}, (4, 5)),
    "grid-blocks-1": ({"grid_blocks": 1}, {}, (4, 5)),
    "grid-blocks-3": ({"grid_blocks": 3}, {}, (4, 5)),
}
# targets small enough that keys defer tiles on the 28 16 x 16 tiles of the 97 x 61 map, and
# on the handful of 8 x 8 tiles a decrease in a 1 x 1 window queues
PRIO_TARGET = {4: 2, 5: 4}
DOMAINS = ("cold", "cold-maze", "cold-const", "cold-corner-16", "cold-corner-15", "seeds",
           "stack", "reset", "decrease", "stack-reset", "stack-decrease")
KEY_CASES = [(d, c, k) for c, (_, _, ks) in CONFIGS.items() for k in ks for d in DOMAINS]


def begin_domain(domain, eng, ptrs, world, oracle):
    """Upload and begin a domain; returns (dev, reference of the final map)."""
    F0, T0 = world["maps"][ref.SHAPES[0]]
    fin = world["fin"]
    if domain.startswith("cold-corner"):  # the goal in the corner of a tile of either size
        shape = ref.GOAL_SHAPES[domain.endswith("15")]
        F, Tc = world["maps"][shape]
        dev = Dev(eng, ptrs, F, np.full_like(F, 5.0), PAD)
        eng.solve_device(dev.dF, dev.dT, shape[0], shape[1], dev.ld, *shape[2])
        return dev, Tc
    if domain.startswith("cold"):
        F = {"cold": F0, "cold-maze": ref.serpentine(F0), "cold-const": np.ones_like(F0)}[domain]
        dev = Dev(eng, ptrs, F, np.full_like(F, 5.0), PAD)
        eng.solve_device(dev.dF, dev.dT, NX, NY, dev.ld, *GOAL)
        return dev, fin(("key", domain), lambda: oracle.fmm(F, GOAL)[0])
    if domain == "seeds":
        dev = Dev(eng, ptrs, F0, np.full_like(F0, 5.0), PAD)
        eng.solve_seeds_device(dev.dF, dev.dT, NX, NY, dev.ld, ref.SEEDS_97)
        return dev, world["seeded"]
    if domain == "stack":
        dev = Dev(eng, ptrs, world["stack_F0"], np.full_like(world["stack_T0"], 5.0), PAD)
        eng.solve_batch_device(dev.dF, dev.dT, NX, NY, 3, dev.ld, ref.STACK_SEEDS)
        return dev, world["stack_T0"]
    # The updates start, as a caller's do, from the map this engine itself converged to under
    # the old speed: a fixed point of the engine's own arithmetic.  (On the oracle's map --
    # equal within the parity bound, but no fixed point of kernel 5's sweep sqrt -- a visit
    # moves kept cells below theta by an ulp, which is a change below every key.)
    dec = domain.endswith("decrease")
    if domain.startswith("stack"):
        _, F1, _ = ref.stack_speeds(F0, 0.5 if dec else 1.5)
        dev, _ = begin_domain("stack", eng, ptrs, world, oracle)
        drive(eng)
        dev.F = ref.pitched(F1, dev.ld, PAD_F)
        eng.h2d(dev.dF, dev.F)
        eng.update_batch_window_device(dev.dF, dev.dT, NX, NY, 3, dev.ld, ref.STACK_SEEDS,
                                       ref.STACK_WINS, decrease_only=dec)
        return dev, fin(("stack", dec), lambda: world["plane_maps"](F1))
    F1, win = (ref.decrease_case if dec else ref.case)("one", F0, GOAL)
    dev, _ = begin_domain("cold", eng, ptrs, world, oracle)
    drive(eng)
    dev.F = ref.pitched(F1, dev.ld, PAD_F)
    eng.h2d(dev.dF, dev.F)
    eng.update_window_device(dev.dF, dev.dT, NX, NY, dev.ld, GOAL[0], GOAL[1], *win, dec)
    return dev, fin((("dec" if dec else "reset"), ref.SHAPES[0], "one"),
                    lambda: oracle.fmm(F1, GOAL)[0])


@pytest.mark.parametrize("domain,config,kernel", KEY_CASES,
                         ids=[f"{d}-{c}-k{k}" for d, c, k in KEY_CASES])
def test_key_bound_pass_by_pass(pool, ptrs, world, oracle, monkeypatch, domain, config, kernel):
    """Before every pass p, with k_p the smallest key, n_p the queued tiles and T_p the map:
    (i) every cell with T_p != T_fin (bitwise) has T_fin >= k_p - 1e-12 max(1, k_p), the
    project's parity bound and the only slack; (ii) n_p = 0 exactly when k_p = +inf, and
    then nothing differs; (iii) T_{p+1} <= T_p everywhere; (iv) the final map meets the
    oracle's."""
    opts, env, _ = CONFIGS[config]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = pool(kernel, prio_target=PRIO_TARGET[kernel], **opts)
    dev, Tref = begin_domain(domain, eng, ptrs, world, oracle)
    keys, pend, maps = [], [], []
    for _ in range(STEP_CAP):
        keys.append(eng.dom_min_key())
        pend.append(eng.dom_pending())
        maps.append(dev.map())
        if pend[-1] == 0:
            break
        eng.dom_run(1)
    else:
        pytest.fail("step cap reached")
    stats = eng.dom_finish()
    T_fin = maps[-1]
    worst_ulps, live_passes = 0.0, 0
    for p, (k, n, T) in enumerate(zip(keys, pend, maps)):
        diff = bits(T) != bits(T_fin)
        assert (n == 0) == (k == INF), f"pass {p}: {n} tiles queued, min key {k}"      # (ii)
        if n == 0:
            assert not diff.any()
        if diff.any():
            low = float(T_fin[diff].min())
            if low < k:
                worst_ulps = max(worst_ulps, (k - low) / np.spacing(k))
            assert low >= k - 1e-12 * max(1.0, k), \
                f"pass {p}: a cell ends at {low!r} below the min key {k!r}"            # (i)
            live_passes += 0.0 < k < INF
        if p:
            assert (T <= maps[p - 1]).all(), f"pass {p}: a value went up"               # (iii)
    print(f"{domain}/{config}/k{kernel}: {len(keys) - 1} passes, {live_passes} with a finite "
          f"key > 0 and cells to change, deferred {sum(pend) - stats['tile_visits']}, "
          f"worst key shortfall {worst_ulps:.1f} ulps")
    assert_parity(T_fin, Tref)                                                         # (iv)
    # not vacuous: entries were deferred (drawn = visited + deferred), and at least half of
    # the passes had a finite key above 0 with cells still to change (not asked of the two
    # 40 x 40 maps: on their 9 tiles of 16 x 16 cells the tiles next to the goal's, queued
    # with key 0, are the smallest key for half of the few passes there are)
    assert sum(pend) - stats["tile_visits"] > 0
    if kernel == 5:
        assert stats["deferred"] > 0
    if not domain.startswith("cold-corner"):
        assert 2 * live_passes >= len(keys) - 1


# ---------------------------------------------------------------------------
# argument and state errors of the two new calls
# ---------------------------------------------------------------------------
def test_stepping_argument_and_state_errors(dymu, pool, ptrs, world):
    lib = dymu.load_fim()
    key = ctypes.c_double()
    assert lib.dymu_set_stepping(None, 1) == ERR_ARG
    assert lib.dymu_dom_min_key(None, None, ctypes.byref(key)) == ERR_ARG
    eng, e3 = pool(4, prio_target=64), pool(3)
    assert lib.dymu_dom_min_key(eng.ctx, None, None) == ERR_ARG
    F0, T0 = world["maps"][ref.SHAPES[0]]
    dev = Dev(eng, ptrs, F0, T0, 0)

    def status(fn, *a, **kw):
        with pytest.raises(dymu.DymuError) as e:
            fn(*a, **kw)
        return e.value.status

    # no live domain
    assert status(eng.dom_min_key) == ERR_STATE
    # stepping on: the entries that cannot leave a domain behind refuse
    assert status(eng.solve, F0, *GOAL) == ERR_STATE
    assert status(eng.resolve_window, F0, GOAL[0], GOAL[1], 3, 3, 4, 4) == ERR_STATE
    assert status(eng.solve_until_device, dev.dF, dev.dT, NX, NY, NX, GOAL[0], GOAL[1], 5, 5) \
        == ERR_STATE
    assert status(eng.solve_seeds_until_device, dev.dF, dev.dT, NX, NY, NX, ref.SEEDS_97,
                  [(5, 5)]) == ERR_STATE
    assert status(eng.solve_batch_until_device, dev.dF, dev.dT, NX, 20, 2, NX,
                  [(0, 1, 1), (1, 2, 2)], [(0, 5, 5)]) == ERR_STATE
    dev.map()  # none of them touched the buffers
    # argument errors come first, as without stepping
    assert status(eng.solve_device, dev.dF, dev.dT, NX, NY, NX, NX, 0) == ERR_ARG
    assert status(eng.dom_min_key) == ERR_STATE
    # a live domain: the goal's key (its tile and, row 40 being the first of an 8 x 8 tile,
    # the tile across that edge), then off again after dom_finish
    eng.solve_device(dev.dF, dev.dT, NX, NY, NX, *GOAL)
    assert eng.dom_min_key() == 0.0 and eng.dom_pending() == 2
    drive(eng)
    assert status(eng.dom_min_key) == ERR_STATE
    # a domain on kernel 3 has no keys
    e3.solve_device(dev.dF, dev.dT, NX, NY, NX, *GOAL)
    assert status(e3.dom_min_key) == ERR_STATE
    drive(e3)
    assert_parity(dev.map(), T0)
    # stepping off again: the entry converges by itself
    eng.set_stepping(False)
    try:
        st = eng.solve_device(dev.dF, dev.dT, NX, NY, NX, *GOAL)
        assert st["passes"] > 0 and status(eng.dom_pending) == ERR_STATE
        assert_parity(dev.map(), T0)
        tc, _ = eng.solve_until_device(dev.dF, dev.dT, NX, NY, NX, GOAL[0], GOAL[1], 60, 35)
        want = T0[34:37, 59:62][[1, 0, 1, 1, 2], [1, 1, 0, 2, 1]].max()
        assert tc == want or abs(tc - want) <= 1e-12 * max(1.0, want)
    finally:
        eng.set_stepping(True)
