"""What a kernel-5 pass sets up before its first list entry -- the list scan's
prefixes and threshold bin, the stored 1 / delta of the key bins, the tile -> (tx, ty)
division, the lane geometry of the visits -- seen from outside: the solved map and the
per-pass statistics.

Engines of this file's own (kernel 5, a per-pass target of 16 tiles so the threshold
binds on small grids), default and deterministic.  The first solve of each is 256^2:
DESIGN.md s8.2 records an unexplained wrong map after a first grid of 48^2 or less on
an engine, which this file must not walk into.

* 256^2: 256 tiles, so the lists exceed the target, b* binds and all 16 shards fill;
* 320x200: a ragged last tile column and row, 20 tiles per row (not a power of two), so
  the tile -> (tx, ty) division matters.

Parity: tests/test_gpu_sweep_reads.py's mask and tolerance -- identical +inf mask and
|T - Tref| <= 1e-12 * max(1, Tref)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-12
ENGINES = {"default": {}, "deterministic": dict(deterministic=1)}
GRIDS = {"256": (256, 256, (171, 60)), "320x200": (320, 200, (43, 150))}  # goal off-centre
LISTED, VISITED, COLOUR, KEY, BSTAR, ENQUEUED = 0, 1, 2, 3, 8, 10  # Engine.PASS_STAT_FIELDS


@pytest.fixture(scope="module")
def maps(oracle):
    out = {}
    for name, (nx, ny, goal) in GRIDS.items():
        F = oracle.synth_speed(nx, ny, seed=7, obst_frac=0.05, obst_seed=11, goal=goal)
        Tref, _ = oracle.fmm(F, goal)
        F.setflags(write=False)
        Tref.setflags(write=False)
        out[name] = (F, Tref, goal)
    return out


@pytest.fixture(scope="module")
def runs(dymu, maps):
    """(T, per-pass statistics) of every engine and grid, 256^2 first on each engine;
    the deterministic engine solves each grid twice."""
    out = {}
    for which, kw in ENGINES.items():
        with dymu.Engine(kernel=5, prio_target=16, **kw) as eng:
            eng.set_pass_stats(True)
            for name in ("256", "320x200"):
                F, _, goal = maps[name]
                r = eng.solve(F, goal[0], goal[1])
                assert r.stats["kernel"] == 5
                out[which, name] = (r.T, eng.last_pass_stats())
                if which == "deterministic":
                    out[which, name, "again"] = eng.solve(F, goal[0], goal[1]).T
    return out


CASES = [(w, g) for w in sorted(ENGINES) for g in sorted(GRIDS)]


@pytest.mark.parametrize("which,grid", CASES)
def test_parity(runs, maps, which, grid):
    T = runs[which, grid][0]
    _, Tref, goal = maps[grid]
    assert (~np.isinf(Tref)).sum() > Tref.size // 2  # the grid is not walled off at the goal
    inf_g, inf_r = np.isinf(T), np.isinf(Tref)
    assert np.array_equal(inf_g, inf_r), f"inf mask differs at {np.argwhere(inf_g != inf_r)[:5]}"
    fin = ~inf_r
    bad = np.abs(T[fin] - Tref[fin]) > RTOL * np.maximum(1.0, Tref[fin])
    assert not bad.any(), f"{bad.sum()} cells beyond {RTOL} relative"
    assert T[goal[1], goal[0]] == 0.0


@pytest.mark.parametrize("which,grid", CASES)
def test_pass_accounting(runs, which, grid):
    ps = runs[which, grid][1].astype(np.int64)
    assert len(ps) > 2
    # every listed entry is visited or deferred, by its colour or by its key
    assert np.array_equal(ps[:, VISITED] + ps[:, COLOUR] + ps[:, KEY], ps[:, LISTED])
    # what a pass appends is what the next one lists
    assert np.array_equal(ps[1:, LISTED], ps[:-1, ENQUEUED])
    # a list no longer than the target is relaxed whole
    assert np.all(ps[ps[:, LISTED] <= 16, BSTAR] == 64)
    # and the threshold is exercised: some pass has one and defers entries by their key
    assert np.any((ps[:, BSTAR] < 64) & (ps[:, KEY] > 0))


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_deterministic_twice(runs, grid):
    a, b = runs["deterministic", grid][0], runs["deterministic", grid, "again"]
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
