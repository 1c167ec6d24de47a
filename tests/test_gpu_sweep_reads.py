"""Kernel 5's in-tile sweep reads its seven neighbours per half-sweep from the
skewed LDS image (rb_update2, img16_row).  These grids are the smallest on which
each address of that read pattern matters, solved by the three sweep loops
(default candidate, exact_sqrt, and the general loop for C < 2^-383) and by the
deterministic schedule, against the oracle FMM:

* 16x16: one tile, every halo cell +inf, the non-interior load path;
* 48x48: 3x3 tiles, the centre one the only interior tile (edge-column W/E
  halos, N/S halo rows); the goal in the centre tile and in each of the eight
  around it, so the front enters the centre tile through every side and corner;
* 50x35: ragged last tiles in both directions.

Tolerance: tests/test_gpu_solver.py's -- identical +inf mask and
|T - Tref| <= 1e-12 * max(1, Tref)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-12
ENGINES = {"default": {}, "exact_sqrt": dict(exact_sqrt=1), "deterministic": dict(deterministic=1)}

CASES = [(16, 16, g) for g in ((0, 0), (7, 9), (15, 15))]
# tile (a, b) of the 3x3, an off-centre cell in it
CASES += [(48, 48, (16 * a + 5, 16 * b + 9)) for b in range(3) for a in range(3)]
CASES += [(50, 35, g) for g in ((20, 17), (49, 34))]


@pytest.fixture(scope="module")
def engines(dymu):
    engs = {k: dymu.Engine(**kw) for k, kw in ENGINES.items()}
    yield engs
    for e in engs.values():
        e.close()


_ref = {}


def reference(oracle, nx, ny, goal):
    """(F, Tref) of a case, computed once and shared read-only."""
    key = (nx, ny, goal)
    if key not in _ref:
        F = oracle.synth_speed(nx, ny, seed=7, obst_frac=0.05, obst_seed=11, goal=goal)
        Tref, _ = oracle.fmm(F, goal)
        F.setflags(write=False)
        Tref.setflags(write=False)
        _ref[key] = (F, Tref)
    return _ref[key]


def assert_parity(T, Tref, floor=True):
    inf_g, inf_r = np.isinf(T), np.isinf(Tref)
    assert np.array_equal(inf_g, inf_r), f"inf mask differs at {np.argwhere(inf_g != inf_r)[:5]}"
    fin = ~inf_r
    scale = np.maximum(1.0, Tref[fin]) if floor else Tref[fin]
    bad = np.abs(T[fin] - Tref[fin]) > RTOL * scale
    assert not bad.any(), f"{bad.sum()} cells beyond {RTOL} relative"


@pytest.mark.parametrize("which", sorted(ENGINES))
@pytest.mark.parametrize("nx,ny,goal", CASES)
def test_sweep_parity(engines, oracle, which, nx, ny, goal):
    F, Tref = reference(oracle, nx, ny, goal)
    assert (~np.isinf(Tref)).sum() > nx * ny // 2  # the grid is not walled off at the goal
    eng = engines[which]
    r = eng.solve(F, goal[0], goal[1])
    assert r.stats["kernel"] == 5
    assert_parity(r.T, Tref)
    assert r.T[goal[1], goal[0]] == 0.0
    if which == "deterministic":
        r2 = eng.solve(F, goal[0], goal[1])
        assert np.array_equal(r2.T.view(np.uint64), r.T.view(np.uint64))


@pytest.mark.parametrize("which", sorted(ENGINES))
@pytest.mark.parametrize("nx,ny,goal", [(48, 48, (21, 25)), (50, 35, (49, 34))])
def test_sweep_parity_tiny_speed(engines, oracle, which, nx, ny, goal):
    """F * 2^-400: every C is below 2^-383, so every visit runs the general sweep
    loop (rb_sweeps4<false>).  The scaling is exact in binary (2 C^2 ~ 2^-795 and
    every T stay normal numbers), so T * 2^400 is compared with the oracle's map of
    the scaled grid, itself scaled back -- relative to Tref alone: the max(1, .)
    floor would be a floor of 2^400 ulp-scales here."""
    F, Tunit = reference(oracle, nx, ny, goal)
    Fs = np.ldexp(F, -400)
    Ts, _ = oracle.fmm(Fs, goal)
    assert np.array_equal(np.isinf(Ts), np.isinf(Tunit))  # the oracle itself copes down there
    Tref = np.ldexp(Ts, 400)
    fin = ~np.isinf(Tref)
    assert np.all(np.abs(Tref[fin] - Tunit[fin]) <= RTOL * Tunit[fin])
    eng = engines[which]
    r = eng.solve(Fs, goal[0], goal[1])
    assert r.stats["kernel"] == 5
    assert_parity(np.ldexp(r.T, 400), Tref, floor=False)
    assert r.T[goal[1], goal[0]] == 0.0
    if which == "deterministic":
        r2 = eng.solve(Fs, goal[0], goal[1])
        assert np.array_equal(r2.T.view(np.uint64), r.T.view(np.uint64))
