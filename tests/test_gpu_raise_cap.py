"""The raise front's pass cap (run_raise), for both callers of the one loop.

The cap is the one error of the raise that a test can reach without a failing HIP call; it
retired the domain before the loop was shared as well.  What the shared loop adds for the
single-goal update -- the domain retired after a failed launch, seeding or read-back too -- no
test reaches.

The raise launches its first four passes before it reads the pending count and tests
`p > max_passes` before each launch, so an engine created with max_passes=2 stops every raise
at its fourth launch, on any grid.  With passes_per_check=64 the host-checked pass loop of the
same engine runs 64 passes before its first check (dom_launch allows max_passes + 128) and
leaves on "nothing pending" before it tests the cap: a cold solve that converges within 64
passes succeeds on that engine.  Each case checks that it does, at 96x64 and 64x96 (6x4 and
4x6 tiles of kernel 5).

The capped raise returns DYMU_ERR_NOT_CONVERGED ("raise: pass cap reached") with its domain
retired, so the same engine then solves the new input cold: the single-goal map against the
oracle FMM within the project's tolerance (test_gpu_solver.assert_parity: the same +inf mask,
1e-12 * max(1, T)), the clearance field against clearance_edit_ref.relax from nothing on the
edited mask under test_gpu_clearance.check_field.  With max_passes=0 the same sequences succeed.
"""
import numpy as np
import pytest

import clearance_edit_ref as cref
from test_gpu_clearance import INF, Maps, check_field
from test_gpu_solver import assert_parity

pytestmark = pytest.mark.gpu

SHAPES = [(96, 64), (64, 96)]
NOT_CONVERGED = -4
C1 = 1.0 / 6.5


def engine(dymu, kernel, max_passes):
    return dymu.Engine(kernel=kernel, max_passes=max_passes, passes_per_check=64)


def expect_cap(dymu, call):
    with pytest.raises(dymu.DymuError) as e:
        call()
    assert e.value.status == NOT_CONVERGED and "raise: pass cap reached" in str(e.value)


# ---- the single-goal update ----
def goal_case(oracle, nx, ny):
    """The speed, and the speed raised in a 12x10 window next to the goal."""
    goal = (nx // 2, ny // 2)
    F0 = oracle.synth_speed(nx, ny, seed=23, obst_frac=0.03, obst_seed=29, goal=goal)
    win = (goal[0] + 2, goal[1] - 5, 12, 10)
    F1 = F0.copy()
    F1[win[1]:win[1] + win[3], win[0]:win[0] + win[2]] *= 1.5
    return goal, F0, F1, win


@pytest.mark.parametrize("max_passes", [2, 0], ids=["capped", "control"])
@pytest.mark.parametrize("kernel", [3, 5])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_single_goal_raise(dymu, oracle, monkeypatch, nx, ny, kernel, max_passes):
    goal, F0, F1, win = goal_case(oracle, nx, ny)
    T1_ref, _ = oracle.fmm(F1, goal)
    monkeypatch.setenv("DYMU_RAISE", "1")
    with engine(dymu, kernel, max_passes) as eng:
        dF, dT = eng.alloc(8 * nx * ny), eng.alloc(8 * nx * ny)
        T = np.empty((ny, nx))
        try:
            eng.h2d(dF, F0)
            st = eng.solve_device(dF, dT, nx, ny, nx, *goal)  # converges under these options
            assert st["kernel"] == kernel and 0 < st["passes"] <= 64
            eng.d2h(T, dT)
            assert_parity(T, oracle.fmm(F0, goal)[0])
            eng.h2d(dF, F1)

            def update():
                return eng.update_window_device(dF, dT, nx, ny, nx, *goal, *win, False)

            if max_passes:
                expect_cap(dymu, update)
                eng.solve_device(dF, dT, nx, ny, nx, *goal)  # the same engine, cold
            else:
                update()
                assert eng.last_update_stats()["raise_passes"] >= 4
            eng.d2h(T, dT)
        finally:
            eng.free(dF)
            eng.free(dT)
    assert_parity(T, T1_ref)


# ---- the clearance edit ----
def block_case(nx, ny):
    """A mask with a wall segment, two single cells and a 3x3 block; the same without the
    block; the block's window; the reference field of the edited mask."""
    F1 = np.full((ny, nx), 2.5)
    F1[ny // 4, 5:nx // 3] = INF
    F1[ny - 7, nx - 9] = INF
    F1[3, nx - 4] = INF
    F0 = F1.copy()
    bi, bj = nx // 2 + 3, ny // 2 - 2
    F0[bj:bj + 3, bi:bi + 3] = INF
    S1_ref = cref.relax(np.full(F1.shape, INF), F1, C1)
    assert (S1_ref <= 1.0).any() and (S1_ref > 1.0).any()
    return F0, F1, (bi, bj, 3, 3), S1_ref


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def block(request):
    return block_case(*request.param)


@pytest.mark.parametrize("max_passes", [2, 0], ids=["capped", "control"])
@pytest.mark.parametrize("kernel", [4, 5])
def test_clearance_edit_raise(dymu, block, kernel, max_passes):
    F0, F1, win, S1_ref = block
    with engine(dymu, kernel, max_passes) as eng:
        m = Maps(eng, F0)
        try:
            st = m.clearance(C1)  # converges under these options
            assert st["kernel"] == kernel and 0 < st["passes"] <= 64
            m.put(m.dF, F1)

            def edit():
                return eng.clearance_edit_device(m.dF, m.dW, m.dS, m.nx, m.ny, m.ld, C1, *win)

            if max_passes:
                expect_cap(dymu, edit)
                m.clearance(C1)  # the same engine, afresh
            else:
                edit()
                assert eng.last_update_stats()["cells_invalidated"] >= 9
            S, _ = m.get(m.dS)
        finally:
            m.close()
    check_field(S, S1_ref, F1)
