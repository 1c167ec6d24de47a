"""The argument dymu_clearance_edit_device rests on, on the CPU.

A valid old field (clearance_edit_ref.ragged_field: converged up to the level, ragged above
it) and a new mask that frees obstacle cells.  Against goalset_ref.fmm_seeds on the new mask,
S_ref, at 97x61:

* after the closure every finite non-obstacle cell is >= S_ref * (1 - 1e-12): what is kept
  bounds the new field from above;
* after the relaxation the conditions of test_gpu_clearance.check_field hold: the cells at or
  below the level hold the new field;
* at least one cell at or below the level rose, so a missing raise would show;
* on an old field that was cut and NOT closed -- cells left standing on values that are gone
  -- the same closure leaves cells below S_ref: its front stops at the holes.  This is the
  failure the GPU tests of the entry catch.
"""
import numpy as np
import pytest

import clearance_edit_ref as cref
import goalset_ref as ref
from test_gpu_clearance import check_field, obstacle_seeds

NX, NY = 97, 61
C1 = 1.0 / 6.5
INF = np.inf


def field_of(oracle, F):
    return ref.fmm_seeds(oracle, np.full(F.shape, C1), obstacle_seeds(F))


@pytest.fixture(scope="module")
def old(oracle):
    F0 = oracle.synth_speed(NX, NY, seed=41, obst_frac=0.02, obst_seed=9, goal=(70, 40))
    S0 = field_of(oracle, F0)
    assert (S0 <= 1.0).any() and (S0 > 1.3).any()
    F0.setflags(write=False)
    S0.setflags(write=False)
    return F0, S0


def new_mask(F0, case):
    """The new mask of a case, from the old one."""
    rng = np.random.default_rng(3)
    F1 = F0.copy()
    cells = np.argwhere(~(F0 < INF))
    if case == "third":
        drop = cells[rng.permutation(len(cells))[:len(cells) // 3]]
    elif case == "mixed":
        drop = cells[rng.permutation(len(cells))[:len(cells) // 3]]
        free = np.argwhere(F0 < INF)
        for j, i in free[rng.permutation(len(free))[:12]]:
            F1[j, i] = INF
    else:  # all but one
        drop = cells[1:]
    for j, i in drop:
        F1[j, i] = 2.5
    return F1


@pytest.fixture(scope="module", params=["third", "mixed", "all-but-one"])
def case(request, oracle, old):
    F0, S0 = old
    F1 = new_mask(F0, request.param)
    S1_ref = field_of(oracle, F1)
    return F0, S0, F1, S1_ref


def test_closure_bounds_and_relaxation_fills(case):
    F0, S0, F1, S1_ref = case
    S_old = cref.ragged_field(S0, F0, C1, np.random.default_rng(11))
    ragged = np.isposinf(S_old) & (S0 <= 1.3)
    assert ragged.any() and np.array_equal(S_old[S0 <= 1.0], S0[S0 <= 1.0])
    S, n_gone = cref.closure(S_old, F1, C1)
    low = cref.below_bound(S, S1_ref, F1)
    rose = (S1_ref <= 1.0) & (F1 < INF) & (S1_ref > S_old * (1.0 + 1e-12))
    print(f"{n_gone} cells invalidated, {low.sum()} kept below the new field, "
          f"{rose.sum()} cells at or below the level rise")
    assert n_gone > 0 and not low.any()
    assert rose.any()
    assert np.isposinf(S[rose]).all()  # every one of them went
    S = cref.relax(S, F1, C1)
    check_field(S, S1_ref, F1)
    freed = (F1 < INF) & ~(F0 < INF)
    assert freed.any() and (S[freed] > 0.0).all()


def test_unclosed_old_field_breaks_the_bound(case):
    """Only 265 cells of the old field lie above the level, so how many are left standing
    behind a hole depends on the draw (0 to 5 of them): five draws, each also closed first,
    which must never break the bound."""
    F0, S0, F1, S1_ref = case
    broken = []
    for seed in range(11, 16):
        S_bad = cref.ragged_field(S0, F0, C1, np.random.default_rng(seed), close=False)
        S, _ = cref.closure(S_bad, F1, C1)
        broken.append(int(cref.below_bound(S, S1_ref, F1).sum()))
        S_ok = cref.ragged_field(S0, F0, C1, np.random.default_rng(seed))
        S, _ = cref.closure(S_ok, F1, C1)
        assert not cref.below_bound(S, S1_ref, F1).any()
    print(f"cells kept below the new field, per draw: {broken}")
    assert sum(broken) > 0


def test_closure_of_a_converged_field_changes_nothing(old):
    F0, S0 = old
    S, n_gone = cref.closure(S0, F0, C1, everywhere=True)
    assert n_gone == 0 and np.array_equal(S.view(np.uint64), S0.view(np.uint64))
