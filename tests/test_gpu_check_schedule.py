"""The host-checked convergence loop (converge_checked): its K schedules,
its outcome pass by pass, and the engine after a refused call.

stats["launches"] counts pass kernels only (dom_launch, once per pass; the stop tests are
not counted), and the loop checks after every batch of K passes, so the count of a call
names the schedule it ran under:

* passes_per_check = k > 0: k passes per check, whatever the environment says;
* else the plain solve and the five-cell probe (solve_until_device): DYMU_FIRST_BATCH
  passes, then twice as many per check, at most 64;
* else the level tests (clearance_device, clearance_update_device): DYMU_FIRST_BATCH passes,
  then DYMU_UNTIL_BATCH per check.

Every map is 128x96 with a wall and a gap between the goal and the far corner, so that a
call needs several checks.
"""
import numpy as np
import pytest

from test_gpu_batch import check_parity
from test_gpu_clearance import INF, Maps

pytestmark = pytest.mark.gpu

ERR_ARG = -1
NX, NY = 128, 96
GOAL, FAR = (5, 5), (NX - 3, NY - 4)
STEP = 1.0 / 40.0  # the clearance level lies 40 cells from an obstacle
BLOCK = (20, 40)   # a new 2x2 obstacle block, 44 cells from the wall: above the old level
CALLS = ("solve", "until", "clearance", "clearance_update")
FIRST, UNTIL = 3, 5


class Case:
    pass


@pytest.fixture(scope="module")
def world(oracle):
    w = Case()
    w.F = oracle.synth_speed(NX, NY, seed=77)
    w.F[:, 64] = INF
    w.F[80:84, 64] = 2.0  # the gap
    w.F_new = w.F.copy()
    w.F_new[BLOCK[1]:BLOCK[1] + 2, BLOCK[0]:BLOCK[0] + 2] = INF
    w.T_ref = oracle.fmm(w.F, GOAL)[0]
    assert np.isfinite(w.T_ref[FAR[1], FAR[0]])
    for a in (w.F, w.F_new, w.T_ref):
        a.setflags(write=False)
    return w


def checked_calls(eng, w):
    """The entries that end in the checked loop: name -> (stats, the map they left)."""
    out = {}
    m = Maps(eng, w.F)
    try:
        st = eng.solve_device(m.dF, m.dS, NX, NY, NX, *GOAL)
        out["solve"] = (st, m.get(m.dS)[0])
        _, st = eng.solve_until_device(m.dF, m.dS, NX, NY, NX, *GOAL, *FAR)
        out["until"] = (st, m.get(m.dS)[0])
        st = m.clearance(STEP)
        out["clearance"] = (st, m.get(m.dS)[0])
        m.put(m.dF, w.F_new)
        st = eng.clearance_update_device(m.dF, m.dW, m.dS, NX, NY, NX, STEP, 0, 0, NX, NY)
        out["clearance_update"] = (st, m.get(m.dS)[0])
    finally:
        m.close()
    assert sorted(out) == sorted(CALLS)
    return out


def outcome(st):
    return (st["passes"], st["launches"], st["tile_visits"], st["inner_sweeps"])


def doubling_counts(first, limit=1 << 16):
    """The launch counts at which a loop of `first` passes, then doubling to 64, can end."""
    out, total, k = set(), 0, first
    while total < limit:
        total += k
        out.add(total)
        k = min(2 * k, 64)
    return out


@pytest.fixture
def schedule_env(monkeypatch):
    """dymu_create reads these: set before the engine exists."""
    monkeypatch.setenv("DYMU_PIPELINE", "0")
    monkeypatch.setenv("DYMU_FIRST_BATCH", str(FIRST))
    monkeypatch.setenv("DYMU_UNTIL_BATCH", str(UNTIL))


# ---- 1. the schedules ----
def test_schedules_from_the_environment(dymu, world, schedule_env):
    with dymu.Engine() as eng:
        got = {k: v[0]["launches"] for k, v in checked_calls(eng, world).items()}
    print(f"launches: {got}")
    assert sorted(doubling_counts(FIRST))[:7] == [3, 9, 21, 45, 93, 157, 221]
    for name in CALLS:
        assert got[name] > FIRST, name  # more than one check
    for name in ("solve", "until"):
        assert got[name] in doubling_counts(FIRST), name
    for name in ("clearance", "clearance_update"):
        assert got[name] % UNTIL == FIRST, name


def test_option_wins_over_the_environment(dymu, world, schedule_env):
    with dymu.Engine(passes_per_check=7) as eng:
        got = {k: v[0]["launches"] for k, v in checked_calls(eng, world).items()}
    print(f"launches: {got}")
    for name in CALLS:
        assert got[name] > 0 and got[name] % 7 == 0, name


# ---- 2. the same outcome, run after run ----
def test_outcome_is_reproducible(dymu, world):
    with dymu.Engine(deterministic=1, passes_per_check=1, kernel=5) as eng:
        a = checked_calls(eng, world)
        b = checked_calls(eng, world)
    for name in CALLS:
        print(f"{name}: (passes, launches, tile_visits, inner_sweeps) = {outcome(a[name][0])}")
    for name in CALLS:
        assert outcome(a[name][0]) == outcome(b[name][0]), name
        assert a[name][0]["launches"] == a[name][0]["passes"] > 0, name
        assert np.array_equal(a[name][1].view(np.uint64), b[name][1].view(np.uint64)), name
    check_parity(a["solve"][1], world.T_ref)


# ---- 3. a refused call leaves the engine usable ----
def test_engine_after_a_refused_call(dymu, world):
    def status(fn, *a):
        with pytest.raises(dymu.DymuError) as e:
            fn(*a)
        return e.value.status

    with dymu.Engine(passes_per_check=1) as eng:
        m = Maps(eng, world.F)
        try:
            # an early exit first, so that the refused call meets an engine with a history
            tc, _ = eng.solve_until_device(m.dF, m.dS, NX, NY, NX, *GOAL, 40, 30)
            assert np.isfinite(tc)
            assert status(eng.solve_seeds_until_device, m.dF, m.dS, NX, NY, NX, [(*GOAL, 0.0)],
                          [FAR, (NX, 5)]) == ERR_ARG
            st = eng.solve_device(m.dF, m.dS, NX, NY, NX, *GOAL)
            T = m.get(m.dS)[0]
        finally:
            m.close()
    assert st["passes"] > 0
    check_parity(T, world.T_ref)
