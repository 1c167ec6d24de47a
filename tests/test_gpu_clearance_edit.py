"""The clearance field after obstacles were freed inside a window.

dymu_clearance_edit_device brings the field left for an OLD mask to the mask of dF, which may
free obstacle cells inside the window, add some, or both: the field is raised where the freed
cells supported it, then re-propagated from the added cells and from the boundary of what
was raised.  The yardstick is the one of test_gpu_clearance.py on the NEW mask
(goalset_ref.fmm_seeds on np.full(shape, c): within 1e-12 up to the level, an upper bound or
+inf above it, +0.0 on an obstacle cell), and the reported box the one of
test_gpu_clearance_update.py: outside it nothing moved.  A raise that stops short leaves a
cell below the new field, which check_field's bounds catch (tests/test_clearance_edit_ref.py
shows the same on the CPU).
"""
import ctypes

import numpy as np
import pytest

import goalset_ref as ref
from test_gpu_clearance import INF, KERNELS, SENT, Maps, check_field, obstacle_seeds, wall_map
from test_gpu_clearance_update import (C1, NX, NY, WINDOW, bits, check_box, fields,  # noqa: F401
                                       update)

pytestmark = pytest.mark.gpu


def edit(m, c, win):
    return m.eng.clearance_edit_device(m.dF, m.dW, m.dS, m.nx, m.ny, m.ld, c, *win)


def field_of(oracle, F, c=C1):
    return ref.fmm_seeds(oracle, np.full(F.shape, c), obstacle_seeds(F))


def check_freed(S, F_old, F_new):
    freed = (F_new < INF) & ~(F_old < INF)
    assert freed.any() and (S[freed] > 0.0).all()


# ---- 1. parity: the update's fixture backwards ----
@pytest.mark.parametrize("pad", [0, 7])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_parity(dymu, fields, kernel, pad):
    F0, S0_ref, F1, S1_ref = fields
    with dymu.Engine(**KERNELS[kernel]) as eng:
        m = Maps(eng, F1, ld=NX + pad)
        try:
            m.clearance(C1)
            S1, _ = m.get(m.dS)
            check_field(S1, S1_ref, F1)
            m.put(m.dF, F0)
            st = edit(m, C1, WINDOW)
            raised = eng.last_update_stats()
            S0, S_pad = m.get(m.dS)
            F_after, F_pad = m.get(m.dF)
            W, W_pad = m.get(m.dW)
            m.put(m.dS, np.full(F0.shape, SENT))
            m.clearance(C1)  # the same inputs, solved afresh on the same engine
            S_fresh, _ = m.get(m.dS)
        finally:
            m.close()
    print(f"kernel {st['kernel']}: raise {raised}, then {st['passes']} passes, "
          f"{st['tile_visits']} tile visits, box {st['box']}")
    assert st["kernel"] == kernel and st["passes"] > 0
    assert raised["raise_passes"] > 0 and raised["raise_visits"] > 0
    assert raised["cells_invalidated"] > 0
    assert np.array_equal(bits(F_after), bits(F0))  # read only
    assert np.array_equal(bits(W), bits(np.full(F0.shape, C1)))  # still c everywhere
    assert (S_pad == SENT).all() and (W_pad == SENT).all() and (F_pad == SENT).all()
    check_field(S0, S0_ref, F0)
    check_freed(S0, F1, F0)
    check_box(S1, S0, st["box"])
    near = S0_ref <= 1.0
    d = np.abs(S0[near] - S_fresh[near]).max()
    print(f"edit against a fresh solve, cells at or below the level: max |dS| = {d:.3e}")
    assert d <= 1e-12


# ---- 2. freed and added in one window ----
def test_freed_and_added_together(dymu, oracle, fields):
    F0, _, F1, _ = fields
    Fa, Fb = F0.copy(), F0.copy()
    Fa[:, :48] = F1[:, :48]  # the old mask holds the left half's extra cells,
    Fb[:, 48:] = F1[:, 48:]  # the new one the right half's
    assert ((Fb < INF) & ~(Fa < INF)).any() and ((Fa < INF) & ~(Fb < INF)).any()
    Sb_ref = field_of(oracle, Fb)
    for kernel in sorted(KERNELS):
        with dymu.Engine(**KERNELS[kernel]) as eng:
            m = Maps(eng, Fa, ld=NX + 7)
            try:
                m.clearance(C1)
                Sa, _ = m.get(m.dS)
                m.put(m.dF, Fb)
                st = edit(m, C1, WINDOW)
                Sb, S_pad = m.get(m.dS)
            finally:
                m.close()
        assert st["passes"] > 0 and (S_pad == SENT).all()
        check_field(Sb, Sb_ref, Fb)
        check_freed(Sb, Fa, Fb)
        check_box(Sa, Sb, st["box"])


# ---- 3. all but one obstacle freed, then all ----
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_all_but_one_then_all_freed(dymu, oracle, fields, kernel):
    F0, _, _, _ = fields
    j1, i1 = (int(v) for v in np.argwhere(~(F0 < INF))[5])
    F_one = np.where(F0 < INF, F0, 2.5)
    F_one[j1, i1] = INF
    F_none = np.where(F0 < INF, F0, 2.5)
    S_one_ref = field_of(oracle, F_one)
    with dymu.Engine(**KERNELS[kernel]) as eng:
        m = Maps(eng, F0)
        try:
            m.clearance(C1)
            S0, _ = m.get(m.dS)
            m.put(m.dF, F_one)
            sa = edit(m, C1, WINDOW)
            S_one, _ = m.get(m.dS)
            m.put(m.dF, F_none)
            sb = edit(m, C1, (i1, j1, 1, 1))
            S_none, _ = m.get(m.dS)
            raised = eng.last_update_stats()
        finally:
            m.close()
    check_field(S_one, S_one_ref, F_one)
    check_freed(S_one, F0, F_one)
    check_box(S0, S_one, sa["box"])
    assert np.isposinf(S_none).all()  # no obstacle: +inf everywhere, DYMU_OK
    check_box(S_one, S_none, sb["box"])
    assert raised["cells_invalidated"] == np.isfinite(S_one).sum()


# ---- 4. an edit, the add-only update, another edit ----
def test_edit_update_edit(dymu, oracle, fields):
    F0, S0_ref, F1, S1_ref = fields
    F2 = F1.copy()
    gone = np.argwhere(~(F0 < INF))[::3]
    for j, i in gone:
        F2[j, i] = 2.5
    S2_ref = field_of(oracle, F2)
    with dymu.Engine(kernel=5, prio_target=16) as eng:
        m = Maps(eng, F1)
        try:
            m.clearance(C1)
            Sa, _ = m.get(m.dS)
            m.put(m.dF, F0)
            s1 = edit(m, C1, WINDOW)
            Sb, _ = m.get(m.dS)
            m.put(m.dF, F1)
            s2 = update(m, C1, WINDOW)  # the state an edit leaves meets its preconditions
            Sc, _ = m.get(m.dS)
            m.put(m.dF, F2)
            s3 = edit(m, C1, WINDOW)
            Sd, _ = m.get(m.dS)
        finally:
            m.close()
    for S_old, S_new, S_ref, F, st in ((Sa, Sb, S0_ref, F0, s1), (Sb, Sc, S1_ref, F1, s2),
                                       (Sc, Sd, S2_ref, F2, s3)):
        assert st["passes"] > 0
        check_field(S_new, S_ref, F)
        check_box(S_old, S_new, st["box"])


# ---- 5. locality ----
def test_edit_stays_local(dymu):
    """The 512x64 wall map, c = 1/8.  The wall's field with a 2x2 block at column 300 added by
    the update, which reports the box it wrote; the edit then frees the block.  The raise
    ends where the values that stood on the block end, which is inside that box, and claims
    at most one more ring of 16-cell tiles; beyond the block's reach the wall's field never
    came, so the cone has no boundary and the passes have nothing to fill."""
    F0, S0_ref = wall_map()
    F1 = F0.copy()
    bi, bj = 300, 30
    F1[bj:bj + 2, bi:bi + 2] = INF
    with dymu.Engine(passes_per_check=1) as eng:
        m = Maps(eng, F0)
        try:
            m.clearance(0.125)
            m.put(m.dF, F1)
            su = update(m, 0.125, (bi, bj, 2, 2))
            S1, _ = m.get(m.dS)
            m.put(m.dF, F0)
            st = edit(m, 0.125, (bi, bj, 2, 2))
            raised = eng.last_update_stats()
            S2, _ = m.get(m.dS)
            fresh = m.clearance(0.125)  # the alternative: the wall alone solved afresh
        finally:
            m.close()
    print(f"kernel {st['kernel']}: update box {su['box']}; edit: raise {raised}, "
          f"{st['passes']} passes, {st['tile_visits']} tile visits, box {st['box']}; fresh solve "
          f"{fresh['passes']} passes, {fresh['tile_visits']} visits")
    check_field(S2, S0_ref, F0)
    check_box(S1, S2, st["box"])
    assert raised["cells_invalidated"] > 0 and np.isposinf(S2[:, 200:]).all()
    ui, uj, uw, uh = su["box"]
    i0, j0, w, h = st["box"]
    assert w > 0 and h > 0
    assert max(ui - 16, 0) <= i0 and i0 + w <= min(ui + uw + 16, 512)
    assert max(uj - 16, 0) <= j0 and j0 + h <= min(uj + uh + 16, 64)
    assert st["tile_visits"] < fresh["tile_visits"]


def tiles_around(finite, tile=16):
    """(i0, j0, i1, j1): the 16-cell tiles that hold a cell of `finite`, grown by one tile on
    every side and clipped to the grid."""
    jj, ii = np.nonzero(finite)
    ny, nx = finite.shape
    return (max(ii.min() // tile * tile - tile, 0), max(jj.min() // tile * tile - tile, 0),
            min((ii.max() // tile + 1) * tile + tile, nx), min((jj.max() // tile + 1) * tile + tile, ny))


def test_edit_of_a_cold_solved_field_stays_local(dymu):
    """The same map with the wall and the block solved cold in one solve, the state a whole
    recompute leaves, then the block freed.  A cold solve runs past the level before its stop
    test sees the keys, so the field around the block is wider than the one an update leaves,
    and all of it stood on the block: the raise invalidates finite cells only and claims the
    tiles across the edges of tiles it invalidated in, so its box lies inside the 16-cell tiles
    that held a finite value around the block, grown by one tile.  The wall's field ends 35
    tiles away, so there is no boundary and the passes visit nothing."""
    F0, S0_ref = wall_map()
    F1 = F0.copy()
    bi, bj = 300, 30
    F1[bj:bj + 2, bi:bi + 2] = INF
    with dymu.Engine(passes_per_check=1) as eng:
        m = Maps(eng, F1)
        try:
            m.clearance(0.125)
            S1, _ = m.get(m.dS)
            m.put(m.dF, F0)
            st = edit(m, 0.125, (bi, bj, 2, 2))
            raised = eng.last_update_stats()
            S2, _ = m.get(m.dS)
            fresh = m.clearance(0.125)
        finally:
            m.close()
    around = np.isfinite(S1)
    around[:, :100] = False
    lo_i, lo_j, hi_i, hi_j = tiles_around(around)
    print(f"kernel {st['kernel']}: finite around the block within {(lo_i, lo_j, hi_i, hi_j)} grown; "
          f"raise {raised}, {st['passes']} passes, {st['tile_visits']} tile visits, box {st['box']}; "
          f"fresh solve {fresh['tile_visits']} visits")
    check_field(S2, S0_ref, F0)
    check_box(S1, S2, st["box"])
    assert raised["cells_invalidated"] == around.sum() and np.isposinf(S2[:, 100:]).all()
    i0, j0, w, h = st["box"]
    assert w > 0 and h > 0
    assert lo_i <= i0 and i0 + w <= hi_i and lo_j <= j0 and j0 + h <= hi_j
    assert st["tile_visits"] < fresh["tile_visits"]


def test_edit_refills_from_the_wall(dymu):
    """A block at columns 10-11, inside the wall's reach, solved cold with the wall and then
    freed: the cells nearer the block than the wall stood on it, the raise takes them, and the
    passes refill them from the wall's field at the cone's boundary.  The block's reach of 8
    cells meets the tile rows 1 and 2 of tile column 0 only (column 16 is two levels from the
    wall), where a fresh solve of the wall has to visit all four tiles of that column."""
    F0, S0_ref = wall_map()
    F1 = F0.copy()
    bi, bj = 10, 30
    F1[bj:bj + 2, bi:bi + 2] = INF
    with dymu.Engine(passes_per_check=1) as eng:
        m = Maps(eng, F1)
        try:
            m.clearance(0.125)
            S1, _ = m.get(m.dS)
            m.put(m.dF, F0)
            st = edit(m, 0.125, (bi, bj, 2, 2))
            raised = eng.last_update_stats()
            S2, _ = m.get(m.dS)
            fresh = m.clearance(0.125)
        finally:
            m.close()
    print(f"kernel {st['kernel']}: raise {raised}, {st['passes']} passes, {st['tile_visits']} tile "
          f"visits, box {st['box']}; fresh solve {fresh['passes']} passes, {fresh['tile_visits']} "
          f"visits")
    check_field(S2, S0_ref, F0)
    check_box(S1, S2, st["box"])
    assert raised["cells_invalidated"] > 0
    assert st["passes"] > 0 and 0 < st["tile_visits"] < fresh["tile_visits"]
    assert np.abs(S2[:, :9] - S0_ref[:, :9]).max() <= 1e-12


# ---- 5b. the epoch wrap between the raise and the passes ----
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_epoch_wrap_between_raise_and_passes(dymu, fields, kernel):
    """The raise and the passes run on two domains, and dom_begin restarts the 32-bit epochs
    (every stamp zeroed) when base + pass cap + 136 would reach 0xFFFFFFF0.  A base four below
    that threshold lets the raise's domain begin, and the domain of the passes, eight epochs
    on, wraps: the raise's stamps are gone when the cone's boundary is looked for."""
    F0, S0_ref, F1, S1_ref = fields
    tile = 16 if kernel == 5 else 8
    ntiles = -(-NX // tile) * -(-NY // tile)
    threshold = 0xFFFFFFF0 - (4 * ntiles + 1024) - 128 - 8
    with dymu.Engine(**KERNELS[kernel]) as eng:
        m = Maps(eng, F1)
        try:
            m.clearance(C1)
            S1, _ = m.get(m.dS)
            m.put(m.dF, F0)
            eng.raise_epoch_base(threshold - 4)
            st = edit(m, C1, WINDOW)
            S0, _ = m.get(m.dS)
            m.put(m.dF, F1)
            s2 = update(m, C1, WINDOW)  # and the engine goes on from the restarted epochs
            S1b, _ = m.get(m.dS)
        finally:
            m.close()
    assert st["passes"] > 0
    check_field(S0, S0_ref, F0)
    check_box(S1, S0, st["box"])
    check_field(S1b, S1_ref, F1)
    check_box(S0, S1b, s2["box"])


# ---- 6. nothing changed ----
def test_nothing_changed(dymu, fields):
    F0, _, _, _ = fields
    with dymu.Engine() as eng:
        m = Maps(eng, F0, ld=NX + 7)
        try:
            m.clearance(C1)
            S0, _ = m.get(m.dS)
            wins = (WINDOW, (20, 10, 30, 25), (96, 60, 1, 1))
            out = [(edit(m, C1, w), eng.last_update_stats()) for w in wins]
            S1, S_pad = m.get(m.dS)
        finally:
            m.close()
    for (st, raised), w in zip(out, wins):
        assert st["passes"] == 0 and st["tile_visits"] == 0
        assert st["box"] == (w[0], w[1], 0, 0)
        assert not any(raised.values())
    assert np.array_equal(bits(S0), bits(S1)) and (S_pad == SENT).all()


# ---- 7. arguments ----
def test_bad_arguments_touch_nothing(dymu, fields):
    F0, _, F1, _ = fields
    with dymu.Engine() as eng:
        m = Maps(eng, F0)
        call = eng._lib.dymu_clearance_edit_device
        box = (4 * np.ones(4, dtype=np.uint32))
        try:
            good = dict(ctx=eng.ctx, dF=m.dF, dW=m.dW, dS=m.dS, nx=NX, ny=NY, ld=NX, c=C1, i0=0,
                        j0=0, w=NX, h=NY)
            bad = [dict(ctx=None), dict(dF=None), dict(dW=None), dict(dS=None), dict(nx=0),
                   dict(ny=0), dict(ld=NX - 1), dict(c=0.0), dict(c=-1.0), dict(c=np.nan),
                   dict(c=INF), dict(w=0), dict(h=0), dict(i0=NX), dict(j0=NY)]
            pbox = box.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
            for b in bad:
                a = {**good, **b}
                rc = call(a["ctx"], a["dF"], a["dW"], a["dS"], a["nx"], a["ny"], a["ld"], a["c"],
                          a["i0"], a["j0"], a["w"], a["h"], None, pbox, None)
                assert rc == -1, b
            S, _ = m.get(m.dS)
            W, _ = m.get(m.dW)
            assert (S == SENT).all() and (W == SENT).all() and (box == 4).all()
            eng.set_stepping(True)
            with pytest.raises(dymu.DymuError) as e:
                edit(m, C1, WINDOW)
            assert e.value.status == -7
            S, _ = m.get(m.dS)
            assert (S == SENT).all()
            eng.set_stepping(False)
            m.put(m.dF, F1)
            m.clearance(C1)  # and the context still works, box and stats being optional
            m.put(m.dF, F0)
            assert call(eng.ctx, m.dF, m.dW, m.dS, NX, NY, NX, C1, 0, 0, NX, NY, None, None,
                        None) == 0
            S, _ = m.get(m.dS)
            assert (S[~(F0 < INF)] == 0.0).all() and (S[(F0 < INF)] > 0.0).all()
        finally:
            m.close()


# ---- 8. determinism ----
def test_deterministic_runs_are_bit_identical(dymu, fields):
    F0, S0_ref, F1, _ = fields
    out = []
    for _ in range(2):
        with dymu.Engine(deterministic=1) as eng:
            m = Maps(eng, F1, ld=NX + 7)
            try:
                m.clearance(C1)
                m.put(m.dF, F0)
                st = edit(m, C1, WINDOW)
                out.append((m.get(m.dS)[0], st["box"], eng.last_update_stats()))
            finally:
                m.close()
        assert st["kernel"] == 5
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and out[0][1:] == out[1][1:]
    check_field(out[0][0], S0_ref, F0)


# ---- 9. the planner ----
PNX, PNY = 128, 96
PGOAL = (90, 60)


@pytest.fixture(scope="module")
def pcase(oracle):
    """128x96, 2 % obstacles (none next to the goal), and a 3x3 box in clear terrain."""
    from test_gpu_global_risk import risk_ref, speed
    F = oracle.synth_speed(PNX, PNY, seed=33, obst_frac=0.02, obst_seed=17, goal=PGOAL)
    blk = F[PGOAL[1] - 1:PGOAL[1] + 2, PGOAL[0] - 1:PGOAL[0] + 2]
    blk[~np.isfinite(blk)] = 3.0
    cost = np.where(np.isfinite(F), F, -1.0)
    clear = risk_ref(oracle, ~(speed(cost) < INF)) == 0
    i, j = next((i, j) for j in range(8, PNY - 11) for i in range(8, PNX - 11)
                if clear[j - 4:j + 7, i - 4:i + 7].all()
                and abs(i - PGOAL[0]) + abs(j - PGOAL[1]) > 16)
    cost1 = cost.copy()
    cost1[j:j + 3, i:i + 3] = INF  # cost +inf: obstacles of the mask that a finite cost frees
    cost2 = cost1.copy()
    cost2[j:j + 3, i:i + 3] = [[2.0, 2.5, 3.0], [1.5, 2.0, 2.5], [3.5, 3.0, 2.0]]
    cost2[j + 1, i + 3] = -1.0  # and another obstacle beside the freed block
    for a in (cost, cost1, cost2):
        a.setflags(write=False)
    return cost, cost1, cost2, (i, j)


@pytest.mark.parametrize("track", [True, False], ids=["tracked", "untracked"])
def test_planner_frees_a_block(dymu, oracle, pcase, track):
    from test_gpu_cost_window import check_risk_and_map
    from test_gpu_global_risk import new_planner, wp
    cost, cost1, cost2, (i, j) = pcase
    p = new_planner(dymu, cost)
    try:
        if track:
            p.trackObstacleRemoval(True)
        assert p.setGoal(wp(*PGOAL)) and p.computeEntireTotalCostMap()
        assert p.lastRiskUpdateKind() == 1
        assert p.setCostMapWindow(i, j, cost1[j:j + 3, i:i + 3])
        R1 = check_risk_and_map(p, oracle, dymu, cost1)
        assert p.lastRiskUpdateKind() == 2
        assert (R1[j:j + 3, i:i + 3] == 1.0).all()
        # the block freed, another cell added beside it, in one box
        assert p.setCostMapWindow(i, j, cost2[j:j + 3, i:i + 4])
        R2 = check_risk_and_map(p, oracle, dymu, cost2)
        assert p.lastRiskUpdateKind() == (3 if track else 1)
        assert (R2[j:j + 3, i:i + 3] < 1.0).all() and R2[j + 1, i + 3] == 1.0
        assert R2[j + 1, i] < R1[j + 1, i]  # R fell as well as rose
        up = p.lastRiskUpdate()
        print(f"kind {p.lastRiskUpdateKind()}: box {up['box']}, {up['passes']} passes")
        bw, bh = up["box"][2:]
        if track:
            assert 0 < bw * bh < PNX * PNY
            assert p.lastRiskRaise()["cells_invalidated"] >= 9
        else:
            assert up["box"] == (0, 0, PNX, PNY)
            assert not any(p.lastRiskRaise().values())
    finally:
        p.close()
