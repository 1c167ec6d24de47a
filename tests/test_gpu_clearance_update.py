"""Incremental update of the clearance field after obstacles were added.

dymu_clearance_update_device brings the field dymu_clearance_device left for an OLD mask to
the mask of dF, which adds obstacle cells inside a window, by a decrease-only warm start from
the new cells.  The yardstick is the one of test_gpu_clearance.py, on the NEW mask:
goalset_ref.fmm_seeds on np.full(shape, c), S_ref; where S_ref <= 1 the field is within
1e-12 of it, every other cell holds an upper bound or +inf, an obstacle cell +0.0.  On top
of that the call reports the box of the cells it may have written: every cell outside it is
bit for bit what it was, and every cell that changed lies inside it.
"""
import numpy as np
import pytest

import goalset_ref as ref
from test_gpu_clearance import INF, KERNELS, SENT, Maps, check_field, obstacle_seeds, wall_map

pytestmark = pytest.mark.gpu

NX, NY = 97, 61
C1 = 1.0 / 6.5
# tile corners, both edge columns of 8- and 16-cell tiles, the grid border
HAND = [(0, 0), (96, 60), (15, 21), (16, 21), (31, 15), (32, 16), (7, 40), (8, 41), (96, 30)]
NAN_CELL = (50, 33)
WINDOW = (0, 0, 200, 200)  # clipped to the grid


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def update(m, c, win):
    return m.eng.clearance_update_device(m.dF, m.dW, m.dS, m.nx, m.ny, m.ld, c, *win)


def in_box(shape, box):
    i0, j0, w, h = box
    inside = np.zeros(shape, dtype=bool)
    inside[j0:j0 + h, i0:i0 + w] = True
    return inside


def check_box(S0, S1, box):
    """Outside the box nothing moved; every cell that changed is inside it."""
    inside = in_box(S0.shape, box)
    changed = bits(S0) != bits(S1)
    print(f"box {box}: {inside.sum()} cells, {changed.sum()} changed")
    assert np.array_equal(bits(S0)[~inside], bits(S1)[~inside])
    assert not (changed & ~inside).any()


@pytest.fixture(scope="module")
def fields(oracle):
    """97x61 with 2 % obstacles (the old mask), and the new mask: the hand-placed cells, a NaN
    cell and a 2x2 block where the old field is above the level; both references, once."""
    F0 = oracle.synth_speed(NX, NY, seed=41, obst_frac=0.02, obst_seed=9, goal=(70, 40))
    S0_ref = ref.fmm_seeds(oracle, np.full(F0.shape, C1), obstacle_seeds(F0))
    far = np.where(np.isfinite(S0_ref), S0_ref, 0.0)
    far[-1, :] = far[:, -1] = 0.0  # room for the 2x2 block
    bj, bi = np.unravel_index(np.argmax(far), far.shape)
    assert S0_ref[bj, bi] > 1.0  # the block lands where the old solve stopped short
    F1 = F0.copy()
    for i, j in HAND:
        assert F0[j, i] < INF
        F1[j, i] = INF
    F1[NAN_CELL[1], NAN_CELL[0]] = np.nan
    F1[bj:bj + 2, bi:bi + 2] = INF
    S1_ref = ref.fmm_seeds(oracle, np.full(F1.shape, C1), obstacle_seeds(F1))
    for a in (F0, F1, S0_ref, S1_ref):
        a.setflags(write=False)
    return F0, S0_ref, F1, S1_ref


# ---- 1. parity ----
@pytest.mark.parametrize("pad", [0, 7])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_parity(dymu, fields, kernel, pad):
    F0, S0_ref, F1, S1_ref = fields
    with dymu.Engine(**KERNELS[kernel]) as eng:
        m = Maps(eng, F0, ld=NX + pad)
        try:
            m.clearance(C1)
            S0, _ = m.get(m.dS)
            check_field(S0, S0_ref, F0)
            m.put(m.dF, F1)
            st = update(m, C1, WINDOW)
            S1, S_pad = m.get(m.dS)
            F_after, F_pad = m.get(m.dF)
            W, W_pad = m.get(m.dW)
            m.put(m.dS, np.full(F1.shape, SENT))
            m.clearance(C1)  # the same inputs, solved afresh on the same engine
            S_fresh, _ = m.get(m.dS)
        finally:
            m.close()
    assert st["kernel"] == kernel and st["passes"] > 0
    assert np.array_equal(bits(F_after), bits(F1))  # read only
    assert np.array_equal(bits(W), bits(np.full(F1.shape, C1)))  # still c everywhere
    assert (S_pad == SENT).all() and (W_pad == SENT).all() and (F_pad == SENT).all()
    check_field(S1, S1_ref, F1)
    check_box(S0, S1, st["box"])
    # the same contract as a fresh solve: both within the parity bound up to the level
    near = S1_ref <= 1.0
    d = np.abs(S1[near] - S_fresh[near]).max()
    print(f"update against a fresh solve, cells at or below the level: max |dS| = {d:.3e}")
    assert d <= 1e-12


# ---- 2. nothing new, two in a row, a freed cell ----
def test_nothing_new(dymu, fields):
    F0, _, _, _ = fields
    with dymu.Engine() as eng:
        m = Maps(eng, F0, ld=NX + 7)
        try:
            m.clearance(C1)
            S0, _ = m.get(m.dS)
            out = [update(m, C1, w) for w in (WINDOW, (20, 10, 30, 25), (96, 60, 1, 1))]
            S1, S_pad = m.get(m.dS)
        finally:
            m.close()
    for st in out:
        assert st["passes"] == 0 and st["tile_visits"] == 0
        assert st["box"][2] == 0 and st["box"][3] == 0
    assert np.array_equal(bits(S0), bits(S1)) and (S_pad == SENT).all()


def test_two_updates_in_a_row(dymu, oracle, fields):
    F0, _, F1, S1_ref = fields
    Fa = F0.copy()
    Fa[:, :48] = F1[:, :48]  # first the left half's new cells, then the rest
    Sa_ref = ref.fmm_seeds(oracle, np.full(Fa.shape, C1), obstacle_seeds(Fa))
    with dymu.Engine(kernel=5, prio_target=16) as eng:
        m = Maps(eng, F0)
        try:
            m.clearance(C1)
            S0, _ = m.get(m.dS)
            m.put(m.dF, Fa)
            sa = update(m, C1, (0, 0, 48, NY))
            Sa, _ = m.get(m.dS)
            m.put(m.dF, F1)
            sb = update(m, C1, (48, 0, NX - 48, NY))
            Sb, _ = m.get(m.dS)
        finally:
            m.close()
    assert sa["passes"] > 0 and sb["passes"] > 0
    check_field(Sa, Sa_ref, Fa)
    check_box(S0, Sa, sa["box"])
    check_field(Sb, S1_ref, F1)
    check_box(Sa, Sb, sb["box"])


def test_freed_cell_is_refused(dymu, fields):
    F0, _, F1, _ = fields
    j, i = (int(v) for v in np.argwhere(~(F0 < INF))[3])
    F = F1.copy()
    F[j, i] = 2.5  # an old obstacle gone, among new ones
    with dymu.Engine() as eng:
        m = Maps(eng, F0, ld=NX + 7)
        try:
            m.clearance(C1)
            S0, _ = m.get(m.dS)
            m.put(m.dF, F)
            with pytest.raises(dymu.DymuError) as e:
                update(m, C1, WINDOW)
            assert e.value.status == -7
            S1, S_pad = m.get(m.dS)
            assert np.array_equal(bits(S0), bits(S1)) and (S_pad == SENT).all()
            st = update(m, C1, (96, 60, 1, 1))  # a window without it: not seen
            assert st["passes"] > 0
        finally:
            m.close()


# ---- 3. arguments ----
def test_bad_arguments_touch_nothing(dymu, fields):
    F0, _, F1, _ = fields
    with dymu.Engine() as eng:
        m = Maps(eng, F1)
        call = eng._lib.dymu_clearance_update_device
        box = (4 * np.ones(4, dtype=np.uint32))
        try:
            good = dict(ctx=eng.ctx, dF=m.dF, dW=m.dW, dS=m.dS, nx=NX, ny=NY, ld=NX, c=C1, i0=0,
                        j0=0, w=NX, h=NY)
            bad = [dict(ctx=None), dict(dF=None), dict(dW=None), dict(dS=None), dict(nx=0),
                   dict(ny=0), dict(ld=NX - 1), dict(c=0.0), dict(c=-1.0), dict(c=np.nan),
                   dict(c=INF), dict(w=0), dict(h=0), dict(i0=NX), dict(j0=NY)]
            import ctypes
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
                update(m, C1, WINDOW)
            assert e.value.status == -7
            S, _ = m.get(m.dS)
            assert (S == SENT).all()
            eng.set_stepping(False)
            m.put(m.dF, F0)
            m.clearance(C1)  # and the context still works, box and stats being optional
            m.put(m.dF, F1)
            assert call(eng.ctx, m.dF, m.dW, m.dS, NX, NY, NX, C1, 0, 0, NX, NY, None, None,
                        None) == 0
            S, _ = m.get(m.dS)
            assert (S[~(F1 < INF)] == 0.0).all()
        finally:
            m.close()


# ---- 4. locality ----
def test_update_stays_local(dymu, oracle):
    """The 512x64 wall map, c = 1/8: the level lies 8 cells from an obstacle.  A 2x2 block at
    column 300 lies where the old solve never came (+inf).  Cells further than the level's
    reach from the block keep their old value or end above the level, so only the 16-cell
    tiles that meet the block grown by 8 cells hold a key at or below the level; a tile is
    claimed when a visit of a neighbour changes their shared edge, which adds at most one
    ring of tiles around those.  The update visits tiles in key order (a per-pass target of
    one tile) and checks after every pass here, so no tile beyond those is visited."""
    F0, _ = wall_map()
    F1 = F0.copy()
    bi, bj = 300, 30
    F1[bj:bj + 2, bi:bi + 2] = INF
    S1_ref = ref.fmm_seeds(oracle, np.full(F1.shape, 0.125), obstacle_seeds(F1))
    with dymu.Engine(passes_per_check=1) as eng:
        m = Maps(eng, F0)
        try:
            m.clearance(0.125)
            S0, _ = m.get(m.dS)
            m.put(m.dF, F1)
            st = update(m, 0.125, (bi, bj, 2, 2))
            S1, _ = m.get(m.dS)
            fresh = m.clearance(0.125)  # the alternative: the new mask solved afresh
        finally:
            m.close()
    print(f"kernel {st['kernel']}: update {st['passes']} passes, {st['tile_visits']} tile visits, "
          f"box {st['box']}; fresh solve {fresh['passes']} passes, {fresh['tile_visits']} visits")
    check_field(S1, S1_ref, F1)
    check_box(S0, S1, st["box"])
    assert st["tile_w"] == 16
    reach, tile = 8, 16
    lo_i = (bi - reach) // tile * tile - tile
    hi_i = ((bi + 2 + reach - 1) // tile + 1) * tile + tile
    lo_j = max((bj - reach) // tile * tile - tile, 0)
    hi_j = min(((bj + 2 + reach - 1) // tile + 1) * tile + tile, 64)
    i0, j0, w, h = st["box"]
    assert lo_i <= i0 and i0 + w <= hi_i and lo_j <= j0 and j0 + h <= hi_j
    assert st["tile_visits"] < fresh["tile_visits"]


# ---- 5. determinism ----
def test_deterministic_runs_are_bit_identical(dymu, fields):
    F0, _, F1, S1_ref = fields
    out = []
    for _ in range(2):
        with dymu.Engine(deterministic=1) as eng:
            m = Maps(eng, F0, ld=NX + 7)
            try:
                m.clearance(C1)
                m.put(m.dF, F1)
                st = update(m, C1, WINDOW)
                out.append((m.get(m.dS)[0], st["box"]))
            finally:
                m.close()
        assert st["kernel"] == 5
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and out[0][1] == out[1][1]
    check_field(out[0][0], S1_ref, F1)
