"""Obstacle clearance field and risk-inflated speed.

dymu_clearance_device is, by definition, dymu_solve_seeds_device on a constant map with
one seed at 0 per obstacle cell, stopped at the level 1.  The yardstick is
goalset_ref.fmm_seeds on np.full(shape, c) with those seeds, S_ref: where S_ref <= 1 the
field is within the project's parity bound 1e-12 * max(1, S_ref) = 1e-12 of it; every
other cell holds an upper bound (S >= S_ref * (1 - 1e-12)) or +inf; an obstacle cell holds
+0.0 exactly.  dymu_inflate_speed_device is the numpy expression bit for bit.  Every map
is uploaded with sentinel padding columns, which no call may touch.
"""
import numpy as np
import pytest

import goalset_ref as ref

pytestmark = pytest.mark.gpu

KERNELS = {4: dict(kernel=4, prio_target=64), 5: dict(kernel=5, prio_target=16)}
SENT = -7.25  # in the padding columns nx .. ld-1 and in output maps before a call
INF = np.inf


class Maps:
    """F uploaded at pitch ld, with a work map and an output map of the same shape."""

    def __init__(self, eng, F, ld=None, S0=None):
        self.eng = eng
        self.ny, self.nx = F.shape
        self.ld = ld or self.nx
        self.dF, self.dW, self.dS = (eng.alloc(8 * self.ld * self.ny) for _ in range(3))
        self.put(self.dF, F)
        self.put(self.dW, np.full(F.shape, SENT))
        self.put(self.dS, np.full(F.shape, SENT) if S0 is None else S0)

    def put(self, ptr, a):
        h = np.full((self.ny, self.ld), SENT)
        h[:, :self.nx] = a
        self.eng.h2d(ptr, h)

    def get(self, ptr):
        """(the map, its padding columns)"""
        h = np.empty((self.ny, self.ld))
        self.eng.d2h(h, ptr)
        return h[:, :self.nx].copy(), h[:, self.nx:].copy()

    def clearance(self, c):
        return self.eng.clearance_device(self.dF, self.dW, self.dS, self.nx, self.ny, self.ld, c)

    def close(self):
        for p in (self.dF, self.dW, self.dS):
            self.eng.free(p)


def obstacle_seeds(F):
    return [(int(i), int(j), 0.0) for j, i in np.argwhere(~(F < INF))]


def check_field(S, S_ref, F):
    """The contract of dymu_clearance_device against the converged reference."""
    obst = ~(F < INF)
    assert np.array_equal(S[obst].view(np.uint64), np.zeros(obst.sum(), dtype=np.uint64))
    assert not np.isnan(S).any()
    near = S_ref <= 1.0
    err = np.abs(S[near] - S_ref[near]).max() if near.any() else 0.0
    far = ~near & np.isfinite(S)
    low = (S[far] / S_ref[far]).min() if far.any() else INF
    print(f"{near.sum()} cells at or below the level: max |dS| = {err:.3e}; {far.sum()} finite "
          f"cells above it, min S / S_ref = {low:.15f}")
    assert err <= 1e-12
    assert (S[~near] >= S_ref[~near] * (1.0 - 1e-12)).all()


# ---- 1. parity ----
NX, NY = 97, 61
C1 = 1.0 / 6.5
HAND = [(0, 0), (96, 60), (15, 20), (16, 20), (31, 15), (32, 16)]  # tile corners, edge columns
NAN_CELL = (50, 33)


@pytest.fixture(scope="module")
def field(oracle):
    """97x61, 2 % obstacles plus hand-placed ones on tile corners and on both edge columns
    of 8- and 16-cell tiles, one of them a NaN; the reference field, computed once."""
    F = oracle.synth_speed(NX, NY, seed=41, obst_frac=0.02, obst_seed=9, goal=(70, 40))
    for i, j in HAND:
        F[j, i] = INF
    F[NAN_CELL[1], NAN_CELL[0]] = np.nan
    S_ref = ref.fmm_seeds(oracle, np.full(F.shape, C1), obstacle_seeds(F))
    assert (S_ref <= 1.0).any() and (S_ref > 1.0).any()
    S_ref.setflags(write=False)
    F.setflags(write=False)
    return F, S_ref


@pytest.mark.parametrize("pad", [0, 7])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_parity(dymu, field, kernel, pad):
    F, S_ref = field
    with dymu.Engine(**KERNELS[kernel]) as eng:
        m = Maps(eng, F, ld=NX + pad)
        try:
            st = m.clearance(C1)
            S, S_pad = m.get(m.dS)
            F_after, _ = m.get(m.dF)
            _, W_pad = m.get(m.dW)
        finally:
            m.close()
    assert st["kernel"] == kernel and st["passes"] > 0
    assert np.array_equal(F_after.view(np.uint64), F.view(np.uint64))  # read only
    assert (S_pad == SENT).all() and (W_pad == SENT).all()
    check_field(S, S_ref, F)


# ---- 2. the stop at the level ----
def wall_map():
    F = np.full((64, 512), 2.0)
    F[:, 0] = INF
    return F, np.broadcast_to(np.arange(512) / 8.0, (64, 512))


def test_stops_at_the_level(dymu):
    """Obstacles in column 0 of 512x64, c = 1/8: the field is i / 8, the level lies at
    column 8.  Column 511 is 31 tiles of 16 cells from the seeds and a value travels at most
    one tile per pass, so a solve that stops at the level never reaches it."""
    F, S_ref = wall_map()
    with dymu.Engine(passes_per_check=1) as eng:
        m = Maps(eng, F)
        try:
            st = m.clearance(0.125)
            S, _ = m.get(m.dS)
        finally:
            m.close()
    print(f"kernel {st['kernel']}: {st['passes']} passes, {st['tile_visits']} tile visits")
    assert st["tile_w"] == 16
    assert st["passes"] < 31
    assert np.isposinf(S[:, 511]).all()
    assert np.abs(S[:, :9] - S_ref[:, :9]).max() <= 1e-12
    check_field(S, S_ref, F)


def test_default_cadence_meets_the_contract(dymu):
    F, S_ref = wall_map()
    with dymu.Engine() as eng:
        m = Maps(eng, F)
        try:
            st = m.clearance(0.125)
            S, _ = m.get(m.dS)
        finally:
            m.close()
    print(f"kernel {st['kernel']}: {st['passes']} passes")
    assert np.abs(S[:, :9] - S_ref[:, :9]).max() <= 1e-12
    check_field(S, S_ref, F)


# ---- 3. edges ----
def test_no_obstacle(dymu):
    F = np.full((64, 80), 3.0)
    with dymu.Engine() as eng:
        m = Maps(eng, F)
        try:
            st = m.clearance(0.25)
            S, _ = m.get(m.dS)
        finally:
            m.close()
    assert st["passes"] == 0
    assert np.isposinf(S).all()


def test_all_obstacles(dymu):
    F = np.full((64, 80), INF)
    F[::3, ::5] = np.nan
    with dymu.Engine() as eng:
        m = Maps(eng, F)
        try:
            m.clearance(0.25)
            S, _ = m.get(m.dS)
        finally:
            m.close()
    assert np.array_equal(S.view(np.uint64), np.zeros(S.shape, dtype=np.uint64))


def test_bad_arguments_touch_nothing(dymu, field):
    F, _ = field
    with dymu.Engine() as eng:
        m = Maps(eng, F)
        call = eng._lib.dymu_clearance_device
        try:
            good = dict(ctx=eng.ctx, dF=m.dF, dW=m.dW, dS=m.dS, nx=NX, ny=NY, ld=NX, c=C1)
            bad = [dict(ctx=None), dict(dF=None), dict(dW=None), dict(dS=None), dict(nx=0),
                   dict(ny=0), dict(ld=NX - 1), dict(c=0.0), dict(c=-1.0), dict(c=np.nan),
                   dict(c=INF)]
            for b in bad:
                a = {**good, **b}
                rc = call(a["ctx"], a["dF"], a["dW"], a["dS"], a["nx"], a["ny"], a["ld"], a["c"],
                          None, None)
                assert rc == -1, b
            S, _ = m.get(m.dS)
            W, _ = m.get(m.dW)
            assert (S == SENT).all() and (W == SENT).all()
            eng.set_stepping(True)
            with pytest.raises(dymu.DymuError) as e:
                m.clearance(C1)
            assert e.value.status == -7
            S, _ = m.get(m.dS)
            assert (S == SENT).all()
            eng.set_stepping(False)
            m.clearance(C1)  # and the context still works
            S, _ = m.get(m.dS)
            assert (S[~(F < INF)] == 0.0).all()
        finally:
            m.close()


def test_deterministic_runs_are_bit_identical(dymu, field):
    F, S_ref = field
    out = []
    for _ in range(2):
        with dymu.Engine(deterministic=1) as eng:
            m = Maps(eng, F, ld=NX + 7)
            try:
                st = m.clearance(C1)
                out.append(m.get(m.dS)[0])
            finally:
                m.close()
        assert st["kernel"] == 5
    assert np.array_equal(out[0].view(np.uint64), out[1].view(np.uint64))
    check_field(out[0], S_ref, F)


# ---- 4. the inflated speed ----
def inflate_ref(F, S, ratio):
    with np.errstate(invalid="ignore"):
        R = np.fmax(1.0 - S, 0.0)
        return F * (ratio * R + 1.0)


@pytest.mark.parametrize("pad", [0, 7])
def test_inflate_speed(dymu, pad):
    rng = np.random.default_rng(5)
    ny, nx = 37, 301  # more than one 256-lane strip per row, odd sizes
    F = rng.uniform(0.5, 40.0, (ny, nx))
    S = rng.uniform(0.0, 2.0, (ny, nx))
    fv = [1.75, INF, np.nan, 0.0]
    sv = [0.0, 0.3, 1.0, 1.5, INF]
    for a, f in enumerate(fv):  # every special F against every special S
        for b, s in enumerate(sv):
            F[3 + a, 250 + b], S[3 + a, 250 + b] = f, s
    with dymu.Engine() as eng:
        m = Maps(eng, F, ld=nx + pad, S0=S)
        try:
            for ratio in (2.5, 0.0):
                eng.inflate_speed(m.dF, m.dS, m.dW, nx, ny, m.ld, ratio)
                out, out_pad = m.get(m.dW)
                assert np.array_equal(out.view(np.uint64),
                                      inflate_ref(F, S, ratio).view(np.uint64)), ratio
                assert (out_pad == SENT).all()
            assert np.array_equal(out.view(np.uint64), F.view(np.uint64))  # ratio 0: F itself
            eng.inflate_speed(m.dF, m.dS, m.dF, nx, ny, m.ld, 2.5)  # in place
            out, out_pad = m.get(m.dF)
            assert np.array_equal(out.view(np.uint64), inflate_ref(F, S, 2.5).view(np.uint64))
            assert (out_pad == SENT).all()
            far = S > 1.0
            assert np.array_equal(out[far].view(np.uint64), F[far].view(np.uint64))
            call = eng._lib.dymu_inflate_speed_device
            for ratio in (-1.0, np.nan, INF):
                assert call(eng.ctx, m.dF, m.dS, m.dW, nx, ny, m.ld, ratio, None) == -1
            assert call(eng.ctx, m.dF, m.dS, m.dW, nx, ny, nx - 1, 1.0, None) == -1
            assert call(eng.ctx, None, m.dS, m.dW, nx, ny, m.ld, 1.0, None) == -1
        finally:
            m.close()
