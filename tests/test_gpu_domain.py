"""The row-slab domain step, called directly (include/dymu_fim.h, "row-slab domains"):
dom_begin, dom_merge_ghosts, dom_exchange, dom_round and dom_round_peer on one engine, against
tests/slab_ref.py.  Ghost rows and the queued-tile counts the sharded loops terminate on are
compared bit for bit / as exact integers; converged owned rows against the oracle FMM at the
project's parity bound.

Every T buffer has nrows + 4 rows of pitch ld: a guard row, the ghost-lo slot, the owned
rows, the ghost-hi slot, a guard row.  The guards, the padding columns nx .. ld-1 of every
row and the ghost slot of a side without a ghost hold a sentinel bit pattern that no call
may change.  Every test runs at ld = nx and at ld = nx + 7.
"""
import numpy as np
import pytest

import slab_ref as ref
from test_gpu_solver import assert_parity

pytestmark = pytest.mark.gpu

SENT = np.uint64(0x7FF8C0DEC0DEC0DE)  # a quiet NaN with a payload no computation produces
KERNELS = {"fim": dict(kernel=3), "prio": dict(kernel=4, prio_target=32),
           "prio16": dict(kernel=5, prio_target=8)}
PADS = (0, 7)
NXS = (5, 100, 300)
SHAPES = ((16, True, True), (48, True, True), (19, True, False))  # nrows, ghost_lo, ghost_hi
ERR_ARG, ERR_STATE = -1, -7

kernels = pytest.mark.parametrize("kname", sorted(KERNELS))
pads = pytest.mark.parametrize("pad", PADS, ids=["tight", "pitched"])


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Slab:
    """Device buffers of one slab domain and their host mirror."""

    def __init__(self, eng, nx, nrows, lo, hi, pad, F=None):
        self.eng, self.nx, self.nrows, self.lo, self.hi = eng, nx, nrows, lo, hi
        self.ld = ld = nx + pad
        self.rows = nrows + 4
        Fh = np.full((nrows, ld), SENT, dtype=np.uint64)
        Fh[:, :nx] = u64(np.ones((nrows, nx)) if F is None else F)
        self.dF = eng.alloc(8 * nrows * ld)
        self.dT = eng.alloc(8 * self.rows * ld)
        self.stage = eng.alloc(16 * nx + 64)  # two received rows and an int32 count
        self.d_count = self.stage + 16 * nx
        eng.h2d(self.dF, Fh)
        self.T0 = self.dT + 8 * 2 * ld  # the first owned row
        self.poison = np.zeros((self.rows, ld), dtype=bool)
        self.poison[0] = self.poison[-1] = True
        self.poison[:, nx:] = True
        if not lo:
            self.poison[1] = True
        if not hi:
            self.poison[-2] = True

    def begin(self, goal=None):
        self.eng.h2d(self.dT, np.full((self.rows, self.ld), SENT, dtype=np.uint64))
        gi, gj = goal if goal is not None else (0, -1)
        self.eng.dom_begin(self.dF, self.T0, self.nx, self.nrows, self.ld, self.lo, self.hi, gi, gj)

    def read(self):
        """the whole buffer as uint64 [rows, ld], the sentinel checked"""
        buf = np.empty((self.rows, self.ld), dtype=np.uint64)
        self.eng.d2h(buf, self.dT)
        bad = np.argwhere(self.poison & (buf != SENT))
        assert len(bad) == 0, f"guard / padding / unflagged ghost cells written at {bad[:5]}"
        return buf

    def owned(self, buf):
        return buf[2:2 + self.nrows, :self.nx]

    def ghost(self, buf, side):
        """a flagged ghost row as float64, None for a side without one"""
        if not (self.hi if side else self.lo):
            return None
        return buf[self.nrows + 2 if side else 1, :self.nx].view(np.float64).copy()

    def set_ghost(self, side, row):
        r = self.nrows + 2 if side else 1
        self.eng.h2d(self.dT + 8 * r * self.ld, np.ascontiguousarray(row, dtype=np.float64))

    def send(self, lo_row, hi_row):
        """upload received rows; the device pointers (0 for None)"""
        p = [0, 0]
        for side, row in enumerate((lo_row, hi_row)):
            if row is not None:
                p[side] = self.stage + 8 * self.nx * side
                self.eng.h2d(p[side], np.ascontiguousarray(row, dtype=np.float64))
        return p

    def count(self, poison=-77):
        out = np.empty(1, dtype=np.int32)
        self.eng.d2h(out, self.d_count)
        self.eng.h2d(self.d_count, np.array([poison], dtype=np.int32))
        return int(out[0])

    def free(self):
        for p in (self.dF, self.dT, self.stage):
            self.eng.free(p)


def deliver(eng, sl, path, lo_row, hi_row):
    """received rows through one of the paths under test; the count it reports, or None"""
    p = sl.send(lo_row, hi_row)
    sl.count()  # poison the count word
    if path == "merge":
        eng.dom_merge_ghosts(p[0], p[1], sl.d_count)
    elif path == "exchange":
        eng.dom_exchange(p[0], p[1], sl.d_count)
    else:
        eng.dom_round(2, p[0], p[1], sl.d_count)
    return sl.count()


def same_bits(a, b):
    return (a is None and b is None) or np.array_equal(u64(a), u64(b))


def shapes():
    for nx in NXS:
        for nrows, lo, hi in SHAPES:
            yield nx, nrows, lo, hi


# ---------------------------------------------------------------------------
@kernels
@pads
def test_begin_state(dymu, kname, pad):
    eng = dymu.Engine(**KERNELS[kname])
    inf_bits = u64(np.array([np.inf]))[0]
    try:
        for nx, nrows, lo, hi in shapes():
            sl = Slab(eng, nx, nrows, lo, hi, pad)
            for goal in (None, (nx - 1, nrows - 1), (0, 0)):
                sl.begin(goal)
                assert eng.dom_pending() == (0 if goal is None else 1)
                buf = sl.read()
                want = np.full((nrows, nx), inf_bits, dtype=np.uint64)
                if goal is not None:
                    want[goal[1], goal[0]] = 0  # the bits of 0.0
                assert np.array_equal(sl.owned(buf), want)
                for side in (0, 1):
                    g = sl.ghost(buf, side)
                    assert g is None or (u64(g) == inf_bits).all()
            eng.dom_finish()
            sl.free()
    finally:
        eng.close()


def merge_sequence(eng, sl, tw, variant, path):
    """The constructed rows through `path` on a goal-less domain: first merge, the same rows
    again, lower values in queued tiles, then quiet rows.  Exact ghosts and counts each time."""
    nx, nrows, hi = sl.nx, sl.nrows, sl.hi
    nty = -(-nrows // tw)
    old_lo, new_lo = ref.constructed_rows(nx, tw, variant)
    old_hi, new_hi = ref.constructed_rows(nx, tw, variant + 3) if hi else (None, None)
    sl.begin()
    sl.set_ghost(0, old_lo)
    if hi:
        sl.set_ghost(1, old_hi)
    before = sl.read()
    queued = set()
    g_lo, g_hi = old_lo, old_hi
    steps = [("first", lambda: (new_lo, new_hi)),
             ("again", lambda: (new_lo, new_hi)),
             ("lower", lambda: (ref.lower_rows(g_lo, ref.tile_cols(queued, 0, nx, tw)),
                                ref.lower_rows(g_hi, ref.tile_cols(queued, nty - 1, nx, tw))
                                if hi else None)),
             ("quiet", lambda: (ref.quiet_rows(g_lo), ref.quiet_rows(g_hi) if hi else None))]
    for what, rows in steps:
        r_lo, r_hi = rows()
        w_lo, w_hi, q = ref.merge_ref(g_lo, g_hi, r_lo, r_hi, nx, nrows, tw, tw)
        n_before = len(queued)
        queued |= q
        if what == "first":
            assert q
        else:
            assert len(queued) == n_before  # nothing new: the count must not move
        got = deliver(eng, sl, path, r_lo, r_hi)
        where = (what, path, nx, nrows, variant)
        assert got == len(queued), where
        assert eng.dom_pending() == len(queued), where
        buf = sl.read()
        assert same_bits(sl.ghost(buf, 0), w_lo), where
        assert same_bits(sl.ghost(buf, 1), w_hi), where
        assert np.array_equal(sl.owned(buf), sl.owned(before)), where
        if what == "lower":
            assert not same_bits(w_lo, g_lo)
        g_lo, g_hi = w_lo, w_hi


def null_sides(eng, sl, tw, variant, path):
    """A NULL side leaves that ghost row alone and queues nothing for it."""
    nx, nrows = sl.nx, sl.nrows
    old_lo, new_lo = ref.constructed_rows(nx, tw, variant)
    old_hi, new_hi = ref.constructed_rows(nx, tw, variant + 3)
    sl.begin()
    sl.set_ghost(0, old_lo)
    sl.set_ghost(1, old_hi)
    w_lo, _, q_lo = ref.merge_ref(old_lo, old_hi, new_lo, None, nx, nrows, tw, tw)
    assert deliver(eng, sl, path, new_lo, None) == len(q_lo)
    buf = sl.read()
    assert same_bits(sl.ghost(buf, 0), w_lo) and same_bits(sl.ghost(buf, 1), old_hi)
    _, w_hi, q_hi = ref.merge_ref(w_lo, old_hi, None, new_hi, nx, nrows, tw, tw)
    assert deliver(eng, sl, path, None, new_hi) == len(q_lo | q_hi)
    assert eng.dom_pending() == len(q_lo | q_hi)
    buf = sl.read()
    assert same_bits(sl.ghost(buf, 0), w_lo) and same_bits(sl.ghost(buf, 1), w_hi)
    if path == "merge":  # no row at all: only the count
        eng.dom_merge_ghosts(0, 0, sl.d_count)
        assert sl.count() == len(q_lo | q_hi)


@kernels
@pads
def test_merge_ghosts_exact(dymu, kname, pad):
    eng = dymu.Engine(**KERNELS[kname])
    tw = ref.tile_size(KERNELS[kname]["kernel"])
    try:
        for nx, nrows, lo, hi in shapes():
            sl = Slab(eng, nx, nrows, lo, hi, pad)
            for variant in range(ref.NVARIANTS):
                merge_sequence(eng, sl, tw, variant, "merge")
            if hi:
                null_sides(eng, sl, tw, 1, "merge")
            eng.dom_finish()
            sl.free()
    finally:
        eng.close()


@kernels
@pads
def test_exchange_equals_merge(dymu, kname, pad):
    """dom_exchange: the same ghosts, and *d_total right on every one of several calls in a
    row (the count word is poisoned between them: a ticket that did not reset would leave
    it unwritten).  nx = 300 runs two blocks."""
    eng = dymu.Engine(**KERNELS[kname])
    tw = ref.tile_size(KERNELS[kname]["kernel"])
    try:
        for nx, nrows, lo, hi in shapes():
            sl = Slab(eng, nx, nrows, lo, hi, pad)
            for variant in range(ref.NVARIANTS):
                merge_sequence(eng, sl, tw, variant, "exchange")
            if hi:
                null_sides(eng, sl, tw, 2, "exchange")
            eng.dom_finish()
            sl.free()
    finally:
        eng.close()


@pytest.mark.parametrize("grid_blocks", [1, 3, 0])
@pads
def test_round_merge_exact(dymu, grid_blocks, pad):
    """The in-pass merge of dom_round (kernel 5) at one workgroup, at more workgroups than
    most widths have column groups, and at the default grid: after a round of 2 passes on an
    empty list the ghosts are merge_ref's and *d_total = 0 tiles for the first pass + the
    merged tiles for the second; rows that improve nothing give 0 and change no bit."""
    eng = dymu.Engine(kernel=5, prio_target=8, grid_blocks=grid_blocks)
    try:
        for nx, nrows, lo, hi in shapes():
            sl = Slab(eng, nx, nrows, lo, hi, pad)
            assert eng.dom_round_capable(nx, nrows, 2) == 1
            assert eng.dom_round_capable(nx, nrows, 1) == 0
            for variant in range(ref.NVARIANTS):
                old_lo, new_lo = ref.constructed_rows(nx, 16, variant)
                old_hi, new_hi = ref.constructed_rows(nx, 16, variant + 3) if hi else (None, None)
                w_lo, w_hi, q = ref.merge_ref(old_lo, old_hi, new_lo, new_hi, nx, nrows, 16, 16)
                # rows that improve nothing: the fixed-point signal, and no bit changes
                sl.begin()
                assert eng.dom_round_supported(2) == 1 and eng.dom_round_supported(1) == 0
                sl.set_ghost(0, old_lo)
                if hi:
                    sl.set_ghost(1, old_hi)
                before = sl.read()
                got = deliver(eng, sl, "round", ref.quiet_rows(old_lo),
                              ref.quiet_rows(old_hi) if hi else None)
                assert got == 0 and eng.dom_pending() == 0, (nx, nrows, variant)
                assert np.array_equal(sl.read(), before), (nx, nrows, variant)
                # the constructed rows (only merges write ghost rows)
                got = deliver(eng, sl, "round", new_lo, new_hi)
                assert got == len(q), (nx, nrows, variant)
                buf = sl.read()
                assert same_bits(sl.ghost(buf, 0), w_lo), (nx, nrows, variant)
                assert same_bits(sl.ghost(buf, 1), w_hi), (nx, nrows, variant)
            eng.dom_finish()
            sl.free()
    finally:
        eng.close()


# ---------------------------------------------------------------------------
def run_to_fixed_point(eng, sl, tw, K=8):
    """dom_run until nothing is queued, within the domain's own pass cap"""
    cap = 4 * (-(-sl.nx // tw)) * (-(-sl.nrows // tw)) + 1024
    passes = 0
    while eng.dom_pending() != 0:
        assert passes + K <= cap, f"not converged within {cap} passes"
        eng.dom_run(K)
        passes += K
    return passes


DIRICHLET = [(k, p) for k in sorted(KERNELS) for p in ("merge", "exchange")] + [("prio16", "round")]


@pytest.mark.parametrize("kname,path", DIRICHLET, ids=[f"{k}-{p}" for k, p in DIRICHLET])
@pads
def test_dirichlet_slab(dymu, oracle, kname, path, pad):
    """A slab alone with the FMM's neighbour rows delivered once converges to the FMM's owned
    rows (tests/test_slab_ref.py shows the reference fixed point is exactly those rows)."""
    eng = dymu.Engine(**KERNELS[kname])
    tw = ref.tile_size(KERNELS[kname]["kernel"])
    try:
        for name in sorted(ref.CASES):
            F, Tref, goal, r0, nrows = ref.case(oracle, name)
            ny, nx = F.shape
            lo, hi = r0 > 0, r0 + nrows < ny
            sl = Slab(eng, nx, nrows, lo, hi, pad, F=F[r0:r0 + nrows])
            inside = r0 <= goal[1] < r0 + nrows
            sl.begin((goal[0], goal[1] - r0) if inside else None)
            row_lo = Tref[r0 - 1] if lo else None
            row_hi = Tref[r0 + nrows] if hi else None
            deliver(eng, sl, path, row_lo, row_hi)
            run_to_fixed_point(eng, sl, tw)
            buf = sl.read()
            assert_parity(sl.owned(buf).view(np.float64), Tref[r0:r0 + nrows])
            # passes never write ghost rows: still the delivered rows (+inf stayed +inf)
            assert same_bits(sl.ghost(buf, 0), row_lo), name
            assert same_bits(sl.ghost(buf, 1), row_hi), name
            eng.dom_finish()
            sl.free()
    finally:
        eng.close()


# ---------------------------------------------------------------------------
class Peer:
    """The buffers of dymu_peer_links on one engine: receive rows and tags written by the
    host, send rows / last rows / send tags plain device buffers, ctl as dymu_dist.cpp
    starts it (zeros, the two rmin words all ones)."""

    def __init__(self, dymu, eng, nx):
        self.eng, self.nx = eng, nx
        self.rows = eng.alloc(8 * 6 * nx)   # recv[2], send[2], last[2]
        self.tags = eng.alloc(8 * 4)        # recv_tag[2], send_tag[2]
        self.ctl = eng.alloc(dymu.PEER_CTL_BYTES)
        eng.h2d(self.rows, np.full(6 * nx, np.inf))
        eng.h2d(self.tags, np.zeros(4, dtype=np.uint64))
        ctl = np.zeros(dymu.PEER_CTL_BYTES, dtype=np.uint8)
        off, n = dymu.PEER_CTL_RMIN
        ctl[off:off + n] = 0xFF
        eng.h2d(self.ctl, ctl)
        L = dymu.DymuPeerLinks()
        for s in range(2):
            L.recv[s] = self.rows + 8 * nx * s
            L.send[s] = self.rows + 8 * nx * (2 + s)
            L.last[s] = self.rows + 8 * nx * (4 + s)
            L.recv_tag[s] = self.tags + 8 * s
            L.send_tag[s] = self.tags + 8 * (2 + s)
        L.ctl = self.ctl
        self.links = L

    def receive(self, side, row):
        self.eng.h2d(self.rows + 8 * self.nx * side, np.ascontiguousarray(row, dtype=np.float64))
        self.eng.h2d(self.tags + 8 * side, np.array([1], dtype=np.uint64))

    def state(self):
        rows = np.empty((6, self.nx))
        tags = np.empty(4, dtype=np.uint64)
        self.eng.d2h(rows, self.rows)
        self.eng.d2h(tags, self.tags)
        return rows, tags

    def free(self):
        for p in (self.rows, self.tags, self.ctl):
            self.eng.free(p)


@pytest.mark.parametrize("walled", [False, True], ids=["open", "walled"])
def test_peer_round_push(dymu, oracle, walled):
    """dom_round_peer on one engine at ld = nx + 7: the tagged merge gives merge_ref's ghosts,
    the push leaves the first / last owned row in send and last (+inf never pushed), a tag
    counts pushes that carried a decrease -- 0 for a boundary row of obstacles only."""
    F, Tref, goal, r0, nrows = ref.walled_case(oracle) if walled else ref.case(oracle, "mid")
    nx = F.shape[1]
    eng = dymu.Engine(kernel=5, prio_target=8)
    try:
        sl = Slab(eng, nx, nrows, True, True, 7, F=F[r0:r0 + nrows])
        pr = Peer(dymu, eng, nx)
        sl.begin(None)
        pr.receive(0, Tref[r0 - 1])
        pr.receive(1, Tref[r0 + nrows])
        cap = 4 * (-(-nx // 16)) * (-(-nrows // 16)) + 1024
        prev, passes = None, 0
        while True:
            assert passes + 2 <= cap, f"not converged within {cap} passes"
            eng.dom_round_peer(2, pr.links)
            passes += 2
            rows, tags = pr.state()
            cur = (eng.dom_pending(), u64(rows[2:4]).tolist(), tags[2:].tolist())
            if prev is not None:
                assert tags[2] >= prev[2][0] and tags[3] >= prev[2][1]  # tags never decrease
                if prev[0] == 0 and cur == prev:
                    break
            prev = cur
        buf = sl.read()
        inf_row = np.full(nx, np.inf)
        w_lo, w_hi, _ = ref.merge_ref(inf_row, inf_row, Tref[r0 - 1], Tref[r0 + nrows], nx, nrows,
                                      16, 16)
        assert same_bits(sl.ghost(buf, 0), w_lo) and same_bits(sl.ghost(buf, 1), w_hi)
        own = sl.owned(buf)
        assert_parity(own.view(np.float64), Tref[r0:r0 + nrows])
        for s, r in ((0, 0), (1, nrows - 1)):
            assert np.array_equal(u64(rows[2 + s]), own[r]), f"send[{s}]"
            assert np.array_equal(u64(rows[4 + s]), own[r]), f"last[{s}]"
            if np.isfinite(own[r].view(np.float64)).any():
                assert tags[2 + s] >= 1
            else:
                assert tags[2 + s] == 0
        assert np.isfinite(own[0].view(np.float64)).any()
        assert np.isfinite(own[-1].view(np.float64)).any() != walled
        assert np.array_equal(u64(rows[0]), u64(Tref[r0 - 1]))  # receive rows are read only
        assert np.array_equal(u64(rows[1]), u64(Tref[r0 + nrows]))
        assert tags[0] == 1 and tags[1] == 1
        eng.dom_finish()
        pr.free()
        sl.free()
    finally:
        eng.close()


# ---------------------------------------------------------------------------
def test_domain_errors(dymu, oracle):
    """DYMU_ERR_STATE / DYMU_ERR_ARG of the dom_* family; after every rejected call the
    engine still solves a small map correctly."""
    Fs = oracle.synth_speed(41, 33, seed=3, obst_frac=0.05, obst_seed=7, goal=(20, 16))
    Ts, _ = oracle.fmm(Fs, (20, 16))

    def rejected(eng, status, fn, *args):
        with pytest.raises(dymu.DymuError) as e:
            fn(*args)
        assert e.value.status == status, (fn.__name__, e.value.status)
        assert_parity(eng.solve(Fs, 20, 16).T, Ts)

    engines = []
    try:
        for kname in sorted(KERNELS):
            eng = dymu.Engine(**KERNELS[kname])
            engines.append(eng)
            k5 = kname == "prio16"
            sl = Slab(eng, 100, 16, True, False, 7)
            row = sl.send(np.ones(100), np.ones(100))
            # before any dom_begin (no solve in between), then again without a live domain
            early = ((eng.dom_run, (1,)), (eng.dom_merge_ghosts, (row[0], 0, sl.d_count)),
                     (eng.dom_exchange, (row[0], 0, sl.d_count)),
                     (eng.dom_round, (2, row[0], 0, sl.d_count)),
                     (eng.dom_pending, ()), (eng.dom_finish, ()))
            for fn, args in early:
                assert eng.dom_round_supported(2) == 0
                with pytest.raises(dymu.DymuError) as e:
                    fn(*args)
                assert e.value.status == ERR_STATE, fn.__name__
            for fn, args in early:
                rejected(eng, ERR_STATE, fn, *args)
            # a row for a side without a ghost, a NULL count
            calls = [(eng.dom_merge_ghosts, (0, row[1], sl.d_count)),
                     (eng.dom_merge_ghosts, (row[0], row[1], 0)),
                     (eng.dom_exchange, (0, row[1], sl.d_count)),
                     (eng.dom_exchange, (row[0], 0, 0))]
            if k5:
                calls += [(eng.dom_round, (2, 0, row[1], sl.d_count)),
                          (eng.dom_round, (2, row[0], 0, 0))]
            for fn, args in calls:
                sl.begin()
                rejected(eng, ERR_ARG, fn, *args)
            sl2 = Slab(eng, 100, 16, False, True, 0)
            sl2.begin()
            rejected(eng, ERR_ARG, eng.dom_merge_ghosts, row[0], 0, sl.d_count)
            # fused rounds: kernel 5, passes >= 2
            sl.begin()
            assert eng.dom_round_supported(2) == (1 if k5 else 0)
            assert eng.dom_round_supported(1) == 0
            assert eng.dom_round_capable(100, 16, 2) == (1 if k5 else 0)
            rejected(eng, ERR_STATE, eng.dom_round, 1, row[0], 0, sl.d_count)
            if not k5:
                sl.begin()
                rejected(eng, ERR_STATE, eng.dom_round, 2, row[0], 0, sl.d_count)
            # dom_begin: hi ghost with a ragged last tile row, ld < nx, goal column off the grid
            rejected(eng, ERR_ARG, eng.dom_begin, sl.dF, sl.T0, 100, 19, 107, True, True, 0, -1)
            rejected(eng, ERR_ARG, eng.dom_begin, sl.dF, sl.T0, 100, 16, 99, True, False, 0, -1)
            rejected(eng, ERR_ARG, eng.dom_begin, sl.dF, sl.T0, 100, 16, 107, True, False, 100, 3)
            sl.read()  # no rejected call wrote outside the domain
            sl.free()
            sl2.free()
        # deterministic engines run kernel 5 but not fused rounds
        eng = dymu.Engine(kernel=5, prio_target=8, deterministic=1)
        engines.append(eng)
        sl = Slab(eng, 100, 16, True, False, 7)
        row = sl.send(np.ones(100), None)
        sl.begin()
        assert eng.dom_round_supported(2) == 0 and eng.dom_round_capable(100, 16, 2) == 0
        rejected(eng, ERR_STATE, eng.dom_round, 2, row[0], 0, sl.d_count)
        sl.free()
    finally:
        for eng in engines:
            eng.close()
