"""The references of tests/update_ref.py, pinned on the CPU.

* Every reference equals a slow per-cell loop transcribed clause by clause from
  include/dymu_fim.h ("dynamic update", "windowed updates of seeded maps and of stacks").
  The loops work on the pitched buffers the C-ABI takes (nx, ny, ld), with the padding
  poisoned exactly as tests/test_gpu_stages.py poisons it.  The raise loop is a front that
  starts in the window and follows 4-neighbours, where raise_ref tests every cell in rounds.
* Non-vacuity of the shared cases on the oracle's maps: the oracle map is an exact fixed
  point of the reference update (so raise_ref with the old speed invalidates nothing), no
  cell lies in the raise margin, every reset case but "goal" and "unreached" resets some
  but not all finite cells, the raise cone is a subset of the theta reset, the dominated
  seed is dominated and reset.
* Mutant separation: every listed mutant of a loop differs from the true loop on at least
  one shared case -- a kernel carrying that bug would fail the GPU comparison.
"""
import numpy as np
import pytest

import update_ref as ref
from update_ref import INF, PAD, PAD_F, PAD_T

TILES = (8, 16)
PITCHES = (0, PAD)


@pytest.fixture(scope="module")
def maps(oracle):
    """(nx, ny, goal) -> (old speed, the oracle's converged map of it)."""
    out = {}
    for nx, ny, goal in ref.ALL_SHAPES:
        F0 = ref.base_speed(oracle, nx, ny, goal)
        out[(nx, ny, goal)] = (F0, oracle.fmm(F0, goal)[0])
    return out


def shared_cases(maps):
    for (nx, ny, goal), (F0, T0) in maps.items():
        for name in ref.cases_for(nx, ny):
            F1, win = ref.case(name, F0, goal)
            yield name, nx, ny, goal, T0, F1, win


# ---------------------------------------------------------------------------
# per-cell loops on pitched buffers; `mut` names one deliberate bug
# ---------------------------------------------------------------------------
def nb4(i, j, nx, ny, mut=""):
    """The in-grid 4-neighbours of (i, j)."""
    out = []
    if j > 0 and mut != "drop_S":
        out.append((i, j - 1))
    if i > 0 and mut != "drop_W":
        out.append((i - 1, j))
    if i + 1 < nx and mut != "drop_E":
        out.append((i + 1, j))
    if j + 1 < ny and mut != "drop_N":
        out.append((i, j + 1))
    return out


def theta_loop(Tb, nx, ny, ld, wins, mut=""):
    T = Tb.ravel().tolist()
    st = nx if mut == "nx_for_ld" else ld
    right = ld if mut == "pad_cols" else nx
    th = INF
    for i0, j0, w, h in wins:
        i1, j1 = min(i0 + w, nx), min(j0 + h, ny)  # the clipped window ...
        g = 0 if mut == "no_ring" else 1           # ... grown by one cell on every side ...
        a0, b0 = max(i0 - g, 0), max(j0 - g, 0)    # ... and clipped again
        a1, b1 = min(i1 + g, right), min(j1 + g, ny)
        if mut == "clip_hi":
            a1, b1 = min(i1 + g, nx - 1), min(j1 + g, ny - 1)
        for j in range(b0, b1):
            for i in range(a0, a1):
                th = min(th, T[j * st + i])
    return th


def seed_window_loop(nx, ny, wins, tile, mut=""):
    out = set()
    for i0, j0, w, h in wins:
        i1, j1 = min(i0 + w, nx), min(j0 + h, ny)
        if mut == "unclipped":
            i1, j1 = i0 + w, j0 + h
        for j in range(j0, j1 + (1 if mut == "clip_hi" else 0)):
            for i in range(i0, i1 + (1 if mut == "clip_hi" else 0)):
                out.add((j // tile, i // tile))  # the tiles that meet the clipped window
    return out


def reset_loop(Tb, Fb, nx, ny, ld, wins, tile, goal=None, seeds=None, mut=""):
    """(buffer after, queued tiles, theta, cells reset) of the theta reset."""
    T, F = Tb.ravel().tolist(), Fb.ravel().tolist()
    out = list(T)
    theta = theta_loop(Tb, nx, ny, ld, wins)
    if mut == "tile_other":
        tile = 24 - tile
    exempt = goal if mut != "goal_not_exempt" else None
    tiles, n_reset = set(), 0

    def at_or_above(v):
        return v > theta if mut == "gt" else v >= theta

    def kept(i, j):  # old T < theta, or the goal
        return T[j * ld + i] < theta or (exempt is not None and (i, j) == tuple(exempt))

    if goal is not None or theta < INF:
        for j in range(ny):
            for i in range(nx):
                k = j * ld + i
                if exempt is not None and (i, j) == tuple(exempt):
                    continue  # the goal is not reset
                if not at_or_above(T[k]):
                    continue  # every other cell is not written
                if T[k] < INF:  # cells that already hold +inf are not written either
                    out[k] = INF
                    n_reset += 1
                # queued: a reset cell of finite new speed with a kept in-grid 4-neighbour
                if (mut == "ignore_F" or F[k] < INF) and any(kept(ii, jj)
                                                              for ii, jj in nb4(i, j, nx, ny, mut)):
                    tiles.add((j // tile, i // tile))
    for i, j, t0 in (seeds or []):
        if mut != "no_seed_back":
            out[j * ld + i] = t0 if mut == "seed_overwrite" else min(out[j * ld + i], t0)
        if mut != "no_seed_tile":
            tiles.add((j // tile, i // tile))  # the seed's tile ...
            if mut != "no_seed_across":       # ... and the tile across each tile edge it lies on
                for ii, jj in nb4(i, j, nx, ny):
                    tiles.add((jj // tile, ii // tile))
    return out, tiles, theta, n_reset


def update_of(T, F, nx, ny, ld, i, j, mut=""):
    """The reference update of cell (i, j) from its in-grid 4-neighbours (:531-535)."""
    def at(ii, jj):
        return T[jj * ld + ii] if 0 <= ii < nx and 0 <= jj < ny else INF
    tx = min(at(i - 1, j), at(i + 1, j))
    ty = min(at(i, j - 1), at(i, j + 1))
    c = F[j * ld + i]
    d = tx - ty if tx < INF or ty < INF else INF
    if abs(d) < c and tx < INF and ty < INF:
        return (tx + ty + float(np.sqrt(np.float64(2.0 * (c * c) - d * d)))) / 2
    return min(tx, ty) + c


def raise_loop(Tb, Fb, nx, ny, ld, goal, win, tol=ref.RAISE_TOL, mut=""):
    """(buffer after, invalidated cells) of the raise front: a work list that starts with
    the clipped window's cells and re-examines the 4-neighbours of every cell that goes."""
    T0, F = Tb.ravel().tolist(), Fb.ravel().tolist()
    T = list(T0)
    i0, j0, w, h = win
    work = [(i, j) for j in range(j0, min(j0 + h, ny)) for i in range(i0, min(i0 + w, nx))]
    gone = set()
    while work:
        i, j = work.pop()
        k = j * ld + i
        if (i, j) in gone or not T0[k] < INF or (i, j) == tuple(goal):
            continue  # live cells only: finite T, not the goal
        blocked = not F[k] < INF and mut != "no_obstacle_rule"
        if blocked or update_of(T, F, nx, ny, ld, i, j) > T0[k] * (1.0 + tol):
            gone.add((i, j))
            T[k] = INF
            work.extend(nb4(i, j, nx, ny, mut))
    return T, gone


def cone_seed_loop(Tb, Fb, nx, ny, ld, goal, tile, mut=""):
    T, F = Tb.ravel().tolist(), Fb.ravel().tolist()
    tiles, key = set(), INF
    for j in range(ny):
        for i in range(nx):
            k = j * ld + i
            if T[k] != INF or (not F[k] < INF and mut != "ignore_F"):
                continue
            if (i, j) == tuple(goal) and mut != "goal_not_exempt":
                continue
            m = min([T[jj * ld + ii] for ii, jj in nb4(i, j, nx, ny, mut)], default=INF)
            if m < INF:
                tiles.add((j // tile, i // tile))
                key = min(key, m)
    return tiles, key


def unpitch(buf, nx, ny, ld):
    return np.array(buf).reshape(ny, ld)[:, :nx]


# ---------------------------------------------------------------------------
# the references equal the loops
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pad", PITCHES)
def test_theta_and_reset_equal_the_loops(maps, pad):
    for name, nx, ny, goal, T0, F1, win in shared_cases(maps):
        ld = nx + pad
        Tb, Fb = ref.pitched(T0, ld, PAD_T), ref.pitched(F1, ld, PAD_F)
        assert ref.theta_ref(T0, [win]) == theta_loop(Tb, nx, ny, ld, [win]), name
        for tile in TILES:
            want, tiles, th, n = reset_loop(Tb, Fb, nx, ny, ld, [win], tile, goal=goal)
            got = ref.reset_ref(T0, F1, [win], tile, goal=goal)
            assert np.array_equal(ref.bits(got[0]), ref.bits(unpitch(want, nx, ny, ld))), name
            assert (got[1], got[2], got[3]) == (tiles, th, n), name
            assert np.array_equal(np.array(want).reshape(ny, ld)[:, nx:], Tb[:, nx:])
            assert ref.seed_window_ref([win], nx, ny, tile) == seed_window_loop(nx, ny, [win], tile)


@pytest.fixture(scope="module")
def seeded(oracle, maps):
    import goalset_ref
    nx, ny, goal = ref.SHAPES[0]
    F0 = maps[(nx, ny, goal)][0]
    return F0, goalset_ref.fmm_seeds(oracle, F0, ref.SEEDS_97)


def test_seeded_reset_equals_the_loop(seeded):
    F0, T0 = seeded
    ny, nx = F0.shape
    hit = 0
    for name in ref.SEEDED_CASES:
        F1, win = ref.case(name, F0, ref.SEEDS_97[0][:2])
        for tile in TILES:
            for pad in PITCHES:
                ld = nx + pad
                Tb, Fb = ref.pitched(T0, ld, PAD_T), ref.pitched(F1, ld, PAD_F)
                want, tiles, th, n = reset_loop(Tb, Fb, nx, ny, ld, [win], tile,
                                                seeds=ref.SEEDS_97)
                got = ref.reset_ref(T0, F1, [win], tile, seeds=ref.SEEDS_97)
                assert np.array_equal(ref.bits(got[0]), ref.bits(unpitch(want, nx, ny, ld)))
                assert (got[1], got[2], got[3]) == (tiles, th, n), name
        # the dominated seed: below its t0 in the old map, at its t0 after a reset that covers it
        i, j, t0 = ref.SEEDS_97[1]
        assert T0[j, i] < t0
        if T0[j, i] >= th:
            assert got[0][j, i] == t0
            hit += 1
    assert hit >= 2


def test_stack_reset_plane_by_plane(oracle, seeded):
    import goalset_ref
    F0, _ = seeded
    ny, nx = F0.shape
    Fo, Fn, P = ref.stack_speeds(F0)
    Ts = ref.stacked([goalset_ref.fmm_seeds(oracle, Fo[b * P:b * P + ny],
                                            [s[1:] for s in ref.STACK_SEEDS if s[0] == b])
                      for b in range(3)], ny, P, INF)
    for tile in TILES:
        out, tiles, thetas, n = ref.stack_ref(Ts, Fn, ny, P, ref.STACK_WINS, ref.STACK_SEEDS, tile)
        assert thetas[1] == INF and thetas[0] < INF and thetas[2] < INF
        assert np.array_equal(ref.bits(out[P:2 * P]), ref.bits(Ts[P:2 * P]))  # untouched plane
        total = 0
        for b in range(3):
            w_b = [w[1:] for w in ref.STACK_WINS if w[0] == b]
            s_b = [s[1:] for s in ref.STACK_SEEDS if s[0] == b]
            Tp, Fp = Ts[b * P:b * P + ny], Fn[b * P:b * P + ny]
            want, t_b, th, k = reset_loop(Tp, Fp, nx, ny, nx, w_b, tile, seeds=s_b)
            assert np.array_equal(ref.bits(out[b * P:b * P + ny]), ref.bits(unpitch(want, nx, ny, nx)))
            assert th == thetas[b]
            assert {(ty + b * P // tile, tx) for ty, tx in t_b} <= tiles
            total += k
            assert 0 < k < np.isfinite(Tp).sum() or b == 1
        assert n == total and np.isinf(out[[b * P + ny for b in range(3)]]).all()
        # plane 1 contributes its seed's tile only
        assert {t for t in tiles if P // tile <= t[0] < 2 * P // tile} == {((P + 20) // tile, 20 // tile)}
        dec = ref.stack_ref(Ts, Fn, ny, P, ref.STACK_WINS, ref.STACK_SEEDS, tile, decrease_only=True)
        assert np.array_equal(ref.bits(dec[0]), ref.bits(Ts)) and dec[3] == 0
        assert dec[1] == {(ty + b * P // tile, tx) for b in (0, 2) for ty, tx in
                          seed_window_loop(nx, ny, [w[1:] for w in ref.STACK_WINS if w[0] == b], tile)}


def test_raise_and_cone_equal_the_loops(maps):
    for name, nx, ny, goal, T0, F1, win in shared_cases(maps):
        for pad in PITCHES:
            ld = nx + pad
            Tb, Fb = ref.pitched(T0, ld, PAD_T), ref.pitched(F1, ld, PAD_F)
            want, gone = raise_loop(Tb, Fb, nx, ny, ld, goal, win)
            T1, S, margin = ref.raise_ref(T0, F1, goal)
            assert np.array_equal(ref.bits(T1), ref.bits(unpitch(want, nx, ny, ld))), name
            assert set(zip(*np.nonzero(S)[::-1])) == gone, name
            for tile in TILES:
                assert ref.cone_seed_ref(T1, F1, goal, tile) == cone_seed_loop(
                    ref.pitched(T1, ld, PAD_T), Fb, nx, ny, ld, goal, tile), name


# ---------------------------------------------------------------------------
# what keeps the GPU cases from being vacuous
# ---------------------------------------------------------------------------
def test_oracle_map_is_an_exact_fixed_point(maps):
    for (nx, ny, goal), (F0, T0) in maps.items():
        assert not np.isnan(F0).any() and F0.min() > 0
        live = np.isfinite(T0)
        live[goal[1], goal[0]] = False
        u = ref.cell_update(T0, F0)
        assert np.array_equal(ref.bits(u[live]), ref.bits(T0[live]))  # residual 0
        T1, S, margin = ref.raise_ref(T0, F0, goal)
        assert not S.any() and not margin.any()


def test_shares_of_the_shared_cases(maps):
    rows = []
    for name, nx, ny, goal, T0, F1, win in shared_cases(maps):
        finite = int(np.isfinite(T0).sum())
        _, tiles, th, n = ref.reset_ref(T0, F1, [win], 8, goal=goal)
        T1, S, margin = ref.raise_ref(T0, F1, goal)
        rows.append((f"{nx}x{ny}", name, win, n, finite, int(S.sum())))
        assert not margin.any(), name                       # the raise margin is empty
        assert not (S & ~(T0 >= th)).any(), name            # the cone lies in the theta reset
        if name == "goal":
            assert th == 0.0 and n == finite - 1 and S.sum() == finite - 1
        elif name == "unreached":
            assert th == INF and n == 0 and not tiles and not S.any()
            i0, j0, w, h = win
            assert np.isinf(T0[j0 - 1:j0 + h + 1, i0 - 1:i0 + w + 1]).all()
            assert np.isfinite(F1[j0:j0 + h, i0:i0 + w]).all()
        else:
            assert 0 < n < finite - 1, name
            assert tiles, name
            if name == "cleared":   # cells that were +inf are queued without being written
                newly = np.isinf(T0) & np.isfinite(F1)
                assert newly.any() and not S.any()
            else:
                assert 0 < S.sum() <= n, name
        if name == "one":
            assert np.isfinite(T0[win[1], win[0]])
    for r in rows:
        print("%-6s %-9s window %-20s reset %5d of %5d finite, raise cone %5d" % r)


# ---------------------------------------------------------------------------
# mutant separation
# ---------------------------------------------------------------------------
def theta_inputs(maps, seeded):
    for name, nx, ny, goal, T0, F1, win in shared_cases(maps):
        for pad in PITCHES:
            yield (ref.pitched(T0, nx + pad, PAD_T), nx, ny, nx + pad, [win])
    F0, T0 = seeded
    ny, nx = F0.shape
    for name in ref.SEEDED_CASES:
        yield (ref.pitched(T0, nx, PAD_T), nx, ny, nx, [ref.case(name, F0, (0, 0))[1]])


def reset_inputs(maps, seeded):
    for name, nx, ny, goal, T0, F1, win in shared_cases(maps):
        for pad in PITCHES:
            for tile in TILES:
                ld = nx + pad
                yield (ref.pitched(T0, ld, PAD_T), ref.pitched(F1, ld, PAD_F), nx, ny, ld, [win],
                       tile, goal)


def raise_inputs(maps, seeded):
    for name, nx, ny, goal, T0, F1, win in shared_cases(maps):
        yield (ref.pitched(T0, nx, PAD_T), ref.pitched(F1, nx, PAD_F), nx, ny, nx, goal, win)


def cone_inputs(maps, seeded):
    for name, nx, ny, goal, T0, F1, win in shared_cases(maps):
        T1 = ref.raise_ref(T0, F1, goal)[0]
        for tile in TILES:
            yield (ref.pitched(T1, nx, PAD_T), ref.pitched(F1, nx, PAD_F), nx, ny, nx, goal, tile)


def window_inputs(maps, seeded):
    for name, nx, ny, goal, T0, F1, win in shared_cases(maps):
        for tile in TILES:
            yield (nx, ny, [win], tile)


KINDS = {"theta": (theta_loop, theta_inputs), "reset": (reset_loop, reset_inputs),
         "raise": (raise_loop, raise_inputs), "cone": (cone_seed_loop, cone_inputs),
         "window": (seed_window_loop, window_inputs)}

MUTANTS = [
    # theta without the ring; the grown window clipped one cell short of the grid's far edge;
    # the padding columns read as cells; the map read at pitch nx
    ("theta", "no_ring"), ("theta", "clip_hi"), ("theta", "pad_cols"),
    ("theta", "nx_for_ld"),
    # > for >= against theta; one neighbour direction dropped from the seed test; the goal
    # reset like any cell; 8 x 8 tiles where 16 x 16 are meant and back; obstacles queued
    ("reset", "gt"), ("reset", "drop_S"), ("reset", "drop_W"), ("reset", "drop_E"),
    ("reset", "drop_N"), ("reset", "goal_not_exempt"), ("reset", "tile_other"),
    ("reset", "ignore_F"),
    # a blocked cell keeps its value; the front does not follow one direction
    ("raise", "no_obstacle_rule"), ("raise", "drop_S"), ("raise", "drop_W"), ("raise", "drop_E"),
    ("raise", "drop_N"),
    ("cone", "drop_S"), ("cone", "drop_W"), ("cone", "drop_E"), ("cone", "drop_N"),
    ("cone", "ignore_F"),
    # the window's tiles: not clipped to the grid; one cell too far
    ("window", "unclipped"), ("window", "clip_hi"),
]


def same(a, b):
    return repr(a) == repr(b)  # exact: repr of floats is unique per value


@pytest.mark.parametrize("kind,mut", MUTANTS, ids=[f"{k}-{m}" for k, m in MUTANTS])
def test_mutant_is_separated(maps, seeded, kind, mut):
    fn, inputs = KINDS[kind]
    hits = total = 0
    for args in inputs(maps, seeded):
        total += 1
        if not same(fn(*args), fn(*args, mut=mut)):
            hits += 1
    print(f"{kind}/{mut}: separated on {hits} of {total} inputs")
    assert hits >= 1


SEED_MUTANTS = ["no_seed_back", "seed_overwrite", "no_seed_tile", "no_seed_across", "gt",
                "tile_other"]


@pytest.mark.parametrize("mut", SEED_MUTANTS)
def test_seeded_mutant_is_separated(seeded, mut):
    F0, T0 = seeded
    ny, nx = F0.shape
    hits = total = 0
    for name in ref.SEEDED_CASES:
        F1, win = ref.case(name, F0, ref.SEEDS_97[0][:2])
        for tile in TILES:
            args = (ref.pitched(T0, nx, PAD_T), ref.pitched(F1, nx, PAD_F), nx, ny, nx, [win], tile)
            total += 1
            hits += not same(reset_loop(*args, seeds=ref.SEEDS_97),
                             reset_loop(*args, seeds=ref.SEEDS_97, mut=mut))
    print(f"seeded reset/{mut}: separated on {hits} of {total} inputs")
    assert hits >= 1


def test_raise_tolerance_zero_is_separated_on_a_map_with_rounding(maps):
    """On the oracle's exact fixed point a tolerance of 0 invalidates what 1e-13 does; on a
    map that is converged only to the last ulps, as the engine's own maps are, it does not."""
    nx, ny, goal = ref.SHAPES[0]
    F0, T0 = maps[(nx, ny, goal)]
    rng = np.random.default_rng(3)
    Tn = T0 * (1.0 + rng.uniform(-4, 4, T0.shape) * 2.0 ** -52)
    Tn[goal[1], goal[0]] = 0.0
    assert not ref.raise_ref(Tn, F0, goal)[1].any()            # 1e-13 covers the rounding
    assert ref.raise_ref(Tn, F0, goal, tol=0.0)[1].sum() > 100  # 0 does not
    F1, win = ref.case("interior", F0, goal)
    a, b = ref.raise_ref(Tn, F1, goal)[1], ref.raise_ref(Tn, F1, goal, tol=0.0)[1]
    print(f"raise tol 0: {int(b.sum())} cells against {int(a.sum())}")
    assert b.sum() > a.sum()
