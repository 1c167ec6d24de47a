"""References for the preparation stage of the windowed updates (include/dymu_fim.h,
"dynamic update" and "windowed updates of seeded maps and of stacks"), in plain numpy,
written from the header's wording, not from the kernels.  tests/test_update_ref.py pins
each of them to a per-cell loop and shows that the shared cases separate the loops from
their mutants; tests/test_gpu_stages.py compares the engine with them exactly.

Maps are [ny, nx] arrays; a window is (i0, j0, w, h), clipped here as the engine clips it;
a set of tiles is a set of (tile row, tile column) pairs.
"""
import numpy as np

INF = np.inf
RAISE_TOL = 1e-13     # the raise front keeps a cell supported within this (relative)
MARGIN = 1e-15        # relative band around the raise threshold that must hold no cell
SHAPES = [(97, 61, (70, 40)), (33, 65, (1, 1))]
PAD = 7               # ld = nx + PAD in the pitched cases
PAD_T = 0.0           # T padding: below every theta > 0, so a read of it lowers theta
PAD_F = 7.0           # F padding: a finite speed no cell holds (synth speeds are in [1, 5])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def tile_size(kernel):
    """Tiles are 8 x 8 cells for kernels 3 and 4, 16 x 16 for kernel 5."""
    return 16 if kernel == 5 else 8


def pitched(A, ld, pad):
    ny, nx = A.shape
    out = np.full((ny, ld), pad, dtype=np.float64)
    out[:, :nx] = A
    return out


def clip(win, nx, ny):
    """(i0, j0, i1, j1) of the window clipped to the grid, exclusive upper corner."""
    i0, j0, w, h = win
    return i0, j0, min(i0 + w, nx), min(j0 + h, ny)


def theta_ref(T, wins):
    """The minimum of old T over every clipped window grown by one cell on each side and
    clipped again; +inf without a window or when all of it is +inf."""
    ny, nx = T.shape
    th = INF
    for win in wins:
        i0, j0, i1, j1 = clip(win, nx, ny)
        th = min(th, float(T[max(j0 - 1, 0):min(j1 + 1, ny), max(i0 - 1, 0):min(i1 + 1, nx)].min()))
    return th


def seed_window_ref(wins, nx, ny, tile):
    """The tiles that meet a clipped window."""
    out = set()
    for win in wins:
        i0, j0, i1, j1 = clip(win, nx, ny)
        out |= {(ty, tx) for ty in range(j0 // tile, (j1 - 1) // tile + 1)
                for tx in range(i0 // tile, (i1 - 1) // tile + 1)}
    return out


def _shift(A, fill):
    """The four in-grid neighbour values of every cell ((i, j-1), (i-1, j), (i+1, j),
    (i, j+1)), `fill` where the neighbour is off the grid."""
    S, W, E, N = (np.full_like(A, fill) for _ in range(4))
    S[1:, :] = A[:-1, :]
    N[:-1, :] = A[1:, :]
    W[:, 1:] = A[:, :-1]
    E[:, :-1] = A[:, 1:]
    return S, W, E, N


def _tiles_of(mask, tile):
    jj, ii = np.nonzero(mask)
    return set(zip((jj // tile).tolist(), (ii // tile).tolist()))


def seed_tiles(i, j, nx, ny, tile, across=True):
    """The tiles a seed at (i, j) queues: its own and (across: kernels 4 and 5) the tile
    across each tile edge its cell lies on."""
    out = {(j // tile, i // tile)}
    if not across:
        return out
    if i % tile == 0 and i > 0:
        out.add((j // tile, i // tile - 1))
    if i % tile == tile - 1 and i + 1 < nx:
        out.add((j // tile, i // tile + 1))
    if j % tile == 0 and j > 0:
        out.add((j // tile - 1, i // tile))
    if j % tile == tile - 1 and j + 1 < ny:
        out.add((j // tile + 1, i // tile))
    return out


def reset_ref(T, F, wins, tile, goal=None, seeds=None, across=True):
    """The theta reset of one map: (T after, queued tiles, theta, cells reset).
    goal = (i, j): the single-goal form (the goal is exempt and counts as kept);
    seeds = [(i, j, t0)]: the seeded form (no exempt cell; the seeds min-written back and
    their tiles queued; with theta = +inf nothing else happens)."""
    ny, nx = T.shape
    theta = theta_ref(T, wins)
    kept = T < theta
    hit = T >= theta
    if goal is not None:
        kept[goal[1], goal[0]] = True
        hit[goal[1], goal[0]] = False
    out = T.copy()
    tiles = set()
    n_reset = 0
    if goal is not None or theta < INF:
        reset = hit & (T < INF)
        out[reset] = INF
        n_reset = int(reset.sum())
        near = np.zeros_like(kept)
        for nb in _shift(kept, False):
            near |= nb
        tiles = _tiles_of(hit & (F < INF) & near, tile)
    for i, j, t0 in (seeds or []):
        out[j, i] = min(out[j, i], t0)
        tiles |= seed_tiles(i, j, nx, ny, tile, across)
    return out, tiles, theta, n_reset


def stack_ref(T, F, ny, P, wins, seeds, tile, decrease_only=False, across=True):
    """The preparation of dymu_update_batch_window_device on a stack of B planes at a
    plane pitch of P rows (T, F: [B * P, nx]; one plain seeded map: B = 1, P = ny).
    wins: (plane, i0, j0, w, h); seeds: (plane, i, j, t0).
    Returns (T after, queued tiles in stacked tile rows, theta per plane, cells reset)."""
    B = T.shape[0] // P
    nx = T.shape[1]
    out = T.copy()
    tiles, thetas, n_reset = set(), [], 0
    for b in range(B):
        r0 = b * P
        w_b = [w[1:] for w in wins if w[0] == b]
        s_b = [s[1:] for s in seeds if s[0] == b]
        if decrease_only:
            thetas.append(theta_ref(T[r0:r0 + ny], w_b))
            t_b = seed_window_ref(w_b, nx, ny, tile)
        else:
            out[r0:r0 + ny], t_b, th, n = reset_ref(T[r0:r0 + ny], F[r0:r0 + ny], w_b, tile,
                                                    seeds=s_b, across=across)
            thetas.append(th)
            n_reset += n
            for i, j, _ in s_b:  # tile edges are those of the whole stacked domain
                tiles |= seed_tiles(i, r0 + j, nx, B * P, tile, across)
        tiles |= {(ty + r0 // tile, tx) for ty, tx in t_b}
    return out, tiles, thetas, n_reset


def ref_update(tx, ty, c):
    """The reference update (:531-535) of neighbour minima tx, ty and speed c, in the
    operation order of the engine's host-checked arithmetic."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = tx - ty
        two = (np.abs(d) < c) & (tx < INF) & (ty < INF)
        r = 2.0 * (c * c) - d * d
        a = (tx + ty + np.sqrt(np.where(two, r, 0.0))) / 2
        return np.where(two, a, np.minimum(tx, ty) + c)


def cell_update(T, F):
    """The reference update of every cell from its in-grid 4-neighbours' current values."""
    S, W, E, N = _shift(T, INF)
    return ref_update(np.minimum(W, E), np.minimum(S, N), F)


def raise_ref(T, F, goal, tol=RAISE_TOL):
    """The raise front: (T after, invalidated mask S, margin mask).  S grows from the empty
    set by the header's rule until nothing changes: a live cell (finite T, not the goal)
    goes when its new speed is not finite, or when the reference update of its current
    neighbours (S at +inf) exceeds T * (1 + tol).  margin: the live cells whose update
    came within MARGIN (relative) of that threshold in some round."""
    live = np.isfinite(T)
    live[goal[1], goal[0]] = False
    cur = T.copy()
    gone = np.zeros_like(live)
    margin = np.zeros_like(live)
    thr = T * (1.0 + tol)
    blocked = ~(F < INF)
    while True:
        u = cell_update(cur, F)
        cand = live & ~gone
        with np.errstate(invalid="ignore"):
            margin |= cand & ~blocked & (np.abs(u - thr) <= MARGIN * thr)
            now = cand & (blocked | (u > thr))
        if not now.any():
            return cur, gone, margin
        gone |= now
        cur[now] = INF


def cone_seed_ref(T, F, goal, tile):
    """After the raise: the tiles holding a non-goal cell with T = +inf and finite speed
    that has a finite in-grid 4-neighbour, and the smallest such neighbour value."""
    m = np.minimum.reduce(_shift(T, INF))
    hit = (T == INF) & (F < INF) & (m < INF)
    hit[goal[1], goal[0]] = False
    return _tiles_of(hit, tile), float(m[hit].min()) if hit.any() else INF


# ---------------------------------------------------------------------------
# the shared cases (tests/test_update_ref.py asserts what makes them non-vacuous)
# ---------------------------------------------------------------------------
ENCLOSURE = (40, 8)   # corner of a 7 x 7 obstacle block of the old speed (97 x 61 map)
CASES = ("interior", "corner", "edge", "one", "goal", "unreached", "blocked", "cleared")
# Two small maps whose goal sits in the corner of an 8- and a 16-cell tile, so that each of
# its four neighbours lies in another tile and is queued through one direction of the seed
# test alone: only the "goal" case runs on them.
GOAL_SHAPES = [(40, 40, (16, 16)), (40, 40, (15, 15))]
ALL_SHAPES = SHAPES + GOAL_SHAPES


def cases_for(nx, ny):
    """The cases of a map: all of them on 97 x 61; on 33 x 65, whose goal sits in the
    (0, 0) corner and which has no walled-off block, those that differ from "goal"."""
    if (nx, ny) == (97, 61):
        return CASES
    return ("interior", "edge", "one", "blocked") if (nx, ny) == (33, 65) else ("goal",)


# the seeded map: three seeds, the middle one dominated (its t0 is above what the first
# seed propagates to its cell) and, in three of the cases, inside the reset region; the
# last one in the grid's last cell, so that the "edge" window's theta sits there
SEEDS_97 = [(70, 40, 0.0), (30, 8, 500.0), (96, 60, 3.0)]
SEEDED_CASES = ("interior", "edge", "one", "unreached")
# the stack: three planes of the 97 x 61 speed scaled by these factors, one seed each plus
# the dominated one in plane 0; two windows in plane 0, none in plane 1, a clipped one in 2
STACK_SCALE = (1.0, 0.5, 2.0)
STACK_SEEDS = [(0, 70, 40, 0.0), (0, 30, 8, 500.0), (1, 20, 20, 0.0), (2, 5, 55, 1.5)]
STACK_WINS = [(0, 23, 9, 9, 7), (0, 80, 5, 4, 4), (2, 92, 57, 500, 500)]


def plane_rows(ny):
    """dymu_batch_plane_rows: 16 * ceil((ny + 1) / 16)."""
    return 16 * ((ny + 16) // 16)


def stacked(maps, ny, P, wall):
    """Planes [ny, nx] stacked at a plane pitch of P rows, the wall rows set to `wall`."""
    out = np.full((len(maps) * P, maps[0].shape[1]), wall, dtype=np.float64)
    for b, m in enumerate(maps):
        out[b * P:b * P + ny] = m
    return out


def stack_speeds(F0, factor=1.5):
    """(old stacked speed, new stacked speed, P) of the three-plane stack: every window's
    speed times `factor`."""
    ny, nx = F0.shape
    P = plane_rows(ny)
    old = [F0 * s for s in STACK_SCALE]
    new = [f.copy() for f in old]
    for b, i0, j0, w, h in STACK_WINS:
        a0, b0, a1, b1 = clip((i0, j0, w, h), nx, ny)
        new[b][b0:b1, a0:a1] *= factor
    return stacked(old, ny, P, INF), stacked(new, ny, P, INF), P


def decrease_case(name, F0, goal):
    """(new speed, window) of a case for the decrease-only form, whose promise is that no
    speed went up: the case's window at half its speed (obstacles stay), except for the two
    cases that are decreases already."""
    F1, win = case(name, F0, goal)
    if name in ("unreached", "cleared"):
        return F1, win
    ny, nx = F0.shape
    i0, j0, i1, j1 = clip(win, nx, ny)
    F1 = F0.copy()
    F1[j0:j1, i0:i1] *= 0.5
    return F1, win


def serpentine(F, period=16):
    """1-cell walls every `period` rows, one gap each at alternating ends."""
    F = F.copy()
    nx = F.shape[1]
    for k, j in enumerate(range(period // 2, F.shape[0], period)):
        F[j, :] = INF
        F[j, 1 if k % 2 == 0 else nx - 2] = 2.0
    return F


def base_speed(oracle, nx, ny, goal):
    """oracle.synth_speed with 4 % obstacles; the 97 x 61 map with a walled-off block whose
    inside the "unreached" case clears."""
    F = oracle.synth_speed(nx, ny, seed=11, obst_frac=0.04, obst_seed=13, goal=goal)
    if (nx, ny) == (97, 61):
        i, j = ENCLOSURE
        F[j:j + 7, i:i + 7] = INF
    return F


def no_nan(F):
    """The speed as the oracle takes it: a NaN is an obstacle."""
    return np.where(np.isnan(F), INF, F)


def case(name, F0, goal):
    """(new speed, window) of a case: 9 x 7 windows whose speed rises by 1.5, except where
    the name says otherwise.  The interior windows end on a tile boundary."""
    ny, nx = F0.shape
    F1 = F0.copy()
    if name == "unreached":   # cleared cells inside the wall: the window and its ring are +inf
        i, j = ENCLOSURE
        F1[j + 1:j + 6, i + 1:i + 6] = 2.0
        return F1, (i + 1, j + 1, 5, 5)
    if name == "blocked":     # a blocked disc: +inf, and NaN (an obstacle as well) in its core
        ci, cj = nx // 4, ny // 2
        j, i = np.mgrid[0:ny, 0:nx]
        d2 = (i - ci) ** 2 + (j - cj) ** 2
        F1[d2 <= 16] = INF
        F1[d2 <= 2] = np.nan
        return F1, (ci - 4, cj - 4, 9, 9)
    if name == "cleared":     # obstacles removed and the rest cheaper: cells become reachable
        win = (28, 20, 9, 7)
        i0, j0, i1, j1 = clip(win, nx, ny)
        box = F1[j0:j1, i0:i1]
        box[~np.isfinite(box)] = 2.0
        box *= 0.5
        return F1, win
    win = {"interior": (23, 9, 9, 7) if nx == 97 else (7, 25, 9, 7), "corner": (0, 0, 9, 7),
           "edge": (nx - 5, ny - 4, 500, 500), "one": (nx // 2, ny // 2, 1, 1),
           "goal": (max(goal[0] - 4, 0), max(goal[1] - 3, 0), 9, 7)}[name]
    i0, j0, i1, j1 = clip(win, nx, ny)
    F1[j0:j1, i0:i1] *= 1.5
    return F1, win


