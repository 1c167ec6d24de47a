"""References and constructed maps for the kernels that read a finished map: the early
exit's mask, counts and region (dymu_early_exit_mask, dymu_count_equal, dymu_find_equal,
dymu_region_stats, dymu_scatter) and the label pass (dymu_goal_labels_device).

The references are plain numpy written from the wording of include/dymu_fim.h; they are
pinned to per-cell loops and separated from their mutants in tests/test_postproc_ref.py
and compared bit for bit with the kernels in tests/test_gpu_postproc.py.

Domain of every constructed T: +0.0 <= T <= +inf, no NaN, no -0.0 (the kernels order
values by bit pattern).  F may hold finite positives, +inf and NaN.
"""
import numpy as np

from goalset_ref import NONE, labels_from_T  # noqa: F401  (re-exported for the tests)

INF = np.inf
SHAPES = [(1, 1), (37, 1), (1, 37), (33, 65), (97, 61)]
OFFSETS = (0.0, 0.5, 2.0)
PAD = 7            # ld = nx + PAD in the pitched cases
PAD_T = 0.0        # T padding: <= any thr >= 0, CLOSED for any tc >= 0, below any parent
PAD_F = 7.0        # F padding: a finite speed no cell of a constructed F holds
PLATEAU = 1.5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def early_mask_ref(F, T, tc):
    """(T_after, band_idx_sorted).  CLOSED iff T <= tc; a non-CLOSED cell with F < inf and
    an in-grid 4-neighbour that is CLOSED is band (keeps T, listed as j*nx+i); every other
    non-CLOSED cell becomes +inf."""
    F = np.asarray(F, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    ny, nx = T.shape
    closed = T <= tc
    pad = np.zeros((ny + 2, nx + 2), dtype=bool)
    pad[1:-1, 1:-1] = closed
    nb = pad[:-2, 1:-1] | pad[1:-1, :-2] | pad[1:-1, 2:] | pad[2:, 1:-1]
    with np.errstate(invalid="ignore"):
        band = ~closed & (F < INF) & nb
    out = T.copy()
    out[~closed & ~band] = INF
    return out, np.flatnonzero(band.ravel()).astype(np.uint64)


def find_equal_ref(T, value):
    """Sorted indices j*nx+i of the cells whose bit pattern is that of `value`."""
    v = np.array([value], dtype=np.float64).view(np.uint64)[0]
    return np.flatnonzero(bits(T).ravel() == v).astype(np.uint64)


def count_equal_ref(T, value):
    """Bitwise compare of the uint64 views: -0.0 != +0.0."""
    return int(find_equal_ref(T, value).size)


def region_ref(F, T, goal, thr, lo, hi):
    """(box or None, n_range, r_const): box = (i0, j0, i1, j1) inclusive of the cells with
    T <= thr; n_range = cells with lo <= T <= hi; r_const = sqrt of the least integer
    squared distance from the goal to a cell with F != F[goal] (NaN and +inf differ from
    any finite speed), +inf if there is none."""
    F = np.asarray(F, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    ny, nx = T.shape
    gi, gj = goal
    jj, ii = np.nonzero(T <= thr)
    box = None
    if ii.size:
        box = (int(ii.min()), int(jj.min()), int(ii.max()), int(jj.max()))
    n_range = int(((T >= lo) & (T <= hi)).sum())
    with np.errstate(invalid="ignore"):
        dj, di = np.nonzero(F != F[gj, gi])
    r_const = INF
    if di.size:
        d2 = ((di.astype(np.int64) - gi) ** 2 + (dj.astype(np.int64) - gj) ** 2).min()
        r_const = float(np.sqrt(np.float64(d2)))
    return box, n_range, r_const


def labels_fast(T, seeds):
    """labels_from_T without its per-cell loop, for the one large case: the same parents
    and roots, then every chain shortened by lab = lab[par] with par = par[par] until
    nothing moves.  Trusted only because test_postproc_ref.py pins it to labels_from_T."""
    T = np.ascontiguousarray(T, dtype=np.float64)
    ny, nx = T.shape
    n = nx * ny
    t = T.ravel()
    pad = np.full((ny + 2, nx + 2), INF)
    pad[1:-1, 1:-1] = T
    idx = np.arange(n)
    best = np.full(n, INF)
    par = idx.copy()
    # (i,j-1), (i-1,j), (i+1,j), (i,j+1): a later neighbour wins only if strictly smaller
    for nb, off in ((pad[:-2, 1:-1], -nx), (pad[1:-1, :-2], -1), (pad[1:-1, 2:], 1),
                    (pad[2:, 1:-1], nx)):
        v = nb.ravel()
        m = v < best
        best = np.where(m, v, best)
        par = np.where(m, idx + off, par)
    has = (t < INF) & (best < t)
    lab = np.full(n, NONE, dtype=np.uint32)
    root = np.zeros(n, dtype=bool)
    tb = bits(t)
    for k in range(len(seeds) - 1, -1, -1):  # descending: the lowest index is written last
        i, j, t0 = seeds[k]
        c = j * nx + i
        if tb[c] == bits(np.float64(t0) + 0.0):
            lab[c] = k
            root[c] = True
    ptr = np.where(has & ~root, par, idx)  # roots and cells without a parent end a chain
    while True:
        nxt = ptr[ptr]
        if np.array_equal(nxt, ptr):
            break
        ptr = nxt
    return lab[ptr].reshape(ny, nx)


# ---------------------------------------------------------------------------
# constructed maps (deterministic from a seed, any (nx, ny))
# ---------------------------------------------------------------------------
def sites_for(nx, ny):
    return [(nx // 5, ny // 4), ((4 * nx) // 5, ny // 2), (nx // 3, (5 * ny) // 6)]


def cone(nx, ny):
    """Manhattan distance to the nearest of three sites plus the site's offset: exact
    values (multiples of 0.5) with ties everywhere."""
    jj, ii = np.mgrid[0:ny, 0:nx]
    T = np.full((ny, nx), INF)
    for (si, sj), off in zip(sites_for(nx, ny), OFFSETS):
        T = np.minimum(T, (np.abs(ii - si) + np.abs(jj - sj)).astype(np.float64) + off)
    return T


def cone_pits(nx, ny, seed=3, pits=0.004, walls=0.03):
    """The cone with `pits` of the cells lowered to 3 below their cone value (floored at
    0.25: finite local minima that are no seed) and `walls` set to +inf; the sites keep
    their values."""
    T = cone(nx, ny)
    u = np.random.default_rng(seed).random((ny, nx))
    for si, sj in sites_for(nx, ny):
        u[sj, si] = 1.0
    pit = u < pits
    T[pit] = np.maximum(T[pit] - 3.0, 0.25)
    T[(u >= pits) & (u < pits + walls)] = INF
    return T


def plateau(nx, ny):
    return np.full((ny, nx), PLATEAU)


def all_inf(nx, ny):
    return np.full((ny, nx), INF)


def one_finite(nx, ny, at):
    T = all_inf(nx, ny)
    T[at[1], at[0]] = 0.0
    return T


FAMILIES = ("cone", "cone_pits", "plateau", "all_inf", "one_first", "one_last")


def family(name, nx, ny):
    if name == "cone":
        return cone(nx, ny)
    if name == "cone_pits":
        return cone_pits(nx, ny)
    if name == "plateau":
        return plateau(nx, ny)
    if name == "all_inf":
        return all_inf(nx, ny)
    if name == "one_first":
        return one_finite(nx, ny, (0, 0))
    if name == "one_last":
        return one_finite(nx, ny, (nx - 1, ny - 1))
    raise KeyError(name)


def speed_field(nx, ny, seed=5):
    """F: speeds 1, 2 and 3.5 with 6 % +inf and 4 % NaN cells."""
    rng = np.random.default_rng(seed)
    F = rng.choice(np.array([1.0, 2.0, 3.5]), size=(ny, nx))
    u = rng.random((ny, nx))
    F[u < 0.06] = INF
    F[(u >= 0.06) & (u < 0.10)] = np.nan
    return F


def tie_value(T):
    """The finite value T holds most often (the smallest such), 1.0 if it has none."""
    fin = T[np.isfinite(T)]
    if fin.size == 0:
        return 1.0
    vals, cnt = np.unique(fin, return_counts=True)
    return float(vals[np.argmax(cnt)])


def thresholds(T):
    """name -> tc / thr: nothing closed, 0, a value the map holds many times (tests <=),
    one ulp below it, everything closed."""
    v = tie_value(T)
    return {"neg": -1.0, "zero": 0.0, "tie": v, "tie_below": float(np.nextafter(v, -INF)),
            "inf": INF}


def _lower_neighbour_cell(T):
    """A finite cell that is no site and has a strictly lower neighbour (scanned from the
    middle of the grid), or None."""
    ny, nx = T.shape
    sites = set(sites_for(nx, ny))
    n = nx * ny
    for q in range(n):
        c = (n // 2 + q) % n
        i, j = c % nx, c // nx
        t = T[j, i]
        if not t < INF or (i, j) in sites:
            continue
        for ii, jj in ((i, j - 1), (i - 1, j), (i + 1, j), (i, j + 1)):
            if 0 <= ii < nx and 0 <= jj < ny and T[jj, ii] < t:
                return i, j
    return None


def seed_lists(name, T):
    """Seed lists (i, j, t0) of a family's map T.  Cone families:
      "sites"  the three sites with their offsets (0..2), a duplicate of site 0 with a
               larger t0 (3), a duplicate of site 1 with an equal t0 (4: the lowest k wins),
               a seed whose t0 differs from its cell's T (5: dominated, nobody's label) and
               a seed on a cell with a lower neighbour and t0 == T there (6: a root all the
               same; on a grid too small to have such a cell, one more duplicate of site 0);
      "negzero" the sites with site 0 given -0.0 on its cell holding +0.0 (accepted, = +0.0).
    Other families: one list that puts a seed on every site and on the finite cell."""
    ny, nx = T.shape
    s = sites_for(nx, ny)
    if name in ("cone", "cone_pits"):
        base = [(s[k][0], s[k][1], OFFSETS[k]) for k in range(3)]
        far = (nx - 1, 0)
        t_far = T[far[1], far[0]]
        low = _lower_neighbour_cell(T)
        extra = [(s[0][0], s[0][1], 3.0), (s[1][0], s[1][1], OFFSETS[1]),
                 (far[0], far[1], float(t_far) + 1.0 if t_far < INF else 1.0),
                 (low[0], low[1], float(T[low[1], low[0]])) if low else base[0]]
        return {"sites": base + extra, "negzero": [(s[0][0], s[0][1], -0.0)] + base[1:]}
    if name == "plateau":
        return {"sites": [(i, j, PLATEAU) for i, j in s]}
    if name == "all_inf":
        return {"sites": [(i, j, 0.0) for i, j in s]}
    at = (0, 0) if name == "one_first" else (nx - 1, ny - 1)
    return {"sites": [(i, j, 0.0) for i, j in s] + [(at[0], at[1], 0.0)]}


# ---------------------------------------------------------------------------
# pitched buffers
# ---------------------------------------------------------------------------
def pitched(A, ld, pad):
    """[ny, ld] float64 copy of A [ny, nx] with the padding columns set to `pad`."""
    A = np.asarray(A, dtype=np.float64)
    ny, nx = A.shape
    B = np.full((ny, ld), pad, dtype=np.float64)
    B[:, :nx] = A
    return B
