"""References for the row-slab domain step (include/dymu_fim.h, "row-slab domains"), in
plain numpy, written from the header text:

* ``merge_ref``     -- dymu_dom_merge_ghosts / dymu_dom_exchange / the first pass of
  dymu_dom_round: the strict min-merge of received rows into the ghost rows and the set of
  tiles it queues.
* ``dirichlet_ref`` -- the fixed point of one slab alone with its true neighbour rows as
  boundary values (what dymu_dom_run converges to once those rows are in the ghosts).
* ``constructed_rows`` / ``lower_rows`` / ``CASES`` -- the inputs shared by
  tests/test_slab_ref.py (CPU) and tests/test_gpu_domain.py.
"""
import numpy as np

import goalset_ref

INF = float("inf")


def tile_size(kernel):
    """tile_w = tile_h of a pass kernel: 8 for kernels 3 and 4, 16 for kernel 5."""
    return 16 if kernel == 5 else 8


def merge_ref(ghost_lo_row, ghost_hi_row, new_lo, new_hi, nx, nrows, tile_w, tile_h):
    """(lo_out, hi_out, queued): the ghost rows after the merge and the set of queued tiles.

    A ghost value is replaced where the received one is strictly below it; an equal value
    or a NaN keeps the old one (bit for bit).  Tile t = trow * ntx + i // tile_w is queued
    when some column i < nx of it improved, trow = 0 for the lo side and nty - 1 for the hi
    side; a tile reached from both sides is one element of the set.  A side whose ghost
    row or received row is None is left alone."""
    ntx = -(-nx // tile_w)
    nty = -(-nrows // tile_h)
    queued = set()
    out = []
    for old, new, trow in ((ghost_lo_row, new_lo, 0), (ghost_hi_row, new_hi, nty - 1)):
        if old is None or new is None:
            out.append(None if old is None else np.array(old[:nx], dtype=np.float64))
            continue
        old = np.asarray(old[:nx], dtype=np.float64)
        new = np.asarray(new[:nx], dtype=np.float64)
        with np.errstate(invalid="ignore"):
            better = new < old  # False for NaN on either side
        out.append(np.where(better, new, old))
        queued |= {trow * ntx + int(i) // tile_w for i in np.flatnonzero(better)}
    return out[0], out[1], queued


def dirichlet_ref(oracle, F, Tref, r0, nrows):
    """Rows [r0, r0 + nrows) of the fixed point of the slab alone: the reference FMM
    (goalset_ref.fmm_seeds) on the slab extended by one +inf-speed row per ghost side,
    seeded with every finite cell of Tref[r0 - 1] and Tref[r0 + nrows] at its value, and
    with the goal (the cell where Tref is 0) at 0 if it lies in the slab."""
    F = np.asarray(F, dtype=np.float64)
    ny, nx = F.shape
    lo, hi = r0 > 0, r0 + nrows < ny
    Fe = np.full((nrows + lo + hi, nx), INF)
    Fe[lo:lo + nrows] = F[r0:r0 + nrows]
    seeds = []
    if lo:
        seeds += [(i, 0, Tref[r0 - 1, i]) for i in range(nx) if Tref[r0 - 1, i] < INF]
    if hi:
        seeds += [(i, lo + nrows, Tref[r0 + nrows, i]) for i in range(nx)
                  if Tref[r0 + nrows, i] < INF]
    for j, i in np.argwhere(Tref[r0:r0 + nrows] == 0.0):
        seeds.append((int(i), lo + int(j), 0.0))
    if not seeds:
        return np.full((nrows, nx), INF)
    return goalset_ref.fmm_seeds(oracle, Fe, seeds)[lo:lo + nrows]


# ---- constructed rows for the merge (tests/test_slab_ref.py, tests/test_gpu_domain.py) ----
KINDS = ("below", "equal", "above", "inf", "nan", "first", "last", "none")
NVARIANTS = len(KINDS)  # variant v gives column group t the kind KINDS[(t + v) % 8]


def _quiet(old, new, c0, c1):
    """columns [c0, c1) non-improving: equal on even columns, above on odd ones"""
    for c in range(c0, c1):
        new[c] = old[c] if c % 2 == 0 else old[c] * 2.0  # +inf stays +inf: equal


def constructed_rows(nx, tile_w, variant):
    """(old, new): a ghost row and a received row of nx columns.  old is U(1, 100) with
    about a tenth +inf.  new is built per column group of tile_w columns, the group's kind
    cycling with the variant: below (old / 2; 7.0 under an old +inf), equal, above (2 old),
    +inf, NaN, one improved column at the group's first / at its last column among
    non-improving ones, none improved.  On top of that columns 255, 256 and nx - 1 are single
    improved columns of otherwise non-improving groups."""
    rng = np.random.default_rng(1000 * nx + 10 * tile_w + variant)
    old = rng.uniform(1.0, 100.0, nx)
    old[rng.random(nx) < 0.1] = INF
    new = np.empty(nx)
    for t in range(-(-nx // tile_w)):
        c0, c1 = t * tile_w, min(nx, (t + 1) * tile_w)
        kind = KINDS[(t + variant) % len(KINDS)]
        if kind == "below":
            new[c0:c1] = np.where(np.isinf(old[c0:c1]), 7.0, old[c0:c1] * 0.5)
        elif kind == "equal":
            new[c0:c1] = old[c0:c1]
        elif kind == "above":
            new[c0:c1] = old[c0:c1] * 2.0
        elif kind == "inf":
            new[c0:c1] = INF
        elif kind == "nan":
            new[c0:c1] = np.nan
        else:
            _quiet(old, new, c0, c1)
            if kind != "none":
                c = c0 if kind == "first" else c1 - 1
                old[c], new[c] = 50.0, 25.0
    for c in (255, 256, nx - 1):
        if 0 <= c < nx:
            t = c // tile_w
            _quiet(old, new, t * tile_w, min(nx, (t + 1) * tile_w))
    for c in (255, 256, nx - 1):
        if 0 <= c < nx:
            old[c], new[c] = 50.0, 25.0
    return old, new


def lower_rows(ghost, queued_cols):
    """A received row that lowers the ghost row only in the given columns (of tiles that
    are queued already) and equals it elsewhere: half the value, 3.0 under a +inf."""
    new = np.array(ghost, dtype=np.float64)
    for c in queued_cols:
        new[c] = 3.0 if not ghost[c] < INF else ghost[c] * 0.5
    return new


def tile_cols(queued, trow, nx, tile_w):
    """the columns under the queued tiles of tile row trow"""
    ntx = -(-nx // tile_w)
    cols = []
    for t in sorted(queued):
        if t // ntx == trow:
            c0 = (t % ntx) * tile_w
            cols += range(c0, min(nx, c0 + tile_w))
    return cols


def quiet_rows(ghost):
    """A received row that improves nothing: equal, above, +inf and NaN in turn."""
    new = np.array(ghost, dtype=np.float64)
    k = np.arange(len(new)) % 4
    new[k == 1] = new[k == 1] * 2.0
    new[k == 2] = INF
    new[k == 3] = np.nan
    return new


# ---- slabs whose Dirichlet fixed point is the FMM's rows (checked in test_slab_ref.py) ----
# (nx, ny, goal (i, j), r0, nrows, obstacle fraction); speed: synth_speed(seed=31, obst_seed=5)
CASES = {
    "mid": (100, 96, (50, 10), 32, 32, 0.03),
    "goal_in": (100, 96, (50, 40), 32, 32, 0.03),
    "wide": (300, 112, (7, 100), 32, 48, 0.05),
    "first": (37, 80, (30, 70), 0, 32, 0.05),
    "last_ragged": (261, 83, (130, 5), 64, 19, 0.10),
    "narrow": (5, 64, (2, 1), 16, 32, 0.0),
}
_case_cache = {}


def case(oracle, name):
    """(F, Tref, goal, r0, nrows) of a CASES entry; computed once, do not modify."""
    if name not in _case_cache:
        nx, ny, goal, r0, nrows, frac = CASES[name]
        F = oracle.synth_speed(nx, ny, seed=31, obst_frac=frac, obst_seed=5, goal=goal)
        Tref, _ = oracle.fmm(F, goal)
        F.setflags(write=False)
        Tref.setflags(write=False)
        _case_cache[name] = (F, Tref, goal, r0, nrows)
    return _case_cache[name]


def walled_case(oracle):
    """The "mid" slab with its last owned row all obstacles: nothing below it is reachable,
    so that row and the hi neighbour row stay +inf.  (F, Tref, goal, r0, nrows)."""
    if "walled" not in _case_cache:
        nx, ny, goal, r0, nrows, frac = CASES["mid"]
        F = oracle.synth_speed(nx, ny, seed=31, obst_frac=frac, obst_seed=5, goal=goal)
        F[r0 + nrows - 1, :] = INF
        Tref, _ = oracle.fmm(F, goal)
        F.setflags(write=False)
        Tref.setflags(write=False)
        _case_cache["walled"] = (F, Tref, goal, r0, nrows)
    return _case_cache["walled"]
