"""Reference for the clearance field after obstacles were freed, in numpy.

The field S of a constant speed c is seeded at +0.0 on every obstacle cell of a mask F
(!(F < +inf)).  dymu_clearance_edit_device takes the field of an old mask to a new one that
frees obstacle cells, adds some, or both, without a whole solve.  What it rests on, restated
here cell by cell:

* ``closure``  -- the freed cells go to +inf, then every finite non-obstacle cell whose
  update from its current neighbours exceeds its value by more than tol follows, a front of
  4-neighbours at a time until nothing changes.  The front only moves through cells it
  invalidated, as the kernel's does from tile to tile.
* ``relax``    -- Gauss-Seidel sweeps with the reference update, decrease-only, to the fixed
  point: what the passes do to the state the closure leaves.
* ``ragged_field`` -- a valid old field that is not converged above the level: a converged
  field cut at a random level in (1, 1.3] per cell, then closed over the whole map so that
  nothing is left standing on a value that is gone.  Without that closing it is not a
  supersolution, and the closure of an edit cannot be trusted on it.
"""
import math

import numpy as np

INF = np.inf
TOL = 1e-13


def ref_update(tx, ty, c):
    """The reference's Eikonal update (src/DyMu_GlobalPathPlanning.cpp:531-535), arrays."""
    with np.errstate(invalid="ignore"):
        d = tx - ty
        two = (np.abs(d) < c) & (tx < INF) & (ty < INF)
        dd = np.where(two, d, 0.0)
        s = np.where(two, tx, 0.0) + np.where(two, ty, 0.0)
        return np.where(two, (s + np.sqrt(2.0 * (c * c) - dd * dd)) / 2, np.minimum(tx, ty) + c)


def update_all(S, c):
    """u of every cell from its current in-grid 4-neighbours."""
    pad = np.full((S.shape[0] + 2, S.shape[1] + 2), INF)
    pad[1:-1, 1:-1] = S
    tx = np.minimum(pad[1:-1, :-2], pad[1:-1, 2:])
    ty = np.minimum(pad[:-2, 1:-1], pad[2:, 1:-1])
    return ref_update(tx, ty, c)


def grow(mask):
    """The 4-neighbours of the cells of mask."""
    out = np.zeros_like(mask)
    out[1:, :] |= mask[:-1, :]
    out[:-1, :] |= mask[1:, :]
    out[:, 1:] |= mask[:, :-1]
    out[:, :-1] |= mask[:, 1:]
    return out


def closure(S, F, c, tol=TOL, everywhere=False):
    """(S', cells invalidated): S closed under the rule above for the mask of F.
    everywhere: every cell is tested in the first pass, not the freed cells' front alone."""
    S = S.copy()
    obst = ~(F < INF)
    freed = ~obst & (S.view(np.uint64) == 0)
    S[freed] = INF
    count = int(freed.sum())
    front = np.ones(S.shape, dtype=bool) if everywhere else grow(freed)
    while front.any():
        with np.errstate(invalid="ignore"):
            gone = front & ~obst & (S < INF) & (update_all(S, c) > S * (1.0 + tol))
        S[gone] = INF
        count += int(gone.sum())
        front = grow(gone)
    return S, count


def relax(S, F, c):
    """The fixed point below S: obstacle cells at +0.0, then Gauss-Seidel sweeps in the four
    diagonal orders, each cell lowered to its update, until a round changes nothing."""
    ny, nx = S.shape
    T = [row[:] for row in np.where(~(F < INF), 0.0, S).tolist()]
    obst = (~(F < INF)).tolist()
    sqrt, inf, cc2 = math.sqrt, math.inf, 2.0 * (c * c)
    changed = True
    while changed:
        changed = False
        for js, is_ in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            for j in (range(ny) if js > 0 else range(ny - 1, -1, -1)):
                row, ob = T[j], obst[j]
                up = T[j - 1] if j > 0 else None
                dn = T[j + 1] if j + 1 < ny else None
                for i in (range(nx) if is_ > 0 else range(nx - 1, -1, -1)):
                    if ob[i]:
                        continue
                    tx = min(row[i - 1] if i > 0 else inf, row[i + 1] if i + 1 < nx else inf)
                    ty = min(up[i] if up else inf, dn[i] if dn else inf)
                    d = tx - ty
                    if abs(d) < c and tx < inf and ty < inf:
                        u = (tx + ty + sqrt(cc2 - d * d)) / 2
                    else:
                        u = min(tx, ty) + c
                    if u < row[i]:
                        row[i] = u
                        changed = True
    return np.array(T)


def ragged_field(S_conv, F, c, rng, close=True):
    """S_conv (converged for the mask of F) cut at a random level in (1, 1.3] per cell; with
    close, closed over the whole map, which makes it a state a solve stopped at the level can
    leave.  Without: cells still stand on values that are gone."""
    level = 1.3 - 0.3 * rng.random(S_conv.shape)
    S = np.where(S_conv > level, INF, S_conv)
    if close:
        S, _ = closure(S, F, c, everywhere=True)
    return S


def below_bound(S, S_ref, F):
    """The finite non-obstacle cells of S below the parity bound of S_ref: none when S bounds
    the field from above."""
    free = (F < INF) & np.isfinite(S)
    return free & (S < S_ref * (1.0 - 1e-12))
