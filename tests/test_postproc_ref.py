"""The references of tests/postproc_ref.py, pinned on the CPU.

* Every reference equals a slow per-cell loop transcribed clause by clause from
  include/dymu_fim.h.  The loops work on the pitched buffers the C-ABI takes (nx, ny, ld),
  with the padding poisoned exactly as tests/test_gpu_postproc.py poisons it.
* labels_fast equals goalset_ref.labels_from_T on every small map.
* Non-vacuity: the label family yields enough labelled, finite-NONE and tied-parent cells,
  and the early-mask inputs hold the cells each clause is about.
* Mutant separation: every listed mutant of a loop differs from the true loop on at least
  one constructed input -- a kernel carrying that bug would fail the GPU comparison.
"""
import math
import struct

import numpy as np
import pytest

import postproc_ref as ref
from postproc_ref import INF, NONE, PAD, PAD_F, PAD_T

SMALL = ref.SHAPES
PITCHES = (0, PAD)


def fbits(v):
    return struct.pack("<d", v)


# ---------------------------------------------------------------------------
# per-cell loops on pitched buffers; `mut` names one deliberate bug
# ---------------------------------------------------------------------------
def _extent(nx, ny, mut):
    return (nx - 1 if mut == "skip_last_col" else nx), (ny - 1 if mut == "skip_last_row" else ny)


def early_mask_loop(Fb, Tb, nx, ny, ld, tc, mut=""):
    """(buffer after, sorted band indices) of dymu_early_exit_mask."""
    F, T = Fb.ravel().tolist(), Tb.ravel().tolist()
    out = list(T)
    band = []
    st = nx if mut == "nx_for_ld" else ld   # the pitch the cell is read with
    so = ld if mut == "ld_for_nx" else nx   # the pitch the band index is formed with
    right = ld if mut == "pad_cols" else nx  # the extent the right neighbour is tested against

    def closed(v):  # a cell is CLOSED iff T <= t_closed
        return v < tc if mut == "lt" else v <= tc

    cols, rows = _extent(nx, ny, mut)
    for j in range(rows):
        for i in range(cols):
            k = j * st + i
            if closed(T[k]):
                continue  # ... and keeps T
            b = False
            if mut == "ignore_F" or F[k] < INF:  # a finite-speed ...
                # ... 4-neighbour of a CLOSED cell is in the narrow band
                b = ((j > 0 and closed(T[k - st])) or (i > 0 and closed(T[k - 1])) or
                     (i + 1 < right and closed(T[k + 1])) or (j + 1 < ny and closed(T[k + st])))
            if b:
                band.append(j * so + i)  # keeps its current T, listed as j*nx + i
            else:
                out[k] = INF  # every other cell gets +inf
    return out, sorted(band)


def equal_loop(Tb, nx, ny, ld, value, mut=""):
    """Sorted indices of the cells whose value is bitwise `value`."""
    T = Tb.ravel().tolist()
    st = nx if mut == "nx_for_ld" else ld
    so = ld if mut == "ld_for_nx" else nx
    cols, rows = _extent(nx, ny, mut)
    if mut == "pad_cols":
        cols = ld
    vb = fbits(value)
    return sorted(j * so + i for j in range(rows) for i in range(cols)
                  if (T[j * st + i] == value if mut == "float_eq" else fbits(T[j * st + i]) == vb))


def region_loop(Fb, Tb, nx, ny, ld, goal, thr, lo, hi, mut=""):
    """(box or None, n_range, r_const) of dymu_region_stats."""
    F, T = Fb.ravel().tolist(), Tb.ravel().tolist()
    st = nx if mut == "nx_for_ld" else ld
    cols, rows = _extent(nx, ny, mut)
    if mut == "pad_cols":
        cols = ld
    gi, gj = goal
    f0 = F[gj * st + gi]
    mi = mj = xi = xj = None
    n_range = 0
    d2 = None
    for j in range(rows):
        for i in range(cols):
            t = T[j * st + i]
            if t < thr if mut == "lt" else t <= thr:  # the bounding box of the cells with T <= thr
                mi = i if mi is None else min(mi, i)
                mj = j if mj is None else min(mj, j)
                xi = i if xi is None else max(xi, i)
                xj = j if xj is None else max(xj, j)
            if lo <= t <= hi:  # the number of cells with lo <= T <= hi
                n_range += 1
            if F[j * st + i] != f0:  # the nearest cell whose speed differs from the goal's
                q = (i - gi) ** 2 + (j - gj) ** 2
                d2 = q if d2 is None else min(d2, q)
    box = None if mi is None else (mi, mj, xi, xj)
    if mut == "box_none" and box == (0, 0, 0, 0):  # maxima left at their initial 0 taken for "none"
        box = None
    return box, n_range, (INF if d2 is None else math.sqrt(d2))


def labels_loop(Tb, nx, ny, ld, seeds, mut=""):
    """Labels (list, pitch nx) of dymu_goal_labels_device."""
    T = Tb.ravel().tolist()
    st = nx if mut == "nx_for_ld" else ld
    cols, rows = _extent(nx, ny, mut)
    n = nx * ny
    par = [-1] * n
    for j in range(rows):
        for i in range(cols):
            t = T[j * st + i]
            if not t < INF:
                continue  # DYMU_LABEL_NONE for T = +inf
            nbs = [(i, j - 1), (i - 1, j), (i + 1, j), (i, j + 1)]
            if mut == "rev_order":
                nbs.reverse()
            best, bc = None, -1
            for ii, jj in nbs:  # among the in-grid 4-neighbours in that order ...
                if 0 <= ii < nx and 0 <= jj < ny:
                    u = T[jj * st + ii]
                    # ... the first one holding the smallest T
                    if best is None or u < best or (mut == "last_smallest" and u == best):
                        best, bc = u, jj * nx + ii
            # ... if that is strictly below T[c]
            if best is not None and (best < t or (mut == "le_strict" and best == t)):
                par[j * nx + i] = bc
    roots = {}
    for k, (i, j, t0) in enumerate(seeds):
        c = j * nx + i
        # c is a root with label k if it is seed k's cell and T[c] is bitwise t0_k
        # (-0.0 is accepted and equals +0.0)
        if mut != "ignore_t0" and fbits(T[j * st + i]) != fbits(t0 + 0.0):
            continue  # dominated: no root
        if c not in roots or mut == "highest_k":  # the lowest k among equal ones
            roots[c] = k
    lab = [NONE] * n
    done = [False] * n
    for c in range(n):
        path, seen, x = [], set(), c
        while not done[x]:
            if x in roots:
                lab[x], done[x] = roots[x], True
            elif par[x] < 0 or x in seen:  # no strictly smaller neighbour (a cycle: mutants only)
                lab[x], done[x] = NONE, True
            else:
                seen.add(x)
                path.append(x)
                x = par[x]
        for y in path:  # label(c) = label(parent(c)); NONE drains upstream
            lab[y], done[y] = lab[x], True
    return lab


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def grids():
    for nx, ny in SMALL:
        for pad in PITCHES:
            yield nx, ny, nx + pad


def seeded_maps(nx, ny):
    for name in ref.FAMILIES:
        T = ref.family(name, nx, ny)
        for sname, seeds in ref.seed_lists(name, T).items():
            yield f"{name}/{sname}", T, seeds


def unpitch(buf, nx, ny, ld):
    return np.asarray(buf, dtype=np.float64).reshape(ny, ld)[:, :nx]


# ---------------------------------------------------------------------------
# references == loops
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,ld", list(grids()))
def test_early_mask_ref_is_loop(nx, ny, ld):
    F = ref.speed_field(nx, ny)
    Fb = ref.pitched(F, ld, PAD_F)
    for name in ref.FAMILIES:
        T = ref.family(name, nx, ny)
        Tb = ref.pitched(T, ld, PAD_T)
        for tname, tc in ref.thresholds(T).items():
            want_T, want_band = ref.early_mask_ref(F, T, tc)
            out, band = early_mask_loop(Fb, Tb, nx, ny, ld, tc)
            out = np.array(out).reshape(ny, ld)
            assert np.array_equal(ref.bits(out[:, :nx]), ref.bits(want_T)), (name, tname)
            assert np.array_equal(ref.bits(out[:, nx:]), ref.bits(Tb[:, nx:])), (name, tname)
            assert band == want_band.tolist(), (name, tname)


@pytest.mark.parametrize("nx,ny,ld", list(grids()))
def test_count_and_region_ref_is_loop(nx, ny, ld):
    F = ref.speed_field(nx, ny)
    Fb = ref.pitched(F, ld, PAD_F)
    goal = ref.sites_for(nx, ny)[0]
    for name in ref.FAMILIES:
        T = ref.family(name, nx, ny)
        v = ref.tie_value(T)
        for value in (v, 0.0, -0.0, INF, 0.123):
            Tb = ref.pitched(T, ld, value)  # the padding holds the searched value
            got = equal_loop(Tb, nx, ny, ld, value)
            assert got == ref.find_equal_ref(T, value).tolist(), (name, value)
            assert len(got) == ref.count_equal_ref(T, value)
        Tb = ref.pitched(T, ld, PAD_T)
        for tname, thr in ref.thresholds(T).items():
            for lo, hi in ((v, v), (v - 0.5, v + 0.5), (1.0, 0.0), (-INF, INF)):
                want = ref.region_ref(F, T, goal, thr, lo, hi)
                got = region_loop(Fb, Tb, nx, ny, ld, goal, thr, lo, hi)
                assert got[:2] == want[:2], (name, tname, lo, hi)
                assert fbits(got[2]) == fbits(want[2]), (name, tname)


@pytest.mark.parametrize("nx,ny,ld", list(grids()))
def test_labels_ref_is_loop_and_fast(nx, ny, ld):
    for name, T, seeds in seeded_maps(nx, ny):
        want = ref.labels_from_T(T, seeds)
        got = labels_loop(ref.pitched(T, ld, PAD_T), nx, ny, ld, seeds)
        assert got == want.ravel().tolist(), name
        assert np.array_equal(ref.labels_fast(T, seeds), want), name


def r_const_cases(nx, ny):
    """name -> (F, goal, expected r_const): the constant-speed radius on constructed F."""
    far = (nx - 1, ny - 1)
    d_far = math.sqrt((nx - 1) ** 2 + (ny - 1) ** 2)
    one = nx * ny == 1
    cases = {"constant": (np.full((ny, nx), 2.0), (0, 0), INF)}
    for tag, v in (("far_finite", 3.0), ("far_inf", INF), ("far_nan", np.nan)):
        F = np.full((ny, nx), 2.0)
        F[far[1], far[0]] = v
        # on 1x1 the far corner is the goal: a NaN goal differs from itself, others do not
        cases[tag] = (F, (0, 0), (0.0 if tag == "far_nan" else INF) if one else d_far)
    F = np.full((ny, nx), 2.0)
    F[0, 0] = INF
    cases["goal_inf"] = (F, (0, 0), INF if one else 1.0)
    return cases


@pytest.mark.parametrize("nx,ny,ld", list(grids()))
def test_r_const_cases(nx, ny, ld):
    T = ref.cone(nx, ny)
    for name, (F, goal, want) in r_const_cases(nx, ny).items():
        assert ref.region_ref(F, T, goal, 0.0, 0.0, 0.0)[2] == want, name
        got = region_loop(ref.pitched(F, ld, PAD_F), ref.pitched(T, ld, PAD_T), nx, ny, ld, goal,
                          0.0, 0.0, 0.0)
        assert got[2] == want, name


# ---------------------------------------------------------------------------
# non-vacuity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(97, 61), (33, 65)])
def test_label_family_outcomes(nx, ny):
    """At least 10 % of the finite cells of the cone with pits and walls are labelled, at
    least 10 % are finite and NONE, at least 10 % have a tied smallest neighbour; all
    three labels occur."""
    T = ref.cone_pits(nx, ny)
    seeds = ref.seed_lists("cone_pits", T)["sites"]
    lab = ref.labels_from_T(T, seeds)
    fin = np.isfinite(T)
    pad = np.full((ny + 2, nx + 2), INF)
    pad[1:-1, 1:-1] = T
    nb = np.stack([pad[:-2, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:], pad[2:, 1:-1]])
    best = nb.min(axis=0)
    tied = fin & (best < T) & ((nb == best).sum(axis=0) >= 2)
    n_fin = int(fin.sum())
    n_lab, n_none, n_tied = int((lab != NONE).sum()), int((fin & (lab == NONE)).sum()), int(tied.sum())
    print(f"{nx}x{ny}: finite {n_fin}, labelled {n_lab}, finite NONE {n_none}, tied {n_tied}")
    assert min(n_lab, n_none, n_tied) >= 0.10 * n_fin
    assert {0, 1, 2} <= set(np.unique(lab).tolist())
    # seed 6 sits on a cell with a lower neighbour and is a root with upstream cells;
    # the duplicates (3, 4) and the dominated seed (5) are nobody's label
    assert (lab == 6).sum() >= 2
    assert not np.isin(lab, (3, 4, 5)).any()
    i, j, t0 = seeds[6]
    assert min(T[jj, ii] for ii, jj in ((i, j - 1), (i - 1, j), (i + 1, j), (i, j + 1))
               if 0 <= ii < nx and 0 <= jj < ny) < t0 == T[j, i]


@pytest.mark.parametrize("nx,ny", [(97, 61), (33, 65)])
def test_early_mask_inputs_hold_every_clause(nx, ny):
    F = ref.speed_field(nx, ny)
    T = ref.cone_pits(nx, ny)
    th = ref.thresholds(T)
    tc = th["tie"]
    closed = T <= tc
    pad = np.zeros((ny + 2, nx + 2), dtype=bool)
    pad[1:-1, 1:-1] = closed
    nb = pad[:-2, 1:-1] | pad[1:-1, :-2] | pad[1:-1, 2:] | pad[2:, 1:-1]
    assert (~closed & nb & np.isposinf(F)).any()   # +inf speed next to a closed cell
    assert (~closed & nb & np.isnan(F)).any()      # NaN speed next to a closed cell
    assert (~closed & np.isfinite(T) & np.isposinf(F)).any()  # finite T on F = +inf: reset
    assert (T == tc).sum() >= 20 and (T <= th["tie_below"]).sum() < closed.sum()
    _, band = ref.early_mask_ref(F, T, tc)
    assert band.size > 5  # cap = 5 truncates


# ---------------------------------------------------------------------------
# mutant separation
# ---------------------------------------------------------------------------
def mask_inputs():
    for nx, ny, ld in grids():
        F = ref.speed_field(nx, ny)
        for name in ref.FAMILIES:
            T = ref.family(name, nx, ny)
            for tc in ref.thresholds(T).values():
                yield ref.pitched(F, ld, PAD_F), ref.pitched(T, ld, PAD_T), nx, ny, ld, tc


def equal_inputs():
    for nx, ny, ld in grids():
        for name in ref.FAMILIES:
            T = ref.family(name, nx, ny)
            for value in (ref.tie_value(T), 0.0, -0.0, INF):
                yield ref.pitched(T, ld, value), nx, ny, ld, value
            T = T.copy()
            T[ny - 1, nx - 1] = 12345.678  # once, at the last cell
            yield ref.pitched(T, ld, 12345.678), nx, ny, ld, 12345.678


def region_inputs():
    for nx, ny, ld in grids():
        F = ref.speed_field(nx, ny)
        goal = ref.sites_for(nx, ny)[0]
        for name in ref.FAMILIES:
            T = ref.family(name, nx, ny)
            v = ref.tie_value(T)
            for thr in ref.thresholds(T).values():
                yield (ref.pitched(F, ld, PAD_F), ref.pitched(T, ld, PAD_T), nx, ny, ld, goal, thr,
                       v, v)
        for F, goal, _ in r_const_cases(nx, ny).values():
            yield (ref.pitched(F, ld, PAD_F), ref.pitched(ref.cone(nx, ny), ld, PAD_T), nx, ny, ld,
                   goal, 0.0, 0.0, 0.0)


def label_inputs():
    for nx, ny, ld in grids():
        for _, T, seeds in seeded_maps(nx, ny):
            yield ref.pitched(T, ld, PAD_T), nx, ny, ld, seeds


MUTANTS = [
    # neighbour order reversed in the parent choice / last smallest instead of first
    ("labels", "rev_order"), ("labels", "last_smallest"),
    # < for <= against tc or thr
    ("mask", "lt"), ("region", "lt"),
    # <= for < in "strictly below"
    ("labels", "le_strict"),
    # the last row or the last column skipped
    ("mask", "skip_last_row"), ("mask", "skip_last_col"), ("equal", "skip_last_row"),
    ("equal", "skip_last_col"), ("region", "skip_last_row"), ("region", "skip_last_col"),
    ("labels", "skip_last_row"), ("labels", "skip_last_col"),
    # the index computed with ld where nx belongs, and the reverse
    ("mask", "ld_for_nx"), ("mask", "nx_for_ld"), ("equal", "ld_for_nx"), ("equal", "nx_for_ld"),
    ("region", "nx_for_ld"), ("labels", "nx_for_ld"),
    # padding columns included in a count, a min or a max (and in the band test)
    ("equal", "pad_cols"), ("region", "pad_cols"), ("mask", "pad_cols"),
    # band test ignoring F
    ("mask", "ignore_F"),
    # root rule taking the highest k / ignoring T != t0
    ("labels", "highest_k"), ("labels", "ignore_t0"),
    # box not distinguishing "only (0,0)" from "none"
    ("region", "box_none"),
    # value compare instead of bit compare: -0.0 would count the +0.0 goal
    ("equal", "float_eq"),
]
KINDS = {"mask": (early_mask_loop, mask_inputs), "equal": (equal_loop, equal_inputs),
         "region": (region_loop, region_inputs), "labels": (labels_loop, label_inputs)}


def _same(a, b):
    return repr(a) == repr(b)  # exact: repr of floats is unique per value, nan == nan, -0.0 != 0.0


@pytest.mark.parametrize("kind,mut", MUTANTS, ids=[f"{k}-{m}" for k, m in MUTANTS])
def test_mutant_is_separated(kind, mut):
    fn, inputs = KINDS[kind]
    hits = total = 0
    for args in inputs():
        total += 1
        if not _same(fn(*args), fn(*args, mut=mut)):
            hits += 1
            if hits >= 3:
                break
    print(f"{kind}/{mut}: separated on {hits} of the first {total} inputs")
    assert hits >= 1
