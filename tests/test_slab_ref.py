"""CPU checks of tests/slab_ref.py, the references tests/test_gpu_domain.py compares the
slab-domain kernels with:

* merge_ref equals a per-cell Python loop on every constructed input.
* Non-vacuity: the constructed inputs hold the columns each clause of the merge rule is about.
* dirichlet_ref (the slab alone, true neighbour rows as boundary values) reproduces the
  oracle FMM's rows on every case the GPU file runs, so converging a slab against the FMM's
  neighbour rows must give the FMM's owned rows.
* Mutant separation: every listed mutant of the loop differs from merge_ref on at least one
  constructed input -- a kernel carrying that bug would fail the GPU comparison.
"""
import math

import numpy as np
import pytest

import slab_ref as ref

NXS = (5, 100, 300)
SHAPES = ((16, True, True), (48, True, True), (19, True, False))  # nrows, ghost_lo, ghost_hi
TILES = (8, 16)
RTOL = 1e-12  # the project's parity bound (include/dymu_fim.h)


def merge_loop(old_lo, old_hi, new_lo, new_hi, nx, nrows, tw, th, mut=None):
    """The merge, cell by cell.  Returns (lo_out, hi_out, queued) with queued a sorted LIST:
    a tile listed twice is a tile queued twice.  mut: one deliberate bug."""
    ntx, nty = -(-nx // tw), -(-nrows // th)
    rows, listed = [], []
    for side, (old, new) in enumerate(((old_lo, new_lo), (old_hi, new_hi))):
        if old is None or new is None:
            rows.append(None if old is None else list(old[:nx]))
            continue
        trow = 0 if side == 0 else nty - 1
        if mut == "hi_row0" and side == 1:
            trow = 0
        if mut == "lo_rowlast" and side == 0:
            trow = nty - 1
        out, mine = [], set()
        for i in range(nx):
            o, n = float(old[i]), float(new[i])
            if mut == "le":
                better = n <= o
            elif mut == "nan":
                better = not n >= o
            else:
                better = n < o
            if mut == "cut256" and i >= 256:
                better = False
            out.append(n if (better or mut == "overwrite") else o)
            if better:
                t = i // (tw // 2) if mut == "half_tile" else i // tw
                if mut == "drop_ragged" and nx % tw and t == ntx - 1:
                    continue
                mine.add(trow * ntx + t)
        rows.append(out)
        if mut == "twice":
            listed += sorted(mine)
        else:
            listed = sorted(set(listed) | mine)
    return rows[0], rows[1], sorted(listed)


def bits(row):
    return None if row is None else np.asarray(row, dtype=np.float64).view(np.uint64).tolist()


def same(a, b):
    return bits(a[0]) == bits(b[0]) and bits(a[1]) == bits(b[1]) and sorted(a[2]) == sorted(b[2])


def merge_inputs():
    """(old_lo, old_hi, new_lo, new_hi, nx, nrows, tw, th): the first, the repeated, the
    lowering and the one-sided merges of test_gpu_domain.py, for every shape and variant."""
    for nx in NXS:
        for nrows, lo, hi in SHAPES:
            for tw in TILES:
                for v in range(ref.NVARIANTS):
                    ol, nl = ref.constructed_rows(nx, tw, v)
                    oh, nh = ref.constructed_rows(nx, tw, v + 3) if hi else (None, None)
                    yield ol, oh, nl, nh, nx, nrows, tw, tw
                    g_lo, g_hi, q = ref.merge_ref(ol, oh, nl, nh, nx, nrows, tw, tw)
                    yield g_lo, g_hi, nl, nh, nx, nrows, tw, tw  # the same rows again
                    nty = -(-nrows // tw)
                    l3 = ref.lower_rows(g_lo, ref.tile_cols(q, 0, nx, tw))
                    h3 = ref.lower_rows(g_hi, ref.tile_cols(q, nty - 1, nx, tw)) if hi else None
                    yield g_lo, g_hi, l3, h3, nx, nrows, tw, tw
                    yield ol, oh, nl, None, nx, nrows, tw, tw  # a NULL side
                    if hi:
                        yield ol, oh, None, nh, nx, nrows, tw, tw
                    yield g_lo, g_hi, ref.quiet_rows(g_lo), (ref.quiet_rows(g_hi) if hi else None), \
                        nx, nrows, tw, tw


def test_merge_ref_equals_loop():
    n = 0
    for args in merge_inputs():
        assert same(ref.merge_ref(*args), merge_loop(*args)), args[4:]
        n += 1
    assert n > 500


def test_constructed_rows_hold_every_clause():
    for tw in TILES:
        seen = set()
        for nx in NXS:
            for v in range(ref.NVARIANTS):
                old, new = ref.constructed_rows(nx, tw, v)
                with np.errstate(invalid="ignore"):
                    better = new < old
                assert better[nx - 1]
                if nx > 256:
                    assert better[255] and better[256]
                    assert better[248:264].sum() == 2  # alone in their tiles
                for t in range(-(-nx // tw)):
                    c0, c1 = t * tw, min(nx, (t + 1) * tw)
                    b = better[c0:c1]
                    if b.sum() == 1 and b[0] and c1 - c0 == tw:
                        seen.add("first")
                    if b.sum() == 1 and b[-1] and c1 - c0 == tw:
                        seen.add("last")
                    if b.sum() == 1 and b[-1] and c1 - c0 < tw:
                        seen.add("ragged")
                    if not b.any() and (new[c0:c1] == old[c0:c1]).any():
                        seen.add("equal_only")
                    if np.isnan(new[c0:c1]).all():
                        seen.add("nan")
                    if b.all():
                        seen.add("below")
                    if (np.isinf(old[c0:c1]) & b).any():
                        seen.add("from_inf")
                    if (np.isinf(new[c0:c1]) & np.isfinite(old[c0:c1])).any():
                        seen.add("inf_over_finite")
                    if (new[c0:c1] > old[c0:c1]).any():
                        seen.add("above")
        assert seen == {"first", "last", "ragged", "equal_only", "nan", "below", "from_inf",
                        "inf_over_finite", "above"}, seen


def test_repeat_lower_and_quiet_merges():
    """The second merge of the same rows and a quiet row queue nothing and write nothing;
    the lowering row writes but queues only tiles that are queued already."""
    for nx in NXS:
        for nrows, lo, hi in SHAPES:
            for tw in TILES:
                nty = -(-nrows // tw)
                ol, nl = ref.constructed_rows(nx, tw, 2)
                oh, nh = ref.constructed_rows(nx, tw, 5) if hi else (None, None)
                g_lo, g_hi, q = ref.merge_ref(ol, oh, nl, nh, nx, nrows, tw, tw)
                assert q
                a_lo, a_hi, q2 = ref.merge_ref(g_lo, g_hi, nl, nh, nx, nrows, tw, tw)
                assert not q2 and bits(a_lo) == bits(g_lo) and bits(a_hi) == bits(g_hi)
                l3 = ref.lower_rows(g_lo, ref.tile_cols(q, 0, nx, tw))
                h3 = ref.lower_rows(g_hi, ref.tile_cols(q, nty - 1, nx, tw)) if hi else None
                b_lo, b_hi, q3 = ref.merge_ref(g_lo, g_hi, l3, h3, nx, nrows, tw, tw)
                assert q3 and q3 <= q and bits(b_lo) != bits(g_lo)
                c_lo, c_hi, q4 = ref.merge_ref(g_lo, g_hi, ref.quiet_rows(g_lo),
                                               ref.quiet_rows(g_hi) if hi else None, nx, nrows,
                                               tw, tw)
                assert not q4 and bits(c_lo) == bits(g_lo) and bits(c_hi) == bits(g_hi)


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_dirichlet_ref_is_the_fmm_rows(oracle, name):
    F, Tref, goal, r0, nrows = ref.case(oracle, name)
    T = ref.dirichlet_ref(oracle, F, Tref, r0, nrows)
    want = Tref[r0:r0 + nrows]
    assert np.array_equal(np.isinf(T), np.isinf(want))
    fin = np.isfinite(want)
    assert fin.sum() > nrows  # the slab is reached
    err = np.abs(T[fin] - want[fin]) / np.maximum(1.0, want[fin])
    assert err.max() <= RTOL
    assert np.array_equal(T.view(np.uint64), np.ascontiguousarray(want).view(np.uint64))


def test_dirichlet_ref_walled_case(oracle):
    """The peer test's slab: its last owned row is all obstacles, the rows behind it are
    unreachable, and the slab alone still reproduces the FMM's rows."""
    F, Tref, goal, r0, nrows = ref.walled_case(oracle)
    assert np.isinf(Tref[r0 + nrows - 1:]).all() and np.isfinite(Tref[r0]).any()
    T = ref.dirichlet_ref(oracle, F, Tref, r0, nrows)
    assert np.array_equal(T.view(np.uint64),
                          np.ascontiguousarray(Tref[r0:r0 + nrows]).view(np.uint64))


def test_dirichlet_ref_depends_on_the_boundary(oracle):
    """Not vacuous: without the neighbour rows the slab of a goal outside it stays +inf,
    and a raised boundary row raises the slab."""
    F, Tref, goal, r0, nrows = ref.case(oracle, "mid")
    none = np.full_like(Tref, math.inf)
    assert np.isinf(ref.dirichlet_ref(oracle, F, none, r0, nrows)).all()
    up = np.array(Tref)
    up[r0 - 1] += 1.0
    up[r0 + nrows] = math.inf
    T = ref.dirichlet_ref(oracle, F, up, r0, nrows)
    fin = np.isfinite(T)
    assert (T[fin] > Tref[r0:r0 + nrows][fin]).all()


MUTANTS = [
    "le",           # <= for <: an equal value queues its tile
    "overwrite",    # the received value always written
    "nan",          # NaN propagates: not (new >= old)
    "hi_row0",      # hi side queued into tile row 0
    "lo_rowlast",   # lo side queued into tile row nty - 1
    "half_tile",    # tile index i // (tile_w / 2)
    "drop_ragged",  # the last, ragged tile never queued
    "twice",        # a tile reached from both sides counted twice
    "cut256",       # columns at or beyond 256 dropped
]


@pytest.mark.parametrize("mut", MUTANTS)
def test_mutant_is_separated(mut):
    hits = total = 0
    for args in merge_inputs():
        total += 1
        if not same(ref.merge_ref(*args), merge_loop(*args, mut=mut)):
            hits += 1
    assert hits > 0, f"no constructed input separates mutant {mut} ({total} inputs)"
