"""combineTotalCostMaps, viaCorridor and rendezvous on the planner.

The yardstick is numpy on the planes the planner itself hands out (batchTotalCost): the
header's fold in the listed order, bit for bit, and what follows from it -- the summary,
the corridor's bound, mask, box and count, the rendezvous cell.  The fixture is the 128 x 96
map and the four goals of test_gpu_cost_window.py.
"""
import numpy as np
import pytest

from test_gpu_cost_window import GOAL, GOALS, NX, NY, bits, case  # noqa: F401 (case: a fixture)
from test_gpu_global_risk import INF, new_planner, speed, wp
from test_gpu_plane_reduce import MAX, MIN, NONE, SUM, fold, same_summary, summary_ref

pytestmark = pytest.mark.gpu

PAIR, SLACK = (0, 1), 0.05
OPS = {"sum": SUM, "max": MAX, "min": MIN}


def planner(dymu, case, track=False):
    p = new_planner(dymu, case.cost, risk=None)
    p.trackSpeedChanges(track)
    assert p.computeTotalCostMaps([wp(*g) for g in GOALS])
    return p


def downloads(p):
    planes = [p.batchTotalCost(b) for b in range(p.batchCount())]
    assert all(T is not None for T in planes)
    return planes


def check_combine(p, planes, op, ids=None, weights=None, offsets=None):
    s = p.combineTotalCostMaps(op, planes=ids, weights=weights, offsets=offsets)
    assert s is not False
    ids = list(range(len(planes))) if ids is None else ids
    ref, ref_arg = fold([planes[b] for b in ids], ids, OPS[op], weights, offsets)
    out = p.combinedTotalCost()
    assert np.array_equal(bits(out), bits(ref))
    same_summary(s, summary_ref(ref, ref_arg, OPS[op]))
    arg = p.combinedPlanes()
    if op == "sum":
        assert arg is False  # a sum has no plane map
    else:
        assert np.array_equal(arg, ref_arg)
    flat = p.combinedTotalCost(raw=False)
    assert np.array_equal(flat == -1.0, out == INF)
    assert np.array_equal(bits(flat[out < INF]), bits(out[out < INF]))
    return ref


def corridor_ref(Ta, Tb, slack):
    D = Ta + Tb
    fin = D < INF
    d_min = D[fin].min()
    bound = d_min * (1.0 + slack)
    mask = (D <= bound).astype(np.uint8)
    jj, ii = np.nonzero(mask)
    k = int(np.flatnonzero(fin.ravel() & (D.ravel() == d_min))[0])
    return mask, {"D_min": float(d_min), "cell": (k % D.shape[1], k // D.shape[1]),
                  "count": int(mask.sum()), "box": (ii.min(), jj.min(), ii.max(), jj.max()),
                  "bound": float(bound)}


@pytest.fixture(scope="module")
def premises(oracle, case):
    """On the oracle's FMM maps of the two goals: both goal cells lie inside the reference
    corridor, which is neither empty nor every reachable cell."""
    F = speed(case.cost)
    Ta, Tb = (oracle.fmm(F, GOALS[g])[0] for g in PAIR)
    mask, info = corridor_ref(Ta, Tb, SLACK)
    for g in PAIR:
        assert mask[GOALS[g][1], GOALS[g][0]] == 1, "a goal outside the reference corridor"
    assert 0 < info["count"] < int(((Ta + Tb) < INF).sum())
    return info


def test_combine(dymu, case):
    p = planner(dymu, case)
    try:
        planes = downloads(p)
        assert (np.isinf(planes[0])).any()  # obstacles: +inf takes part
        for op in OPS:
            check_combine(p, planes, op)
            check_combine(p, planes, op, ids=[3, 1])
            check_combine(p, planes, op, ids=[2, 0, 3], weights=[0.5, 2.0, 1.25],
                          offsets=[10.0, 0.0, 2.5])
        # bad lists refuse and leave the last combined map readable
        last = p.combinedTotalCost()
        assert p.combineTotalCostMaps("sum", planes=[0, 4]) is False
        assert p.combineTotalCostMaps("sum", planes=[]) is False
        assert p.combineTotalCostMaps("max", planes=[0, 1], weights=[1.0]) is False
        assert p.combineTotalCostMaps("max", planes=[0, 1], weights=[1.0, 0.0]) is False
        assert p.combineTotalCostMaps("min", planes=[0, 1], offsets=[-1.0, 0.0]) is False
        assert np.array_equal(bits(p.combinedTotalCost()), bits(last))
        assert p.lastCombineKernelMs() > 0.0
    finally:
        p.close()


def test_corridor(dymu, case, premises):
    a, b = PAIR
    p = planner(dymu, case)
    try:
        planes = downloads(p)
        got = p.viaCorridor(a, b, SLACK)
        assert got is not False
        mask, info = got
        ref_mask, ref = corridor_ref(planes[a], planes[b], SLACK)
        assert np.array_equal(mask, ref_mask)
        assert info == ref
        assert info["D_min"] == pytest.approx(premises["D_min"], rel=1e-9)
        for g in PAIR:
            assert mask[GOALS[g][1], GOALS[g][0]] == 1
        via = p.combinedTotalCost()  # the via field stays as the combined map
        assert np.array_equal(bits(via), bits(planes[a] + planes[b]))
        # a = b is legal: twice one map, the corridor around its goal
        mask1, info1 = p.viaCorridor(2, 2, 0.5)
        ref_mask1, ref1 = corridor_ref(planes[2], planes[2], 0.5)
        assert np.array_equal(mask1, ref_mask1) and info1 == ref1
        assert info1["D_min"] == 0.0 and info1["cell"] == GOALS[2] and info1["count"] == 1
        kept = p.combinedTotalCost()
        for bad in ((0, 4, SLACK), (4, 0, SLACK), (0, 1, -0.01), (0, 1, float("nan")),
                    (0, 1, INF)):
            assert p.viaCorridor(*bad) is False
        assert np.array_equal(bits(p.combinedTotalCost()), bits(kept))
    finally:
        p.close()


def rendezvous_ref(planes, ids, minimax, weights=None):
    ref, ref_arg = fold([planes[b] for b in ids], ids, MAX if minimax else SUM, weights)
    s = summary_ref(ref, ref_arg, MAX if minimax else SUM)
    return (s["min_i"], s["min_j"], s["min_value"]), ref


def test_rendezvous(dymu, case):
    p = planner(dymu, case)
    try:
        planes = downloads(p)
        for minimax in (True, False):
            for ids, w in ((None, None), ([0, 1, 3], None), (None, [1.0, 3.0, 0.5, 2.0]),
                           ([3, 0], [4.0, 0.25])):
                got = p.rendezvous(planes=ids, weights=w, minimax=minimax)
                ref, field = rendezvous_ref(planes, ids or [0, 1, 2, 3], minimax, w)
                assert got == ref
                assert np.array_equal(bits(p.combinedTotalCost()), bits(field))
        i, j, v = p.rendezvous(planes=[1], minimax=True)
        assert (i, j) == GOALS[1] and v == 0.0  # one rover: at its own goal
    finally:
        p.close()


def test_truncated_batch_is_completed(dymu, case):
    p = new_planner(dymu, case.cost, risk=None)
    q = planner(dymu, case)
    try:
        gi, gj = GOALS[0]
        near = next((i, j) for j in range(gj + 2, gj + 6) for i in range(gi + 2, gi + 6)
                    if case.cost[j, i] > 0)
        M = p.costMatrix([wp(*g) for g in GOALS], [wp(*near)], until=True)
        assert M is not None and np.isfinite(M).all()
        assert p.batchLevel() < INF
        s = p.combineTotalCostMaps("max")
        assert s is not False
        assert p.batchLevel() == INF and p.lastBatchSolveKind() == 0
        planes = downloads(p)
        ref, ref_arg = fold(planes, range(4), MAX)
        assert np.array_equal(bits(p.combinedTotalCost()), bits(ref))
        assert np.array_equal(p.combinedPlanes(), ref_arg)
        same_summary(s, summary_ref(ref, ref_arg, MAX))
        # within the solver's parity of the batch that was complete from the start
        full = fold(downloads(q), range(4), MAX)[0]
        assert np.array_equal(np.isinf(ref), np.isinf(full))
        fin = np.isfinite(full)
        assert (np.abs(ref[fin] - full[fin]) <= 1e-12 * np.maximum(1.0, full[fin])).all()
    finally:
        p.close()
        q.close()


@pytest.mark.parametrize("track", [True, False], ids=["tracking", "untracked"])
def test_invalidation(dymu, case, track):
    i, j = case.box
    p = planner(dymu, case, track=track)
    try:
        goals = [wp(*g) for g in GOALS]
        before = check_combine(p, downloads(p), "min")
        if track:  # a reuse keeps the combined map
            assert p.computeTotalCostMaps(goals) and p.lastBatchSolveKind() == 2
            assert np.array_equal(bits(p.combinedTotalCost()), bits(before))
        # the speed changes, and a single-goal solve synchronises it
        assert p.setCostMapWindow(i, j, case.block)
        assert p.setGoal(wp(*GOAL)) and p.computeEntireTotalCostMap()
        if not track:  # the batch is gone, and the combined map with it
            assert p.batchCount() == 0
            assert p.combinedTotalCost() is False and p.combinedPlanes() is False
            assert p.combineTotalCostMaps("min") is False
            assert p.viaCorridor(0, 1, SLACK) is False
            assert p.rendezvous() is False
            return
        planes = downloads(p)  # a batch reader: re-propagates the pending box
        assert p.lastBatchSolveKind() == 1
        assert p.combinedTotalCost() is False and p.combinedPlanes() is False
        after = check_combine(p, planes, "min")
        assert (bits(after) != bits(before)).any()  # the box's cells are obstacles now
        assert (after[j:j + 3, i:i + 3] == INF).all()
    finally:
        p.close()
