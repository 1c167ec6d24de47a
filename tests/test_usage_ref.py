"""tests/usage_ref.py, the plain-Python definition of how much of the map drains through
every cell (include/dymu_fim.h), against identities that need no sweep
order: they are evaluated from the parents alone, with numpy scatter-adds."""
import numpy as np
import pytest

import route_ref
import usage_ref as ref

INF = np.inf
NONE = ref.NONE


def bumpy_map(nx, ny, goals, offsets, obst_frac, seed):
    """A map that is no solve's, but has what the definition sees: one value per cell that
    rises away from the goals, rippled so that routes merge and bend, +inf obstacles, a NaN,
    and -- by the ripple -- a few local minima that are no seeds."""
    rng = np.random.default_rng(seed)
    j, i = np.mgrid[0:ny, 0:nx].astype(float)
    T = np.full((ny, nx), INF)
    for (gi, gj), t0 in zip(goals, offsets):
        T = np.minimum(T, t0 + np.hypot(i - gi, j - gj))
    # a seed whose own cone does not reach its cell first is dominated: its cell keeps the map's value
    own = [(g, t0) for g, t0 in zip(goals, offsets) if T[g[1], g[0]] == t0]
    T += 0.45 * np.sin(0.9 * i) * np.cos(0.7 * j) + 0.2 * rng.random((ny, nx))
    T[rng.random((ny, nx)) < obst_frac] = INF
    for (gi, gj), t0 in zip(goals, offsets):
        if not np.isfinite(T[gj, gi]):
            T[gj, gi] = 50.0
    for (gi, gj), t0 in own:
        T[gj, gi] = t0
    T[0, nx - 1] = np.nan
    return T


CASES = {
    "one-goal": dict(nx=41, ny=29, goals=[(30, 17)], offsets=[0.0], obst=0.03),
    "goal-set": dict(nx=37, ny=33, goals=[(30, 20), (5, 4), (12, 28), (29, 19)],
                     offsets=[0.0, 2.5, 0.0, 40.0], obst=0.02),  # the last is dominated
}


class Case:
    pass


@pytest.fixture(scope="module", params=sorted(CASES), ids=str)
def case(request):
    k = CASES[request.param]
    c = Case()
    c.T = bumpy_map(k["nx"], k["ny"], k["goals"], k["offsets"], k["obst"], seed=3)
    c.seeds = [g + (t0,) for g, t0 in zip(k["goals"], k["offsets"])]
    c.nx, c.ny = k["nx"], k["ny"]
    rng = np.random.default_rng(11)
    c.w = rng.integers(0, 2 ** 32, size=(c.ny, c.nx), dtype=np.uint64).astype(np.uint32)
    c.unit = ref.route_usage(c.T, c.seeds)
    c.weighted = ref.route_usage(c.T, c.seeds, c.w)
    c.par, c.root = ref.forest(c.T, c.seeds)
    yield c


def test_usage_is_own_weight_plus_the_children(case):
    for r, w in ((case.unit, np.ones((case.ny, case.nx), dtype=np.uint32)), (case.weighted, case.w)):
        u = r["usage"].ravel().astype(object)  # Python integers: the check cannot overflow
        has = r["sink"].ravel() != NONE
        want = np.where(has, w.ravel().astype(object), 0)
        for c in np.flatnonzero(has & (case.par >= 0)):
            want[case.par[c]] += u[c]
        assert (u[has] == want[has]).all()
        assert (u[~has] == 0).all()
        # a leaf -- no routed cell names it as parent -- holds its own weight
        leaf = has.copy()
        leaf[case.par[has & (case.par >= 0)]] = False
        assert leaf.sum() > 10 and (u[leaf] == w.ravel()[leaf]).all()
    assert case.weighted["usage"].max() > 2 ** 32  # the sums pass 32 bits


def test_sinks_are_the_route_fields_sinks(case):
    rf = route_ref.route_fields(case.T, 1.0, case.seeds)
    assert case.unit["sink"].tobytes() == rf["sink"].tobytes()
    assert case.weighted["sink"].tobytes() == rf["sink"].tobytes()
    has = case.unit["sink"] != NONE
    with np.errstate(invalid="ignore"):
        assert not has[~(case.T < INF)].any()
    assert 0 < (~has & np.isfinite(case.T)).sum()  # the ripple's dead-end basins
    assert has.sum() > 0.5 * has.size


def test_catchments_sum_to_the_routed_weight(case):
    for r, w in ((case.unit, None), (case.weighted, case.w)):
        has = r["sink"] != NONE
        total = int(has.sum()) if w is None else int(w[has].astype(object).sum())
        assert sum(int(x) for x in r["catchment"]) == total
        for k, s in enumerate(case.seeds):
            c = s[1] * case.nx + s[0]
            if case.root.get(c) == k:
                assert r["catchment"][k] == r["usage"][s[1], s[0]] > 0
                sel = r["sink"] == k
                assert int(r["catchment"][k]) == (int(sel.sum()) if w is None else
                                                  int(w[sel].astype(object).sum()))
            else:
                assert r["catchment"][k] == 0
    if len(case.seeds) == 4:
        assert case.unit["catchment"][3] == 0 and (case.unit["catchment"][:3] > 0).all()


def test_far_is_the_maximum_over_own_cost_and_the_children(case):
    r = case.unit
    far = r["far"].ravel()
    has = r["sink"].ravel() != NONE
    want = np.where(has, case.T.ravel(), -INF)
    kids = np.flatnonzero(has & (case.par >= 0))
    np.maximum.at(want, case.par[kids], far[kids])
    assert far[has].tobytes() == want[has].tobytes()
    assert np.isnan(far[~has]).all()
    assert (far[has] >= case.T.ravel()[has]).all()
    assert case.weighted["far"].tobytes() == r["far"].tobytes()  # no function of the weights
    for c, k in case.root.items():
        assert far[c] == case.T[r["sink"] == k].max()


def test_walks_increment_exactly_the_cells_that_count_them(case):
    """usage[c] counts d iff route(d) contains c: replaying the route of every routed cell
    node by node and counting the visits rebuilds the unit-weight map."""
    r = case.unit
    visits = np.zeros((case.ny, case.nx), dtype=np.uint64)
    cells = np.argwhere(r["sink"] != NONE)
    for j, i in cells:
        nodes, k = route_ref.walk(case.T, case.seeds, int(i), int(j))
        assert k == r["sink"][j, i]
        for a, b in nodes:
            visits[b, a] += 1
    assert visits.tobytes() == r["usage"].tobytes()
    # a cell without a route is counted nowhere, even where its walk crosses routed ground
    dead = np.argwhere((r["sink"] == NONE) & np.isfinite(case.T))
    for j, i in dead[:20]:
        nodes, k = route_ref.walk(case.T, case.seeds, int(i), int(j))
        assert k is None
        for a, b in nodes:
            assert r["sink"][b, a] == NONE and r["usage"][b, a] == 0


def test_chain_with_full_weights_carries_past_32_bits():
    nx = 37
    T = np.arange(nx, dtype=np.float64).reshape(1, nx)
    w = np.full((1, nx), 0xFFFFFFFF, dtype=np.uint32)
    r = ref.route_usage(T, [(0, 0, 0.0)], w)
    want = [(nx - i) * (2 ** 32 - 1) for i in range(nx)]
    assert [int(x) for x in r["usage"][0]] == want
    assert (r["far"] == nx - 1).all() and (r["sink"] == 0).all()
    assert int(r["catchment"][0]) == nx * (2 ** 32 - 1)


def test_non_seed_local_minimum_and_its_basin():
    n, goal = 12, (3, 3)
    T = np.full((n, n), 5.0)
    T[goal[1], goal[0]] = 0.0
    T[6:, 6:] = 7.0
    T[8, 8] = 1.0  # a local minimum that is no seed: its basin has no route
    r = ref.route_usage(T, [goal + (0.0,)])
    near = np.zeros((n, n), dtype=bool)
    near[2:5, 2:5] = True
    assert (r["sink"][near] == 0).all() and (r["sink"][~near] == NONE).all()
    assert (r["usage"][~near] == 0).all() and np.isnan(r["far"][~near]).all()
    assert r["usage"][3, 3] == 9 and r["catchment"][0] == 9 and r["far"][3, 3] == 5.0
    assert (r["usage"][near].sum() - 9) == 8  # eight leaves of 1
