"""tests/route_ref.py, the plain-Python definition of every cell's node route
(include/dymu_fim.h), on hand-built maps whose answers are known."""
import numpy as np

import route_ref as ref

INF = np.inf
NONE = ref.NONE
S2 = 1.4142135623730951


def test_exact_distance_map_5x5():
    j, i = np.mgrid[0:5, 0:5].astype(float)
    T = np.hypot(i - 2, j - 2)
    res = 0.5
    r = ref.route_fields(T, res, [(2, 2, 0.0)], [np.ones((5, 5)), i])
    dx, dy = np.abs(i - 2).astype(int), np.abs(j - 2).astype(int)
    assert (r["sink"] == 0).all()
    assert np.array_equal(r["diag"], np.minimum(dx, dy))
    assert np.array_equal(r["axis"], np.abs(dx - dy))
    want = res * r["axis"].astype(float) + (res * S2) * r["diag"].astype(float)
    assert r["length"].tobytes() == want.tobytes()
    assert r["length"][2, 2] == 0.0 and r["length"][0, 0] == 2 * (res * S2)
    assert r["length"][0, 2] == 2 * res and r["length"][1, 0] == res + res * S2
    # a field of ones integrates to the length (the same terms, here exactly); the
    # column index's extrema are the route's ends
    assert np.allclose(r["integral"][0], r["length"], rtol=0, atol=1e-15)
    assert np.array_equal(r["vmin"][1], np.minimum(i, 2.0))
    assert np.array_equal(r["vmax"][1], np.maximum(i, 2.0))
    assert (r["vmin"][0] == 1.0).all() and (r["vmax"][0] == 1.0).all()
    nodes, k = ref.walk(T, [(2, 2, 0.0)], 0, 1)
    assert k == 0 and nodes == [(0, 1), (1, 2), (2, 2)]


def test_diagonal_with_one_side_node_infinite_is_not_taken():
    T = np.array([[0.0, INF, 9.0],
                  [1.0, 1.4, 9.0],
                  [9.0, 9.0, 9.0]])
    par, kind = ref.parents(T)
    assert par[1 * 3 + 1] == 1 * 3 + 0 and kind[4] == 0  # west, not the cut corner to (0, 0)
    r = ref.route_fields(T, 1.0, [(0, 0, 0.0)])
    assert r["axis"][1, 1] == 2 and r["diag"][1, 1] == 0 and r["sink"][1, 1] == 0
    T[0, 1] = 1.2  # both side nodes finite: the diagonal's score 1.4 * 0.7071 beats 0.4
    par, kind = ref.parents(T)
    assert par[4] == 0 and kind[4] == 1
    r = ref.route_fields(T, 1.0, [(0, 0, 0.0)])
    assert r["axis"][1, 1] == 0 and r["diag"][1, 1] == 1 and r["length"][1, 1] == S2


def test_tie_between_axis_and_diagonal():
    a = 2.0 - S2  # exact; 2.0 - a == S2 == (2.0 - 0.0) * 0.7071067811865476, a tie
    assert 2.0 - a == S2 == 2.0 * ref.DIAG
    T = np.array([[0.0, 1.9, 9.0],
                  [a, 2.0, 9.0],
                  [9.0, 9.0, 9.0]])
    par, kind = ref.parents(T)
    assert par[4] == 3 and kind[4] == 0  # equal scores: west comes first in the order
    T[1, 0] = np.nextafter(a, 1.0)  # the axis score one ulp lower: the diagonal wins
    par, kind = ref.parents(T)
    assert par[4] == 0 and kind[4] == 1
    # the factor: the diagonal's fall is larger (1.3 against 1.0), its score is not
    T[1, 0], T[0, 0] = 1.0, 0.7
    par, kind = ref.parents(T)
    assert par[4] == 3 and kind[4] == 0
    # among axis neighbours of equal score the order decides: (i, j-1) before (i-1, j)
    T = np.array([[0.0, 1.0, 9.0],
                  [1.0, 2.0, 9.0],
                  [9.0, 9.0, 9.0]])
    T[0, 0] = 1.5  # no diagonal candidate
    par, _ = ref.parents(T)
    assert par[4] == 1


def test_plateau_and_its_drainage_have_no_route():
    n, goal = 12, (3, 3)
    T = np.full((n, n), 5.0)
    T[goal[1], goal[0]] = 0.0
    T[6:, 6:] = 7.0  # a step down onto the plateau, then nothing lower
    T[0, 11] = INF
    T[0, 10] = np.nan
    r = ref.route_fields(T, 1.0, [goal + (0.0,)], [np.ones((n, n))])
    near = np.zeros((n, n), dtype=bool)
    near[2:5, 2:5] = True
    assert (r["sink"][near] == 0).all()
    assert (r["sink"][~near] == NONE).all()  # the plateau, the 7.0 cells that drain to it, inf, NaN
    assert r["axis"][~near].sum() == 0 and r["diag"][~near].sum() == 0
    assert np.isnan(r["length"][~near]).all() and np.isnan(r["integral"][0][~near]).all()
    assert (r["vmin"][0][~near] == INF).all() and (r["vmax"][0][~near] == -INF).all()
    nodes, k = ref.walk(T, [goal + (0.0,)], 6, 8)
    assert k is None and nodes == [(6, 8), (5, 8)]  # one step down (west), then a dead end


def test_root_with_a_lower_neighbour_stays_terminal():
    T = np.array([[9.0, 9.0, 9.0],
                  [0.0, 1.0, 3.0],
                  [9.0, 9.0, 9.0]])
    seeds = [(2, 1, 3.0), (0, 1, 0.0)]
    f = np.arange(9.0).reshape(3, 3)
    r = ref.route_fields(T, 1.0, seeds, [f])
    assert r["sink"][1, 2] == 0 and r["axis"][1, 2] == 0 and r["length"][1, 2] == 0.0
    assert r["integral"][0][1, 2] == 0.0 and r["vmin"][0][1, 2] == r["vmax"][0][1, 2] == f[1, 2]
    assert r["sink"][1, 1] == 1 and r["sink"][1, 0] == 1
    # above the root the fall of 6 beats the diagonal's 8 * 0.7071: that cell ends on root 0
    assert r["sink"][0, 2] == 0 and r["axis"][0, 2] == 1 and r["sink"][0, 1] == 1
    assert ref.walk(T, seeds, 2, 1) == ([(2, 1)], 0)


def test_dominated_seed_is_no_root():
    T = np.array([[9.0, 9.0, 9.0, 9.0],
                  [0.0, 1.0, 2.0, 3.0],
                  [9.0, 9.0, 9.0, 9.0]])
    seeds = [(2, 1, 6.5), (0, 1, 0.0), (0, 1, 0.0), (0, 1, 4.0)]
    assert ref.roots(T, seeds) == {4: 1}  # duplicates: the smallest t0, the lowest k
    r = ref.route_fields(T, 2.0, seeds)
    assert (r["sink"] == 1).all()
    assert r["axis"][1, 2] == 2 and r["length"][1, 3] == 6.0
    # -0.0 as an offset is +0.0 (the engine stages t0 + 0.0)
    assert ref.roots(T, [(0, 1, -0.0)]) == {4: 0}


def test_minimum_and_maximum_do_not_depend_on_the_order():
    assert np.signbit(ref.rmin(0.0, -0.0)) and np.signbit(ref.rmin(-0.0, 0.0))
    assert not np.signbit(ref.rmax(0.0, -0.0)) and not np.signbit(ref.rmax(-0.0, 0.0))
    assert ref.rmin(INF, 3.0) == 3.0 and ref.rmax(-INF, 3.0) == 3.0
