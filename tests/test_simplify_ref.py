"""tests/simplify_ref.py, the plain-Python statement of getSimplifiedPaths' rule, on
constructed polylines: what it keeps where the answer is known, and its guarantee -- every
dropped waypoint within eps of the segment between its kept neighbours -- wherever it is
not."""
import numpy as np
import pytest

import simplify_ref as ref


def _kept(xy, eps):
    idx = ref.simplify(xy, eps)
    assert ref.check(xy, idx, eps) is None, ref.check(xy, idx, eps)
    return [int(i) for i in idx]


def test_straight_run_gives_two_points():
    t = np.arange(50) * 0.4
    for d in ((1.0, 0.0), (0.0, -1.0), (0.6, 0.8)):
        xy = np.stack([3.0 + d[0] * t, -2.0 + d[1] * t], axis=1)
        assert _kept(xy, 0.05) == [0, 49]
        assert _kept(xy, 1.0) == [0, 49]


def test_right_angle_keeps_the_corner():
    leg = np.arange(0, 21) * 0.5
    xy = np.vstack([np.stack([leg, 0 * leg], axis=1), np.stack([10.0 + 0 * leg[1:], leg[1:]], axis=1)])
    assert _kept(xy, 0.25) == [0, 20, 40]
    # an eps as large as the legs lets the corner go
    assert _kept(xy, 8.0) == [0, 40]


def test_zigzag_below_and_above_eps():
    k = np.arange(60)
    amp = 0.1
    xy = np.stack([0.4 * k, amp * (k % 2)], axis=1)
    assert _kept(xy, 0.25) == [0, 59]  # amplitude below eps: one segment
    few = _kept(xy, 0.01)  # amplitude above eps: nearly every turn is kept
    assert len(few) >= 58
    mid = _kept(xy, 0.06)
    assert 2 < len(mid) <= len(few)


def test_spiral_breaks_by_the_cone():
    t = np.linspace(0, 6 * np.pi, 400)
    xy = np.stack([(1 + 0.3 * t) * np.cos(t), (1 + 0.3 * t) * np.sin(t)], axis=1)
    few, many = _kept(xy, 0.25), _kept(xy, 0.02)
    assert 10 < len(few) < len(many) < 400


def test_doubling_back_breaks_by_far2():
    """Out along a line and back along it: every waypoint is inside the cone all the way,
    only the far2 rule sees the turn -- without it the far end would be dropped, 10 away
    from the kept segment."""
    out = np.arange(0, 26) * 0.4
    x = np.concatenate([out, out[-2::-1][:20]])
    xy = np.stack([x, 0 * x], axis=1)
    kept = _kept(xy, 0.25)
    assert kept == [0, 25, len(xy) - 1]
    # a return that overshoots the start
    x2 = np.concatenate([out, out[-2::-1], -out[1:10]])
    kept2 = _kept(np.stack([x2, 0 * x2], axis=1), 0.25)
    assert kept2 == [0, 25, len(x2) - 1]


def test_repeated_points():
    xy = np.array([[1.0, 1.0]] * 4 + [[2.0, 1.0]] * 3 + [[2.0, 3.0]] * 2 + [[2.0, 3.0]])
    kept = _kept(xy, 0.1)
    assert kept[0] == 0 and kept[-1] == 9
    assert any(4 <= k <= 6 for k in kept)  # the corner at (2, 1), by one of its copies
    same = np.tile([[5.0, -3.0]], (7, 1))
    assert _kept(same, 0.5) == [0, 6]


def test_single_and_empty():
    assert _kept(np.array([[2.5, 3.5]]), 0.3) == [0]
    assert _kept(np.array([[2.5, 3.5], [2.5, 3.9]]), 0.3) == [0, 1]
    assert len(ref.simplify(np.zeros((0, 2)), 0.3)) == 0
    assert ref.check(np.zeros((0, 2)), [], 0.3) is None


@pytest.mark.parametrize("eps", [0.05, 0.25, 1.0])
def test_random_walks(eps):
    rng = np.random.default_rng(5)
    ratios = []
    for trial in range(30):
        n = int(rng.integers(2, 400))
        # a heading that drifts, with now and then a sharp turn; steps of 0.4 like the descent
        turn = rng.normal(0, 0.15, n) + (rng.uniform(size=n) < 0.03) * rng.uniform(-3, 3, n)
        h = np.cumsum(turn)
        xy = np.cumsum(0.4 * np.stack([np.cos(h), np.sin(h)], axis=1), axis=0)
        idx = ref.simplify(xy, eps)
        assert ref.check(xy, idx, eps) is None, (trial, ref.check(xy, idx, eps))
        ratios.append(n / len(idx))
    print(f"eps {eps}: walked / kept {min(ratios):.2f} .. {max(ratios):.2f}")


def test_check_rejects_bad_sets():
    t = np.linspace(0, np.pi, 40)
    xy = np.stack([5 * np.cos(t), 5 * np.sin(t)], axis=1)
    assert ref.check(xy, [0, 39], 0.25) is not None  # the arc is 5 from its chord
    assert ref.check(xy, [0, 20, 20, 39], 10.0) is not None
    assert ref.check(xy, [1, 39], 10.0) is not None and ref.check(xy, [0, 38], 10.0) is not None
    assert ref.check(xy, ref.simplify(xy, 0.25), 0.25) is None


def test_simplify_slots_appends_the_sink():
    xy = np.stack([np.arange(10) * 0.4, np.zeros(10)], axis=1)
    slots = np.hstack([xy, np.zeros((10, 2))])
    assert list(ref.simplify_slots(slots, 1, 0.25)) == [0, 8, 9]  # 9 walked, then the sink
    assert list(ref.simplify_slots(slots, 0, 0.25)) == [0, 9]
    assert list(ref.simplify_slots(slots[:0], -1, 0.25)) == []
